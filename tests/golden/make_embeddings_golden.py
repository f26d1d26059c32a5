"""Generate the row-embedding goldens by running the REFERENCE model (build container only).

Run from the repo root:   python tests/golden/make_embeddings_golden.py

The cases, the reference model and the synthetic weights and inputs are ``make_golden.py``'s; the model is called with
``only_return_standard_out=False``, which returns, beside the decoder outputs, the target token's final state of every
row (``transformer.py:850-864``): ``train_embeddings`` ``[N, 1, E]`` and ``test_embeddings`` ``[Q, 1, E]``.  Before a
file is written its ``standard`` output must equal the committed ``<case>.npz`` logits bit for bit, so the embeddings
belong to exactly the forwards the logits goldens pin.  Written: ``tests/golden/emb/<case>.npz`` with
``train_embeddings`` ``[N, E]`` and ``test_embeddings`` ``[Q, E]``, fp32.
"""

from __future__ import annotations

import os
import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

from make_golden import CASES, build_reference  # noqa: E402  (puts the repo root on the path)
from synth import synth_image, synth_labels, synth_state_dict, synth_table  # noqa: E402

from multimodalpfn_amd.model.spec import ModelConfig, state_dict_spec  # noqa: E402


def run_case(case: dict) -> dict:
    cfg = ModelConfig(**case["cfg"])
    model, _, update_outliers = build_reference(cfg)
    sd = synth_state_dict(state_dict_spec(cfg), case["wseed"])
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    model.eval()
    update_outliers(model=model, remove_outliers_std=12.0, seed=cfg.model_seed, inplace=True)
    model.cache_trainset_representation = False
    S, N = case["S"], case["N"]
    x = synth_table(S, case["F"], case["dseed"], **case["data"]) if case["F"] else None
    y = synth_labels(S, case["n_classes"], case["dseed"])
    image = synth_image(S, case["n_mod"], case["dseed"]) if case["n_mod"] else None
    torch.manual_seed(0)
    with torch.inference_mode():
        out = model(
            None,
            torch.from_numpy(x[:, None, :]) if x is not None else None,
            torch.from_numpy(image) if image is not None else None,
            torch.from_numpy(y[:N]),
            only_return_standard_out=False,
            categorical_inds=list(range(case["data"].get("n_cat", 0))),
            single_eval_pos=N,
        )
    logits = out["standard"].squeeze(1).numpy().astype(np.float32)
    golden = np.load(HERE / f"{case['name']}.npz")["logits"]
    assert logits.shape == golden.shape and np.array_equal(logits, golden), \
        f"{case['name']}: the standard output is not the committed golden's logits"
    res = {k: out[k].squeeze(1).numpy().astype(np.float32) for k in ("train_embeddings", "test_embeddings")}
    assert res["train_embeddings"].shape == (N, cfg.emsize) and res["test_embeddings"].shape == (S - N, cfg.emsize)
    return res


def main():
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    only = set(sys.argv[1:])
    (HERE / "emb").mkdir(exist_ok=True)
    for case in CASES:
        if only and case["name"] not in only:
            continue
        res = run_case(case)
        path = HERE / "emb" / f"{case['name']}.npz"
        np.savez_compressed(path, **res)
        big = max(float(np.abs(v).max()) for v in res.values())
        print(f"{case['name']}: train {res['train_embeddings'].shape}, test {res['test_embeddings'].shape}, "
              f"max |embedding| {big:.2f} -> emb/{path.name} ({path.stat().st_size / 1e3:.0f} kB)")


if __name__ == "__main__":
    main()
