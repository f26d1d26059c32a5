"""Diagnostics: the outputs of one engine library (MMPFN_LIB) over every precision mode and dispatch path, saved to
an .npz, so that two builds meant to be bitwise equal can be compared:  MMPFN_LIB=... python tools/lib_outputs.py out.npz
then  python tools/lib_outputs.py --compare a.npz b.npz
Legs: the fp16, bf16, fp32 (split-bf16) and fp32-MFMA logits of every golden case; the two fp16 + fp8 P.V modes on
pad_ufes_12l; forward_many with 2 lanes and batch 2 on one golden; and a table wider than 64 tokens per row (the bf16
fallback path: the bf16 and fp32 forwards, the cached predict, and the layer-0 attention taps)."""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "tests"), str(ROOT / "tests" / "golden")]


def compare(pa, pb):
    a, b = np.load(pa), np.load(pb)
    bad = [k for k in a.files if k not in b.files or not np.array_equal(a[k], b[k])]
    bad += [k for k in b.files if k not in a.files]
    for k in a.files:
        if k not in bad:
            print(f"{k}: EQUAL")
        elif k in b.files and a[k].shape == b[k].shape:
            print(f"{k}: DIFF max {np.abs(a[k] - b[k]).max():.3e}")
        else:
            print(f"{k}: DIFF (missing or another shape)")
    for k in b.files:
        if k not in a.files:
            print(f"{k}: DIFF (only in {pb})")
    return 1 if bad else 0


def lanes_leg(z, model, _lib):
    """Four label-permuted members of one golden through forward_many, 2 lanes x batch 2."""
    import torch

    eng = model.engine()
    x = torch.from_numpy(z["x"]) if "x" in z else None
    tok = eng.mixer_tokens(torch.from_numpy(z["image"]).cuda(), _lib.PREC_BF16) if "image" in z else None
    y = z["y_train"]
    cls = np.unique(y)
    rng = np.random.default_rng(1)
    items = []
    for _ in range(4):
        perm = dict(zip(cls, rng.permutation(cls)))
        items.append((x, tok, np.array([perm[v] for v in y], dtype=np.float32)))
    with torch.inference_mode():
        outs = eng.forward_many(items, _lib.PREC_BF16, lanes=2, batch=2)
        eng.status()
    return np.stack([o.cpu().numpy() for o in outs])


def wide_legs(_lib):
    """71 tokens per row (140 features): 2 layers, S = 260, N = 200."""
    import torch
    from synth import synth_labels, synth_state_dict, synth_table
    from test_parity_gpu import make_model

    from multimodalpfn_amd.model.spec import ModelConfig, state_dict_spec

    cfg = ModelConfig(nlayers=2, mgm_heads=8, cap_heads=4)
    model = make_model(cfg, synth_state_dict(state_dict_spec(cfg), 21))
    eng = model.engine()
    S, N, F = 260, 200, 140
    x = torch.from_numpy(synth_table(S, F, 21, n_cat=2)).cuda()
    y = synth_labels(S, 3, 21)[:N]
    res = {}
    with torch.inference_mode():
        res["wide_bf16"] = eng.forward(x, None, y, _lib.PREC_BF16)
        res["wide_f32"] = eng.forward(x, None, y, _lib.PREC_F32)
        cache = eng.cache_build(x[:N], None, y, _lib.PREC_BF16)
        res["wide_cached_bf16"] = eng.cache_predict(cache, x[N:], None)
        cache.free()
        X = eng.embed_state(x, None, y, _lib.PREC_F32)
        res["wide_feat_tap_bf16"] = eng.feature_attention(0, X, _lib.PREC_BF16)
        res["wide_item_tap_bf16"] = eng.item_attention_block(0, X, N, _lib.PREC_BF16)
        eng.status()
    return {k: v.cpu().numpy() for k, v in res.items()}


def main():
    if sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    from helpers import CASES, load_case
    from test_parity_gpu import make_model, run_case

    from multimodalpfn_amd import _lib

    modes = (("f16", _lib.PREC_F16), ("bf16", _lib.PREC_BF16), ("f32", _lib.PREC_F32), ("f32mfma", _lib.PREC_F32_MFMA))
    res = {}
    for case in CASES:
        z, meta, cfg, sd = load_case(case)
        model = make_model(cfg, sd)
        for name, p in modes:
            res[f"{case}_{name}"] = run_case(z, model, precision=p)
        if case == "pad_ufes_12l":
            for name, p in (("f16_f8", _lib.PREC_F16_F8), ("f16_f8e5", _lib.PREC_F16_F8E5)):
                res[f"{case}_{name}"] = run_case(z, model, precision=p)
            res[f"{case}_lanes2_batch2_bf16"] = lanes_leg(z, model, _lib)
    res.update(wide_legs(_lib))
    np.savez(sys.argv[1], **res)
    print("saved", len(res), "outputs to", sys.argv[1])


if __name__ == "__main__":
    main()
