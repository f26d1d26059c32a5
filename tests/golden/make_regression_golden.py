"""Regression golden vectors from the REFERENCE (build container only).

Run from the repo root:   python tests/golden/make_regression_golden.py [head]

Imports ``/root/reference`` read-only, runs it on the CPU in fp32 and writes ``tests/golden/regression/*.npz``.
Inputs are regenerated from seeds by the tests (``tests/regression_oracle.py``); only the reference's outputs are
stored.

``head``  ``head_B<bars>.npz``: the reference's ``translate_probs_across_borders`` (utils.py:680-700), ensemble
          mean (regressor.py:699-706) and ``FullSupportBarDistribution`` point estimates on the seeded logits of
          ``regression_oracle.head_cases`` -- per case the final logits, mean, mode and quantiles.  No output may
          hold a NaN, and mean / mode / quantiles must be finite; a final logit is -inf exactly where the
          ensemble's float32 probability of that bar is zero (cancelled bars, bars beyond a 60-logit peak).
``model`` ``model_<case>.npz``: the reference ``PerFeatureTransformer`` of a regression checkpoint (built as
          ``make_golden.py`` builds it, y encoder and decoder of ``max_num_classes == 0``) on the seeded inputs of
          ``regression_oracle.MODEL_CASES`` -- the logits ``[Q, B]`` and the label token of its embedded input.
``api``   ``api_<case>.npz`` (+ ``api_<case>_m<k>.npz`` for the members' logits of a wide model): the reference
          ``MMPFNRegressor`` (``n_estimators=4``) on a synthetic checkpoint file -- per member the target, the
          preprocessed tables, categorical indices, transformed borders, cancel mask and logits; the ``full``
          output per variant.  Re-runs itself with ``PYTHONHASHSEED=0`` like ``make_api_golden.py``.
``borders`` ``borders.npz``: the reference's ``_transform_borders_one`` on ``regression_oracle.border_transform_cases``.
"""

from __future__ import annotations

import json
import os
import subprocess
import sys
import tempfile
import types
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
REPO = HERE.parent.parent
OUT = HERE / "regression"
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(HERE.parent))
sys.path.insert(0, str(HERE))

import regression_oracle as ro  # noqa: E402


def _import_reference():
    sys.modules.setdefault("seaborn", types.ModuleType("seaborn"))
    sys.path.insert(0, "/root/reference")
    from mmpfn.models.mmpfn.model.bar_distribution import FullSupportBarDistribution
    from mmpfn.models.mmpfn.utils import translate_probs_across_borders

    return FullSupportBarDistribution, translate_probs_across_borders


def reference_head(case: dict) -> dict:
    FullSupportBarDistribution, translate = _import_reference()
    to = torch.from_numpy(case["std_borders"])
    bars = []
    for lg, frm, mask in zip(case["logits"], case["borders"], case["masks"]):
        out = lg.clone()
        if case["temperature"] != 1:
            out = out.float() / case["temperature"]
        if mask is not None:
            out[..., mask] = float("-inf")
        bars.append(translate(out, frm=torch.as_tensor(frm), to=to))
    stacked = torch.stack(bars, dim=0)
    final = stacked.log().mean(dim=0).softmax(dim=-1) if case["avg"] else stacked.mean(dim=0)
    logits = final.log()
    crit = FullSupportBarDistribution(to * ro.HEAD_Y_STD + ro.HEAD_Y_MEAN).float()
    assert np.array_equal(crit.borders.numpy(), case["crit_borders"])
    res = {
        "logits": logits.numpy(),
        "mean": crit.mean(logits).numpy(),
        "mode": crit.mode(logits).numpy(),
        "quantiles": np.stack([crit.icdf(logits, q).numpy() for q in case["levels"]]),
    }
    assert np.isclose(float(np.median(crit.median(logits).numpy() - res["quantiles"][2])), 0.0)
    for k, v in res.items():
        assert not np.isnan(v).any(), (case["name"], case["B"], k)
        assert k == "logits" or np.isfinite(v).all(), (case["name"], case["B"], k)
    assert not np.isposinf(res["logits"]).any()
    assert np.isfinite(res["logits"]).any(axis=-1).all()
    return res


def make_head():
    for B in ro.HEAD_BARS:
        res = {}
        for case in ro.head_cases(B):
            for k, v in reference_head(case).items():
                res[f"{case['name']}_{k}"] = v.astype(np.float32)
        path = OUT / f"head_B{B}.npz"
        np.savez_compressed(path, **res)
        print(f"head B={B}: {len(res) // 4} cases -> {path.name} ({path.stat().st_size / 1e3:.0f} kB)")


def make_model():
    from make_golden import build_reference

    from helpers import oracle_spec, torch_sd
    from multimodalpfn_amd.model.spec import CRITERION_PREFIX, ModelConfig, state_dict_spec

    for case in ro.MODEL_CASES:
        cfg = ModelConfig(**case["cfg"])
        model, ref_spec, _ = build_reference(cfg)
        spec = [s for s in state_dict_spec(cfg) if not s[0].startswith(CRITERION_PREFIX)]
        assert sorted(ref_spec) == sorted(spec), set(ref_spec) ^ set(spec)
        sd = ro.reg_state_dict(cfg, case["wseed"])
        model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items() if not k.startswith(CRITERION_PREFIX)},
                              strict=True)
        model.eval()
        model.cache_trainset_representation = False
        d = ro.model_case_inputs(case)
        taps = {}
        hook = model.transformer_encoder.register_forward_hook(
            lambda _m, args, _kw, out: taps.__setitem__("emb", args[0][0].detach().numpy().copy()), with_kwargs=True)
        torch.manual_seed(0)
        with torch.inference_mode():
            out = model(None, torch.from_numpy(d["x"][:, None, :]) if d["x"] is not None else None,
                        torch.from_numpy(d["image"]) if d["image"] is not None else None,
                        torch.from_numpy(d["y_train"]), only_return_standard_out=True,
                        categorical_inds=list(range(case["data"].get("n_cat", 0))), single_eval_pos=case["N"])
        hook.remove()
        res = {"logits": out.squeeze(1).numpy().astype(np.float32), "y_token": taps["emb"][:, -1].astype(np.float32),
               "meta": np.array(json.dumps(case))}
        assert np.isfinite(res["logits"]).all() and res["logits"].shape == (case["S"] - case["N"], cfg.num_buckets)
        # the restatement agrees before anything is written
        mine = ro.forward_value(oracle_spec(cfg), torch_sd(sd), None if d["x"] is None else torch.from_numpy(d["x"]),
                                None if d["image"] is None else torch.from_numpy(d["image"]),
                                torch.from_numpy(d["y_train"]))
        print(f"  restatement vs reference: {float((mine - out.squeeze(1)).abs().max()):.2e}")
        path = OUT / f"model_{case['name']}.npz"
        np.savez_compressed(path, **res)
        print(f"model {case['name']}: logits {res['logits'].shape} -> {path.name} ({path.stat().st_size / 1e3:.0f} kB)")


def _reference_regressor():
    sys.modules.setdefault("seaborn", types.ModuleType("seaborn"))
    sys.path.insert(0, "/root/reference")
    from sklearn.utils.validation import validate_data

    from mmpfn.models.mmpfn.regressor import MMPFNRegressor
    from mmpfn.models.mmpfn.utils import _fix_dtypes, _transform_borders_one

    MMPFNRegressor._validate_data = lambda self, *a, **k: validate_data(self, *a, **k)
    return MMPFNRegressor, _fix_dtypes, _transform_borders_one


def make_api():
    if os.environ.get("PYTHONHASHSEED") != "0":
        env = dict(os.environ, PYTHONHASHSEED="0")
        rc = subprocess.call([sys.executable, __file__, "api"], env=env)
        if rc:
            sys.exit(rc)
        return
    from api_cases import ckpt_config

    from multimodalpfn_amd.model.spec import ModelConfig

    MMPFNRegressor, fix_dtypes, transform_borders = _reference_regressor()
    with tempfile.TemporaryDirectory() as tmp:
        for case in ro.API_CASES:
            cfg = ModelConfig(num_buckets=case["num_buckets"], **ro.API_MODEL)
            sd = ro.reg_state_dict(cfg, case["wseed"])
            ckpt = Path(tmp) / f"{case['name']}.ckpt"
            config = dict(ckpt_config(cfg), num_buckets=case["num_buckets"], task_type="regression")
            torch.save({"state_dict": {k: torch.from_numpy(v) for k, v in sd.items()}, "config": config}, ckpt)
            d = ro.api_case_data(case)
            res, members = {}, {}
            for vi, variant in enumerate(case["variants"]):
                reg = MMPFNRegressor(model_path=str(ckpt), device="cpu", **ro.api_regressor_kwargs(case, variant))
                reg.fit(d["X_train"], None, d["y_train"])
                captured = []
                orig = reg.executor_.iter_outputs

                def spy(*a, orig=orig, captured=captured, **k):
                    for out, c in orig(*a, **k):
                        captured.append(out.detach().float().numpy().copy())
                        yield out, c

                reg.executor_.iter_outputs = spy
                torch.manual_seed(0)
                full = reg.predict(d["X_test"], None, output_type="full", quantiles=ro.API_QUANTILES)
                tag = variant["tag"]
                res[f"{tag}_logits"] = full["logits"].numpy().astype(np.float32)
                for k in ("mean", "median", "mode"):
                    res[f"{tag}_{k}"] = np.asarray(full[k], np.float32)
                res[f"{tag}_quantiles"] = np.stack(full["quantiles"]).astype(np.float32)
                assert not np.isnan(res[f"{tag}_logits"]).any()
                assert all(np.isfinite(res[f"{tag}_{k}"]).all() for k in ("mean", "median", "mode", "quantiles"))
                if vi:
                    continue  # the members do not depend on the variant
                res["y_train_mean"], res["y_train_std"] = np.float64(reg.y_train_mean_), np.float64(reg.y_train_std_)
                res["std_borders"] = reg.bardist_.borders.numpy()
                res["crit_borders"] = reg.renormalized_criterion_.borders.numpy()
                ex = reg.executor_
                X_enc = reg.preprocessor_.transform(fix_dtypes(d["X_test"], cat_indices=reg.categorical_features_indices))
                std_borders = reg.bardist_.borders.cpu().numpy()
                kinds = []
                for m, c in enumerate(ex.ensemble_configs):
                    members[m] = captured[m].astype(np.float32)
                    res[f"m{m}_y_train"] = np.asarray(ex.y_trains[m], np.float64)
                    res[f"m{m}_X_train"] = np.asarray(ex.X_trains[m], np.float64)
                    res[f"m{m}_X_test"] = np.asarray(ex.preprocessors[m].transform(X_enc).X, np.float64)
                    res[f"m{m}_cat_ix"] = np.asarray(ex.cat_ixs[m], np.int64)
                    res[f"m{m}_feature_shift"] = np.asarray(int(c.feature_shift_count))
                    res[f"m{m}_pp"] = np.asarray(str(c.preprocess_config))
                    if c.target_transform is None:
                        frm, mask = std_borders.copy(), None
                    else:
                        mask, desc, frm = transform_borders(std_borders, target_transform=c.target_transform,
                                                            repair_nan_borders_after_transform=True)
                        assert not desc
                    kinds.append(type(c.target_transform).__name__)
                    res[f"m{m}_borders"] = np.asarray(frm)
                    res[f"m{m}_cancel"] = np.zeros(len(frm) - 1, bool) if mask is None else np.asarray(mask, bool)
                print(f"  target transforms: {kinds}")
            res["meta"] = np.array(json.dumps(case))
            if case["num_buckets"] >= 1000:
                for m, lg in members.items():
                    np.savez_compressed(OUT / f"api_{case['name']}_m{m}.npz", logits=lg)
            else:
                res.update({f"m{m}_logits": lg for m, lg in members.items()})
            path = OUT / f"api_{case['name']}.npz"
            np.savez_compressed(path, **res)
            print(f"api {case['name']}: -> {path.name} ({path.stat().st_size / 1e3:.0f} kB)")


def make_borders():
    _, _, transform_borders = _reference_regressor()
    res = {}
    for name, (t, std) in ro.border_transform_cases().items():
        mask, desc, out = transform_borders(std.copy(), target_transform=t, repair_nan_borders_after_transform=True)
        res[f"{name}_borders"] = np.asarray(out, np.float64)
        res[f"{name}_descending"] = np.asarray(bool(desc))
        res[f"{name}_cancel"] = np.zeros(0, bool) if mask is None else np.asarray(mask, bool)
        print(f"borders {name}: cancelled {0 if mask is None else int(mask.sum())}, descending {bool(desc)}")
    assert res["poles_cancel"][0] and res["poles_cancel"][-1] and bool(res["descending_descending"])
    np.savez_compressed(OUT / "borders.npz", **res)


PARTS = {"head": make_head, "model": make_model, "api": make_api, "borders": make_borders}


def main():
    torch.set_num_threads(ro.FIXTURE_THREADS)
    OUT.mkdir(exist_ok=True)
    for name in sys.argv[1:] or list(PARTS):
        PARTS[name]()


if __name__ == "__main__":
    main()
