"""Generate the encoder edge fixtures by running the REFERENCE model (build container only).

Run from the repo root:   python tests/golden/make_encoder_golden.py [case ...]

Same recipe as ``make_golden.py`` (whose ``build_reference`` it uses): the reference
``PerFeatureTransformer`` with the synthetic weights of ``synth.py``, the 12-sigma outlier
step enabled like ``MMPFNClassifier.fit`` does (unless a case says otherwise), called like the
inference engine calls it.  Every case is a small tabular-only table (one layer, F <= 6) built
around one edge of the input encoders: columns constant on the train rows, NaN / inf
placement, values far outside the soft-clip bounds, label gaps and NaN labels, one train row.

Each ``tests/golden/encoder/<case>.npz`` holds ``x``, ``y_train``, ``meta`` (cfg overrides,
weight seed, N, ``expect_raise``) and -- unless the reference raises its "no NaNs in the encoded
x and y" ``ValueError`` -- the reference's ``embedded_input`` (the argument of
``transformer_encoder``) and ``logits``.  The sub-directory keeps the files out of
``helpers.CASES``.

Two notes on sizes.  ``ynan_frac`` needs N >= 100 for its label mean, so it is the one case
above 40 rows (F = 2 keeps it at two tokens per row).  At N <= 40 no single train value lies
more than (N - 1) / sqrt(N) < 12 standard deviations from the train mean, so the first pass
of the two-pass bounds removes nothing in ``outliers``: both passes run and give the bounds
both log branches are then hit against (asserted below); the first pass removing a value is
covered by the row-count tests of ``tests/test_encoder_gpu.py`` (N >= 204 with a 1e4 outlier).
"""

from __future__ import annotations

import json
import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
REPO = HERE.parent.parent
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(HERE))

from make_golden import build_reference  # noqa: E402
from synth import synth_labels, synth_state_dict  # noqa: E402

from multimodalpfn_amd.model.spec import ModelConfig, state_dict_spec  # noqa: E402

OUT = HERE / "encoder"
BASE_CFG = dict(nlayers=1, mgm_heads=2, cap_heads=2)
WSEED = 21  # one set of weights: cases of one cfg share an engine (a raise case is followed by a clean one on it)
NAN, INF = np.float32("nan"), np.float32("inf")


def _table(S, F, seed):
    return np.random.default_rng(seed).standard_normal((S, F)).astype(np.float32)


def _train_const():
    x = _table(40, 4, 201)
    x[:30, 1] = 1.5  # constant on the train rows, varying on the test rows
    return dict(x=x, y=synth_labels(40, 3, 201)[:30])


def _group_all_const():
    x = _table(40, 4, 202)
    x[:, 2], x[:, 3] = 0.5, -2.0  # group 1: both columns constant
    return dict(x=x, y=synth_labels(40, 3, 202)[:30])


def _odd_F():
    return dict(x=_table(40, 5, 203), y=synth_labels(40, 4, 203)[:30])


def _nan_mix():
    S, N = 40, 30
    x = _table(S, 6, 204)
    x[0, 0] = NAN  # row 0 is the row the constancy tests compare against
    x[N:, 1] = NAN  # NaN on every test row
    x[:N, 2] = NAN
    x[3, 2], x[17, 2] = 0.75, -1.25  # two valid train values
    x[S - 1, 3], x[S - 2, 3] = INF, -INF
    return dict(x=x, y=synth_labels(S, 3, 204)[:N])


def _one_valid():
    x = _table(40, 4, 205)
    x[:30, 1] = NAN
    x[11, 1] = 0.6  # one non-NaN train value
    return dict(x=x, y=synth_labels(40, 2, 205)[:30])


def _outliers():
    S, N = 40, 30
    x = _table(S, 4, 206)
    x[2, 1], x[9, 1], x[20, 1] = 1e4, -1e6, 3e3
    for c in (1, 2):  # column 2: benign train rows, so both bounds are O(12) and both branches apply
        x[N, c], x[N + 1, c], x[N + 2, c] = 5e5, -7e4, 1e30
    t = x[:N, 2].astype(np.float64)
    lo, hi = t.mean() - 12 * t.std(ddof=1), t.mean() + 12 * t.std(ddof=1)
    assert x[N, 2] > hi and x[N + 2, 2] > hi and x[N + 1, 2] < lo  # upper and lower log branch
    return dict(x=x, y=synth_labels(S, 3, 206)[:N])


def _fpg1():
    return dict(x=_table(36, 3, 207), y=synth_labels(36, 2, 207)[:27],
                cfg=dict(features_per_group=1, model_seed=7))


def _ynan():
    y = synth_labels(40, 4, 208)[:30]
    y[13] = NAN
    return dict(x=_table(40, 4, 208), y=y)


def _ygap():
    k = synth_labels(40, 4, 209)[:30]
    return dict(x=_table(40, 4, 209), y=(2.5 * k + 1).astype(np.float32))


def _ynan_frac():
    """Fractional labels with one NaN whose float32 ``np.nanmean`` is below the float32 rounding of their
    float64 mean: a host that fills with the former and a device that fills with the latter disagree on the
    class code of every NaN-label row (the filled value counts the host's mean as a smaller class)."""
    S, N = 104, 100
    vals = np.array([0.1, 0.7, 1.3, 2.9], dtype=np.float32)
    for seed in range(1000):
        y = vals[np.random.default_rng(seed).integers(0, 4, size=N)]
        y[:4] = vals
        y[57] = NAN
        host = np.float32(np.nanmean(y))
        ok = ~np.isnan(y)
        dev = np.float32(y[ok].astype(np.float64).sum() / ok.sum())
        if host < dev:
            break
    else:
        raise AssertionError("no seed gives nanmean32 < mean64")
    uniq_host = np.unique(np.where(np.isnan(y), host, y))
    assert (dev > uniq_host).sum() == (dev > np.unique(np.where(np.isnan(y), dev, y))).sum() + 1  # the off-by-one
    return dict(x=_table(S, 2, 210), y=y, note=f"label seed {seed}")


def _n1():
    return dict(x=_table(10, 4, 211), y=np.array([1.0], dtype=np.float32), expect_raise=True)


def _inf_train():
    x = _table(40, 4, 212)
    x[5, 2] = INF
    return dict(x=x, y=synth_labels(40, 3, 212)[:30], expect_raise=True)


def _n1_no_outlier():
    return dict(x=_table(10, 4, 213), y=np.array([1.0], dtype=np.float32), cfg=dict(remove_outliers_sigma=None),
                outliers=False, expect_raise=None)  # None: record whichever the reference does


CASES = {
    "train_const": _train_const, "group_all_const": _group_all_const, "odd_F": _odd_F, "nan_mix": _nan_mix,
    "one_valid": _one_valid, "outliers": _outliers, "fpg1": _fpg1, "ynan": _ynan, "ygap": _ygap,
    "ynan_frac": _ynan_frac, "n1": _n1, "inf_train": _inf_train, "n1_no_outlier": _n1_no_outlier,
}


def run_case(name: str) -> dict:
    case = CASES[name]()
    cfg_over = BASE_CFG | case.get("cfg", {})
    cfg = ModelConfig(**cfg_over)
    wseed = WSEED
    model, ref_spec, update_outliers = build_reference(cfg)
    spec = state_dict_spec(cfg)
    assert sorted(ref_spec) == sorted(spec), (set(ref_spec) ^ set(spec))
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synth_state_dict(spec, wseed).items()}, strict=True)
    model.eval()
    if case.get("outliers", True):
        update_outliers(model=model, remove_outliers_std=12.0, seed=cfg.model_seed, inplace=True)
    model.cache_trainset_representation = False

    x, y = case["x"], case["y"]
    N = len(y)
    taps = {}

    def enc_hook(_m, args, _kw, out):
        taps["embedded_input"] = args[0][0].detach().numpy().astype(np.float32)

    hook = model.transformer_encoder.register_forward_hook(enc_hook, with_kwargs=True)
    raised = None
    torch.manual_seed(0)
    try:
        with torch.inference_mode():
            out = model(None, torch.from_numpy(x[:, None, :]), None, torch.from_numpy(y),
                        only_return_standard_out=True, categorical_inds=[], single_eval_pos=N)
    except ValueError as e:
        raised = str(e)
        assert "no NaNs in the encoded x and y" in raised, raised
    hook.remove()
    expect = case.get("expect_raise", False)
    if expect is not None:
        assert (raised is not None) == expect, (name, raised)
    meta = dict(name=name, cfg=cfg_over, wseed=wseed, N=N, expect_raise=raised is not None)
    if "note" in case:
        meta["note"] = case["note"]
    res = {"x": x, "y_train": y, "meta": np.array(json.dumps(meta))}
    if raised is None:
        res["embedded_input"] = taps["embedded_input"]
        res["logits"] = out.squeeze(1).numpy().astype(np.float32)
    return res


def main():
    torch.set_num_threads(4)
    OUT.mkdir(exist_ok=True)
    only = set(sys.argv[1:])
    for name in CASES:
        if only and name not in only:
            continue
        res = run_case(name)
        path = OUT / f"{name}.npz"
        np.savez_compressed(path, **res)
        what = "raises" if "logits" not in res else f"logits {res['logits'].shape}"
        print(f"{name}: {what} -> {path.name} ({path.stat().st_size / 1e3:.0f} kB)")


if __name__ == "__main__":
    main()
