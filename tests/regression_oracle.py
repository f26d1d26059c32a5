"""Restatement of the reference's regression path in plain torch (the oracle's counterpart for a real-valued
target; ``oracle.forward.encode_y`` hard-codes class codes, so the value-target pieces live here).

* ``head``: the ensemble post-processing of regressor.py:652-765 -- temperature, cancel mask,
  ``translate_probs_across_borders`` (utils.py:649-700), the members' mean, ``log``, then the renormalised
  criterion's ``mean`` / ``mode`` / ``icdf`` (bar_distribution.py:239-332,588-597) -- with the dtype as a
  parameter: float32 repeats the reference's operations in its order (bit-equal on the CPU), float64 is the
  yardstick of the device kernel.  Three switches turn single steps off for the sensitivity tests.
* ``head_cases``: the seeded inputs of the head-only fixtures (``tests/golden/regression/head_B*.npz`` hold the
  reference's outputs for them).
* ``encode_y_value`` / ``embed_inputs_value`` / ``forward_value``: the forward of a value-target model, composed of
  ``oracle.forward``'s functions with the label token of ``max_num_classes == 0``; ``MODEL_CASES`` and their inputs.
* ``API_CASES`` (the regressor on a synthetic checkpoint file) and ``border_transform_cases`` (the inputs of
  ``_transform_borders_one``), shared by ``make_regression_golden.py`` and the tests.
"""

from __future__ import annotations

import contextlib
import math

import numpy as np
import torch

FIXTURE_THREADS = 8  # make_regression_golden.py ran the reference with torch.set_num_threads(8)


@contextlib.contextmanager
def fixture_threads():
    """torch's float32 matrix-vector product (``probs @ bucket_means``, the criterion's mean) splits its sums by
    the thread count, so a bit-for-bit comparison with the recorded outputs runs under the count they were made
    with (measured at 5000 bars: 2-4e-7 off under 1, 2, 4, 16 or 32 threads, equal under 8)."""
    before = torch.get_num_threads()
    torch.set_num_threads(FIXTURE_THREADS)
    try:
        yield
    finally:
        torch.set_num_threads(before)

# ------------------------------------------------------------------------------------------------ head


def share_of_bucket_left(ys, left, width, *, parenthesised=False):
    """utils.py:669 as written (``ys - left / width``); ``parenthesised`` is what bar_distribution.py:84-86 does."""
    return (ys - left) / width if parenthesised else ys - left / width


def bucket_index(ys: torch.Tensor, borders: torch.Tensor) -> torch.Tensor:
    """utils.py:649-653."""
    ix = torch.searchsorted(borders, ys) - 1
    ix[ys == borders[0]] = 0
    ix[ys == borders[-1]] = len(borders) - 2
    return ix


def member_bars(logits: torch.Tensor, frm: torch.Tensor, to: torch.Tensor, *, parenthesised=False) -> torch.Tensor:
    """``translate_probs_across_borders`` (utils.py:659-700): the weight of softmax(logits) over ``frm``'s buckets
    that falls between consecutive borders of ``to``."""
    ys = to.repeat(logits.shape[:-1] + (1,))
    n_bars = len(frm) - 1
    buckets = bucket_index(ys, frm).clamp(0, n_bars - 1)
    probs = torch.softmax(logits, dim=-1)
    left_of_bucket = (torch.cumsum(probs, dim=-1) - probs).gather(index=buckets, dim=-1)
    widths = frm[1:] - frm[:-1]
    share = share_of_bucket_left(ys, frm[buckets], widths[buckets], parenthesised=parenthesised).clamp(0.0, 1.0)
    left = left_of_bucket + probs.gather(index=buckets, dim=-1) * share
    left[ys <= frm[0]] = 0.0
    left[ys >= frm[-1]] = 1.0
    left = left.clip(0.0, 1.0)
    left[..., 0] = 0.0
    left[..., -1] = 1.0
    return (left[..., 1:] - left[..., :-1]).clamp_min(0.0)


def halfnormal_mean(range_max: torch.Tensor) -> torch.Tensor:
    """Mean of the half-normal with half its weight before ``range_max`` (bar_distribution.py:476-484)."""
    one = torch.ones((), dtype=range_max.dtype)
    s = range_max / torch.distributions.HalfNormal(one).icdf(torch.full((), 0.5, dtype=range_max.dtype))
    return torch.distributions.HalfNormal(s).mean


def criterion_tables(borders: torch.Tensor, *, plain_end_means=False) -> dict:
    widths = borders[1:] - borders[:-1]
    plain = borders[:-1] + widths / 2
    means = plain.clone()
    if not plain_end_means:
        means[0] = -halfnormal_mean(widths[0]) + borders[1]
        means[-1] = halfnormal_mean(widths[-1]) + borders[-2]
    return {"borders": borders, "widths": widths, "mode_means": plain, "bucket_means": means}


def icdf(probs: torch.Tensor, borders: torch.Tensor, level: float) -> torch.Tensor:
    """bar_distribution.py:256-283 on probabilities."""
    cum = torch.cumsum(probs, -1)
    at = level * torch.ones(*cum.shape[:-1], 1, dtype=probs.dtype)
    idx = torch.searchsorted(cum, at).squeeze(-1).clamp(0, cum.shape[-1] - 1)
    cum0 = torch.cat([torch.zeros(*cum.shape[:-1], 1, dtype=probs.dtype), cum], -1)
    rest = level - cum0.gather(-1, idx[..., None]).squeeze(-1)
    left, right = borders[idx], borders[idx + 1]
    return left + (right - left) * rest / probs.gather(-1, idx[..., None]).squeeze(-1)


def head(member_logits, member_borders, std_borders, cancel_masks, *, temperature, average_before_softmax,
         crit_borders, levels, dtype, drop_cancel=False, parenthesised=False, plain_end_means=False) -> dict:
    """``member_logits``: M tensors ``[Q, B]`` (float32); ``member_borders``: M arrays ``[B + 1]`` (float32);
    ``cancel_masks``: M bool arrays ``[B]`` or ``None``; ``std_borders`` / ``crit_borders``: the criterion's borders
    before / after renormalisation (float32).  Everything is cast to ``dtype`` first, so float64 rounds nothing
    but the inputs.  Returns ``logits`` ``[Q, B]``, ``probs`` (their softmax), ``mean`` / ``mode`` ``[Q]`` and
    ``quantiles`` ``[K, Q]``."""
    to = torch.as_tensor(np.asarray(std_borders)).to(dtype)
    bars = []
    for lg, frm, mask in zip(member_logits, member_borders, cancel_masks):
        out = torch.as_tensor(lg).to(dtype)
        if temperature != 1:
            out = out / temperature
        if mask is not None and not drop_cancel:
            out = out.clone()
            out[..., torch.as_tensor(np.asarray(mask, dtype=bool))] = float("-inf")
        bars.append(member_bars(out, torch.as_tensor(np.asarray(frm)).to(dtype), to, parenthesised=parenthesised))
    stacked = torch.stack(bars, dim=0)
    if average_before_softmax:
        final = stacked.log().mean(dim=0).softmax(dim=-1)
    else:
        final = stacked.mean(dim=0)
    logits = final.log()
    crit = criterion_tables(torch.as_tensor(np.asarray(crit_borders)).to(dtype), plain_end_means=plain_end_means)
    probs = torch.softmax(logits, -1)
    density = probs / crit["widths"]
    return {
        "logits": logits,
        "probs": probs,
        "mean": probs @ crit["bucket_means"],
        "mode": crit["mode_means"][density.argmax(-1)],
        "mode_index": density.argmax(-1),
        "quantiles": torch.stack([icdf(probs, crit["borders"], float(q)) for q in levels]),
    }


def final_cdf64(probs64: torch.Tensor, borders64: torch.Tensor, ys: torch.Tensor) -> torch.Tensor:
    """The float64 piecewise-linear CDF of a final distribution ``probs64`` ``[Q, B]`` at ``ys`` ``[..., Q]``."""
    cum0 = torch.cat([torch.zeros(probs64.shape[0], 1, dtype=torch.float64), torch.cumsum(probs64, -1)], -1)
    ys = ys.to(torch.float64)
    B = probs64.shape[-1]
    j = (torch.searchsorted(borders64, ys.contiguous(), right=True) - 1).clamp(0, B - 1)
    rows = torch.arange(probs64.shape[0]).expand_as(j)
    frac = ((ys - borders64[j]) / (borders64[j + 1] - borders64[j])).clamp(0.0, 1.0)
    return cum0[rows, j] + probs64[rows, j] * frac


# ------------------------------------------------------------------------------------------------ head cases

HEAD_BARS = (2, 37, 64, 100, 257, 1023, 5000, 8192)
HEAD_LEVELS = (0.1, 0.25, 0.5, 0.9, 0.99)
HEAD_Y_MEAN, HEAD_Y_STD = 1.0, 2.5
BORDER_KINDS = ("identity", "affine", "warp", "cancel")
ROW_KINDS = ("flat", "peaked", "random")


def normal_borders(B: int) -> np.ndarray:
    """``B + 1`` standard-normal quantiles between the levels 0.0005 and 0.9995 (float32, strictly increasing)."""
    lv = torch.linspace(0.0005, 0.9995, B + 1, dtype=torch.float64)
    b = (math.sqrt(2.0) * torch.erfinv(2 * lv - 1)).to(torch.float32).numpy()
    assert (np.diff(b) > 0).all()
    return b


def member_border_set(kind: str, std: np.ndarray):
    """A member's own borders and cancel mask.  ``affine``: shifted and stretched, so target borders fall outside
    at one end; ``stretch``: stretched about the middle, so every target border lies inside; ``warp``: strongly convex -- left of zero many member borders share one target bucket, right of it
    many target borders share one member bucket; ``cancel``: a mild stretch with the outer bars at both ends
    cancelled (as after a target transform whose inverse is not finite there)."""
    B = std.size - 1
    if kind == "identity":
        return std.copy(), None
    if kind == "affine":
        return (std * np.float32(1.1) + np.float32(0.3)).astype(np.float32), None
    if kind == "stretch":
        mid = (std[0] + std[-1]) / np.float32(2)
        return ((std - mid) * np.float32(1.1) + mid).astype(np.float32), None
    if kind == "warp":
        return np.expm1(np.float32(1.2) * std).astype(np.float32), None
    k = max(1, B // 16)
    mask = np.zeros(B, dtype=bool)
    mask[:k] = True
    mask[-k:] = True
    return (std * np.float32(0.95) + np.float32(0.05)).astype(np.float32), mask


def head_cases(B: int) -> list[dict]:
    """The head-only cases of one bar count: Q in {1, 3} x M in {1, 2, 8} with the members' mean of probabilities,
    and two with ``average_before_softmax``.  Member m of case c takes border kind (m + c) % 4 (no ``cancel`` below
    8 bars, where it would cancel every bar) and row q of it row kind (q + m + c) % 3: flat, peaked (one logit 60
    above the rest) or N(0, 2^2).  Inputs come from the seed alone.

    ``average_before_softmax`` takes the log of every member's bars, so a bar that float32 rounds to zero in one
    member is -inf in the ensemble whatever the others say, and the M-th root makes rounding noise of 1e-7 in one
    member's bar an error of 1e-7^(1/M) in the result: the reference's own float32 output is then noise (a NaN row
    where every bar is hit).  Such rows are kept out of those two cases: no peaked rows and N(0, 0.5^2) instead of
    N(0, 2^2) (every bucket's weight stays far above the rounding of a sum near 1), no cancel mask, no warp, and
    criterion borders shifted to lie left of zero -- with borders on both sides of zero utils.py:669's
    ``ys - left / width`` clamps to 1 on one side and to 0 on the other, and the bar at the switch is the
    difference of two roundings of one sum; and the members' borders cover the criterion's (``stretch``, not
    ``affine``), since a target border beyond a member's last one has the CDF 1 by decree next to a neighbour
    whose CDF is the rounded sum of all weights.  Where two target borders share a member's bucket the bar is an exact
    zero in every precision, and the final logit there is -inf in the fixture, the restatement and the kernel alike."""
    grid = [(Q, M, False) for Q in (1, 3) for M in (1, 2, 8)] + [(3, 2, True), (1, 8, True)]
    cases = []
    for c, (Q, M, avg) in enumerate(grid):
        std = (normal_borders(B) - np.float32(8.0)).astype(np.float32) if avg else normal_borders(B)
        crit = (torch.from_numpy(std) * HEAD_Y_STD + HEAD_Y_MEAN).float().numpy()
        g = torch.Generator().manual_seed(100_000 + 97 * B + c)
        kinds = ("identity", "stretch") if avg else tuple(k for k in BORDER_KINDS if k != "cancel" or B >= 8)
        rows = ("flat", "random") if avg else ROW_KINDS
        logits, borders, masks, names = [], [], [], []
        for m in range(M):
            kind = kinds[(m + c) % len(kinds)]
            frm, mask = member_border_set(kind, std)
            lg = torch.zeros(Q, B)
            for q in range(Q):
                row = rows[(q + m + c) % len(rows)]
                if row == "random":
                    lg[q] = (0.5 if avg else 2.0) * torch.randn(B, generator=g)
                elif row == "peaked":
                    lg[q] = 0.1 * torch.randn(B, generator=g)
                    lo, hi = (B // 16 + 1, B - B // 16 - 2) if B >= 8 else (0, B - 1)  # a bar no mask cancels
                    lg[q, int(torch.randint(lo, max(lo, hi) + 1, (1,), generator=g))] += 60.0
            logits.append(lg)
            borders.append(frm)
            masks.append(mask)
            names.append(kind)
        cases.append({"name": f"c{c}_Q{Q}_M{M}_{'avg' if avg else 'mean'}", "Q": Q, "M": M, "B": B, "avg": avg,
                      "temperature": 0.9 if c % 2 == 0 else 1.0, "logits": logits, "borders": borders,
                      "masks": masks, "kinds": names, "std_borders": std, "crit_borders": crit,
                      "levels": HEAD_LEVELS})
    return cases


def run_head(case: dict, dtype, **switches) -> dict:
    return head(case["logits"], case["borders"], case["std_borders"], case["masks"],
                temperature=case["temperature"], average_before_softmax=case["avg"],
                crit_borders=case["crit_borders"], levels=case["levels"], dtype=dtype, **switches)


# ------------------------------------------------------------------------------------------------ value-target model

from oracle import forward as of  # noqa: E402


def encode_y_value(spec, w: dict, y_train: torch.Tensor, S: int) -> torch.Tensor:
    """The y encoder of a regression model (loading.py:374-398 with ``max_num_classes == 0``): NaN-pad the test
    rows, NaN handling (train mean, indicator -2), Linear(2 -> E) at step 1 -- ``oracle.forward.encode_y`` without
    its class-code step, the target itself being the first input."""
    N = y_train.shape[0]
    y = torch.full((S,), float("nan"), dtype=y_train.dtype)
    y[:N] = y_train
    mean = torch.nanmean(y[:N])
    ind = torch.isnan(y).to(y.dtype) * of.NAN_INDICATOR
    y = torch.where(torch.isnan(y), mean, y)
    feats = torch.stack([y, ind], -1)
    return feats @ w["y_encoder.1.layer.weight"].to(y.dtype).T + w["y_encoder.1.layer.bias"].to(y.dtype)


def embed_inputs_value(spec, w, x, image, y_train, dtype=torch.float32, mixer_tokens=None):
    """``oracle.forward.embed_inputs`` with the value-target label token; every other piece is the oracle's."""
    N = y_train.shape[0]
    S = x.shape[0] if x is not None else image.shape[0]
    parts = []
    if x is not None:
        parts.append(of.encode_x(spec, w, x.to(dtype), N))
    if image is not None:
        if mixer_tokens is None:
            mixer_tokens = of.oracle_mixer(spec, w, image.to(dtype))
        parts.append(mixer_tokens.to(dtype))
    tok = torch.cat(parts, dim=1)
    tok = tok + of.subspace_pos_emb(spec, w, tok.shape[1], dtype).unsqueeze(0)
    X = torch.cat([tok, encode_y_value(spec, w, y_train.to(dtype), S).unsqueeze(1)], dim=1)
    if torch.isnan(X).any():
        raise ValueError("There should be no NaNs in the encoded x and y.")
    return X


@torch.inference_mode()
def forward_value(spec, w, x, image, y_train, *, dtype=torch.float32, taps: dict | None = None) -> torch.Tensor:
    """``oracle.forward.oracle_forward`` for a value target: logits ``[Q, B]``."""
    N = y_train.shape[0]
    X = embed_inputs_value(spec, w, x, image, y_train, dtype)
    if taps is not None:
        taps["embedded_input"] = X.clone()
    for l in range(spec.nlayers):
        X = of.layer_forward(spec, w, l, X, N)
    if taps is not None:
        taps["state"] = X.clone()
    h = torch.nn.functional.gelu(of._linear(X[N:, -1], w, "decoder_dict.standard.0"))
    return of._linear(h, w, "decoder_dict.standard.2")


def reg_state_dict(cfg, wseed: int) -> dict:
    """Synthetic weights of a regression model: ``synth_state_dict`` with the criterion's borders set to normal
    quantiles (a checkpoint's are sorted) and its loss statistics to zero."""
    from synth import synth_state_dict

    from multimodalpfn_amd.model.spec import state_dict_spec

    sd = synth_state_dict(state_dict_spec(cfg), wseed)
    sd["criterion.borders"] = normal_borders(cfg.num_buckets)
    sd["criterion.losses_per_bucket"] = np.zeros(cfg.num_buckets, np.float32)
    return sd


_REG = dict(mgm_heads=2, cap_heads=2, max_num_classes=0, remove_outliers_sigma=None)
MODEL_CASES = [
    dict(name="reg_tab_b100", cfg=dict(nlayers=2, num_buckets=100, **_REG), S=80, N=60, F=7,
         data=dict(n_cat=2, nan_frac=0.05), n_mod=0, wseed=31, dseed=131, nan_labels=3),
    dict(name="reg_img_b5000", cfg=dict(nlayers=1, num_buckets=5000, **_REG), S=77, N=57, F=6, data=dict(),
         n_mod=1, wseed=32, dseed=132, nan_labels=0),
]


def model_case_inputs(case: dict) -> dict:
    """Seeded inputs of a model-level case: table, image, and a standardised real-valued target (``nan_labels`` of
    the train labels NaN)."""
    from synth import synth_image, synth_table

    S, N = case["S"], case["N"]
    g = np.random.default_rng(case["dseed"])
    y = g.standard_normal(S)
    y = ((y - y[:N].mean()) / y[:N].std()).astype(np.float32)
    y_train = y[:N].copy()
    if case["nan_labels"]:
        y_train[g.choice(N, size=case["nan_labels"], replace=False)] = np.nan
    return {
        "x": synth_table(S, case["F"], case["dseed"], **case["data"]) if case["F"] else None,
        "image": synth_image(S, case["n_mod"], case["dseed"]) if case["n_mod"] else None,
        "y_train": y_train,
    }


# ------------------------------------------------------------------------------------------------ API cases

API_MODEL = dict(nlayers=1, **_REG)
API_CASES = [
    dict(name="b100", num_buckets=100, N=64, Q=24, F=5, seed=141, wseed=41,
         variants=[dict(tag="mean", average_before_softmax=False), dict(tag="avg", average_before_softmax=True)]),
    dict(name="b5000", num_buckets=5000, N=60, Q=20, F=4, seed=142, wseed=42,
         variants=[dict(tag="mean", average_before_softmax=False)]),
]
API_QUANTILES = [0.1, 0.5, 0.9]


def api_case_data(case: dict) -> dict:
    """Seeded table and a target that depends on it (plus noise), train and test rows."""
    from synth import synth_table

    n = case["N"] + case["Q"]
    X = synth_table(n, case["F"], case["seed"], n_cat=1).astype(np.float64)
    g = np.random.default_rng(case["seed"])
    y = 3.0 + 2.0 * np.nan_to_num(X[:, -1]) - 1.5 * np.nan_to_num(X[:, -2]) ** 2 + 0.5 * g.standard_normal(n)
    N = case["N"]
    return {"X_train": X[:N], "X_test": X[N:], "y_train": y[:N], "y_test": y[N:]}


def api_regressor_kwargs(case: dict, variant: dict) -> dict:
    return dict(mixer_type="MGM+CAP", mgm_heads=2, cap_heads=2, features_per_group=2, n_estimators=4,
                softmax_temperature=0.9, average_before_softmax=variant["average_before_softmax"], random_state=7,
                inference_precision=torch.float32, ignore_pretraining_limits=True)


# ------------------------------------------------------------------------------------------------ border transforms


class PoleTransform:
    """A target transform whose inverse is not finite at both ends (|t| >= 2.5) and beyond the limits near them:
    the cancel-mask branch of utils.py:771-782."""

    def inverse_transform(self, t):
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(np.abs(t) >= 2.5, np.nan, t / (2.5 - np.abs(t)) * 200.0)


class NegateTransform:
    """An inverse that reverses the order: the descending branch of utils.py:786-792."""

    def inverse_transform(self, t):
        return -2.0 * t + 1.0


def border_transform_cases(B: int = 100, n_train: int = 80, seed: int = 151) -> dict:
    """name -> (fitted transform, standard borders): every default target transform of the regressor
    (``safepower``) and the other two it offers (``power``, ``quantile_norm``), fitted on a seeded skewed target;
    a transform with poles at both ends; a reversing one."""
    from multimodalpfn_amd.model.preprocessing import ReshapeFeatureDistributionsStep

    g = np.random.default_rng(seed)
    y = np.exp(0.8 * g.standard_normal(n_train)) - 0.5
    y = (y - y.mean()) / y.std()
    known = ReshapeFeatureDistributionsStep.get_all_preprocessors(num_examples=n_train, random_state=seed)
    std = normal_borders(B).astype(np.float64)
    cases = {}
    for name in ("safepower", "power", "quantile_norm"):
        t = known[name]
        t.fit_transform(y.reshape(-1, 1))
        cases[name] = (t, std)
    cases["poles"] = (PoleTransform(), std)
    cases["descending"] = (NegateTransform(), std)
    return cases
