"""Seeded inputs of the bar-distribution scoring fixtures (``tests/golden/bar_score/score_B*.npz`` hold the
reference's float32 outputs for them, written by ``tests/golden/make_bar_score_golden.py``) and the restatement of
the scoring -- ``FullSupportBarDistribution``'s ``forward`` / ``cdf`` / ``pi`` / ``ei`` / ``mean_of_square``
(bar_distribution.py:59-97,487-571,600-758) in plain torch with the dtype as a parameter: float32 repeats the
reference's operations in its order (bit-equal on the CPU under ``regression_oracle.fixture_threads``), float64 is the
yardstick of ``mmpfn_bar_score``.  Switches make single plausible mistakes for the sensitivity test.
"""

from __future__ import annotations

import numpy as np
import torch

import regression_oracle as ro

BARS = (2, 3, 37, 256, 257, 1024, 1025, 2048, 2049, 5000, 5120, 5121, 8192)
ROWS = ("flat", "peaked", "random")
SHIFT = 1000.0  # the expected improvement's conditioning case: borders far from zero
ZERO_WIDTH_B, ZERO_WIDTH_AT = 37, 20  # one case with borders[20] == borders[21]
N_TARGETS = 9  # column 0 is the NaN target
PER_TARGET = ("nll", "cdf", "pi", "ei")
SAMPLE_SEED, SAMPLE_T = 1234, 0.8


def cases(B: int) -> list[dict]:
    """Per bar count: ``base`` (borders ``normal_borders(B) * 2.5 + 1``, temperature 1), ``shifted`` (the same
    borders + 1000, temperature 0.9) and at 37 bars ``zero_width`` (one empty interior bucket).  Three rows each:
    flat; peaked (+60 on one bar); N(0, 2^2) with a run of -inf logits (none at 2 bars).  Nine targets per row: NaN,
    below the first border, on it, inside the first bucket, on the second border, on an interior border (in the
    third row: inside a -inf bar instead, where the row has one), the middle of the row's largest bar, inside the
    last bucket, above the last border."""
    base = (torch.from_numpy(ro.normal_borders(B)) * 2.5 + 1.0).float().numpy()
    variants = [("base", base, 1.0), ("shifted", (base + np.float32(SHIFT)).astype(np.float32), 0.9)]
    if B == ZERO_WIDTH_B:
        zw = base.copy()
        zw[ZERO_WIDTH_AT + 1] = zw[ZERO_WIDTH_AT]
        variants.append(("zero_width", zw, 1.0))
    out = []
    for v, (name, borders, temperature) in enumerate(variants):
        widths = np.diff(borders)
        assert (widths >= 0).all() and widths[0] > 0 and widths[-1] > 0
        g = torch.Generator().manual_seed(200_000 + 97 * B + v)
        logits = torch.zeros(len(ROWS), B)
        logits[1] = 0.1 * torch.randn(B, generator=g)
        peak = int(torch.randint(1, B - 1, (1,), generator=g)) if B >= 3 else 1
        if name == "zero_width" and peak == ZERO_WIDTH_AT:
            peak += 2
        logits[1, peak] += 60.0
        logits[2] = 2.0 * torch.randn(B, generator=g)
        dead = list(range(max(1, B // 3), max(1, B // 3) + max(1, B // 16))) if B >= 3 else []
        logits[2, dead] = float("-inf")
        ys = np.zeros((len(ROWS), N_TARGETS), np.float32)
        for r in range(len(ROWS)):
            top = int(torch.argmax(logits[r]))
            assert widths[top] > 0
            on_inner = borders[B // 2]
            if r == 2 and dead:
                on_inner = borders[dead[0]] + np.float32(0.5) * widths[dead[0]]
            ys[r] = [np.nan, borders[0] - np.float32(0.5) * widths[0], borders[0],
                     borders[0] + np.float32(0.25) * widths[0], borders[1], on_inner,
                     borders[top] + np.float32(0.5) * widths[top], borders[-2] + np.float32(0.7) * widths[-1],
                     borders[-1] + np.float32(0.3) * widths[-1]]
        assert not (name == "zero_width" and np.isin(ys[:, 1:], borders[ZERO_WIDTH_AT]).any())
        out.append({"name": name, "B": B, "borders": borders, "temperature": temperature, "logits": logits,
                    "ys": torch.from_numpy(ys), "dead": dead})
    return out


# ------------------------------------------------------------------------------------------------ restatement


def _side_normals(borders):
    widths = borders[1:] - borders[:-1]
    half = torch.distributions.HalfNormal(torch.ones((), dtype=borders.dtype)).icdf(
        torch.full((), 0.5, dtype=borders.dtype))
    return torch.distributions.HalfNormal(widths[0] / half), torch.distributions.HalfNormal(widths[-1] / half)


def bucket_of(borders, y, *, right_side=False):
    """bar_distribution.py:156-162; ``right_side``: the mistake of taking a target on a border into the bucket to
    its right."""
    idx = torch.searchsorted(borders, y, right=right_side) - 1
    idx[y == borders[0]] = 0
    idx[y == borders[-1]] = len(borders) - 2
    return idx


def nll(logits, borders, y, *, right_side=False, plain_ends=False):
    """``forward`` (:487-571) with ``ignore_nan_targets``; ``plain_ends``: no half-normal term in the end buckets."""
    B = len(borders) - 1
    widths = borders[1:] - borders[:-1]
    y = y.clone().view(*logits.shape[:-1])
    ignored = torch.isnan(y)
    y[ignored] = borders[0]
    idx = bucket_of(borders, y, right_side=right_side).clamp_(0, B - 1)
    scaled = torch.log_softmax(logits, -1) - torch.log(widths)
    lp = scaled.gather(-1, idx.unsqueeze(-1)).squeeze(-1)
    first, last = _side_normals(borders)
    if not plain_ends:
        lp[idx == 0] += first.log_prob((borders[1] - y[idx == 0]).clamp(min=0.00000001)) + torch.log(widths[0])
        lp[idx == B - 1] += last.log_prob((y[idx == B - 1] - borders[-2]).clamp(min=0.00000001)) + torch.log(widths[-1])
    out = -lp
    out[ignored] = 0.0
    return out


def cdf(logits, borders, ys, *, right_side=False):
    """:59-97 (no NaN targets)."""
    B = len(borders) - 1
    widths = borders[1:] - borders[:-1]
    probs = torch.softmax(logits, dim=-1)
    idx = bucket_of(borders, ys, right_side=right_side).clamp(0, B - 1)
    left_of_bucket = (torch.cumsum(probs, dim=-1) - probs).gather(-1, idx)
    share = ((ys - borders[idx]) / widths[idx]).clamp(0.0, 1.0)
    out = left_of_bucket + probs.gather(-1, idx) * share
    out[ys <= borders[0]] = 0.0
    out[ys >= borders[-1]] = 1.0
    return out.clip(0.0, 1.0)


def _positions(borders, best_f):
    return -(best_f - borders[1]).clamp(max=0.0), (best_f - borders[-2]).clamp(min=0.0)


def pi(logits, borders, best_f, *, linear_ends=False):
    """:629-675, ``best_f`` one per row; ``linear_ends``: the end buckets as ``cdf`` has them."""
    p = torch.softmax(logits, -1)
    widths = borders[1:] - borders[:-1]
    factor = 1.0 - ((best_f[..., None] - borders[:-1]) / widths).clamp(0.0, 1.0)
    if not linear_ends:
        first, last = _side_normals(borders)
        pos0, posl = _positions(borders, best_f)
        factor[..., 0] = 0.0
        factor[..., 0][pos0 > 0.0] = first.cdf(pos0[pos0 > 0.0])
        factor[..., -1] = 1.0
        factor[..., -1][posl > 0.0] = 1.0 - last.cdf(posl[posl > 0.0])
    return (p * factor).sum(-1)


def _ei_halfnormal(scale, best_f):
    """:677-703."""
    u = (torch.tensor(0.0) - best_f) / scale
    normal = torch.distributions.Normal(torch.zeros_like(u), torch.ones_like(u))
    ucdf = normal.cdf(u)
    updf = torch.exp(normal.log_prob(u))
    return 2 * (scale * (updf + u * ucdf))


def ei(logits, borders, best_f, *, drop_partial=False, zero_width_limit=False):
    """:706-758.  ``drop_partial``: the bucket that holds ``best_f`` contributes nothing (its ``(r - f)^2 / (2 w)``
    dropped).  ``zero_width_limit``: an empty bucket contributes its limit ``max(r - f, 0)`` -- the reference
    divides 0 by 0 there, so its expected improvement is NaN for every row once one interior bucket is empty."""
    left, right = borders[:-1], borders[1:]
    per_bar = best_f[..., None].repeat(*[1] * len(best_f.shape), logits.shape[-1])
    inside = per_bar.clamp(left, right)
    contrib = ((right ** 2 - inside ** 2) / 2 - per_bar * (right - inside)) / (right - left)
    if drop_partial:
        contrib = torch.where((per_bar > left) & (per_bar < right), torch.zeros_like(contrib), contrib)
    if zero_width_limit:
        contrib = torch.where((right == left).expand_as(contrib), (right - per_bar).clamp(min=0.0), contrib)
    first, last = _side_normals(borders)
    pos0, posl = _positions(borders, best_f)
    contrib[..., -1] = _ei_halfnormal(last.scale, posl)
    contrib[..., 0] = _ei_halfnormal(first.scale, torch.zeros_like(pos0)) - _ei_halfnormal(first.scale, pos0)
    p = torch.softmax(logits, -1)
    return torch.einsum("...b,...b->...", p, contrib)


def bucket_mean_squares(borders, *, mean_in_last=False):
    """:606-624; ``mean_in_last``: the last bucket with the half-normal's mean where the reference has its variance."""
    left, right = borders[:-1], borders[1:]
    sq = (left.square() + right.square() + left * right) / 3.0
    first, last = _side_normals(borders)
    sq[0] = first.variance + (-first.mean + borders[1]).square()
    sq[-1] = last.variance + ((last.mean if mean_in_last else last.variance) + borders[-2]).square()
    return sq


def score(case: dict, dtype, *, right_side=False, plain_end_nll=False, linear_end_pi=False, drop_partial_ei=False,
          mean_in_last_square=False, zero_width_limit=False) -> dict:
    """Every kind of one case: ``nll`` ``[3, 9]`` (0 at the NaN target); ``cdf`` / ``pi`` / ``ei`` ``[3, 8]`` for the
    targets after the NaN one (the reference's ``cdf`` asserts on a NaN and its ``pi`` / ``ei`` have no rule for
    one); ``mean_of_square`` ``[3]``.  Inputs are cast to ``dtype`` first, so float64 rounds nothing but them."""
    borders = torch.from_numpy(case["borders"]).to(dtype)
    logits = case["logits"].to(dtype)
    if case["temperature"] != 1:
        logits = logits / case["temperature"]
    ys = case["ys"].to(dtype)
    real = ys[:, 1:].contiguous()
    cols = range(real.shape[1])
    return {
        "nll": torch.stack([nll(logits, borders, ys[:, j], right_side=right_side, plain_ends=plain_end_nll)
                            for j in range(ys.shape[1])], -1),
        "cdf": cdf(logits, borders, real, right_side=right_side),
        "pi": torch.stack([pi(logits, borders, real[:, j].contiguous(), linear_ends=linear_end_pi) for j in cols], -1),
        "ei": torch.stack([ei(logits, borders, real[:, j].contiguous(), drop_partial=drop_partial_ei,
                              zero_width_limit=zero_width_limit) for j in cols], -1),
        "mean_of_square": torch.softmax(logits, -1) @ bucket_mean_squares(borders, mean_in_last=mean_in_last_square),
    }


def natural_unit(kind: str, case: dict, ref64: torch.Tensor) -> torch.Tensor | float:
    """What a deviation of ``kind`` is measured in (test_bar_score_gpu): probabilities absolute; an nll relative to
    ``max(1, |ref|)``; the expected improvement as a fraction of the span of the criterion's inner borders (the
    whole span up to 2 bars), as the mean is; the mean of squares as a fraction of the largest squared border."""
    b = case["borders"].astype(np.float64)
    if kind == "nll":
        return ref64.abs().clamp(min=1.0)
    if kind == "ei":
        return float(b[-2] - b[1]) if case["B"] > 2 else float(b[-1] - b[0])
    if kind == "mean_of_square":
        return float((b ** 2).max())
    return 1.0


def deviation(kind: str, case: dict, values: torch.Tensor, ref64: torch.Tensor) -> float:
    """The largest ``|values - ref64|`` in the kind's natural unit over the elements where float64 is finite; NaN
    ``values`` throughout (the reference's ``ei`` with an empty bucket) count as 0."""
    if torch.isnan(values).all():
        return 0.0
    fin = torch.isfinite(ref64)
    unit = natural_unit(kind, case, ref64)
    unit = unit[fin] if torch.is_tensor(unit) else unit
    return float(((values.double() - ref64)[fin].abs() / unit).max())
