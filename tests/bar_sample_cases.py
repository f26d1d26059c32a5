"""Helpers of the sampling tests (``mmpfn_bar_sample``): the generator of the levels restated in numpy, the draw from
a level restated in torch with the dtype as a parameter (built from the reference's operations: ``softmax``,
``cumsum``, ``searchsorted`` on the left side, ``torch.erfinv`` and the half-normal's scale from
``HalfNormal(1).icdf(0.5)``), the supplied levels of the cases, and the measure of a draw in probability space.
The inputs are ``bar_score_cases.cases(B)``.  Switches make single plausible mistakes for the sensitivity test.
"""

from __future__ import annotations

import numpy as np
import torch

import bar_score_cases as bc

LEVEL_MIN, LEVEL_MAX = 2.0 ** -24, 1.0 - 2.0 ** -24  # both exact in float32
N_LEVELS = 256
TAILS = ("linear", "halfnormal")
MISTAKES = ("exclusive_sums", "no_division", "temperature_ignored")

# ------------------------------------------------------------------------------------------------ the generator

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = np.uint32(0x9E3779B9), np.uint32(0xBB67AE85)
_LO = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key) -> np.ndarray:
    """Philox4x32-10 (Salmon, Moraes, Dror, Shaw, SC'11): ``counter`` ``[..., 4]`` and ``key`` ``[..., 2]`` uint32 ->
    the four output words ``[..., 4]`` in Random123's order."""
    c = np.array(counter, dtype=np.uint32)
    k = np.broadcast_to(np.array(key, dtype=np.uint32), c.shape[:-1] + (2,)).copy()
    for r in range(10):
        if r:
            k[..., 0] += _W0
            k[..., 1] += _W1
        p0 = _M0 * c[..., 0].astype(np.uint64)
        p1 = _M1 * c[..., 2].astype(np.uint64)
        hi0, lo0 = (p0 >> np.uint64(32)).astype(np.uint32), (p0 & _LO).astype(np.uint32)
        hi1, lo1 = (p1 >> np.uint64(32)).astype(np.uint32), (p1 & _LO).astype(np.uint32)
        c = np.stack([hi1 ^ c[..., 1] ^ k[..., 0], lo1, hi0 ^ c[..., 3] ^ k[..., 1], lo0], -1)
    return c


def level_of_word(x) -> np.ndarray:
    """``u = (2 (x >> 9) + 1) 2^-24``: an odd multiple of 2^-24, exact in float32, inside [2^-24, 1 - 2^-24]."""
    m = (np.asarray(x, dtype=np.uint32) >> np.uint32(9)).astype(np.float64)
    return ((2.0 * m + 1.0) * 2.0 ** -24).astype(np.float32)


def levels(seed: int, Q: int, first_draw: int, n: int) -> np.ndarray:
    """The levels ``[Q, n]`` of draws ``first_draw .. first_draw + n`` of rows ``0 .. Q``: word ``J & 3`` of the block
    at counter ``(lo32(J >> 2), hi32(J >> 2), q, 0)`` under the key ``(lo32(seed), hi32(seed))``."""
    J = (np.uint64(first_draw) + np.arange(n, dtype=np.uint64))[None, :].repeat(Q, 0)
    blk = J >> np.uint64(2)
    q = np.arange(Q, dtype=np.uint32)[:, None].repeat(n, 1)
    counter = np.stack([(blk & _LO).astype(np.uint32), (blk >> np.uint64(32)).astype(np.uint32), q,
                        np.zeros_like(q)], -1)
    key = [np.uint32(seed & 0xFFFFFFFF), np.uint32((seed >> 32) & 0xFFFFFFFF)]
    words = philox4x32_10(counter, key)
    pick = np.take_along_axis(words, (J & np.uint64(3)).astype(np.int64)[..., None], -1)[..., 0]
    return level_of_word(pick)


def supplied_levels(case: dict, v: int) -> torch.Tensor:
    """The levels ``[3, 256]`` of case ``v`` of its bar count: both ends of the range, the median, then odd multiples
    of 2^-24 from a seeded generator."""
    rng = np.random.default_rng(300_000 + 97 * case["B"] + v)
    u = (2.0 * rng.integers(0, 2 ** 23, size=(len(bc.ROWS), N_LEVELS)) + 1.0) * 2.0 ** -24
    u[:, 0], u[:, 1], u[:, 2] = LEVEL_MIN, LEVEL_MAX, 0.5
    u32 = u.astype(np.float32)
    assert (u32.astype(np.float64) == u).all()
    return torch.from_numpy(u32)


# ------------------------------------------------------------------------------------------------ the draw


def _halfnormal_scales(borders):
    """The scales of the first and the last bucket's half-normals (bar_distribution.py:476-484)."""
    half = torch.distributions.HalfNormal(torch.ones((), dtype=borders.dtype)).icdf(
        torch.full((), 0.5, dtype=borders.dtype))
    return (borders[1] - borders[0]) / half, (borders[-1] - borders[-2]) / half


def draw(logits, borders, u, tails, dtype, *, temperature=1.0, clamps=True, mistake=None, with_acts=False):
    """Draws ``[R, n]`` at the levels ``u`` ``[R, n]`` from the rows ``logits`` ``[R, B]`` at the sampling
    ``temperature``, everything cast to ``dtype`` first.  ``clamps=False``, linear: the reference's ``icdf`` at a
    level per draw in its own order of operations.  ``clamps``: the level is kept at or below the row's rounded
    total and the share of the bar inside [0, 1]; where neither acts the reference's expression stands.
    ``tails="halfnormal"``: the two end buckets follow their half-normals.  ``mistake``: one of ``MISTAKES``.
    ``with_acts``: also where a clamp changed a value."""
    assert tails in TAILS and mistake in (None,) + MISTAKES
    borders = torch.as_tensor(borders).to(dtype)
    logits = logits.to(dtype)
    u = u.to(dtype)
    B = logits.shape[-1]
    if temperature != 1 and mistake != "temperature_ignored":
        logits = logits / temperature
    probs = logits.softmax(-1)
    cum = torch.cumsum(probs, -1)
    lv = torch.minimum(u, cum[..., -1:]) if clamps else u
    searched = cum - probs if mistake == "exclusive_sums" else cum
    idx = torch.searchsorted(searched, lv).clamp(0, B - 1)
    cum0 = torch.cat([torch.zeros(*cum.shape[:-1], 1, dtype=dtype), cum], -1)
    rest = lv - cum0.gather(-1, idx)
    p = probs.gather(-1, idx)
    left, right = borders[idx], borders[idx + 1]
    y = left + (right - left) * rest if mistake == "no_division" else left + (right - left) * rest / p
    share = rest if mistake == "no_division" else rest / p
    acts = torch.zeros_like(idx, dtype=torch.bool)
    if clamps:
        acts = (lv != u) | ~((share >= 0) & (share <= 1))
        share = torch.nan_to_num(share, nan=0.0).clamp(0.0, 1.0)  # fmin(fmax(NaN, 0), 1) = 0
        y = torch.where(acts, left + (right - left) * share, y)
    if tails == "halfnormal":
        s_first, s_last = _halfnormal_scales(borders)
        top = torch.full((), LEVEL_MAX, dtype=dtype)
        root2 = torch.sqrt(torch.full((), 2.0, dtype=dtype))
        sh = share if clamps else rest / p
        y_last = borders[B - 1] + s_last * root2 * torch.erfinv(torch.minimum(sh, top))
        y_first = borders[1] - s_first * root2 * torch.erfinv(torch.minimum(1.0 - sh, top))
        y = torch.where(idx == B - 1, y_last, torch.where(idx == 0, y_first, y))
    return (y, acts) if with_acts else y


# ------------------------------------------------------------------------------------------------ the measure


def prob_error(case: dict, y: torch.Tensor, u: torch.Tensor, tails: str) -> torch.Tensor:
    """Per draw, the distance of its level ``u`` from ``[F64(y-), F64(y)]``: ``F64`` is the float64 CDF of the
    case's row at the sampling temperature, piecewise linear between the borders, with the half-normals in the two
    end buckets when ``tails="halfnormal"``.  The interval is a point except on a doubled border, where it spans the
    empty bucket's weight.  NaN where ``y`` is NaN."""
    assert tails in TAILS
    b = torch.from_numpy(case["borders"]).double()
    B = case["B"]
    probs = (case["logits"].double() / case["temperature"]).softmax(-1)
    cum = torch.cumsum(probs, -1)
    cum0 = torch.cat([torch.zeros(len(probs), 1, dtype=torch.float64), cum], -1)
    y = y.double()
    yy = torch.nan_to_num(y, nan=0.0)
    widths = b[1:] - b[:-1]

    def linear(right_side: bool) -> torch.Tensor:
        j = (torch.searchsorted(b, yy, right=right_side) - 1).clamp(0, B - 1)
        w = widths[j]
        share = torch.where(w > 0, (yy - b[j]) / torch.where(w > 0, w, torch.ones_like(w)),
                            torch.full_like(yy, 1.0 if not right_side else 0.0)).clamp(0.0, 1.0)
        return cum0.gather(-1, j) + probs.gather(-1, j) * share

    lo, hi = linear(False), linear(True)
    if tails == "halfnormal":
        half = torch.distributions.HalfNormal(torch.ones((), dtype=torch.float64)).icdf(
            torch.full((), 0.5, dtype=torch.float64))
        s0, sl = widths[0] / half, widths[-1] / half
        root2 = 2.0 ** 0.5
        first = probs[:, :1] * torch.special.erfc((b[1] - yy).clamp(min=0.0) / (s0 * root2))
        last = cum0[:, B - 1:B] + probs[:, B - 1:B] * torch.erf((yy - b[B - 1]).clamp(min=0.0) / (sl * root2))
        lo = torch.where(yy < b[1], first, torch.where(yy > b[B - 1], last, lo))
        hi = torch.where(yy < b[1], first, torch.where(yy > b[B - 1], last, hi))
    ud = u.double()
    err = torch.maximum(torch.maximum(lo - ud, ud - hi), torch.zeros_like(ud))
    return torch.where(torch.isnan(y), torch.full_like(err, float("nan")), err)


def worst(err: torch.Tensor) -> float:
    """The largest finite-or-infinite entry; NaN entries (a NaN draw of the reference's arithmetic) do not count."""
    err = err[~torch.isnan(err)]
    return float(err.max()) if err.numel() else 0.0


def reference_error(case: dict, u: torch.Tensor, tails: str) -> float:
    """``d_ref``: the measure of the reference's float32 arithmetic on the case -- ``_icdf_at`` for the linear form
    (one call per column of levels), the float32 restatement for the half-normal form, whose pieces are the
    reference's."""
    from multimodalpfn_amd.bar_distribution import FullSupportBarDistribution

    logits = case["logits"] if case["temperature"] == 1 else case["logits"] / case["temperature"]
    if tails == "linear":
        crit = FullSupportBarDistribution(torch.from_numpy(case["borders"]))
        y = torch.stack([crit._icdf_at(logits, u[:, j].contiguous()) for j in range(u.shape[1])], -1)
    else:
        y = draw(case["logits"], case["borders"], u, tails, torch.float32, temperature=case["temperature"])
    return worst(prob_error(case, y, u, tails))
