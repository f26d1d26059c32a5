"""Host side of the bar-distribution head (``mmpfn_bar_head``, csrc/barhead.hip).

A regression model predicts logits over ``B`` bars between ``B + 1`` borders.  Every ensemble member sees the
target through its own transform, so its bars lie between its own borders; the ensemble's distribution is
the mean of the members' distributions moved onto the criterion's borders (regressor.py:691-706,
utils.py:659-700).  What of that depends on the borders alone is computed here once, in float32 as the
reference computes it; what depends on the row runs on the device.

``FullSupportBarDistribution`` is the reference's class (bar_distribution.py:18-758) without its plotting: borders,
widths, the point estimates of ``output_type="full"``, the negative log density (``forward``), ``cdf`` / ``pdf``,
sampling, the acquisition functions ``pi`` / ``ei`` / ``ucb`` and ``mean_of_square`` / ``variance``.  The host
methods are plain torch on any device; ``score_tables`` holds what the device scoring (``mmpfn_bar_score``) needs.
"""

from __future__ import annotations

import math

import numpy as np
import torch

CDF_ZERO, CDF_ONE = -1, -2  # idx codes of ``border_tables``: the member's CDF at that border is 0 / 1 for every row


def share_of_bucket_left(ys, left_border, width):
    """The share of the bucket to the left of ``ys`` exactly as utils.py:669 evaluates it:
    ``ys - borders[idx] / bucket_widths[idx]`` -- the division binds before the subtraction, so this is not
    ``(ys - left) / width`` (bar_distribution.py:84-86 has the parentheses; the regressor's path does not).
    Parity with the reference pins this form (known oddities); the caller clamps to [0, 1]."""
    return ys - left_border / width


def border_tables(frm: np.ndarray, to: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """Per target border ``to[j]``: the bucket of ``frm`` that holds it and its share of that bucket
    (utils.py:649-653,660-670), float32.  Borders at which the reference overwrites the CDF whatever the logits
    (utils.py:675-676: at or outside ``frm``'s ends; :697-698: the first and last target border) carry
    ``CDF_ZERO`` / ``CDF_ONE`` as index, in the reference's order of assignment (the later one wins)."""
    frm = np.ascontiguousarray(frm, dtype=np.float32)
    ys = np.ascontiguousarray(to, dtype=np.float32)
    n_bars = frm.size - 1
    if frm.ndim != 1 or ys.shape != frm.shape or n_bars < 1:
        raise ValueError(f"borders of one length >= 2 expected, got {frm.shape} and {ys.shape}")
    idx = np.searchsorted(frm, ys, side="left").astype(np.int64) - 1
    idx[ys == frm[0]] = 0
    idx[ys == frm[-1]] = n_bars - 1
    idx = np.clip(idx, 0, n_bars - 1)
    widths = frm[1:] - frm[:-1]
    with np.errstate(divide="ignore", invalid="ignore"):
        share = np.clip(share_of_bucket_left(ys, frm[idx], widths[idx]), np.float32(0), np.float32(1))
    share = share.astype(np.float32)
    code = idx.astype(np.int32)
    code[ys <= frm[0]] = CDF_ZERO
    code[ys >= frm[-1]] = CDF_ONE
    code[0] = CDF_ZERO
    code[-1] = CDF_ONE
    return code, share


def linear_share_of_bucket(ys, left_border, width):
    """The share of a bucket left of ``ys`` as ``cdf`` has it (bar_distribution.py:84-86), in every bucket: ``cdf``
    is piecewise linear in the two end buckets too, while ``forward``, ``pi`` and ``ei`` put half-normal tails there
    (known oddities)."""
    return (ys - left_border) / width


def exp_of_negative_log_density(nll):
    """``pdf`` as bar_distribution.py:573-575 evaluates it: the exponential of ``forward``'s result, which is the
    *negative* log density -- the reciprocal of the density (known oddities)."""
    return torch.exp(nll)


def last_bucket_mean_of_square(variance, left_border):
    """The last bucket's mean of squares as bar_distribution.py:621-624 evaluates it: ``variance + (variance +
    left_border)^2`` -- the half-normal's variance where its mean is meant, unlike the first bucket's term
    (known oddities)."""
    return variance + (variance + left_border).square()


def halfnormal_with_p_weight_before(range_max: torch.Tensor, p: float = 0.5) -> torch.distributions.HalfNormal:
    """The half-normal that has weight ``p`` before ``range_max`` (bar_distribution.py:476-484)."""
    unit = torch.distributions.HalfNormal(torch.tensor(1.0))
    return torch.distributions.HalfNormal(range_max / unit.icdf(torch.tensor(p)))


def halfnormal_mean(range_max: torch.Tensor, p: float = 0.5) -> torch.Tensor:
    """Mean of the half-normal that has weight ``p`` before ``range_max`` (bar_distribution.py:476-484)."""
    unit = torch.distributions.HalfNormal(torch.tensor(1.0))
    return torch.distributions.HalfNormal(range_max / unit.icdf(torch.tensor(p))).mean


class FullSupportBarDistribution:
    """Bars between ``borders`` with half-normal tails in the first and last bucket."""

    def __init__(self, borders: torch.Tensor, *, ignore_nan_targets: bool = True):
        borders = torch.as_tensor(borders).contiguous()
        self.ignore_nan_targets = ignore_nan_targets
        if borders.dim() != 1 or borders.numel() < 2:
            raise ValueError("borders: one dimension, at least two entries")
        self.borders = borders
        widths = self.bucket_widths
        if not bool((widths >= 0).all()):
            raise ValueError("borders must be sorted")
        if not (widths[0] > 0 and widths[-1] > 0):  # assert_support (bar_distribution.py:463-474)
            raise ValueError("the first and the last bucket need a width > 0")
        span = self.borders[-1] - self.borders[0]
        if abs(1 - float(widths.sum() / span)) >= 1e-2:
            raise ValueError("bucket widths do not add up to the borders' span")

    def float(self) -> "FullSupportBarDistribution":
        return FullSupportBarDistribution(self.borders.float(), ignore_nan_targets=self.ignore_nan_targets)

    def to(self, *args, **kwargs) -> "FullSupportBarDistribution":
        return FullSupportBarDistribution(self.borders.to(*args, **kwargs), ignore_nan_targets=self.ignore_nan_targets)

    @property
    def bucket_widths(self) -> torch.Tensor:
        return self.borders[1:] - self.borders[:-1]

    @property
    def num_bars(self) -> int:
        return self.borders.numel() - 1

    def plain_bucket_means(self) -> torch.Tensor:
        return self.borders[:-1] + self.bucket_widths / 2

    def bucket_means(self) -> torch.Tensor:
        """Bucket means with the two half-normal end means (bar_distribution.py:588-597)."""
        means = self.plain_bucket_means()
        widths = self.bucket_widths
        means[0] = -halfnormal_mean(widths[0]) + self.borders[1]
        means[-1] = halfnormal_mean(widths[-1]) + self.borders[-2]
        return means

    def mean(self, logits: torch.Tensor) -> torch.Tensor:
        means = self.bucket_means()
        return torch.softmax(logits, -1) @ means.to(logits.device).type(logits.dtype)

    def mode(self, logits: torch.Tensor) -> torch.Tensor:
        density = logits.softmax(-1) / self.bucket_widths
        return self.plain_bucket_means()[density.argmax(-1)]

    def icdf(self, logits: torch.Tensor, left_prob: float) -> torch.Tensor:
        """The position with ``left_prob`` of the weight to its left (bar_distribution.py:256-283)."""
        probs = logits.softmax(-1)
        cum = torch.cumsum(probs, -1)
        level = left_prob * torch.ones(*cum.shape[:-1], 1, device=logits.device)
        idx = torch.searchsorted(cum, level).squeeze(-1).clamp(0, cum.shape[-1] - 1)
        cum0 = torch.cat([torch.zeros(*cum.shape[:-1], 1, device=logits.device), cum], -1)
        rest = left_prob - cum0.gather(-1, idx[..., None]).squeeze(-1)
        left, right = self.borders[idx], self.borders[idx + 1]
        return left + (right - left) * rest / probs.gather(-1, idx[..., None]).squeeze(-1)

    def median(self, logits: torch.Tensor) -> torch.Tensor:
        return self.icdf(logits, 0.5)

    def quantile(self, logits: torch.Tensor, center_prob: float = 0.682) -> torch.Tensor:
        side = (1.0 - center_prob) / 2
        return torch.stack((self.icdf(logits, side), self.icdf(logits, 1.0 - side)), -1)

    def cdf(self, logits: torch.Tensor, ys: torch.Tensor) -> torch.Tensor:
        """Weight to the left of ``ys`` (bar_distribution.py:59-97; with the parentheses, unlike utils.py:669)."""
        if ys.dim() < logits.dim() and ys.dim() == 1:
            ys = ys.repeat(logits.shape[:-1] + (1,))
        probs = torch.softmax(logits, -1)
        idx = torch.searchsorted(self.borders, ys) - 1
        idx[ys == self.borders[0]] = 0
        idx[ys == self.borders[-1]] = self.num_bars - 1
        idx = idx.clamp(0, self.num_bars - 1)
        left_of_bucket = (torch.cumsum(probs, -1) - probs).gather(-1, idx)
        share = linear_share_of_bucket(ys, self.borders[idx], self.bucket_widths[idx]).clamp(0.0, 1.0)
        out = left_of_bucket + probs.gather(-1, idx) * share
        out[ys <= self.borders[0]] = 0.0
        out[ys >= self.borders[-1]] = 1.0
        return out.clip(0.0, 1.0)

    # ------------------------------------------------------------------ density, loss, sampling
    def side_normals(self) -> tuple[torch.distributions.HalfNormal, torch.distributions.HalfNormal]:
        """The half-normals of the first and the last bucket: half their weight lies within the bucket's width."""
        widths = self.bucket_widths
        return halfnormal_with_p_weight_before(widths[0]), halfnormal_with_p_weight_before(widths[-1])

    def map_to_bucket_idx(self, y: torch.Tensor) -> torch.Tensor:
        """The bucket of every ``y`` (bar_distribution.py:156-162): ``searchsorted - 1`` on the left side, so a ``y``
        on a border belongs to the bucket left of it, except on the first border; unclamped (-1 / ``num_bars``
        outside the borders)."""
        idx = torch.searchsorted(self.borders, y) - 1
        idx[y == self.borders[0]] = 0
        idx[y == self.borders[-1]] = self.num_bars - 1
        return idx

    def compute_scaled_log_probs(self, logits: torch.Tensor) -> torch.Tensor:
        """Log density of every bucket under its uniform form (bar_distribution.py:173-176)."""
        return torch.log_softmax(logits, -1) - torch.log(self.bucket_widths)

    def forward(self, logits: torch.Tensor, y: torch.Tensor, mean_prediction_logits: torch.Tensor | None = None):
        """The negative log density of ``y`` ``[...]`` under ``logits`` ``[..., B]`` (bar_distribution.py:487-571).
        The first and the last bucket carry their half-normal's log density; a ``y`` outside the borders is clamped
        into the end bucket on its side; a NaN ``y`` scores 0 with ``ignore_nan_targets``, else ``ValueError``.
        ``mean_prediction_logits`` is not served.  The reference's ``losses_per_bucket`` running statistic is a
        training aid and is not kept."""
        if mean_prediction_logits is not None:
            raise NotImplementedError("mean_prediction_logits is not served")
        if self.num_bars < 2:
            raise ValueError("the negative log density needs at least two bars")
        if logits.shape[-1] != self.num_bars:
            raise ValueError(f"{logits.shape[-1]} logits for {self.num_bars} bars")
        y = y.clone().view(*logits.shape[:-1])
        ignored = torch.isnan(y)
        if ignored.any() and not self.ignore_nan_targets:
            raise ValueError(f"Found NaN in target {y}")
        y[ignored] = self.borders[0]
        idx = self.map_to_bucket_idx(y).clamp_(0, self.num_bars - 1)
        log_probs = self.compute_scaled_log_probs(logits).gather(-1, idx.unsqueeze(-1)).squeeze(-1)
        first, last = self.side_normals()
        widths = self.bucket_widths
        in_first, in_last = idx == 0, idx == self.num_bars - 1
        log_probs[in_first] += first.log_prob((self.borders[1] - y[in_first]).clamp(min=1e-8)) + torch.log(widths[0])
        log_probs[in_last] += last.log_prob((y[in_last] - self.borders[-2]).clamp(min=1e-8)) + torch.log(widths[-1])
        nll = -log_probs
        if ignored.any():
            nll[ignored] = 0.0
        return nll

    __call__ = forward

    def pdf(self, logits: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        return exp_of_negative_log_density(self.forward(logits, y))

    def sample(self, logits: torch.Tensor, t: float = 1.0) -> torch.Tensor:
        """One draw per row at temperature ``t`` (bar_distribution.py:577-585): the reference's uniform draw
        ``torch.rand(*logits.shape[:-1])`` (on the CPU generator, so a seed gives its stream), then one ``icdf`` over
        all rows."""
        level = torch.rand(*logits.shape[:-1]).to(logits.device)
        return self._icdf_at(logits / t, level)

    def _icdf_at(self, logits: torch.Tensor, level: torch.Tensor) -> torch.Tensor:
        """``icdf`` with a level per row."""
        probs = logits.softmax(-1)
        cum = torch.cumsum(probs, -1)
        idx = torch.searchsorted(cum, level.unsqueeze(-1)).squeeze(-1).clamp(0, cum.shape[-1] - 1)
        cum0 = torch.cat([torch.zeros(*cum.shape[:-1], 1, device=logits.device), cum], -1)
        rest = level - cum0.gather(-1, idx[..., None]).squeeze(-1)
        left, right = self.borders[idx], self.borders[idx + 1]
        return left + (right - left) * rest / probs.gather(-1, idx[..., None]).squeeze(-1)

    # ------------------------------------------------------------------ acquisition
    @staticmethod
    def _per_row(best_f, logits: torch.Tensor) -> torch.Tensor:
        if not torch.is_tensor(best_f) or not len(best_f.shape):
            best_f = torch.full(logits[..., 0].shape, best_f, device=logits.device)
        if best_f.shape != logits[..., 0].shape:
            raise ValueError(f"best_f.shape: {best_f.shape}, logits.shape: {logits.shape}")
        return best_f

    def _positions_in_side_normals(self, best_f: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
        """How far ``best_f`` reaches into the first bucket's half-normal (from ``borders[1]`` leftwards) and into
        the last one's (from ``borders[-2]`` rightwards); 0 outside them."""
        return -(best_f - self.borders[1]).clamp(max=0.0), (best_f - self.borders[-2]).clamp(min=0.0)

    def pi(self, logits: torch.Tensor, best_f, *, maximize: bool = True) -> torch.Tensor:
        """Probability of improvement over ``best_f`` (a number or one per row; bar_distribution.py:629-675)."""
        if maximize is not True:
            raise ValueError("only maximize=True is served")
        best_f = self._per_row(best_f, logits)
        probs = torch.softmax(logits, -1)
        factor = 1.0 - ((best_f[..., None] - self.borders[:-1]) / self.bucket_widths).clamp(0.0, 1.0)
        first, last = self.side_normals()
        in_first, in_last = self._positions_in_side_normals(best_f)
        factor[..., 0] = 0.0
        factor[..., 0][in_first > 0.0] = first.cdf(in_first[in_first > 0.0])
        factor[..., -1] = 1.0
        factor[..., -1][in_last > 0.0] = 1.0 - last.cdf(in_last[in_last > 0.0])
        return (probs * factor).sum(-1)

    def ei_for_halfnormal(self, scale, best_f, *, maximize: bool = True) -> torch.Tensor:
        """Expected improvement of a half-normal of ``scale`` over ``best_f`` (bar_distribution.py:677-703): twice
        that of the normal N(0, scale^2)."""
        if not maximize:
            raise ValueError("only maximize=True is served")
        u = (torch.tensor(0.0) - best_f) / scale
        unit = torch.distributions.Normal(torch.zeros_like(u), torch.ones_like(u))
        return 2 * (scale * (torch.exp(unit.log_prob(u)) + u * unit.cdf(u)))

    def ei(self, logits: torch.Tensor, best_f, *, maximize: bool = True) -> torch.Tensor:
        """Expected improvement over ``best_f`` (bar_distribution.py:706-758)."""
        if torch.isnan(logits).any():
            raise ValueError(f"logits contains NaNs: {logits}")
        if not maximize:
            raise ValueError("only maximize=True is served")
        best_f = self._per_row(best_f, logits)
        left, right = self.borders[:-1], self.borders[1:]
        per_bar = best_f[..., None].repeat(*[1] * best_f.dim(), logits.shape[-1])
        inside = per_bar.clamp(left, right)
        per_bucket = ((right ** 2 - inside ** 2) / 2 - per_bar * (right - inside)) / (right - left)
        first, last = self.side_normals()
        in_first, in_last = self._positions_in_side_normals(best_f)
        per_bucket[..., -1] = self.ei_for_halfnormal(last.scale, in_last)
        per_bucket[..., 0] = (self.ei_for_halfnormal(first.scale, torch.zeros_like(in_first))
                              - self.ei_for_halfnormal(first.scale, in_first))
        return torch.einsum("...b,...b->...", torch.softmax(logits, -1), per_bucket)

    def ucb(self, logits: torch.Tensor, best_f=None, rest_prob: float = (1 - 0.682) / 2, *,
            maximize: bool = True) -> torch.Tensor:
        """The quantile that leaves ``rest_prob`` above (below, when minimising) it (bar_distribution.py:296-326);
        ``best_f`` is unused, as in the reference."""
        return self.icdf(logits, 1 - rest_prob if maximize else rest_prob)

    def bucket_mean_squares(self) -> torch.Tensor:
        """E[x^2] of every bucket (bar_distribution.py:606-624): uniform inside, the half-normals' at the ends."""
        left, right = self.borders[:-1], self.borders[1:]
        squares = (left.square() + right.square() + left * right) / 3.0
        first, last = self.side_normals()
        squares[0] = first.variance + (-first.mean + self.borders[1]).square()
        squares[-1] = last_bucket_mean_of_square(last.variance, self.borders[-2])
        return squares

    def mean_of_square(self, logits: torch.Tensor) -> torch.Tensor:
        return torch.softmax(logits, -1) @ self.bucket_mean_squares()

    def variance(self, logits: torch.Tensor) -> torch.Tensor:
        return self.mean_of_square(logits) - self.mean(logits).square()

    # ------------------------------------------------------------------ device tables
    def head_tables(self) -> dict[str, torch.Tensor]:
        """The criterion's float32 tables ``mmpfn_bar_head`` reads."""
        c = self.float()
        return {"borders": c.borders, "bucket_means": c.bucket_means(), "mode_means": c.plain_bucket_means(),
                "widths": c.bucket_widths}

    def score_tables(self) -> dict[str, torch.Tensor]:
        """What ``mmpfn_bar_score`` reads beside ``head_tables``' borders and widths, float32: ``log_widths`` and
        ``mean_squares`` ``[B]`` as the reference computes them; ``ei_mids`` ``[B]``, the interior buckets' plain
        means about ``centre``, a border in the middle -- each border's distance from it is exact to its own size,
        so borders far from zero lose nothing -- and 0 in the two end buckets, whose terms are the half-normals';
        ``ends`` ``[9]``: per end bucket (first, last) the half-normal's scale, 1 / scale, 1 / (2 scale^2) and its
        log density at 0 plus the log of the bucket's width, then ``centre`` (include/mmpfn_hip.h)."""
        c = self.float()
        widths = c.bucket_widths
        first, last = c.side_normals()
        centre = c.borders[c.num_bars // 2]
        mids = ((c.borders[:-1] - centre) + (c.borders[1:] - centre)) / 2
        mids[0] = mids[-1] = 0.0
        ends = torch.zeros(9)
        zero = torch.tensor(0.0)
        for k, (normal, width) in enumerate(((first, widths[0]), (last, widths[-1]))):
            ends[k] = normal.scale
            ends[2 + k] = 1.0 / normal.scale
            ends[4 + k] = 1.0 / (2 * normal.scale ** 2)
            ends[6 + k] = normal.log_prob(zero) + torch.log(width)
        ends[8] = centre
        return {"log_widths": torch.log(widths), "mean_squares": c.bucket_mean_squares(), "ei_mids": mids, "ends": ends}
