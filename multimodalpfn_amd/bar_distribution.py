"""Host side of the bar-distribution head (``mmpfn_bar_head``, csrc/barhead.hip).

A regression model predicts logits over ``B`` bars between ``B + 1`` borders.  Every ensemble member sees the
target through its own transform, so its bars lie between its own borders; the ensemble's distribution is
the mean of the members' distributions moved onto the criterion's borders (regressor.py:691-706,
utils.py:659-700).  What of that depends on the borders alone is computed here once, in float32 as the
reference computes it; what depends on the row runs on the device.

``FullSupportBarDistribution`` is the reading half of the reference's class (bar_distribution.py:448-597):
borders, widths and the point estimates of ``output_type="full"``; no loss, sampling, acquisition or plotting.
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


def halfnormal_mean(range_max: torch.Tensor, p: float = 0.5) -> torch.Tensor:
    """Mean of the half-normal that has weight ``p`` before ``range_max`` (bar_distribution.py:476-484)."""
    unit = torch.distributions.HalfNormal(torch.tensor(1.0))
    return torch.distributions.HalfNormal(range_max / unit.icdf(torch.tensor(p))).mean


class FullSupportBarDistribution:
    """Bars between ``borders`` with half-normal tails in the first and last bucket."""

    def __init__(self, borders: torch.Tensor):
        borders = torch.as_tensor(borders).contiguous()
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
        return FullSupportBarDistribution(self.borders.float())

    def to(self, *args, **kwargs) -> "FullSupportBarDistribution":
        return FullSupportBarDistribution(self.borders.to(*args, **kwargs))

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
        share = ((ys - self.borders[idx]) / self.bucket_widths[idx]).clamp(0.0, 1.0)
        out = left_of_bucket + probs.gather(-1, idx) * share
        out[ys <= self.borders[0]] = 0.0
        out[ys >= self.borders[-1]] = 1.0
        return out.clip(0.0, 1.0)

    def head_tables(self) -> dict[str, torch.Tensor]:
        """The criterion's float32 tables ``mmpfn_bar_head`` reads."""
        c = self.float()
        return {"borders": c.borders, "bucket_means": c.bucket_means(), "mode_means": c.plain_bucket_means(),
                "widths": c.bucket_widths}
