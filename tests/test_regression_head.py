"""CPU: the bar-distribution head's restatement and host tables against the reference's recorded outputs
(``tests/golden/regression/head_B*.npz``, written by ``tests/golden/make_regression_golden.py``), and what the
restatement's three switches are worth."""

import numpy as np
import pytest
import torch

import regression_oracle as ro
from helpers import GOLDEN

from multimodalpfn_amd import _lib
from multimodalpfn_amd.bar_distribution import (CDF_ONE, CDF_ZERO, FullSupportBarDistribution, border_tables,
                                                share_of_bucket_left)

REG = GOLDEN / "regression"
PROB_FLOOR = 64 * 2.0 ** -24  # the head's absolute bound on a probability (test_regression_head_gpu)


def head_fixture(B: int):
    return np.load(REG / f"head_B{B}.npz")


@pytest.mark.parametrize("B", ro.HEAD_BARS)
def test_float32_restatement_is_the_reference_bit_for_bit(B):
    """Same operations in the same order: final logits (-inf included), mean, mode and quantiles ``torch.equal``."""
    z = head_fixture(B)
    cases = ro.head_cases(B)
    assert len(z.files) == 4 * len(cases)
    for case in cases:
        with ro.fixture_threads():
            got = ro.run_head(case, torch.float32)
        for k in ("logits", "mean", "mode", "quantiles"):
            ref = torch.from_numpy(z[f"{case['name']}_{k}"])
            assert got[k].dtype == torch.float32 and got[k].shape == ref.shape
            assert not torch.isnan(ref).any()
            assert torch.equal(got[k], ref), (B, case["name"], k)


@pytest.mark.parametrize("B", ro.HEAD_BARS)
def test_host_border_tables_are_the_restatements(B):
    """``border_tables`` (numpy float32) against the torch restatement's bucket index, clamped share and the borders
    at which the reference overwrites the CDF; and the CDF rebuilt from the tables equals ``member_bars``."""
    for case in ro.head_cases(B)[:4]:
        to = torch.from_numpy(case["std_borders"])
        for frm_np, lg in zip(case["borders"], case["logits"]):
            frm = torch.from_numpy(frm_np)
            idx, share = border_tables(frm_np, case["std_borders"])
            assert idx.dtype == np.int32 and share.dtype == np.float32 and idx.shape == share.shape == (B + 1,)
            buckets = ro.bucket_index(to.clone(), frm).clamp(0, B - 1)
            widths = frm[1:] - frm[:-1]
            ref_share = ro.share_of_bucket_left(to, frm[buckets], widths[buckets]).clamp(0.0, 1.0)
            forced0 = (to <= frm[0]) & ~(to >= frm[-1])
            forced1 = to >= frm[-1]
            forced0[0], forced1[0] = True, False
            forced0[-1], forced1[-1] = False, True
            free = ~(forced0 | forced1)
            assert np.array_equal(idx == CDF_ZERO, forced0.numpy())
            assert np.array_equal(idx == CDF_ONE, forced1.numpy())
            assert np.array_equal(idx[free.numpy()], buckets[free].numpy())
            assert np.array_equal(share[free.numpy()], ref_share[free].numpy())
            # the member's bars from the tables, in the restatement's operations
            probs = torch.softmax(lg, -1)
            c = torch.cumsum(probs, -1) - probs
            ix = torch.from_numpy(idx.astype(np.int64)).clamp_min(0)
            left = (c[:, ix] + probs[:, ix] * torch.from_numpy(share)).clip(0.0, 1.0)
            left[:, idx == CDF_ZERO] = 0.0
            left[:, idx == CDF_ONE] = 1.0
            bars = (left[:, 1:] - left[:, :-1]).clamp_min(0.0)
            assert torch.equal(bars, ro.member_bars(lg, frm, to))


def test_share_keeps_the_reference_precedence():
    """utils.py:669: the division binds first."""
    assert share_of_bucket_left(np.float32(3.0), np.float32(1.0), np.float32(4.0)) == np.float32(2.75)
    assert ro.share_of_bucket_left(3.0, 1.0, 4.0) == 2.75 and ro.share_of_bucket_left(3.0, 1.0, 4.0, parenthesised=True) == 0.5


@pytest.mark.parametrize("B", [2, 100, 5000])
def test_full_support_bar_distribution_matches_reference_outputs(B):
    """The package's criterion on the reference's final logits: ``torch.equal`` mean, mode, quantiles, median."""
    z = head_fixture(B)
    for case in ro.head_cases(B):
        crit = FullSupportBarDistribution(torch.from_numpy(case["std_borders"]) * ro.HEAD_Y_STD + ro.HEAD_Y_MEAN).float()
        assert crit.num_bars == B and crit.bucket_widths.shape == (B,)
        logits = torch.from_numpy(z[f"{case['name']}_logits"])
        with ro.fixture_threads():
            mean = crit.mean(logits)
        assert torch.equal(mean, torch.from_numpy(z[f"{case['name']}_mean"]))
        assert torch.equal(crit.mode(logits), torch.from_numpy(z[f"{case['name']}_mode"]))
        for k, q in enumerate(case["levels"]):
            assert torch.equal(crit.icdf(logits, q), torch.from_numpy(z[f"{case['name']}_quantiles"][k]))
        assert torch.equal(crit.median(logits), torch.from_numpy(z[f"{case['name']}_quantiles"][2]))
        assert crit.quantile(logits).shape == (case["Q"], 2)
        tabs = crit.head_tables()
        ref = ro.criterion_tables(torch.from_numpy(case["crit_borders"]))
        for k in ("borders", "bucket_means", "mode_means", "widths"):
            assert torch.equal(tabs[k], ref[k]), k
    # cdf: 0 / 1 at the ends, the weight left of an inner border in between
    lg = torch.zeros(1, B)
    c = crit.cdf(lg, crit.borders.clone())
    assert c[0, 0] == 0 and c[0, -1] == 1
    assert torch.allclose(c[0], torch.arange(B + 1) / B, atol=1e-6)


def test_full_support_bar_distribution_refuses_bad_borders():
    with pytest.raises(ValueError):
        FullSupportBarDistribution(torch.tensor([0.0, 0.0, 1.0]))  # empty first bucket
    with pytest.raises(ValueError):
        FullSupportBarDistribution(torch.tensor([0.0, 2.0, 1.0, 3.0]))  # unsorted
    with pytest.raises(ValueError):
        FullSupportBarDistribution(torch.tensor([1.0]))


def test_library_refuses_bar_head_without_context():
    lib = _lib.load_library()
    args = [None] * 22
    args[2:5] = [1, 1, 2]
    args[6], args[9], args[10], args[11], args[17] = 2, 3, 1.0, 0, 0
    assert lib.mmpfn_bar_head(*args) == _lib.MMPFN_ERR_INVALID


# ------------------------------------------------------------------------------------------------ sensitivity


def _span(case):
    b = case["crit_borders"].astype(np.float64)
    return float(b[-2] - b[1])


def test_sensitivity_cancel_mask():
    """Without the cancel mask the cancelled outer bars keep their weight: in every case with such a member (one
    of 8 members at the least) a probability moves by >= 100 bounds (measured: 127 .. 12500)."""
    n = 0
    for B in (37, 257):
        for case in ro.head_cases(B):
            if "cancel" not in case["kinds"]:
                continue
            a = ro.run_head(case, torch.float64)
            b = ro.run_head(case, torch.float64, drop_cancel=True)
            assert float((a["probs"] - b["probs"]).abs().max()) > 100 * PROB_FLOOR, (B, case["name"])
            n += 1
    assert n >= 6


def test_sensitivity_share_precedence():
    """``(ys - left) / width`` instead of utils.py:669's ``ys - left / width``: probabilities move by >= 100 bounds
    on every case of the grid's mid sizes (measured: 256 at the least, a single identity member with a flat row
    over 1023 bars, up to 0.98 of the whole weight)."""
    for B in (37, 100, 1023):
        for case in ro.head_cases(B):
            a = ro.run_head(case, torch.float64)
            b = ro.run_head(case, torch.float64, parenthesised=True)
            assert float((a["probs"] - b["probs"]).abs().max()) > 100 * PROB_FLOOR, (B, case["name"])


def test_sensitivity_halfnormal_end_means():
    """Plain bucket means at the two ends instead of the half-normal ones (bar_distribution.py:588-597): the mean
    moves by >= 100 bounds of the span where the end bars carry weight (flat and random rows of a small grid)."""
    moved = 0.0
    for B in (37, 64):
        for case in ro.head_cases(B):
            a = ro.run_head(case, torch.float64)
            b = ro.run_head(case, torch.float64, plain_end_means=True)
            assert torch.equal(a["probs"], b["probs"]) and torch.equal(a["quantiles"], b["quantiles"])
            moved = max(moved, float((a["mean"] - b["mean"]).abs().max()) / _span(case))
    assert moved > 100 * PROB_FLOOR, moved
