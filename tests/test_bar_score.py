"""CPU: the bar distribution's scoring -- the restatement (``bar_score_cases``) and ``FullSupportBarDistribution``'s host
methods against the reference's recorded outputs (``tests/golden/bar_score/score_B*.npz``, written by
``tests/golden/make_bar_score_golden.py``), what the host refuses, what the restatement's switches are worth, and the
scoring kernels' code generation."""

from pathlib import Path

import numpy as np
import pytest
import torch

import bar_score_cases as bc
import regression_oracle as ro
from helpers import GOLDEN, report
from test_codegen import HIPCC, _asm, _resources
from test_regression_head import PROB_FLOOR

from multimodalpfn_amd import _lib
from multimodalpfn_amd.bar_distribution import FullSupportBarDistribution

KINDS = ("nll", "cdf", "pi", "ei", "mean_of_square")


def fixture(B: int):
    return np.load(GOLDEN / "bar_score" / f"score_B{B}.npz")


def _bits_equal(a: torch.Tensor, ref: torch.Tensor) -> bool:
    """``torch.equal`` that takes a NaN for a NaN (the reference's ``ei`` with an empty bucket)."""
    return a.dtype == ref.dtype and a.shape == ref.shape and torch.equal(torch.isnan(a), torch.isnan(ref)) and \
        torch.equal(torch.nan_to_num(a, nan=0.0), torch.nan_to_num(ref, nan=0.0))


@pytest.mark.parametrize("B", bc.BARS)
def test_float32_restatement_is_the_reference_bit_for_bit(B):
    z = fixture(B)
    cases = bc.cases(B)
    assert len(z.files) == 8 * len(cases)
    for case in cases:
        with ro.fixture_threads():
            got = bc.score(case, torch.float32)
        for k in KINDS:
            assert _bits_equal(got[k], torch.from_numpy(z[f"{case['name']}_{k}"])), (B, case["name"], k)
        if case["dead"]:
            assert torch.isposinf(got["nll"][2, 5])  # a target in a -inf bar


def _host_scores(case):
    crit = FullSupportBarDistribution(torch.from_numpy(case["borders"]))
    logits = case["logits"] if case["temperature"] == 1 else case["logits"] / case["temperature"]
    ys = case["ys"]
    real = ys[:, 1:].contiguous()
    cols = range(real.shape[1])
    res = {
        "nll": torch.stack([crit(logits, ys[:, j]) for j in range(ys.shape[1])], -1),
        "pdf": torch.stack([crit.pdf(logits, ys[:, j]) for j in range(ys.shape[1])], -1),
        "cdf": crit.cdf(logits, real),
        "pi": torch.stack([crit.pi(logits, real[:, j].contiguous()) for j in cols], -1),
        "ei": torch.stack([crit.ei(logits, real[:, j].contiguous()) for j in cols], -1),
        "mean_of_square": crit.mean_of_square(logits),
        "variance": crit.variance(logits),
    }
    torch.manual_seed(bc.SAMPLE_SEED)
    res["sample"] = crit.sample(logits, bc.SAMPLE_T)
    return crit, logits, res


@pytest.mark.parametrize("B", bc.BARS)
def test_host_methods_are_the_reference_bit_for_bit(B):
    """``forward`` / ``__call__``, ``pdf``, ``cdf``, ``pi``, ``ei``, ``mean_of_square``, ``variance`` and the seeded
    ``sample`` of the package's class, every case; ``ucb`` is the ``icdf`` of its level; ``score_tables`` holds the
    reference's per-bucket values."""
    z = fixture(B)
    for case in bc.cases(B):
        with ro.fixture_threads():
            crit, logits, got = _host_scores(case)
            for k, v in got.items():
                assert _bits_equal(v, torch.from_numpy(z[f"{case['name']}_{k}"])), (B, case["name"], k)
            rest = (1 - 0.682) / 2
            assert torch.equal(crit.ucb(logits, 0.0), crit.icdf(logits, 1 - rest))
            assert torch.equal(crit.ucb(logits, None, 0.1, maximize=False), crit.icdf(logits, 0.1))
            tabs = crit.score_tables()
            assert torch.equal(tabs["log_widths"], torch.log(crit.bucket_widths))
            assert torch.equal(tabs["mean_squares"], bc.bucket_mean_squares(crit.borders))
        assert all(t.dtype == torch.float32 for t in tabs.values()) and tabs["ends"].shape == (_lib.BAR_SCORE_ENDS,)
        assert tabs["ei_mids"][0] == 0 and tabs["ei_mids"][-1] == 0 and tabs["ends"][8] in crit.borders
        # the centred means are the plain ones to float64's accuracy although the borders are far from zero
        mid64 = (crit.borders[:-1].double() + crit.borders[1:].double()) / 2 - tabs["ends"][8].double()
        span = float(crit.borders[-1] - crit.borders[0])
        assert float((tabs["ei_mids"].double() - mid64)[1:-1].abs().max() if B > 2 else 0.0) <= 2.0 ** -22 * span


def test_host_keeps_the_reference_oddities():
    """``pdf`` is the exponential of the *negative* log density; ``cdf`` is linear in the end buckets where ``pi`` has
    the half-normal tails (so ``cdf + pi`` is not 1 there, and is 1 inside)."""
    case = bc.cases(37)[0]
    crit, logits, got = _host_scores(case)
    assert torch.equal(got["pdf"], torch.exp(got["nll"]))
    total = got["cdf"] + got["pi"]
    # (columns of cdf / pi: the targets after the NaN one)
    assert float((total[:, 3] - 1).abs().max()) < 1e-6  # a target on borders[1]: nothing of an end bucket is cut
    assert float((total[0, 2] - 1).abs()) > 1e-3  # inside the first bucket of the flat row
    assert crit.float().ignore_nan_targets and not FullSupportBarDistribution(crit.borders, ignore_nan_targets=False).to(
        torch.float64).ignore_nan_targets


def test_host_refusals():
    case = bc.cases(37)[0]
    borders, logits, ys = torch.from_numpy(case["borders"]), case["logits"], case["ys"]
    strict = FullSupportBarDistribution(borders, ignore_nan_targets=False)
    with pytest.raises(ValueError):
        strict(logits, ys[:, 0])  # a NaN target
    assert torch.isfinite(strict(logits, ys[:, 3])).all()
    crit = FullSupportBarDistribution(borders)
    assert (crit(logits, ys[:, 0]) == 0).all()
    with pytest.raises(NotImplementedError):
        crit(logits, ys[:, 3], mean_prediction_logits=logits)
    bad = logits.clone()
    bad[1, 3] = float("nan")
    with pytest.raises(ValueError):
        crit.ei(bad, 0.5)
    with pytest.raises(ValueError):
        crit.pi(logits, torch.zeros(2))  # one incumbent per row


def test_library_refuses_bar_score_without_context():
    lib = _lib.load_library()
    assert lib.mmpfn_bar_score(*([None] * 2 + [1, 2, 1.0] + [None] * 7 + [1] + [None] * 5)) == _lib.MMPFN_ERR_INVALID
    head = [None] * 22
    head[2:5] = [1, 1, 2]
    head[6], head[9], head[10], head[11], head[17] = 2, 3, 1.0, 0, 0
    assert lib.mmpfn_bar_head_score(*head, *([None] * 5 + [1] + [None] * 5)) == _lib.MMPFN_ERR_INVALID


# ------------------------------------------------------------------------------------------------ sensitivity

SENSITIVITY = {  # switch -> (the kinds it may move, the least factor it must reach: 5 GPU bounds)
    "right_side": ("nll", "cdf"),
    "plain_end_nll": ("nll",),
    "linear_end_pi": ("pi",),
    "drop_partial_ei": ("ei",),
    "mean_in_last_square": ("mean_of_square",),
}


@pytest.mark.parametrize("switch", SENSITIVITY)
def test_sensitivity_of_the_float64_yardstick(switch):
    """Each plausible kernel mistake, made in the float64 restatement, moves some output by at least 5 of the GPU
    test's bounds ``max(2 d_ref, 64 x 2^-24)`` (natural units, ``d_ref`` from the fixtures) in every bar count of the
    grid's small and mid sizes.  Measured factors (moved / bound) at B = 3 / 37 / 257 / 1025:
    a target on a border taken into the bucket to its right inf (it lands in a -inf bar) / 1.5e+05 / 6.7e+04 / 7.0e+04;
    the half-normal term dropped from an end bucket's nll 8.8e+04 / 5.0e+04 / 4.1e+04 / 3.8e+04;
    ``cdf``'s linear end buckets in ``pi`` 9.6e+04 / 3.5e+03 / 5.1e+02 / 1.3e+02;
    the partial bucket's ``(r - f)^2 / (2 w)`` dropped from ``ei`` 3.3e+04 / 6.8e+02 / 7.8e+01 / 8.8e+01;
    the last bucket's mean of squares with the half-normal's mean ("fixed") 2.1e+06 / 1.2e+04 / 6.0e+01 / 2.4e+01
    (the end buckets' weight shrinks with the bar count, and the shifted borders' fixtures carry a large ``d_ref``)."""
    factors = []
    for B in (3, 37, 257, 1025):
        z = fixture(B)
        best = 0.0
        for case in bc.cases(B):
            limit = case["name"] == "zero_width"
            a = bc.score(case, torch.float64, zero_width_limit=limit)
            b = bc.score(case, torch.float64, zero_width_limit=limit, **{switch: True})
            for k in KINDS:
                moved = bc.deviation(k, case, b[k], a[k])
                if k not in SENSITIVITY[switch]:
                    assert moved == 0.0, (switch, B, case["name"], k)
                    continue
                bound = max(2 * bc.deviation(k, case, torch.from_numpy(z[f"{case['name']}_{k}"]), a[k]), PROB_FLOOR)
                best = max(best, moved / bound)
        factors.append(best)
        assert best >= 5, (switch, B, best)
    report(f"bar score sensitivity {switch}: moved / bound per B = 3, 37, 257, 1025: "
           + ", ".join(f"{f:.1e}" for f in factors))


# ------------------------------------------------------------------------------------------------ codegen


@pytest.mark.skipif(not Path(HIPCC).exists(), reason="hipcc not available")
def test_scoring_kernels_use_no_scratch():
    """``bar_score_kernel`` and every ``bar_head_kernel`` instantiation (``SCORE`` on and off), NV = 1, 2, 5, 8: no
    VGPR spills and no private segment."""
    res = _resources("barhead.hip")
    hits = {k: v for k, v in res.items() if "bar_score_kernel" in k or "bar_head_kernel" in k}
    assert len(hits) == 12 and sum("Lb1E" in k for k in hits) == 4, sorted(hits)
    assert max(hits.values()) == 0, hits
    import re

    sizes = re.findall(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size: (\d+)", _asm("barhead.hip"))
    sizes = {n: int(v) for n, v in sizes if "bar_" in n}
    assert len(sizes) == 12 and not any(sizes.values()), sizes
