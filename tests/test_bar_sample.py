"""CPU: the yardsticks of the device sampling (``mmpfn_bar_sample``) -- the generator's restatement against Random123's
known answers, the float32 restatement of a draw against the reference's ``icdf`` (``FullSupportBarDistribution.
_icdf_at``, pinned to the reference's ``sample`` by ``test_bar_score``), the float64 restatement against the measure
it is judged by, what three planted mistakes are worth in that measure, what the library refuses without a context,
and the sampling kernel's code generation."""

import re
from pathlib import Path

import numpy as np
import pytest
import torch

import bar_sample_cases as sc
import bar_score_cases as bc
import regression_oracle as ro
from helpers import report
from test_codegen import HIPCC, _asm, _resources
from test_regression_head import PROB_FLOOR

from multimodalpfn_amd import _lib
from multimodalpfn_amd.bar_distribution import FullSupportBarDistribution

KNOWN_ANSWERS = [  # Random123 kat_vectors, philox4x32 10: counter, key -> output
    ([0, 0, 0, 0], [0, 0], [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]),
    ([0xFFFFFFFF] * 4, [0xFFFFFFFF] * 2, [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]),
    ([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], [0xA4093822, 0x299F31D0],
     [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]),
]


def _philox_ints(counter, key):
    """Philox4x32-10 on Python integers, written apart from the numpy restatement."""
    c0, c1, c2, c3 = counter
    k0, k1 = key
    for r in range(10):
        if r:
            k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & 0xFFFFFFFF, (p0 >> 32) ^ c3 ^ k1, p0 & 0xFFFFFFFF
    return [c0, c1, c2, c3]


def test_philox_restatement_gives_the_known_answers():
    for counter, key, out in KNOWN_ANSWERS:
        assert sc.philox4x32_10(counter, key).tolist() == out
        assert _philox_ints(counter, key) == out
    rng = np.random.default_rng(11)
    counters = rng.integers(0, 2 ** 32, size=(64, 4), dtype=np.uint64).astype(np.uint32)
    keys = rng.integers(0, 2 ** 32, size=(64, 2), dtype=np.uint64).astype(np.uint32)
    got = sc.philox4x32_10(counters, keys)
    for c, k, g in zip(counters.tolist(), keys.tolist(), got.tolist()):
        assert _philox_ints(c, k) == g


def test_levels_are_odd_multiples_inside_the_open_interval():
    """The mapping's ends and exactness, and ``levels``' addressing: draw J reads word J & 3 of block J >> 2 of its
    row, whatever the call's first draw."""
    u = sc.level_of_word(np.array([0, 0x1FF, 0x200, 0xFFFFFFFF], dtype=np.uint32))
    assert u.dtype == np.float32 and u.tolist() == [2.0 ** -24, 2.0 ** -24, 3 * 2.0 ** -24, 1 - 2.0 ** -24]
    seed, first = 0x9E3779B97F4A7C15, 2 ** 34 - 3
    got = sc.levels(seed, 3, first, 11)
    assert got.shape == (3, 11) and got.min() >= sc.LEVEL_MIN and got.max() <= sc.LEVEL_MAX
    for q in range(3):
        for j in (0, 2, 3, 10):
            J = first + j
            words = _philox_ints([(J >> 2) & 0xFFFFFFFF, J >> 34, q, 0], [seed & 0xFFFFFFFF, seed >> 32])
            assert got[q, j] == np.float32((2 * (words[J & 3] >> 9) + 1) * 2.0 ** -24)
    assert np.array_equal(sc.levels(seed, 3, first + 5, 6), got[:, 5:])


@pytest.mark.parametrize("B", bc.BARS)
def test_float32_restatement_is_the_reference_icdf(B):
    """Without the clamps and with linear tails ``draw`` in float32 is ``_icdf_at`` bit for bit; with the clamps it
    differs only where one of them acts."""
    acted = total = 0
    for v, case in enumerate(bc.cases(B)):
        u = sc.supplied_levels(case, v)
        crit = FullSupportBarDistribution(torch.from_numpy(case["borders"]))
        t = case["temperature"]
        logits = case["logits"] if t == 1 else case["logits"] / t
        with ro.fixture_threads():
            ref = torch.stack([crit._icdf_at(logits, u[:, j].contiguous()) for j in range(u.shape[1])], -1)
            plain = sc.draw(case["logits"], case["borders"], u, "linear", torch.float32, temperature=t, clamps=False)
            kept, acts = sc.draw(case["logits"], case["borders"], u, "linear", torch.float32, temperature=t,
                                 with_acts=True)
        assert plain.dtype == torch.float32 and torch.equal(plain.view(torch.int32), ref.view(torch.int32)), (B, case["name"])
        assert torch.equal(kept[~acts].view(torch.int32), ref[~acts].view(torch.int32)), (B, case["name"])
        b = case["borders"]
        assert torch.isfinite(kept).all() and kept.min() >= b[0] and kept.max() <= b[-1], (B, case["name"])
        acted += int(acts.sum())
        total += acts.numel()
    print(f"bar sample B={B}: a clamp acts at {acted} of {total} draws")


@pytest.mark.parametrize("B", bc.BARS)
def test_float64_restatement_meets_its_own_measure(B):
    """The float64 draws are finite, inside the borders (linear) and at most 1e-10 from their levels in
    probability."""
    for v, case in enumerate(bc.cases(B)):
        u = sc.supplied_levels(case, v)
        for tails in sc.TAILS:
            y = sc.draw(case["logits"], case["borders"], u, tails, torch.float64, temperature=case["temperature"])
            assert torch.isfinite(y).all(), (B, case["name"], tails)
            if tails == "linear":
                assert y.min() >= case["borders"][0] and y.max() <= case["borders"][-1]
            err = sc.worst(sc.prob_error(case, y, u, tails))
            print(f"bar sample B={B} {case['name']} {tails}: float64 restatement prob_error {err:.2e}")
            assert err <= 1e-10, (B, case["name"], tails, err)


@pytest.mark.parametrize("mistake", sc.MISTAKES)
def test_sensitivity_of_the_measure(mistake):
    """Each planted mistake, made in the float64 restatement, moves the measure by at least 5 of the GPU test's
    bounds ``max(2 d_ref, 64 x 2^-24)`` in every case of the bar counts up to 257 (the sampling temperature: in the
    ``shifted`` cases, the ones that have one).  Measured here (moved, against bounds of 3.8e-6 .. 1.3e-3): the
    search on the exclusive sums 0.5 .. 1.0; the rest not divided by the bar's weight 0.06 .. 0.25; the temperature
    ignored 1.3e-2 .. 3.7e-2."""
    factors = []
    for B in (b for b in bc.BARS if b <= 257):
        for v, case in enumerate(bc.cases(B)):
            if mistake == "temperature_ignored" and case["temperature"] == 1:
                continue
            u = sc.supplied_levels(case, v)
            bound = max(2 * sc.reference_error(case, u, "linear"), PROB_FLOOR)
            y = sc.draw(case["logits"], case["borders"], u, "linear", torch.float64, temperature=case["temperature"],
                        mistake=mistake)
            moved = sc.worst(sc.prob_error(case, y, u, "linear"))
            print(f"bar sample sensitivity {mistake} B={B} {case['name']}: moved {moved:.2e} bound {bound:.2e}")
            factors.append(moved / bound)
            assert moved >= 5 * bound, (mistake, B, case["name"], moved, bound)
    report(f"bar sample sensitivity {mistake}: moved / bound over B <= 257 from {min(factors):.1e} to {max(factors):.1e}")


def test_library_refuses_bar_sample_without_context():
    lib = _lib.load_library()
    assert lib.mmpfn_bar_sample(None, None, 1, 2, 1.0, None, None, 0, None, 0, 0, 1, None, None) == _lib.MMPFN_ERR_INVALID
    assert _lib.BAR_MAX_DRAWS >= 2 ** 20 and _lib.BAR_MAX_DRAWS % _lib.BAR_SAMPLE_CHUNK == 0


@pytest.mark.skipif(not Path(HIPCC).exists(), reason="hipcc not available")
def test_sampling_kernel_uses_no_scratch():
    """Every ``bar_sample_kernel`` instantiation, NV = 1, 2, 5, 8: no VGPR spills and no private segment."""
    res = _resources("barsample.hip")
    hits = {k: v for k, v in res.items() if "bar_sample_kernel" in k}
    assert len(hits) == 4 and max(hits.values()) == 0, res
    sizes = re.findall(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size: (\d+)", _asm("barsample.hip"))
    sizes = {n: int(v) for n, v in sizes if "bar_sample_kernel" in n}
    assert len(sizes) == 4 and not any(sizes.values()), sizes
