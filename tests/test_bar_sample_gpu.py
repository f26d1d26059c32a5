"""GPU: draws from the bar distribution on the device -- ``mmpfn_bar_sample`` alone and through ``MMPFNRegressor``.

A draw is judged in probability space (``bar_sample_cases.prob_error``: the distance of its level from the float64
CDF of its row at the draw -- the head test's "quantiles in probability space", per draw).  Per case the bound is the
head's and the scores' rule ``max(2 d_ref, 64 x 2^-24)``: ``d_ref`` is the same measure of the reference's float32
arithmetic on the same inputs (``_icdf_at`` for the linear form; for the half-normal form, which the reference has
no ``sample`` for, the float32 restatement built from the reference's pieces), the factor 2 for two float32
evaluations in different orders, the floor ``aggregate_kernel``'s bound on a probability.
"""

import time

import numpy as np
import pytest
import torch

import bar_sample_cases as sc
import bar_score_cases as bc
import regression_oracle as ro
from helpers import report
from test_bar_score_gpu import _engine, _fit, _same, _tables
from test_regression_head import PROB_FLOOR
from test_regression_host import api_case

from multimodalpfn_amd import _lib
from multimodalpfn_amd.bar_distribution import FullSupportBarDistribution

pytestmark = pytest.mark.gpu

CHUNK = _lib.BAR_SAMPLE_CHUNK
TAIL_CODES = {"linear": 0, "halfnormal": 1}


def _raw_sample(eng, logits, Q, B, inv_t, tabs, tails, uniforms, seed, first, n, out, u_out, *, ends=True):
    """The C entry point on device tensors (``None``: a NULL pointer)."""
    eng._bind_stream()
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    rc = eng.lib.mmpfn_bar_sample(eng.ctx, p(logits), Q, B, inv_t, p(tabs["borders"]), p(tabs["ends"]) if ends else None,
                                  tails, p(uniforms), seed, first, n, p(out), p(u_out))
    torch.cuda.synchronize()
    return rc


# ------------------------------------------------------------------------------------------------ 1. levels


def test_generated_levels_are_the_philox_restatement():
    """The block counter carries into its high word inside the call: draws 2^34 - 3 .. 2^34 + 1027."""
    eng = _engine()
    case = bc.cases(37)[0]
    seed, first, n = 0x9E3779B97F4A7C15, 2 ** 34 - 3, 1030
    y, u = eng.bar_sample(case["logits"].cuda(), _tables(case["borders"]), n, seed=seed, first_draw=first,
                          return_uniforms=True)
    assert y.shape == (3, n) and u.shape == (3, n) and u.dtype == torch.float32
    assert torch.equal(u.cpu(), torch.from_numpy(sc.levels(seed, 3, first, n)))
    assert float(u.min()) >= sc.LEVEL_MIN and float(u.max()) <= sc.LEVEL_MAX


# ------------------------------------------------------------------------------------------------ 2. draws vs float64


@pytest.mark.parametrize("tails", sc.TAILS)
@pytest.mark.parametrize("B", bc.BARS)
def test_draws_match_float64_in_probability(B, tails):
    eng = _engine()
    worst = (0.0, 1.0, 0.0)
    for v, case in enumerate(bc.cases(B)):
        u = sc.supplied_levels(case, v)
        y, used = eng.bar_sample(case["logits"].cuda(), _tables(case["borders"]), u.shape[1], uniforms=u.cuda(),
                                 temperature=case["temperature"], tails=tails, return_uniforms=True)
        y = y.cpu()
        assert torch.equal(used.cpu(), u)  # levels inside the range pass through the clamp
        assert y.shape == u.shape and torch.isfinite(y).all(), (B, case["name"])
        if tails == "linear":
            assert float(y.min()) >= case["borders"][0] and float(y.max()) <= case["borders"][-1], (B, case["name"])
        err = sc.worst(sc.prob_error(case, y, u, tails))
        d_ref = sc.reference_error(case, u, tails)
        bound = max(2 * d_ref, PROB_FLOOR)
        print(f"bar sample B={B} {case['name']} {tails}: err {err:.2e} d_ref {d_ref:.2e} bound {bound:.2e}")
        if err / bound >= worst[0] / worst[1]:
            worst = (err, bound, d_ref)
        assert err <= bound, (B, case["name"], tails, err, bound)
    report(f"bar sample B={B} {tails}: worst error / bound {worst[0]:.2e} / {worst[1]:.2e} (d_ref {worst[2]:.2e})")


@pytest.mark.parametrize("tails", sc.TAILS)
def test_nan_levels_and_dead_rows_give_nan_and_nothing_else(tails):
    """A NaN level gives a NaN draw (and comes back as the level used); levels outside the range are clamped into it;
    a row of all -inf gives NaN draws, and its neighbours' draws keep their bits."""
    eng = _engine()
    case = bc.cases(257)[0]
    tabs = _tables(case["borders"])
    u = sc.supplied_levels(case, 0).clone()
    lg = case["logits"].cuda()
    plain = eng.bar_sample(lg, tabs, u.shape[1], uniforms=u.cuda(), tails=tails)
    odd = u.clone()
    odd[:, 5] = float("nan")
    odd[:, 6], odd[:, 7], odd[:, 8], odd[:, 9] = 0.0, 1.0, -3.0, float("inf")
    y, used = eng.bar_sample(lg, tabs, u.shape[1], uniforms=odd.cuda(), tails=tails, return_uniforms=True)
    assert torch.isnan(y[:, 5]).all() and torch.isnan(used[:, 5]).all()
    want = odd.clone()
    want[:, 6], want[:, 7], want[:, 8], want[:, 9] = sc.LEVEL_MIN, sc.LEVEL_MAX, sc.LEVEL_MIN, sc.LEVEL_MAX
    keep = [j for j in range(u.shape[1]) if j != 5]
    assert torch.equal(used[:, keep].cpu(), want[:, keep])
    assert _same(y[:, 6], plain[:, 0]) and _same(y[:, 7], plain[:, 1]) and _same(y[:, 8], plain[:, 0])
    assert _same(y[:, 10:], plain[:, 10:]) and torch.isfinite(y[:, keep]).all()
    dead = case["logits"].clone()
    dead[1] = float("-inf")
    y = eng.bar_sample(dead.cuda(), tabs, u.shape[1], uniforms=u.cuda(), tails=tails)
    assert torch.isnan(y[1]).all() and _same(y[0], plain[0]) and _same(y[2], plain[2])
    seeded = eng.bar_sample(dead.cuda(), tabs, CHUNK + 3, seed=5, tails=tails)
    assert torch.isnan(seeded[1]).all() and torch.isfinite(seeded[0]).all() and torch.isfinite(seeded[2]).all()


# ------------------------------------------------------------------------------------------------ 3. one definition


@pytest.mark.parametrize("B", [37, 5000])
def test_a_draw_depends_on_seed_row_and_index_alone(B):
    """n on both sides of a wave, a block's stride and a chunk: the seeded call is, bit for bit, the call on its own
    levels, the two calls of a split at an odd first draw, and the leading columns of a longer call."""
    eng = _engine()
    case = bc.cases(B)[1]
    tabs = _tables(case["borders"])
    lg = case["logits"].cuda()
    seed, first = 0xC0FFEE1234, 6
    kw = dict(seed=seed, temperature=case["temperature"], tails="halfnormal")
    counts = (1, 255, 256, 257, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 5)
    longest, longest_u = eng.bar_sample(lg, tabs, counts[-1], first_draw=first, return_uniforms=True, **kw)
    assert torch.equal(longest_u.cpu(), torch.from_numpy(sc.levels(seed, 3, first, counts[-1])))
    for n in counts:
        y, u = eng.bar_sample(lg, tabs, n, first_draw=first, return_uniforms=True, **kw)
        assert y.shape == (3, n) and _same(y, longest[:, :n]) and _same(u, longest_u[:, :n]), (B, n)
        again = eng.bar_sample(lg, tabs, n, uniforms=u, temperature=case["temperature"], tails="halfnormal")
        assert _same(again, y), (B, n)
        k = min(n, 129)  # the second call starts at the odd draw first + k
        head = eng.bar_sample(lg, tabs, k, first_draw=first, **kw)
        tail = eng.bar_sample(lg, tabs, n - k, first_draw=first + k, **kw)
        assert tail.shape == (3, n - k) and _same(torch.cat([head, tail], 1), y), (B, n)


# ------------------------------------------------------------------------------------------------ 4. surroundings


@pytest.mark.parametrize("B", [37, 5000])
def test_bar_sample_touches_nothing_beyond_its_arrays(B):
    """Draws, levels used, supplied levels and the logits rows inside NaN-filled allocations, at an offset that
    misaligns them by 4 bytes and at one that aligns them: the guard words keep their bit pattern and the results are
    the plain call's."""
    eng = _engine()
    n = CHUNK + 7
    for v, case in enumerate(bc.cases(B)[:2]):
        tabs = {k: t.cuda() for k, t in _tables(case["borders"]).items()}
        lg = case["logits"].cuda()
        Q = lg.shape[0]
        inv_t = 1.0 / case["temperature"]
        u = torch.from_numpy(sc.levels(77 + v, Q, 3, n)).cuda()
        for tails in sc.TAILS:
            plain = eng.bar_sample(lg, tabs, n, uniforms=u, temperature=case["temperature"], tails=tails)
            for off in (1, 4):
                sizes = {"logits": Q * B, "uniforms": Q * n, "out": Q * n, "u_out": Q * n}
                bufs = {k: torch.full((m + 64,), float("nan")).cuda() for k, m in sizes.items()}
                views = {k: bufs[k][off:off + m] for k, m in sizes.items()}
                views["logits"].copy_(lg.reshape(-1))
                views["uniforms"].copy_(u.reshape(-1))
                before = {k: b.view(torch.int32).clone() for k, b in bufs.items()}
                rc = _raw_sample(eng, views["logits"], Q, B, inv_t, tabs, TAIL_CODES[tails], views["uniforms"], 0, 0, n,
                                 views["out"], views["u_out"])
                assert rc == _lib.MMPFN_OK
                for k, m in sizes.items():
                    after = bufs[k].view(torch.int32)
                    assert torch.equal(after[:off], before[k][:off]) and torch.equal(after[off + m:], before[k][off + m:]), k
                    if k in ("logits", "uniforms"):
                        assert torch.equal(after, before[k]), k
                assert _same(views["out"].reshape(Q, n), plain), (B, case["name"], tails, off)
                assert _same(views["u_out"].reshape(Q, n), u), (B, case["name"], tails, off)


# ------------------------------------------------------------------------------------------------ 5. refusals


def test_bar_sample_refuses_what_the_kernel_does_not_hold():
    eng = _engine()
    B = 16
    borders = (torch.from_numpy(ro.normal_borders(B)) * 2.5 + 1.0).float().numpy()
    tabs = {k: v.cuda() for k, v in _tables(borders).items()}
    lg = torch.zeros(2, B).cuda()
    big = _lib.BAR_MAX_BARS + 1
    wide = torch.zeros(1, big).cuda()
    for bad in (dict(logits=wide), dict(logits=torch.zeros(2, 1).cuda()), dict(n=-1), dict(n=_lib.BAR_MAX_DRAWS + 1),
                dict(temperature=0.0), dict(temperature=-1.0), dict(tails="normal"), dict(tails=2),
                dict(uniforms=torch.zeros(2, 3))):
        kw = dict(logits=lg, n=4) | bad
        with pytest.raises(ValueError):
            eng.bar_sample(kw.pop("logits"), tabs, kw.pop("n"), **kw)
    with pytest.raises(ValueError):
        eng.bar_sample(lg, {"borders": tabs["borders"][:-1]}, 4)
    out, u_out = torch.zeros(2 * 8).cuda(), torch.zeros(2 * 8).cuda()
    raw = lambda **k: _raw_sample(eng, **(dict(logits=lg, Q=2, B=B, inv_t=1.0, tabs=tabs, tails=0, uniforms=None,  # noqa: E731
                                               seed=1, first=0, n=8, out=out, u_out=u_out) | k))
    assert raw() == _lib.MMPFN_OK
    assert raw(B=big) == _lib.MMPFN_ERR_INVALID and raw(B=1) == _lib.MMPFN_ERR_INVALID
    assert raw(n=-1) == _lib.MMPFN_ERR_INVALID and raw(n=_lib.BAR_MAX_DRAWS + 1) == _lib.MMPFN_ERR_INVALID
    assert raw(inv_t=0.0) == _lib.MMPFN_ERR_INVALID and raw(inv_t=-2.0) == _lib.MMPFN_ERR_INVALID
    assert raw(inv_t=float("nan")) == _lib.MMPFN_ERR_INVALID
    assert raw(tails=2) == _lib.MMPFN_ERR_INVALID and raw(tails=-1) == _lib.MMPFN_ERR_INVALID
    assert raw(out=None) == _lib.MMPFN_ERR_INVALID
    assert raw(tails=1, ends=False) == _lib.MMPFN_ERR_INVALID  # half-normal tails need their scales
    assert raw(logits=None) == _lib.MMPFN_ERR_INVALID
    assert raw(ends=False, u_out=None) == _lib.MMPFN_OK  # linear tails read no ends; the levels need not be stored
    assert raw(Q=0) == _lib.MMPFN_OK and raw(n=0) == _lib.MMPFN_OK and raw(n=0, out=None) == _lib.MMPFN_OK
    empty = eng.bar_sample(lg, tabs, 0)
    assert empty.shape == (2, 0)
    assert eng.bar_sample(torch.zeros(0, B).cuda(), tabs, 5).shape == (0, 5)


# ------------------------------------------------------------------------------------------------ 6. end to end


def test_regressor_samples_end_to_end(tmp_path):
    """``sample_device`` with supplied levels is ``HipEngine.bar_sample`` on the ``full`` logits with the criterion's
    tables, bit for bit, for both tails and two sampling temperatures; a ``random_state`` fixes the draws."""
    case, z = api_case("b100")
    reg, d = _fit(case, tmp_path, case["variants"][0])
    Q, n = case["Q"], 300
    X = d["X_test"]
    full = reg.predict(X, None, output_type="full")
    crit = full["criterion"]
    tabs = {**crit.head_tables(), **crit.score_tables()}
    u = torch.from_numpy(sc.levels(9, Q, 0, n))
    eng = reg.model_.engine(reg.sample_device(X, None).device)
    lo, hi = float(crit.borders[0]), float(crit.borders[-1])
    for tails in sc.TAILS:
        for t in (1.0, 0.8):
            got = reg.sample_device(X, None, n, uniforms=u, temperature=t, tails=tails)
            want = eng.bar_sample(full["logits"], tabs, n, uniforms=u, temperature=t, tails=tails)
            assert got.is_cuda and got.shape == (Q, n) and _same(got, want), (tails, t)
            assert torch.isfinite(got).all()
            if tails == "linear":
                assert float(got.min()) >= lo and float(got.max()) <= hi
    a = reg.sample(X, None, n, random_state=7)
    assert isinstance(a, np.ndarray) and a.dtype == np.float32 and a.shape == (Q, n)
    assert np.array_equal(a, reg.sample(X, None, n, random_state=7))
    assert not np.array_equal(a, reg.sample(X, None, n, random_state=8))
    assert np.array_equal(a, reg.sample(X, None, n, random_state=np.random.default_rng(7)))
    assert reg.sample(X, None).shape == (Q, 1)
    # a coarse check of scale and sign: half of a row's draws lie below the head's median (n = 4000: 6 standard
    # deviations of the fraction are 0.047)
    below = (reg.sample(X, None, 4000, random_state=1) <= full["median"][:, None]).mean(1)
    assert (np.abs(below - 0.5) <= 0.047).all(), below


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_regressor_samples_16bit_modes_report(dtype, tmp_path):
    """The 16-bit modes sample end to end; how far their draws lie from the fp32 mode's at the same levels is
    reported, not bounded."""
    case, z = api_case("b100")
    reg32, d = _fit(case, tmp_path, case["variants"][0])
    reg, _ = _fit(case, tmp_path, case["variants"][0], inference_precision=dtype)
    u = torch.from_numpy(sc.levels(3, case["Q"], 0, 64))
    got = reg.sample(d["X_test"], None, 64, uniforms=u)
    ref = reg32.sample(d["X_test"], None, 64, uniforms=u)
    span = float(z["crit_borders"][-2] - z["crit_borders"][1])
    off = float(np.abs(got - ref).max()) / span
    report(f"regressor b100 {dtype}: draws off the fp32 mode's at the same levels by {off:.3e} of the inner borders' span")
    assert got.shape == (case["Q"], 64) and np.isfinite(got).all() and np.isfinite(off)


# ------------------------------------------------------------------------------------------------ 7. time, reported


def test_bar_sample_time_report():
    """HIP-event time of one call at Q = 460, B = 5000, beside the host route to the same draws without the kernel:
    the logits copied to the host and ``_icdf_at`` once per column of levels (timed over 4 columns, scaled to n)."""
    eng = _engine()
    Q, B = 460, 5000
    g = torch.Generator().manual_seed(17)
    borders = (torch.from_numpy(ro.normal_borders(B)) * 2.5 + 1.0).float()
    lg = (2.0 * torch.randn(Q, B, generator=g)).cuda()
    tabs = {k: v.cuda() for k, v in _tables(borders.numpy()).items()}
    crit = FullSupportBarDistribution(borders)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    host = lg.cpu()
    cols = 4
    levels = torch.from_numpy(sc.levels(1, Q, 0, cols))
    for j in range(cols):
        crit._icdf_at(host, levels[:, j].contiguous())
    per_column = (time.perf_counter() - t0) / cols
    for n in (1024, 65536):
        eng.bar_sample(lg, tabs, n, seed=1)  # warm-up
        best = float("inf")
        for _ in range(3):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            y = eng.bar_sample(lg, tabs, n, seed=1)
            stop.record()
            stop.synchronize()
            best = min(best, start.elapsed_time(stop))
        assert y.shape == (Q, n) and bool(torch.isfinite(y[:, ::97]).all())
        report(f"bar sample Q={Q} B={B} n={n}: device call {best:.3f} ms ({Q * n / best / 1e6:.2f} G draws/s); host "
               f"_icdf_at on the copied logits {per_column * 1e3:.1f} ms per column of levels, {per_column * n:.1f} s "
               f"for n columns (scaled from {cols})")
