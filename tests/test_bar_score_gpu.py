"""GPU: the bar distribution's scores on the device -- ``mmpfn_bar_score`` alone, fused into the head
(``mmpfn_bar_head_score``), and through ``MMPFNRegressor``.

Bounds of ``mmpfn_bar_score`` against the float64 restatement (``bar_score_cases.score``), per element, the head
test's rule ``max(2 d_ref, floor)``: ``d_ref`` is the reference fixture's own float32 deviation from float64 for that
kind and case, the floor the project's ``PROB_FLOOR`` = 64 x 2^-24 in each kind's natural unit
(``bar_score_cases.natural_unit``): ``cdf`` / ``pi`` absolute; ``nll`` of ``max(1, |ref64|)``; ``ei`` of the span of the
criterion's inner borders; ``mean_of_square`` of the largest squared border.  Where float64 is infinite (a target in
a -inf bar) the output is that infinity; at the NaN target ``nll`` is 0 and the other kinds are NaN (this project's
definition: the reference asserts or has no rule).  With an empty interior bucket the reference's ``ei`` is 0 / 0 =
NaN for every row; the device gives the bucket its limit, and the yardstick there is the restatement with
``zero_width_limit`` (``d_ref`` counts as 0).
"""

import numpy as np
import pytest
import torch

import bar_score_cases as bc
import regression_oracle as ro
from helpers import GOLDEN, rel_err, report
from test_regression_head import PROB_FLOOR
from test_regression_host import api_case, write_ckpt

from multimodalpfn_amd import MMPFNRegressor, _lib
from multimodalpfn_amd.bar_distribution import FullSupportBarDistribution, border_tables

pytestmark = pytest.mark.gpu

KINDS = ("nll", "cdf", "pi", "ei", "mean_of_square")
TABLE_KEYS = ("borders", "widths", "log_widths", "mean_squares", "ei_mids", "ends")
_ENGINE: list = []


def _engine():
    from synth import synth_state_dict

    from multimodalpfn_amd.engine import HipEngine
    from multimodalpfn_amd.model.spec import ModelConfig, state_dict_spec

    if not _ENGINE:
        cfg = ModelConfig(nlayers=1, mgm_heads=2, cap_heads=2)
        _ENGINE.append(HipEngine(cfg, synth_state_dict(state_dict_spec(cfg), 23), torch.device("cuda")))
    return _ENGINE[0]


def _tables(borders) -> dict:
    crit = FullSupportBarDistribution(torch.as_tensor(borders))
    return {**crit.head_tables(), **crit.score_tables()}


def _same(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Bit for bit (NaNs included)."""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _raw_score(eng, logits, Q, B, inv_t, tabs, ys, J, outs):
    """The C entry point on device tensors (``None``: a NULL pointer); ``outs`` in ``KINDS`` order."""
    eng._bind_stream()
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    rc = eng.lib.mmpfn_bar_score(eng.ctx, p(logits), Q, B, inv_t, *(p(tabs[k]) for k in TABLE_KEYS), p(ys), J,
                                 *(p(o) for o in outs))
    torch.cuda.synchronize()
    return rc


# ------------------------------------------------------------------------------------------------ 1. alone, vs float64


@pytest.mark.parametrize("B", bc.BARS)
def test_bar_score_matches_float64_restatement(B):
    eng = _engine()
    z = np.load(GOLDEN / "bar_score" / f"score_B{B}.npz")
    worst = {k: (0.0, 1.0) for k in KINDS}
    for case in bc.cases(B):
        name = case["name"]
        r64 = bc.score(case, torch.float64, zero_width_limit=name == "zero_width")
        got = eng.bar_score(case["logits"].cuda(), _tables(case["borders"]), case["ys"].cuda(),
                            softmax_temperature=case["temperature"])
        got = {k: v.cpu() for k, v in got.items()}
        assert got["mean_of_square"].shape == (3,) and all(got[k].shape == (3, bc.N_TARGETS) for k in bc.PER_TARGET)
        assert (got["nll"][:, 0] == 0).all() and all(torch.isnan(got[k][:, 0]).all() for k in ("cdf", "pi", "ei"))
        for k in KINDS:
            g = got[k] if k in ("nll", "mean_of_square") else got[k][:, 1:]
            ref = r64[k]
            fix = torch.from_numpy(z[f"{name}_{k}"]).double()
            inf = torch.isinf(ref)
            assert torch.equal(g[inf].double(), ref[inf]), (B, name, k)
            assert torch.isfinite(g[~inf]).all() and not torch.isnan(ref).any(), (B, name, k)
            unit = bc.natural_unit(k, case, ref)
            unit = unit[~inf] if torch.is_tensor(unit) else unit
            err = float(((g.double() - ref)[~inf].abs() / unit).max())
            d_ref = 0.0 if torch.isnan(fix).all() else float(((fix - ref)[~inf].abs() / unit).max())
            bound = max(2 * d_ref, PROB_FLOOR)
            print(f"bar score B={B} {name} {k}: err {err:.2e} d_ref {d_ref:.2e} bound {bound:.2e}")
            if err / bound >= worst[k][0] / worst[k][1]:
                worst[k] = (err, bound)
            assert err <= bound, (B, name, k, err, bound)
    report(f"bar score B={B}: worst error / bound -- " + ", ".join(f"{k} {e:.2e} / {b:.2e}" for k, (e, b) in worst.items()))


# ------------------------------------------------------------------------------------------------ 2. surroundings


@pytest.mark.parametrize("B", [37, 257, 5000])
def test_bar_score_touches_nothing_beyond_its_arrays(B):
    """Targets, every output and the logits rows inside NaN-filled allocations, at an offset that misaligns them by
    4 bytes and at one that aligns them: the guard words keep their bit pattern and the results are the plain call's."""
    eng = _engine()
    for case in bc.cases(B)[:2]:
        tabs = {k: v.cuda() for k, v in _tables(case["borders"]).items()}
        lg, ys = case["logits"].cuda(), case["ys"].cuda()
        Q, J = ys.shape
        inv_t = 1.0 / case["temperature"]
        plain = eng.bar_score(lg, tabs, ys, softmax_temperature=case["temperature"])
        for off in (1, 4):
            sizes = {"logits": Q * B, "ys": Q * J, **{k: Q * J for k in bc.PER_TARGET}, "mean_of_square": Q}
            bufs = {k: torch.full((n + 64,), float("nan")).cuda() for k, n in sizes.items()}
            views = {k: bufs[k][off:off + n] for k, n in sizes.items()}
            views["logits"].copy_(lg.reshape(-1))
            views["ys"].copy_(ys.reshape(-1))
            before = {k: b.view(torch.int32).clone() for k, b in bufs.items()}
            rc = _raw_score(eng, views["logits"], Q, B, inv_t, tabs, views["ys"], J, [views[k] for k in KINDS])
            assert rc == _lib.MMPFN_OK
            for k, n in sizes.items():
                after = bufs[k].view(torch.int32)
                assert torch.equal(after[:off], before[k][:off]) and torch.equal(after[off + n:], before[k][off + n:]), k
                if k in KINDS:
                    assert _same(views[k].reshape(plain[k].shape), plain[k]), (B, case["name"], off, k)
                else:
                    assert torch.equal(after, before[k]), k


# ------------------------------------------------------------------------------------------------ 3. J


def _many_targets(borders: np.ndarray, Q: int, J: int, seed: int) -> torch.Tensor:
    """Targets all over the borders' span and beyond, one NaN per row, some exactly on borders."""
    g = torch.Generator().manual_seed(seed)
    lo, hi = float(borders[0]), float(borders[-1])
    ys = lo - 0.1 * (hi - lo) + 1.2 * (hi - lo) * torch.rand(Q, J, generator=g)
    on = torch.randint(0, len(borders), (Q, J // 4), generator=g)
    ys[:, : J // 4] = torch.from_numpy(borders)[on]
    ys[:, -1] = float("nan")
    return ys[:, torch.randperm(J, generator=g)].contiguous()


@pytest.mark.parametrize("B", [37, 2049])
def test_bar_score_any_target_count_and_null_outputs(B):
    """J = 1, 9, 64 give the matching columns of the J = 64 call bit for bit; so does every call with one output
    NULL; and ``mean_of_square`` alone needs no targets."""
    eng = _engine()
    case = bc.cases(B)[1]
    tabs = _tables(case["borders"])
    lg = case["logits"].cuda()
    ys = _many_targets(case["borders"], 3, _lib.BAR_MAX_TARGETS, 7 + B).cuda()
    full = eng.bar_score(lg, tabs, ys, softmax_temperature=case["temperature"])
    assert not torch.isnan(full["nll"]).any() and torch.isnan(full["ei"]).sum() == 3
    for J in (1, 9, 64):
        part = eng.bar_score(lg, tabs, ys[:, :J].contiguous(), softmax_temperature=case["temperature"])
        for k in bc.PER_TARGET:
            assert _same(part[k], full[k][:, :J]), (B, J, k)
        assert _same(part["mean_of_square"], full["mean_of_square"])
    for drop in KINDS:
        want = tuple(k for k in KINDS if k != drop)
        part = eng.bar_score(lg, tabs, ys, softmax_temperature=case["temperature"], want=want)
        assert set(part) == set(want)
        for k in want:
            assert _same(part[k], full[k]), (B, drop, k)
    only = eng.bar_score(lg, tabs, None, softmax_temperature=case["temperature"], want=("mean_of_square",))
    assert list(only) == ["mean_of_square"] and _same(only["mean_of_square"], full["mean_of_square"])


# ------------------------------------------------------------------------------------------------ 4. fused = standalone


def _head_tables(case):
    tabs = [border_tables(frm, case["std_borders"]) for frm in case["borders"]]
    cancel = None
    if any(m is not None for m in case["masks"]):
        cancel = np.stack([np.zeros(case["B"], bool) if m is None else m for m in case["masks"]])
    return np.stack([t[0] for t in tabs]), np.stack([t[1] for t in tabs]), cancel


@pytest.mark.parametrize("B", [37, 257, 5000])
def test_fused_head_scores_equal_the_standalone_kernel(B):
    """``mmpfn_bar_head_score``: mean / mode / quantiles / logits are ``mmpfn_bar_head``'s, and the scores are
    ``mmpfn_bar_score``'s on the head's own ``out_logits`` at temperature 1 -- one definition over the same floats in
    the same thread mapping -- with and without the logits output."""
    eng = _engine()
    for c, case in enumerate(ro.head_cases(B)):
        idx, share, cancel = _head_tables(case)
        crit = FullSupportBarDistribution(torch.from_numpy(case["crit_borders"]))
        lg = torch.stack(case["logits"]).cuda()
        kw = dict(cancel=cancel, softmax_temperature=case["temperature"], average_before_softmax=case["avg"],
                  quantiles=case["levels"])
        plain = eng.bar_head(lg, idx, share, crit.head_tables(), want_logits=True, **kw)
        ys = _many_targets(case["crit_borders"], case["Q"], 9, 31 * B + c).cuda()
        alone = eng.bar_score(plain["logits"], {**crit.head_tables(), **crit.score_tables()}, ys)
        for want in (True, False):
            fused = eng.bar_head(lg, idx, share, crit.head_tables(), want_logits=want, targets=ys,
                                 score_tables=crit.score_tables(), **kw)
            assert (fused["logits"] is None) == (not want)
            for k in ("mean", "mode", "quantiles") + (("logits",) if want else ()):
                assert _same(fused[k], plain[k]), (B, case["name"], want, k)
            for k in KINDS:
                assert _same(fused[k], alone[k]), (B, case["name"], want, k)


# ------------------------------------------------------------------------------------------------ 5. refusals


def test_bar_score_refuses_what_the_kernel_does_not_hold():
    eng = _engine()
    B = 16
    case_borders = (torch.from_numpy(ro.normal_borders(B)) * 2.5 + 1.0).float().numpy()
    tabs = {k: v.cuda() for k, v in _tables(case_borders).items()}
    lg = torch.zeros(2, B).cuda()
    with pytest.raises(ValueError):
        eng.bar_score(lg, tabs, torch.zeros(2, _lib.BAR_MAX_TARGETS + 1))
    with pytest.raises(ValueError):
        eng.bar_score(lg, tabs, None)  # per-target outputs without targets
    with pytest.raises(ValueError):
        eng.bar_score(lg, tabs, torch.zeros(2, 1), softmax_temperature=0.0)
    big = _lib.BAR_MAX_BARS + 1
    with pytest.raises(ValueError):
        eng.bar_score(torch.zeros(1, big).cuda(), tabs, torch.zeros(1, 1))
    idx, share = border_tables(ro.normal_borders(B), ro.normal_borders(B))
    with pytest.raises(ValueError):
        eng.bar_head(lg[None], idx[None], share[None], tabs, targets=torch.zeros(2, _lib.BAR_MAX_TARGETS + 1),
                     score_tables=tabs)
    ys, out = torch.zeros(2 * 65).cuda(), [torch.zeros(2 * 65).cuda() for _ in KINDS]
    assert _raw_score(eng, lg, 2, B, 1.0, tabs, ys, _lib.BAR_MAX_TARGETS + 1, out) == _lib.MMPFN_ERR_INVALID
    assert _raw_score(eng, lg, 2, big, 1.0, tabs, ys, 1, out) == _lib.MMPFN_ERR_INVALID
    assert _raw_score(eng, lg, 2, B, 1.0, tabs, None, 1, out) == _lib.MMPFN_ERR_INVALID
    assert _raw_score(eng, lg, 2, B, 1.0, tabs, None, 1, [None, None, out[2], None, None]) == _lib.MMPFN_ERR_INVALID
    assert _raw_score(eng, lg, 0, B, 1.0, tabs, ys, 1, out) == _lib.MMPFN_OK  # no rows
    assert _raw_score(eng, lg, 2, B, 1.0, tabs, None, 0, [None] * 4 + [out[4]]) == _lib.MMPFN_OK
    # the fused entry point refuses the same
    p = lg.data_ptr()
    head = (eng.ctx, p, 1, 2, B, None, 0, p, p, B + 1, 1.0, 0, p, p, p, p, None, 0, None, p, p, None)
    score = [tabs[k].data_ptr() for k in TABLE_KEYS[2:]]
    outs = [o.data_ptr() for o in out]
    eng._bind_stream()
    assert eng.lib.mmpfn_bar_head_score(*head, *score, ys.data_ptr(), 65, *outs) == _lib.MMPFN_ERR_INVALID
    assert eng.lib.mmpfn_bar_head_score(*head, *score, None, 1, *outs) == _lib.MMPFN_ERR_INVALID
    head0 = head[:3] + (0,) + head[4:]
    assert eng.lib.mmpfn_bar_head_score(*head0, *score, ys.data_ptr(), 1, *outs) == _lib.MMPFN_OK
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 6. end to end


def _fit(case, tmp_path, variant, **over):
    d = ro.api_case_data(case)
    path, _, _ = write_ckpt(case, tmp_path)
    reg = MMPFNRegressor(model_path=str(path), **(ro.api_regressor_kwargs(case, variant) | over))
    reg.fit(d["X_train"], None, d["y_train"])
    return reg, d


def _head_logits(z, logits, dtype):
    masks = [z[f"m{m}_cancel"] if z[f"m{m}_cancel"].any() else None for m in range(4)]
    return ro.head(logits, [z[f"m{m}_borders"].astype(np.float32) for m in range(4)], z["std_borders"], masks,
                   temperature=0.9, average_before_softmax=False, crit_borders=z["crit_borders"], levels=[0.5],
                   dtype=dtype)["logits"]


def _targets(z, Q):
    """The reference's recorded mean plus seeded noise, one entry NaN."""
    y = (z["mean_mean"] + np.random.default_rng(3).standard_normal(Q) * 0.7).astype(np.float32)
    y[Q // 2] = np.nan
    return y


def test_regressor_scores_end_to_end_fp32(tmp_path):
    """``score_samples`` against the float64 scoring of the float64 head of the reference's recorded member logits:
    ``test_regressor_end_to_end_fp32``'s rule -- twice what the 1e-4 logit band moves the value (random sign patterns
    through the float64 head and scoring) plus the scoring bound ``max(2 d_ref, floor)``, ``d_ref`` the float32
    restatement's own deviation.  ``predict_device(targets=...)`` is ``HipEngine.bar_score`` on the ``full`` logits
    bit for bit; ``acquisition`` is the host criterion's method on those logits within the scoring bound, ``ucb``
    bit for bit the quantile of its level."""
    case, z = api_case("b100")
    reg, d = _fit(case, tmp_path, case["variants"][0])
    Q = case["Q"]
    y = _targets(z, Q)
    b32 = torch.from_numpy(z["crit_borders"]).float()
    b64 = b32.double()
    ref_logits = [torch.from_numpy(z[f"m{m}_logits"]) for m in range(4)]
    y_t = torch.from_numpy(y)
    ref64 = bc.nll(_head_logits(z, ref_logits, torch.float64), b64, y_t.double())
    ref32 = bc.nll(_head_logits(z, ref_logits, torch.float32), b32, y_t).double()
    unit = ref64.abs().clamp(min=1.0)
    g = torch.Generator().manual_seed(5)
    move = 0.0
    for _ in range(4):
        pert = [lg + (torch.randint(0, 2, lg.shape, generator=g) * 2.0 - 1.0) * 1e-4 * max(1.0, float(lg.abs().max()))
                for lg in ref_logits]
        move = max(move, float(((bc.nll(_head_logits(z, pert, torch.float64), b64, y_t.double()) - ref64).abs() / unit).max()))
    got = reg.score_samples(d["X_test"], None, y)
    assert got.shape == (Q,) and got.dtype == np.float32 and got[Q // 2] == 0 and np.isfinite(got).all()
    err = float(((torch.from_numpy(got).double() + ref64).abs() / unit).max())
    d_ref = float(((ref32 - ref64).abs() / unit).max())
    bound = 2 * move + max(2 * d_ref, PROB_FLOOR)
    report(f"regressor b100 score_samples: error {err:.3e} of max(1, |ref|), bound {bound:.3e} (the logit band moves it "
           f"{move:.3e}, the float32 restatement's own error {d_ref:.3e})")
    assert err <= bound, (err, bound)

    # predict_device with targets = bar_score on the full logits
    full = reg.predict(d["X_test"], None, output_type="full", quantiles=ro.API_QUANTILES)
    crit = full["criterion"]
    ys = np.stack([y, y + 0.5, np.full(Q, 2.0, np.float32)], 1)
    dev = reg.predict_device(d["X_test"], None, targets=ys)
    eng = reg.model_.engine(dev["mean"].device)
    alone = eng.bar_score(full["logits"], {**crit.head_tables(), **crit.score_tables()}, ys)
    for k in KINDS:
        assert _same(dev[k], alone[k]), k
    assert dev["nll"].shape == (Q, 3) and dev["variance"].shape == (Q,)
    assert torch.equal(dev["variance"], dev["mean_of_square"] - dev["mean"].square())
    assert np.array_equal(dev["mean"].cpu().numpy(), full["mean"]) and (dev["variance"] > 0).all()

    # acquisition against the host criterion on the full logits
    span = float(z["crit_borders"][-2] - z["crit_borders"][1])
    best = float(np.median(z["mean_mean"]))
    lg64 = full["logits"].double()
    f64 = torch.full((Q,), best, dtype=torch.float64)
    for kind, unit_k, host, r64 in (("ei", span, crit.ei, bc.ei(lg64, b64, f64)), ("pi", 1.0, crit.pi, bc.pi(lg64, b64, f64))):
        got = torch.from_numpy(reg.acquisition(d["X_test"], None, best, kind=kind)).double()
        h32 = host(full["logits"], best).double()
        d_ref = float((h32 - r64).abs().max()) / unit_k
        bound = max(2 * d_ref, PROB_FLOOR)
        err, off_host = float((got - r64).abs().max()) / unit_k, float((got - h32).abs().max()) / unit_k
        report(f"regressor b100 acquisition {kind}: error {err:.3e}, bound {bound:.3e}; off the host method {off_host:.3e}")
        assert err <= bound and off_host <= bound + d_ref, (kind, err, off_host, bound)
        per_row = reg.acquisition(d["X_test"], None, np.full(Q, best, np.float32), kind=kind)
        assert np.array_equal(per_row, got.float().numpy())
    rest = (1 - 0.682) / 2
    ucb = reg.acquisition(d["X_test"], None, best, kind="ucb")
    level = reg.predict(d["X_test"], None, output_type="quantiles", quantiles=[1.0 - rest])[0]
    assert np.array_equal(ucb, level)
    with pytest.raises(ValueError):
        reg.acquisition(d["X_test"], None, best, kind="lcb")


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_regressor_scores_16bit_modes_report(dtype, tmp_path):
    """The 16-bit modes score end to end; their distance from the fp32 reference's scoring is reported, not bounded."""
    case, z = api_case("b100")
    reg, d = _fit(case, tmp_path, case["variants"][0], inference_precision=dtype)
    y = _targets(z, case["Q"])
    got = reg.score_samples(d["X_test"], None, y)
    ref_logits = [torch.from_numpy(z[f"m{m}_logits"]) for m in range(4)]
    ref64 = bc.nll(_head_logits(z, ref_logits, torch.float64), torch.from_numpy(z["crit_borders"]).double(),
                   torch.from_numpy(y).double())
    err = rel_err(got, -ref64.numpy())
    report(f"regressor b100 {dtype}: score_samples rel err vs the fp32 reference's float64 scoring {err:.3e}")
    assert np.isfinite(got).all() and np.isfinite(err)
