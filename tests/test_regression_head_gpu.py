"""GPU: ``mmpfn_bar_head`` (csrc/barhead.hip) alone against the float64 restatement over the head-only grid.

Bounds, per case, with ``d_ref`` the reference fixture's own float32 deviation from the float64 restatement ``P64``
(computed here on the CPU and reported):

* bar probabilities ``softmax(final logits)``: ``max |P - P64| <= delta = max(2 d_ref, 64 x 2^-24)`` -- both are
  float32 sums in different orders (factor 2); the floor is ``aggregate_kernel``'s bound;
* mean: the same rule on ``|mean - mean64|`` as a fraction of the span between the criterion's second and
  second-to-last borders (two bars have no such span: the whole span there);
* quantiles, in probability space: ``|F64(q) - level| <= max(2 d_ref, 64 x 2^-24)`` with ``F64`` the float64
  piecewise-linear CDF of the final distribution and ``d_ref`` the reference's own quantiles under the same measure
  -- every level of every case.  (A float32 quantile cannot do better than half its own spacing times the
  density: in a peaked row of 257 bars the reference's and the kernel's quantiles both sit 4.2e-6 off the level,
  with bar probabilities 8.6e-8 / 1.3e-7 off.  So the deviation that counts is the quantile's own kind.)
* mode: the float64 density of the engine's bucket is at least the float64 maximum minus ``delta / width``.
"""

import numpy as np
import pytest
import torch

import regression_oracle as ro
from helpers import report
from test_regression_head import PROB_FLOOR, head_fixture

from multimodalpfn_amd import _lib
from multimodalpfn_amd.bar_distribution import border_tables

pytestmark = pytest.mark.gpu

_ENGINE: list = []


def _engine():
    from synth import synth_state_dict

    from multimodalpfn_amd.engine import HipEngine
    from multimodalpfn_amd.model.spec import ModelConfig, state_dict_spec

    if not _ENGINE:
        cfg = ModelConfig(nlayers=1, mgm_heads=2, cap_heads=2)
        _ENGINE.append(HipEngine(cfg, synth_state_dict(state_dict_spec(cfg), 23), torch.device("cuda")))
    return _ENGINE[0]


def _tables(case):
    tabs = [border_tables(frm, case["std_borders"]) for frm in case["borders"]]
    idx, share = np.stack([t[0] for t in tabs]), np.stack([t[1] for t in tabs])
    cancel = None
    if any(m is not None for m in case["masks"]):
        cancel = np.stack([np.zeros(case["B"], bool) if m is None else m for m in case["masks"]])
    return idx, share, cancel, ro.criterion_tables(torch.from_numpy(case["crit_borders"]))


def _run(eng, case, logits=None, want_logits=True):
    idx, share, cancel, crit = _tables(case)
    lg = torch.stack(case["logits"]).cuda() if logits is None else logits
    out = eng.bar_head(lg, idx, share, crit, cancel=cancel, softmax_temperature=case["temperature"],
                       average_before_softmax=case["avg"], quantiles=case["levels"], want_logits=want_logits)
    return {k: (None if v is None else v.cpu()) for k, v in out.items()}


def _span(case):
    b = case["crit_borders"].astype(np.float64)
    return float(b[-2] - b[1]) if case["B"] > 2 else float(b[-1] - b[0])


def _errors(case, r64, logits, mean, quantiles):
    """Deviation of float32 outputs from the float64 restatement, per kind."""
    b64 = torch.from_numpy(case["crit_borders"]).double()
    probs = torch.softmax(logits.double(), -1)
    lv = torch.tensor(case["levels"], dtype=torch.float64)[:, None]
    return {
        "probs": float((probs - r64["probs"]).abs().max()),
        "mean": float((mean.double() - r64["mean"]).abs().max()) / _span(case),
        "quantiles": float((ro.final_cdf64(r64["probs"], b64, quantiles) - lv).abs().max()),
    }


@pytest.mark.parametrize("B", ro.HEAD_BARS)
def test_bar_head_matches_float64_restatement(B):
    eng = _engine()
    z = head_fixture(B)
    worst = {"probs": (0.0, 0.0), "mean": (0.0, 0.0), "quantiles": (0.0, 0.0), "mode": (0.0, 0.0)}
    for case in ro.head_cases(B):
        name = case["name"]
        r64 = ro.run_head(case, torch.float64)
        d_ref = _errors(case, r64, torch.from_numpy(z[f"{name}_logits"]), torch.from_numpy(z[f"{name}_mean"]),
                        torch.from_numpy(z[f"{name}_quantiles"]))
        got = _run(eng, case)
        assert got["logits"].shape == (case["Q"], B) and got["quantiles"].shape == (len(case["levels"]), case["Q"])
        assert not torch.isnan(got["logits"]).any()
        for k in ("mean", "mode", "quantiles"):
            assert torch.isfinite(got[k]).all(), (name, k)
        err = _errors(case, r64, got["logits"], got["mean"], got["quantiles"])
        delta = max(2 * d_ref["probs"], PROB_FLOOR)
        bound = {k: max(2 * d_ref[k], PROB_FLOOR) for k in ("probs", "mean", "quantiles")}
        # mode: the engine returns its bucket's plain mean, an entry of the table it was given
        crit32 = ro.criterion_tables(torch.from_numpy(case["crit_borders"]))
        w64 = crit32["widths"].double()
        dens64 = r64["probs"] / w64
        gap = 0.0
        for q in range(case["Q"]):
            j = torch.nonzero(crit32["mode_means"] == got["mode"][q]).flatten()
            assert j.numel() >= 1, (name, q, float(got["mode"][q]))
            gap = max(gap, float((dens64[q].max() - dens64[q, j[0]]) * w64[j[0]]))
        err["mode"], bound["mode"] = gap, delta
        print(f"bar head B={B} {name}: " + ", ".join(
            f"{k} err {err[k]:.2e} d_ref {d_ref.get(k, float('nan')):.2e} bound {bound[k]:.2e}" for k in err))
        for k in err:
            if err[k] / bound[k] >= worst[k][0] / max(worst[k][1], 1e-300):
                worst[k] = (err[k], bound[k])
            assert err[k] <= bound[k], (B, name, k, err[k], bound[k], d_ref)
    report(f"bar head B={B}: worst error / bound -- " + ", ".join(f"{k} {e:.2e} / {b:.2e}" for k, (e, b) in worst.items()))


@pytest.mark.parametrize("B", [37, 257, 1023, 5000])
def test_bar_head_ignores_what_lies_beyond_a_row(B):
    """The logits inside a NaN-filled allocation, at an offset that leaves no row 16-byte aligned and at one that
    aligns the first: bit for bit the outputs of the plain call, and the same without the logits output."""
    eng = _engine()
    for case in ro.head_cases(B)[4:7]:
        plain = _run(eng, case)
        lg = torch.stack(case["logits"])
        for off in (1, 4):
            buf = torch.full((lg.numel() + 64,), float("nan")).cuda()
            view = buf[off:off + lg.numel()].view(lg.shape)
            view.copy_(lg)
            for want in (True, False):
                got = _run(eng, case, logits=view, want_logits=want)
                assert (got["logits"] is None) == (not want)
                for k in ("mean", "mode", "quantiles") + (("logits",) if want else ()):
                    assert torch.equal(got[k], plain[k]), (B, case["name"], off, want, k)
            assert torch.isnan(buf[:off]).all() and torch.isnan(buf[off + lg.numel():]).all()


@pytest.mark.parametrize("B", [37, 257, 5000])
def test_bar_head_dense_and_padded_tables_agree(B):
    """``HipEngine.bar_head`` uploads its tables and mask with rows padded to a multiple of 4 entries (read in 16- /
    4-byte pieces); the C entry point with dense rows (``ldt = B + 1``, ``ldc = B``: dword and byte loads) gives
    the same outputs bit for bit."""
    eng = _engine()
    for case in [c for c in ro.head_cases(B) if "cancel" in c["kinds"] or c["avg"]][:3]:
        plain = _run(eng, case)
        idx, share, cancel, crit = _tables(case)
        M, Q, K = case["M"], case["Q"], len(case["levels"])
        dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt).cuda()  # noqa: E731
        lg = torch.stack(case["logits"]).cuda()
        t = {k: v.float().contiguous().cuda() for k, v in crit.items()}
        d_idx, d_share = dev(idx, torch.int32), dev(share, torch.float32)
        d_cm = None if cancel is None else dev(cancel.astype(np.uint8), torch.uint8)
        lv = torch.tensor(case["levels"], dtype=torch.float32).cuda()
        out = torch.empty(Q, B).cuda()
        mean, mode, qs = torch.empty(Q).cuda(), torch.empty(Q).cuda(), torch.empty(K, Q).cuda()
        eng._bind_stream()
        rc = eng.lib.mmpfn_bar_head(eng.ctx, lg.data_ptr(), M, Q, B, None if d_cm is None else d_cm.data_ptr(), B,
                                    d_idx.data_ptr(), d_share.data_ptr(), B + 1, 1.0 / case["temperature"],
                                    int(case["avg"]), t["borders"].data_ptr(), t["bucket_means"].data_ptr(),
                                    t["mode_means"].data_ptr(), t["widths"].data_ptr(), lv.data_ptr(), K,
                                    out.data_ptr(), mean.data_ptr(), mode.data_ptr(), qs.data_ptr())
        assert rc == _lib.MMPFN_OK
        for k, v in (("logits", out), ("mean", mean), ("mode", mode), ("quantiles", qs)):
            assert torch.equal(v.cpu(), plain[k]), (B, case["name"], k)


def test_bar_head_refuses_what_the_kernel_does_not_hold():
    """B, M or K beyond the kernel: ``ValueError`` from the engine, ``MMPFN_ERR_INVALID`` from the C ABI; the sizes
    the regressor needs (5000 bars, 32 members, 16 levels) are inside."""
    eng = _engine()
    assert _lib.BAR_MAX_BARS >= 5000 and _lib.BAR_MAX_MEMBERS >= 32 and _lib.BAR_MAX_LEVELS >= 16
    B = 16
    std = ro.normal_borders(B)
    crit = ro.criterion_tables(torch.from_numpy(std))
    idx, share = border_tables(std, std)
    lg = torch.zeros(1, 2, B).cuda()
    with pytest.raises(ValueError):
        eng.bar_head(lg, idx[None], share[None], crit, quantiles=[0.5] * (_lib.BAR_MAX_LEVELS + 1))
    with pytest.raises(ValueError):
        eng.bar_head(lg, idx[None], share[None], crit, softmax_temperature=0.0)
    big = _lib.BAR_MAX_BARS + 1
    with pytest.raises(ValueError):
        eng.bar_head(torch.zeros(1, 1, big).cuda(), np.zeros((1, big + 1)), np.zeros((1, big + 1)), crit)
    one = torch.zeros(8).cuda()
    p = one.data_ptr()
    rc = eng.lib.mmpfn_bar_head(eng.ctx, p, 1, 1, big, None, 0, p, p, big + 1, 1.0, 0, p, p, p, p, None, 0, None, p, p,
                                None)
    assert rc == _lib.MMPFN_ERR_INVALID
    rc = eng.lib.mmpfn_bar_head(eng.ctx, p, _lib.BAR_MAX_MEMBERS + 1, 1, 2, None, 0, p, p, 3, 1.0, 0, p, p, p, p, None,
                                0, None, p, p, None)
    assert rc == _lib.MMPFN_ERR_INVALID
    rc = eng.lib.mmpfn_bar_head(eng.ctx, p, 1, 1, 2, None, 0, p, p, 2, 1.0, 0, p, p, p, p, None, 0, None, p, p, None)
    assert rc == _lib.MMPFN_ERR_INVALID  # a table row shorter than B + 1
    # 32 members and 16 levels run
    out = eng.bar_head(torch.randn(32, 3, B, generator=torch.Generator().manual_seed(0)).cuda(), np.stack([idx] * 32),
                       np.stack([share] * 32), crit, quantiles=[(k + 1) / 17 for k in range(16)])
    assert torch.isfinite(out["quantiles"]).all() and out["quantiles"].shape == (16, 3)
    assert (out["quantiles"][1:] >= out["quantiles"][:-1]).all()
