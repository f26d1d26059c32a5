"""GPU: the layer's tail, attention output -> state, on the kernels the forwards run, alone.

``mmpfn_outproj_mlp_ln`` goes through the host function the forwards' layers go through (capi.cpp ``layer_tail``): in
the 16-bit modes one launch of ``mlp_rows_kernel`` with the out-projection prologue (``RES``), which
``mmpfn_item_attention_block`` and ``mmpfn_mlp_ln`` never reach; in the fp32 modes the out-projection + LayerNorm
kernel and then the MLP kernel.  Operands, float64 references and bounds come from tests/layer_tail_cases.py (no bound
there comes from a kernel run); tests/test_layer_tail_sensitivity.py shows on the CPU what they catch.

* Integer cases, exact up to the last fp32 LayerNorm, held to per-element bounds: the prologue alone (the Wout halves,
  their swizzle, the fp16 row order, the O-row -> lane map, clamped rows) and the MLP behind a trivial prologue (W1's and
  W2's packing, every chunk's ring slot, the last chunk), over row counts at, below and above the 16-row tile, the
  32-row wave and the 128-row block, and one three-block grid; 64 sentinel rows behind the fp32 state must stay
  untouched.  The 16-bit modes' ``mmpfn_mlp_ln`` (the ``RES = false`` form) gets the MLP case with X = +-1 itself.
* Hidden widths nhid = 192 .. 960 (6 .. 30 chunks of mlp_rows_kernel, 1 .. 5 of mlp_fused_kernel, 6 .. 30 of
  mlp_x3_kernel) on models without a mixer: the integer MLP case at 129 rows, normal data at 257.
* Normal data at 257 and 300 rows: the 16-bit modes within q, the rounding's own effect, in max norm and RMS; the fp32
  modes within twice the taps' tolerance.
* Refusals leave the context usable.

One-layer models; an engine per (nhid_factor, weights), shared by the precision modes.

Worst kernel / bound measured on an MI355X, modes 0 / 1 / 2 / 5 (``helpers.report`` prints them with every run):
integer prologue 0.007 / 0.007 / 0.009 / 0.92; integer MLP over the row counts below 0.001 in the fp32-state modes,
0.13 in mode 5, over the widths 0.001 / 0.001 / 0.002 / 0.52; ``mmpfn_mlp_ln`` 0.019 (mode 1), 0.95 (mode 5); normal
data in max norm 0.063 / 0.36 / 0.021 / 0.40, in RMS 0.043 (mode 1), 0.27 (mode 5).  Mode 5's integer ratios are its
store's half ulp, which is most of its bound there.
"""

import pytest
import torch

import layer_tail_cases as L
from helpers import report
from synth import synth_state_dict
from test_taps_gpu import TOL

from multimodalpfn_amd.model.spec import ModelConfig, state_dict_spec

pytestmark = pytest.mark.gpu

K = ("X", "O", "Wout", "W1", "W2")
SENTINEL = -12345.0
GUARD = 64
_ENGINES: dict = {}  # (nhid_factor, weights kind) -> engine
_CASES: dict = {}  # (kind, nhid_factor, rows) -> case; (kind, nhid_factor, rows, mode) -> reference
_WORST: dict = {}  # (group, precision) -> (ratio, where)

MAKE = dict(prologue=L.prologue_case, mlp=L.mlp_case, normal=L.normal_case,
            mlp_unit=lambda rows, nhid: L.mlp_case(rows, nhid, unit=True),
            mlp_light=lambda rows, nhid: L.mlp_case(rows, nhid, light=True))
WEIGHTS = dict(mlp_unit="mlp")  # the unit-row case shares the MLP case's weights


@pytest.fixture(scope="module", autouse=True)
def _report_and_close():
    yield
    for grp in sorted({g for g, _ in _WORST}):
        report(f"layer tail {grp}: worst kernel / bound " + ", ".join(
            f"prec {p} {_WORST[grp, p][0]:.3f} ({_WORST[grp, p][1]})" for p in L.MODES if (grp, p) in _WORST))
    for eng in _ENGINES.values():
        eng.close()
    _ENGINES.clear(), _CASES.clear(), _WORST.clear()


def _case(kind: str, factor: int, rows: int) -> dict:
    if (kind, factor, rows) not in _CASES:
        _CASES[kind, factor, rows] = MAKE[kind](rows, L.E * factor)
    return _CASES[kind, factor, rows]


def _engine(factor: int, kind: str):
    from multimodalpfn_amd.engine import HipEngine

    kind = WEIGHTS.get(kind, kind)
    if (factor, kind) not in _ENGINES:
        cfg = ModelConfig(nlayers=1, nhid_factor=factor, mixer_type=None)
        sd = L.state_dict_with(synth_state_dict(state_dict_spec(cfg), 71), _case(kind, factor, 1))
        _ENGINES[factor, kind] = HipEngine(cfg, sd, torch.device("cuda", 0))
    return _ENGINES[factor, kind]


def _ref(kind: str, factor: int, rows: int, mode: int) -> dict:
    """The restatement of a case in a mode (``mlp_unit``: of mmpfn_mlp_ln), computed once."""
    key = (kind, factor, rows, mode)
    if key not in _CASES:
        c = _case(kind, factor, rows)
        _CASES[key] = (L.mlp_only(mode, c["X"], c["W1"], c["W2"]) if kind == "mlp_unit"
                       else L.tail(mode, **{k: c[k] for k in K}))
    return _CASES[key]


def _odt(prec: int):
    return L.OP[prec] or torch.float32


def _tap(eng, prec: int, X: torch.Tensor, O: torch.Tensor | None) -> torch.Tensor:
    """``mmpfn_outproj_mlp_ln`` (O None: ``mmpfn_mlp_ln``) of layer 0 on a state with sentinel rows behind it, which
    must come back untouched (mode 5 works on the context's fp16 copy: nothing of the caller's to overrun)."""
    rows = X.shape[0]
    buf = torch.full((rows + GUARD, L.E), SENTINEL, device=eng.device, dtype=torch.float32)
    buf[:rows] = X.float().to(eng.device)
    eng._bind_stream()
    if O is None:
        rc = eng.lib.mmpfn_mlp_ln(eng.ctx, 0, buf.data_ptr(), rows, prec)
    else:
        Od = O.float().to(_odt(prec)).to(eng.device).contiguous()
        rc = eng.lib.mmpfn_outproj_mlp_ln(eng.ctx, 0, buf.data_ptr(), Od.data_ptr(), rows, prec)
    eng._check(rc, "tap")
    out = buf.cpu()
    assert torch.equal(out[rows:], torch.full((GUARD, L.E), SENTINEL)), "rows behind the state were written"
    assert torch.isfinite(out[:rows]).all()
    return out[:rows].double()


def _note(group: str, prec: int, ratio: float, where: str) -> None:
    print(f"{group} prec {prec} {where}: kernel / bound {ratio:.3f}")
    if not ratio <= _WORST.get((group, prec), (-1.0, ""))[0]:
        _WORST[group, prec] = (ratio, where)


def _check_int(group: str, prec: int, where: str, got: torch.Tensor, ref: dict, bound: torch.Tensor) -> None:
    ratio = float(((got - ref["pre"]).abs() / bound).max())  # pre: in front of mode 5's store, which the bound holds
    _note(group, prec, ratio, where)
    assert ratio <= 1.0, (group, prec, where, ratio)


def _check_normal(prec: int, factor: int, rows: int, got: torch.Tensor) -> None:
    c, r = _case("normal", factor, rows), _ref("normal", factor, rows, prec)
    b = L.normal_bounds(prec, r, L.tail(prec, exact=True, **{k: c[k] for k in K}), TOL)
    mx, rms = L.normal_ratios(prec, got, r, b)
    where = f"nhid {L.E * factor} rows {rows}"
    _note("normal max", prec, mx, where)
    if rms is not None:
        _note("normal rms", prec, rms, where)
    assert mx <= 1.0 and (rms is None or rms <= 1.0), (prec, where, mx, rms, b)


# ---------------------------------------------------------------------------------------------- rows
@pytest.mark.parametrize("rows", L.ROWS)
@pytest.mark.parametrize("prec", L.MODES)
def test_integer_cases_over_row_counts(prec, rows):
    for kind, bound in (("prologue", lambda r, c: L.prologue_bound(prec, r)),
                        ("mlp", lambda r, c: L.mlp_bound(prec, r, c["W2"]))):
        c, r = _case(kind, 4, rows), _ref(kind, 4, rows, prec)
        got = _tap(_engine(4, kind), prec, c["X"], c["O"])
        _check_int(f"int {kind}", prec, f"rows {rows}", got, r, bound(r, c))


@pytest.mark.parametrize("rows", L.ROWS)
@pytest.mark.parametrize("prec", [1, 5])
def test_mlp_ln_16bit_integer_case_over_row_counts(prec, rows):
    """The ``RES = false`` form of mlp_rows_kernel (no forward launches it; the mmpfn_mlp_ln tap does) gets the same
    structural check: X = +-1 fed directly, an exact integer in front of the LayerNorm."""
    c, r = _case("mlp_unit", 4, rows), _ref("mlp_unit", 4, rows, prec)
    got = _tap(_engine(4, "mlp_unit"), prec, c["X"], None)
    _check_int("int mlp_ln", prec, f"rows {rows}", got, r, L.mlp_bound(prec, r, c["W2"], exact_residual=True))


@pytest.mark.parametrize("prec", L.MODES)
def test_light_mlp_case(prec):
    """The MLP case with an MLP term of the residual's order: what catches a whole row's MLP term scaled (an
    unnormalised up-projection operand), which the LayerNorm behind a dominant MLP term would hide."""
    c, r = _case("mlp_light", 4, 129), _ref("mlp_light", 4, 129, prec)
    got = _tap(_engine(4, "mlp_light"), prec, c["X"], c["O"])
    _check_int("int mlp light", prec, "rows 129", got, r, L.mlp_bound(prec, r, c["W2"]))


# ---------------------------------------------------------------------------------------------- hidden widths
@pytest.mark.parametrize("factor", L.NHID_FACTORS)
@pytest.mark.parametrize("prec", L.MODES)
def test_hidden_widths(prec, factor):
    c, r = _case("mlp", factor, 129), _ref("mlp", factor, 129, prec)
    got = _tap(_engine(factor, "mlp"), prec, c["X"], c["O"])
    _check_int("int mlp width", prec, f"nhid {L.E * factor}", got, r, L.mlp_bound(prec, r, c["W2"]))
    if L.OP[prec] is not None:
        c, r = _case("mlp_unit", factor, 129), _ref("mlp_unit", factor, 129, prec)
        got = _tap(_engine(factor, "mlp_unit"), prec, c["X"], None)
        _check_int("int mlp_ln width", prec, f"nhid {L.E * factor}", got, r,
                   L.mlp_bound(prec, r, c["W2"], exact_residual=True))
    c = _case("normal", factor, 257)
    got = _engine(factor, "normal").outproj_mlp_ln(0, c["X"].float(), c["O"].float(), prec).cpu().double()
    _check_normal(prec, factor, 257, got)


# ---------------------------------------------------------------------------------------------- normal data
@pytest.mark.parametrize("rows", [257, 300])
@pytest.mark.parametrize("prec", L.MODES)
def test_normal_data(prec, rows):
    c = _case("normal", 4, rows)
    if prec == L.MODES[0]:
        report(f"layer tail normal rows {rows}: variance shares X %.3f, O.Wout^T %.3f, MLP %.3f" % L.variance_shares(c))
    X = c["X"].float()
    got = _engine(4, "normal").outproj_mlp_ln(0, X, c["O"].float(), prec)
    assert got.dtype == torch.float32 and got.shape == X.shape
    assert torch.equal(X, c["X"].float())  # the tap works on a copy
    _check_normal(prec, 4, rows, got.cpu().double())


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals_leave_the_context_usable():
    from multimodalpfn_amd import _lib

    eng = _engine(4, "normal")
    c = _case("normal", 4, 33)
    X = c["X"].float().to(eng.device)
    O = c["O"].float().to(eng.device)
    X0 = X.clone()
    call = eng.lib.mmpfn_outproj_mlp_ln
    for what, args in [("row count", (0, X.data_ptr(), O.data_ptr(), 0, 0)),
                       ("row count", (0, X.data_ptr(), O.data_ptr(), -3, 0)),
                       ("null attention output", (0, X.data_ptr(), None, 33, 0)),
                       ("layer index", (1, X.data_ptr(), O.data_ptr(), 33, 0)),
                       ("layer index", (-1, X.data_ptr(), O.data_ptr(), 33, 0)),
                       ("precision", (0, X.data_ptr(), O.data_ptr(), 33, 8)),
                       ("precision", (0, X.data_ptr(), O.data_ptr(), 33, -1))]:
        # set a marker first, so that a stale message of the call before cannot pass for this one's
        assert eng.lib.mmpfn_mlp_ln(eng.ctx, 0, X.data_ptr(), 0, 0) == _lib.MMPFN_ERR_INVALID
        marker = eng.lib.mmpfn_last_error(eng.ctx).decode()
        assert call(eng.ctx, *args) == _lib.MMPFN_ERR_INVALID, what
        msg = eng.lib.mmpfn_last_error(eng.ctx).decode()
        assert what in msg and (msg != marker or what == "row count"), (what, msg)
    assert call(eng.ctx, 0, None, O.data_ptr(), 33, 0) == _lib.MMPFN_ERR_INVALID  # (tap_check: a null state)
    torch.cuda.synchronize()
    assert torch.equal(X, X0)  # a refused call launches nothing
    for prec in L.MODES:
        _check_normal(prec, 4, 33, eng.outproj_mlp_ln(0, c["X"].float(), c["O"].float(), prec).cpu().double())
