"""GPU: the attention-between-features sublayer alone, per element, on every form the forwards run it in.

``mmpfn_feature_attention_ex`` goes through the host function the forwards' layers go through (capi.cpp
``feat_sublayer``): in the 16-bit modes at T <= 64 one launch of ``feat_rows_kernel`` (featrow.hip) over the rows of all
members, full or in the pruned last layer's form; otherwise the general path (q|k|v projection, key-tiled attention,
out-projection + LayerNorm).  Operands, the float64 restatement and the bounds come from tests/feat_block_cases.py (no
bound there comes from a kernel run); tests/test_feat_block_sensitivity.py shows on the CPU what they catch.

* Integer cases, exact up to the fp32 LayerNorm, held to per-element bounds -- the selection case (every query's softmax
  one-hot on a key drawn per member and row: the Q / K row permutation, the key order of P against V^T, the tile pairs,
  the head -> Wout K-step map, the fp16 form's row order, the parked fragments, the row and member address) and the
  uniform case (weight 1 / T on every valid key: the padding mask and the row sum) -- over T at, below and above every
  16-token tile and S below, at and above the 4-row block, in all four modes; 64 sentinel rows behind the state must
  stay untouched.
* Several members in one launch, a member boundary inside a 4-row block and on its edge, every member's inputs different.
* The last-layer form: token T - 1 bit for bit the full form's and within the same bounds, every other token as the
  state held it.
* Normal data: the 16-bit modes within q, the rounding's own effect, in max norm and RMS; the fp32 modes within the
  taps' tolerance.
* The general path at T = 65 .. 129: normal data (mode 1 against the restatement of that path's own rounding points,
  feat_block_cases' docstring) and the uniform case, which that path keeps exact too (read from gemm.hip, rowgemm3.hip
  and attention.hip, same docstring); mode 5 at T = 65 is mode 1 bit for bit.
* Refusals leave the context usable.

One-layer models without a mixer; an engine per weight set, shared by the precision modes.

Worst kernel / bound measured on an MI355X, modes 0 / 1 / 2 / 5 (``helpers.report`` prints them with every run):
integer cases over the geometry, selection 0.029 / 0.029 / 0.029 / 0.96, uniform 0.001 / 0.025 / 0.001 / 0.96; several
members, selection 0.029 / 0.029 / 0.028 / 0.97, uniform 0.001 / 0.027 / 0.001 / 0.96; last-layer form (modes 1 / 5),
selection 0.024 / 0.93, uniform 0.021 / 0.94, normal data 0.000 / 0.15; normal data in max norm 0.18 / 0.37 / 0.027 /
0.34, in RMS 0.055 (mode 1), 0.30 (mode 5); the general path (modes 0 / 1 / 2), normal data in max norm 0.14 / 0.13 /
0.023, in RMS 0.033 (mode 1), uniform 0.001 / 0.027 / 0.001.  Mode 5's integer ratios are its store's half ulp, which is
most of its bound there.  No fault found: featrow.hip is unchanged.
"""

import pytest
import torch

import feat_block_cases as F
import layer_tail_cases as L
from helpers import report
from synth import synth_state_dict
from test_taps_gpu import TOL

from multimodalpfn_amd.model.spec import ModelConfig, state_dict_spec

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0
GUARD = 64
LAST_T = (1, 16, 17, 33, 36, 48, 49, 64)
_ENGINES: dict = {}  # weights kind -> engine
_WEIGHTS: dict = {}  # weights kind -> weight set
_CASES: dict = {}  # (kind, M, S, T) -> state; (kind, M, S, T, mode) -> (restatement, bound)
_WORST: dict = {}  # (group, precision) -> (ratio, where)


@pytest.fixture(scope="module", autouse=True)
def _report_and_close():
    yield
    for grp in sorted({g for g, _ in _WORST}):
        report(f"feature block {grp}: worst kernel / bound " + ", ".join(
            f"prec {p} {_WORST[grp, p][0]:.3f} ({_WORST[grp, p][1]})" for p in F.MODES if (grp, p) in _WORST))
    for eng in _ENGINES.values():
        eng.close()
    _ENGINES.clear(), _WEIGHTS.clear(), _CASES.clear(), _WORST.clear()


def _weights(kind: str) -> dict:
    if kind not in _WEIGHTS:
        _WEIGHTS[kind] = F.WEIGHTS[kind]()
    return _WEIGHTS[kind]


def _engine(kind: str):
    from multimodalpfn_amd.engine import HipEngine

    if kind not in _ENGINES:
        cfg = ModelConfig(nlayers=1, mixer_type=None)
        sd = F.state_dict_with(synth_state_dict(state_dict_spec(cfg), 71), _weights(kind))
        _ENGINES[kind] = HipEngine(cfg, sd, torch.device("cuda", 0))
    return _ENGINES[kind]


def _state(kind: str, M: int, S: int, T: int) -> dict:
    if (kind, M, S, T) not in _CASES:
        _CASES[kind, M, S, T] = F.STATES[kind](M, S, T)
    return _CASES[kind, M, S, T]


def _ref(kind: str, M: int, S: int, T: int, mode: int):
    """(restatement, bounds) of a case in a mode, computed once: a per-element bound for the integer cases, whose
    premises are checked here, ``normal_bounds``' dict for normal data."""
    key = (kind, M, S, T, mode)
    if key not in _CASES:
        W, c = _weights(kind), _state(kind, M, S, T)
        r = F.feat_block(mode, c["X"], W)
        if kind == "normal":
            b = F.normal_bounds(mode, r, F.feat_block(mode, c["X"], W, exact=True), TOL)
        else:
            F.INT_CHECK[kind](mode, W, c, r)
            b = F.INT_BOUND[kind](mode, W, r)
        _CASES[key] = (r, b)
    return _CASES[key]


def _tap(eng, prec: int, X: torch.Tensor, last: bool = False) -> torch.Tensor:
    """``mmpfn_feature_attention_ex`` of layer 0 on a state [M][T][S][E] with sentinel rows behind it, which must come
    back untouched (mode 5 works on the context's fp16 copy: nothing of the caller's to overrun)."""
    M, T, S, _ = X.shape
    n = M * T * S
    buf = torch.full((n + GUARD, L.E), SENTINEL, device=eng.device, dtype=torch.float32)
    buf[:n] = X.reshape(n, L.E).float().to(eng.device)
    eng._bind_stream()
    eng._check(eng.lib.mmpfn_feature_attention_ex(eng.ctx, 0, buf.data_ptr(), S, T, M, int(last), prec), "tap")
    out = buf.cpu()
    assert torch.equal(out[n:], torch.full((GUARD, L.E), SENTINEL)), "rows behind the state were written"
    assert torch.isfinite(out[:n]).all()
    return out[:n].reshape(M, T, S, L.E).double()


def _note(group: str, prec: int, ratio: float, where: str) -> None:
    print(f"{group} prec {prec} {where}: kernel / bound {ratio:.3f}")
    if not ratio <= _WORST.get((group, prec), (-1.0, ""))[0]:
        _WORST[group, prec] = (ratio, where)


def _check_int(group: str, prec: int, kind: str, M: int, S: int, T: int, got: torch.Tensor, tokens=slice(None)) -> None:
    r, bound = _ref(kind, M, S, T, prec)
    # pre: in front of mode 5's store, which the bound holds
    ratio = float(((got - r["pre"]).abs() / bound)[:, tokens].max())
    where = f"M {M} S {S} T {T}"
    _note(f"{group} {kind}", prec, ratio, where)
    assert ratio <= 1.0, (group, kind, prec, where, ratio)


def _check_normal(group: str, prec: int, M: int, S: int, T: int, got: torch.Tensor) -> None:
    r, b = _ref("normal", M, S, T, prec)
    mx, rms = L.normal_ratios(prec, got, r, b)
    where = f"M {M} S {S} T {T}"
    _note(f"{group} max", prec, mx, where)
    if rms is not None:
        _note(f"{group} rms", prec, rms, where)
    assert mx <= 1.0 and (rms is None or rms <= 1.0), (group, prec, where, mx, rms, b)


# ---------------------------------------------------------------------------------------------- the geometry
@pytest.mark.parametrize("T", F.T_EDGES)
@pytest.mark.parametrize("prec", F.MODES)
def test_integer_cases_over_the_geometry(prec, T):
    for S in F.S_EDGES:
        for kind in ("selection", "uniform"):
            got = _tap(_engine(kind), prec, _state(kind, 1, S, T)["X"])
            _check_int("int", prec, kind, 1, S, T, got)


@pytest.mark.parametrize("T", [17, 36, 48])
@pytest.mark.parametrize("M,S", F.MS)
@pytest.mark.parametrize("prec", F.MODES)
def test_several_members(prec, M, S, T):
    """All members' rows in one launch of feat_rows_kernel (the general path: member by member).  Every member and row
    has its own targets and values: a member that reads another's rows fails."""
    for kind in ("selection", "uniform"):
        X = _state(kind, M, S, T)["X"]
        assert all(not torch.equal(X[m], X[m - 1]) for m in range(1, M))
        _check_int("members", prec, kind, M, S, T, _tap(_engine(kind), prec, X))


@pytest.mark.parametrize("T", LAST_T)
@pytest.mark.parametrize("prec", [1, 5])
def test_last_layer_form(prec, T):
    M, S = 2, 3
    for kind in ("selection", "uniform", "normal"):
        X = _state(kind, M, S, T)["X"]
        full, last = _tap(_engine(kind), prec, X), _tap(_engine(kind), prec, X, last=True)
        assert torch.equal(last[:, T - 1], full[:, T - 1]), (kind, "token T - 1 differs from the full form's")
        if kind == "normal":
            r, b = _ref(kind, M, S, T, prec)
            d = (last[:, T - 1] - r["pre"][:, T - 1]).abs() - L.store_bound(prec, last[:, T - 1])
            ratio = float(d.clamp(min=0).max()) / b["max"]
            _note("last normal max", prec, ratio, f"M {M} S {S} T {T}")
            assert ratio <= 1.0, (kind, prec, T, ratio)
        else:
            _check_int("last", prec, kind, M, S, T, last, tokens=slice(T - 1, T))
        assert torch.equal(last[:, :T - 1], L.state_in(prec, X)[:, :T - 1]), (kind, "another token was written")


# ---------------------------------------------------------------------------------------------- normal data
@pytest.mark.parametrize("M,S,T", [(1, 5, T) for T in F.T_EDGES] + [(3, 3, 36)])
@pytest.mark.parametrize("prec", F.MODES)
def test_normal_data(prec, M, S, T):
    X = _state("normal", M, S, T)["X"]
    if prec == F.MODES[0]:
        report(f"feature block normal M {M} S {S} T {T}: variance shares X %.3f, attention %.3f"
               % F.variance_shares(_weights("normal"), X))
    Xr = X.float().transpose(1, 2).contiguous()  # [M][S][T][E], reference order: through the engine's wrapper
    X0 = Xr.clone()
    got = _engine("normal").feature_attention_ex(0, Xr, prec)
    assert got.dtype == torch.float32 and got.shape == Xr.shape
    assert torch.equal(Xr, X0)  # the tap works on a copy
    _check_normal("normal", prec, M, S, T, got.cpu().double().transpose(1, 2))
    if M == 1:  # the old entry is the M = 1, last = 0 call
        assert torch.equal(_engine("normal").feature_attention(0, Xr[0], prec), got[0])


# ---------------------------------------------------------------------------------------------- the general path
@pytest.mark.parametrize("T", F.T_GENERAL)
@pytest.mark.parametrize("prec", [0, 1, 2])
def test_general_path(prec, T):
    M, S = 1, 3
    _check_normal("general normal", prec, M, S, T, _tap(_engine("normal"), prec, _state("normal", M, S, T)["X"]))
    _check_int("general", prec, "uniform", M, S, T, _tap(_engine("uniform"), prec, _state("uniform", M, S, T)["X"]))


def test_fp16_mode_past_64_tokens_is_the_bf16_mode():
    for kind in ("normal", "uniform"):
        X = _state(kind, 1, 3, 65)["X"]
        assert torch.equal(_tap(_engine(kind), 5, X), _tap(_engine(kind), 1, X)), kind


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals_leave_the_context_usable():
    from multimodalpfn_amd import _lib

    eng = _engine("normal")
    M, S, T = 3, 3, 36
    X = _state("normal", M, S, T)["X"].float().to(eng.device)
    X0 = X.clone()
    call = eng.lib.mmpfn_feature_attention_ex
    p = X.data_ptr()
    for what, args in [("member count", (0, p, S, T, 0, 0, 1)),
                       ("member count", (0, p, S, T, -2, 0, 1)),
                       ("state geometry", (0, p, 0, T, M, 0, 1)),
                       ("state geometry", (0, p, -1, T, M, 0, 1)),
                       ("state geometry", (0, p, S, 0, M, 0, 1)),
                       ("state geometry", (0, p, S, -5, M, 1, 1)),
                       ("layer index", (1, p, S, T, M, 0, 1)),
                       ("layer index", (-1, p, S, T, M, 0, 1)),
                       ("precision", (0, p, S, T, M, 0, 8)),
                       ("precision", (0, p, S, T, M, 0, -1))]:
        # set a marker first, so that a stale message of the call before cannot pass for this one's
        assert eng.lib.mmpfn_mlp_ln(eng.ctx, 0, p, 0, 0) == _lib.MMPFN_ERR_INVALID
        marker = eng.lib.mmpfn_last_error(eng.ctx).decode()
        assert call(eng.ctx, *args) == _lib.MMPFN_ERR_INVALID, what
        msg = eng.lib.mmpfn_last_error(eng.ctx).decode()
        assert what in msg and msg != marker, (what, msg)
    assert call(eng.ctx, 0, None, S, T, M, 0, 1) == _lib.MMPFN_ERR_INVALID  # (tap_check: a null state)
    torch.cuda.synchronize()
    assert torch.equal(X, X0)  # a refused call launches nothing
    for prec in F.MODES:
        _check_normal("normal", prec, M, S, T, _tap(eng, prec, _state("normal", M, S, T)["X"]))
