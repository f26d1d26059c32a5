"""GPU: the item attention's q|k|v projection on the kernels the forwards run, alone, per element.

``mmpfn_item_qkv`` goes through the host function the forwards' layers go through (capi.cpp ``item_project``): in the
16-bit modes ``rowgemm_qkv2_kernel`` (both row sets in one launch), in mode 0 ``proj3_kernel``, in mode 2 gemm.hip's
``EPI_ITEM_QKV`` epilogue.  Operands, the float64 restatement and the bounds come from tests/item_qkv_cases.py (no bound
there comes from a kernel run); tests/test_item_qkv_sensitivity.py shows on the CPU what they catch.

Every call of the address case pre-fills q, k, vt and 64 rows' worth behind each with a NaN bit pattern and compares
integers: what the kernels store must equal the restatement bit for bit, everything else -- K rows and V^T columns
[N, Npad), all of k / vt in the cache form, the guards -- must still hold the pattern.  The state must come back
unchanged.

* Train rows N at, below and above the 8-key V^T granule, the 32-row wave and tile, the 64-row GEMM tile, the 128-row
  block, each with two of the test-row counts 0, 1, 33, 130 (one at T = 1, M = 1, one at T = 3, M = 2).
* Columns and members: T in {1, 3}, M in {1, 2}, the pruned last layer's form at T = 3; N = 9 and 33 make every proj3
  and GEMM tile straddle a column.
* The cache's predict form, N = 0, with sentinel k / vt and with null ones.
* Mode 5 at T = 65 is mode 1; the fp8 codes are their base modes.
* Mode 0 with more work items than 2 * P3W per CU: every wave of proj3_kernel loops, blocks hold several panels.
* Normal data against the derived per-element bounds.
* Refusals leave the buffers and the context as they were.

Both a plain model and a ``two_sets_of_queries`` one, one layer, no mixer; an engine per (model, weights), shared by
the precision modes.

Worst kernel / bound of the normal case measured on an MI355X (``helpers.report`` prints them with every run), q / k /
vt: mode 0 0.002 / 0.002 / 0.002; mode 1 0.974 / 0.967 / 0.969; mode 2 0.013 / 0.011 / 0.012; mode 5 0.972 / 0.970 /
0.965.  The 16-bit modes' ratios are their bf16 store's half ulp, which is most of their bound (the stored restatement
itself reaches 0.97, tests/test_item_qkv_sensitivity.py); every address-case comparison is bit for bit.
"""

import math

import pytest
import torch

import item_qkv_cases as C
from helpers import report
from synth import synth_state_dict

from multimodalpfn_amd.model.spec import ModelConfig, state_dict_spec

pytestmark = pytest.mark.gpu

GUARD = 64 * C.HD  # elements behind each output: 64 rows' worth
P3W = 8  # rowgemm3.hip: waves per proj3 block
OUTS = ("q", "k", "vt")
WEIGHTS = dict(address=C.address_weights, normal=C.normal_weights)
STATE = dict(address=C.address_state, normal=C.normal_state)
NORMAL_SHAPES = ((70, 33, 3, 2), (200, 129, 1, 1))  # (S, N, T, M)
_ENGINES: dict = {}  # (two, weights kind) -> engine
_REFS: dict = {}
_WORST: dict = {}  # (precision, output) -> (ratio, where)


@pytest.fixture(scope="module", autouse=True)
def _report_and_close():
    yield
    for p in C.MODES:
        if (p, "q") in _WORST:
            report(f"item qkv normal prec {p}: worst kernel / bound " + ", ".join(
                f"{o} {_WORST[p, o][0]:.3f} ({_WORST[p, o][1]})" for o in OUTS))
    for eng in _ENGINES.values():
        eng.close()
    _ENGINES.clear(), _REFS.clear(), _WORST.clear()


def _engine(two: bool, kind: str):
    from multimodalpfn_amd.engine import HipEngine

    if (two, kind) not in _ENGINES:
        cfg = ModelConfig(nlayers=1, mixer_type=None, two_sets_of_queries=two)
        sd = C.state_dict_with(synth_state_dict(state_dict_spec(cfg), 71), WEIGHTS[kind](two))
        _ENGINES[two, kind] = HipEngine(cfg, sd, torch.device("cuda", 0))
    return _ENGINES[two, kind]


def _base(prec: int) -> int:
    return {3: 1, 4: 1, 6: 5, 7: 5}.get(prec, prec)


def _ref(kind: str, two: bool, prec: int, M: int, T: int, S: int, N: int, last: bool) -> dict:
    """The restatement of a case, computed once per decoded mode."""
    mode = C.decode(_base(prec), T)
    key = (kind, two, mode, M, T, S, N, last)
    if key not in _REFS:
        _REFS[key] = C.project(mode, STATE[kind](M, T, S), WEIGHTS[kind](two), N, last=last, want_mag=kind == "normal")
    return _REFS[key]


def _shapes(M: int, T: int, S: int, N: int, last: bool) -> dict:
    TM, Npad = (M if last else M * T), (N + 63) // 64 * 64
    return dict(q=(TM, C.H, S, C.HD), k=(TM, C.H, Npad, C.HD), vt=(TM, C.H, C.HD, Npad))


def _buffers(prec: int, shapes: dict, device) -> dict:
    odt = C.out_dtype(_base(prec))
    return {o: torch.full((math.prod(s) + GUARD,), C.SENTINEL[odt], dtype=C.INT[odt], device=device)
            for o, s in shapes.items()}


def _tap(eng, prec: int, X: torch.Tensor, N: int, last: bool = False, null_kv: bool = False) -> dict:
    """``mmpfn_item_qkv`` of layer 0 on X [M][T][S][E] into sentinel-filled buffers with sentinel guards behind them;
    returns the buffers' contents as integers in the outputs' shapes."""
    M, T, S, _ = X.shape
    shapes = _shapes(M, T, S, N, last)
    Xd = X.float().to(eng.device).contiguous()
    X0 = Xd.clone()
    buf = _buffers(prec, shapes, eng.device)
    eng._bind_stream()
    rc = eng.lib.mmpfn_item_qkv(eng.ctx, 0, Xd.data_ptr(), S, T, N, M, int(last), prec, buf["q"].data_ptr(),
                                None if null_kv else buf["k"].data_ptr(), None if null_kv else buf["vt"].data_ptr())
    eng._check(rc, "mmpfn_item_qkv")
    torch.cuda.synchronize()
    assert torch.equal(Xd.view(torch.int32), X0.view(torch.int32)), "the state was modified"
    out = {}
    for o, s in shapes.items():
        b, n = buf[o].cpu(), math.prod(s)
        sent = C.SENTINEL[C.out_dtype(_base(prec))]
        assert bool((b[n:] == sent).all()), f"{o}: {int((b[n:] != sent).sum())} elements behind the buffer were written"
        out[o] = b[:n].view(s)
    return out


def _check_bits(got: dict, r: dict, where) -> None:
    want = C.bits(r)
    for o in OUTS:
        if torch.equal(got[o], want[o]):
            continue
        bad = got[o] != want[o]
        w = r["written"][o]
        sent = C.SENTINEL[r["out"][o].dtype]
        first = [int(i) for i in bad.nonzero()[0]]
        raise AssertionError(f"{where} {o}: {int(bad.sum())} elements differ, first at {first}; "
                             f"{int((bad & ~w).sum())} outside what the kernel stores (sentinel overwritten), "
                             f"{int((bad & w & (got[o] == sent)).sum())} never written, "
                             f"{int((bad & w & (got[o] != sent)).sum())} with another value")


def _address(two: bool, prec: int, M: int, T: int, S: int, N: int, last: bool = False, null_kv: bool = False) -> dict:
    got = _tap(_engine(two, "address"), prec, C.address_state(M, T, S), N, last, null_kv)
    _check_bits(got, _ref("address", two, prec, M, T, S, N, last), (two, prec, M, T, S, N, last))
    return got


# ---------------------------------------------------------------------------------------------- rows
@pytest.mark.parametrize("i", range(len(C.N_EDGES)), ids=[f"N{n}" for n in C.N_EDGES])
@pytest.mark.parametrize("prec", C.MODES)
def test_train_and_test_row_counts(prec, i):
    N, (qa, qb) = C.N_EDGES[i], C.q_pairs(i)
    for two in (False, True):
        _address(two, prec, 1, 1, N + qa, N)
        _address(two, prec, 2, 3, N + qb, N)


# ---------------------------------------------------------------------------------------------- columns, members
@pytest.mark.parametrize("N,nq", [(9, 33), (33, 0), (33, 1), (64, 130)])
@pytest.mark.parametrize("prec", C.MODES)
def test_columns_members_and_the_last_layers_form(prec, N, nq):
    for two in (False, True):
        for M in (1, 2):
            _address(two, prec, M, 1, N + nq, N)
            for last in (False, True):
                _address(two, prec, M, 3, N + nq, N, last)


# ---------------------------------------------------------------------------------------------- cache form
@pytest.mark.parametrize("S", C.CACHE_S)
@pytest.mark.parametrize("prec", C.MODES)
def test_cache_predict_form(prec, S):
    """N = 0: every row through the test rows' q; k and vt (nothing but guard) untouched, or null."""
    for two in (False, True):
        for last in (False, True):
            a = _address(two, prec, 2, 3, S, 0, last)
            b = _address(two, prec, 2, 3, S, 0, last, null_kv=True)
            assert torch.equal(a["q"], b["q"]) and a["k"].numel() == 0 and a["vt"].numel() == 0


# ---------------------------------------------------------------------------------------------- precision codes
def test_fp16_past_64_tokens_is_the_bf16_mode():
    for two in (False, True):
        a, b = _address(two, 5, 1, 65, 40, 33), _address(two, 1, 1, 65, 40, 33)
        assert C.same_bits(a, b)
        c = _address(two, 5, 1, 64, 40, 33)  # (at 64 tokens it is the fp16 form: other bits)
        assert not torch.equal(c["q"], _address(two, 1, 1, 64, 40, 33)["q"])


@pytest.mark.parametrize("prec,base", [(3, 1), (4, 1), (6, 5), (7, 5)])
def test_fp8_codes_run_their_base_modes_projection(prec, base):
    for two in (False, True):
        assert C.same_bits(_address(two, prec, 2, 3, 70, 33), _address(two, base, 2, 3, 70, 33))


# ---------------------------------------------------------------------------------------------- many work items
def test_many_work_items_per_proj3_block():
    """More (set, panel, tile) work items than 2 * P3W per CU: proj3_kernel's grid is one block per CU, so every
    block holds more than 2 * P3W items, every wave loops, and blocks run across panel and set boundaries."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    T, nq = 40, 256
    need = (2 * P3W * cus - math.ceil(T * nq / 32)) / 3  # ceil(T N / 32) must exceed it
    N = max(64, math.ceil((math.floor(need) + 1) * 32 / T / 64) * 64)
    items = 3 * math.ceil(T * N / 32) + math.ceil(T * nq / 32)
    assert items > 2 * P3W * cus, (cus, N, items)
    _address(False, 0, 1, T, N + nq, N)


# ---------------------------------------------------------------------------------------------- normal data
@pytest.mark.parametrize("S,N,T,M", NORMAL_SHAPES)
@pytest.mark.parametrize("prec", C.MODES)
def test_normal_data_within_the_derived_bounds(prec, S, N, T, M):
    for two in (False, True):
        eng = _engine(two, "normal")
        X = C.normal_state(M, T, S)
        r = _ref("normal", two, prec, M, T, S, N, False)
        odt = C.out_dtype(prec)
        fill = torch.tensor(float("nan"), dtype=odt)
        q, k, vt = eng.item_qkv(0, X.transpose(1, 2).float(), N, prec, fill=fill)
        got = dict(q=q.cpu(), k=k.cpu(), vt=vt.cpu())
        for o in OUTS:
            assert got[o].dtype == odt and got[o].shape == r["pre"][o].shape
            assert torch.equal(torch.isnan(got[o]), ~r["written"][o]), f"{o}: stored where it should not, or not stored"
        worst = C.ratios(got, r)
        where = f"S {S} N {N} T {T} M {M} two {two}"
        print(f"normal prec {prec} {where}: kernel / bound", {o: round(v, 3) for o, v in worst.items()})
        for o, v in worst.items():
            if not v <= _WORST.get((prec, o), (-1.0, ""))[0]:
                _WORST[prec, o] = (v, where)
        assert max(worst.values()) <= 1.0, (prec, where, worst)


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals_leave_buffers_and_context_as_they_were():
    from multimodalpfn_amd import _lib

    eng = _engine(True, "address")
    M, T, S, N = 2, 3, 70, 33
    X = C.address_state(M, T, S).float().to(eng.device)
    buf = _buffers(0, _shapes(M, T, S, N, False), eng.device)
    before = {o: b.clone() for o, b in buf.items()}
    x, q, k, vt = X.data_ptr(), buf["q"].data_ptr(), buf["k"].data_ptr(), buf["vt"].data_ptr()
    call = eng.lib.mmpfn_item_qkv
    eng._bind_stream()
    for what, args in [("geometry", (0, x, 0, T, 0, M, 0, 0, q, k, vt)),
                       ("geometry", (0, x, -1, T, 0, M, 0, 0, q, k, vt)),
                       ("geometry", (0, x, S, 0, N, M, 0, 0, q, k, vt)),
                       ("geometry", (0, x, S, -2, N, M, 0, 0, q, k, vt)),
                       ("member count", (0, x, S, T, N, 0, 0, 0, q, k, vt)),
                       ("member count", (0, x, S, T, N, -1, 0, 0, q, k, vt)),
                       ("geometry", (0, x, S, T, -1, M, 0, 0, q, k, vt)),
                       ("geometry", (0, x, S, T, S + 1, M, 0, 0, q, k, vt)),
                       ("null projection output", (0, x, S, T, N, M, 0, 0, None, k, vt)),
                       ("null projection output", (0, x, S, T, N, M, 0, 0, q, None, vt)),
                       ("null projection output", (0, x, S, T, N, M, 0, 0, q, k, None)),
                       ("layer index", (1, x, S, T, N, M, 0, 0, q, k, vt)),
                       ("layer index", (-1, x, S, T, N, M, 0, 0, q, k, vt)),
                       ("precision", (0, x, S, T, N, M, 0, 8, q, k, vt)),
                       ("precision", (0, x, S, T, N, M, 0, -1, q, k, vt))]:
        # set a marker first, so that a stale message of the call before cannot pass for this one's
        assert eng.lib.mmpfn_mlp_ln(eng.ctx, 0, x, 0, 0) == _lib.MMPFN_ERR_INVALID
        marker = eng.lib.mmpfn_last_error(eng.ctx).decode()
        assert call(eng.ctx, *args) == _lib.MMPFN_ERR_INVALID, (what, args)
        msg = eng.lib.mmpfn_last_error(eng.ctx).decode()
        assert what in msg and msg != marker, (what, msg)
    assert call(eng.ctx, 0, None, S, T, N, M, 0, 0, q, k, vt) == _lib.MMPFN_ERR_INVALID  # (tap_check: a null state)
    assert call(None, 0, x, S, T, N, M, 0, 0, q, k, vt) == _lib.MMPFN_ERR_INVALID  # (no context: no message)
    torch.cuda.synchronize()
    for o in OUTS:
        assert torch.equal(buf[o], before[o]), f"a refused call wrote to {o}"
    for prec in C.MODES:  # a good call afterwards passes
        _address(True, prec, M, T, S, N)
