"""GPU: the item attention's softmax(Q K^T) V alone, per element, in the forms the forwards launch it in.

``mmpfn_item_attention_forward`` launches ``attn_pipe_kernel`` (16-bit codes), ``attn_item3_kernel`` (mode 0) or
``attn_item_kernel<0, 4>`` (mode 2) with the arguments of capi.cpp ``item_attn_args``, the function the layers call: Q
prescaled in the 16-bit modes, the full layer's, the pruned last layer's and the cache predict's task maps.  The older
taps (``mmpfn_item_attention_layer``, ``_layer_ex`` code 5, ``_cached``) give the unprescaled Q load and fp16 Q / K.
Operands, the float64 restatement, the bounds and the faults they catch: tests/item_attn_cases.py (no bound there comes
from a kernel run) and tests/test_item_attn_sensitivity.py.

Every launch writes into a sentinel-filled out buffer with a sentinel guard behind it; q, k and vt (K rows and V^T
columns [N, Npad) NaN) must come back bit-unchanged.

* Selection case, bit for bit (modes 0 and 2: sentinels on bits, values within 4 u |v|), with and without the per-query
  shifts that send waves through the re-run and the backstop: form 0 over 1 .. 12 key tiles with and without a partial
  one, each N with two of 0 / 1 / 43 / 130 test rows at T = 1 and T = 3; form 1 with a0 = 0, a0 > 0 and na = 0; form 2;
  H = 1 and H = 8; every precision code (the fp8 codes here only).
* Form 1's stored rows equal form 0's, and form 2's equal form 0's test rows, bit for bit on the same operands.
* Spread case against the derived per-element bound over the same N / Q / T lists and forms, plain and shifted (state
  2; the unprescaled taps state 1, see item_attn_cases), modes 0, 1, 2, 5 and the older taps.
* Refusals launch nothing.

Worst kernel / bound of the spread case measured on an MI355X (``helpers.report`` prints them with every run), forms
0 / 1 / 2: mode 0 0.822 / 0.713 / 0.597 (at N = 1, where the dropped V lo x P lo product is nearly the whole bound; 0.597
in the shifted state); mode 1 0.925 / 0.834 / 0.813 (shifted 0.915); mode 2 0.023 / 0.018 / 0.013; mode 5 0.746 / 0.569 /
0.624 (shifted 0.746); ``mmpfn_item_attention_layer`` 0.907, ``_layer_ex`` code 5 0.762, ``_cached`` 0.803.  The 16-bit
ratios are mostly the output's half ulp and P's (the stored restatement itself reaches 0.78 in bf16,
tests/test_item_attn_sensitivity.py).  Every selection-case comparison is bit for bit (modes 0 and 2: within 4 u |v|).
"""

import math

import pytest
import torch

import item_attn_cases as C
from helpers import report

pytestmark = pytest.mark.gpu

GUARD = 64 * C.H * C.HD  # elements behind out: 64 rows' worth
FWD_CODES = (0, 1, 2, 3, 4, 5, 6, 7)
_CASES: dict = {}
_REFS: dict = {}
_WORST: dict = {}  # (tap, form) -> (ratio, where)
_CTX: list = []


@pytest.fixture(scope="module", autouse=True)
def _context_and_report():
    yield
    for key in sorted(_WORST):
        report(f"item attention spread {key[0]} form {key[1]}: worst kernel / bound {_WORST[key][0]:.3f} ({_WORST[key][1]})")
    if _CTX:
        torch.cuda.synchronize()
        _CTX[0][0].mmpfn_destroy(_CTX[0][1])
    _CTX.clear(), _CASES.clear(), _REFS.clear(), _WORST.clear()


def _ctx():
    if not _CTX:
        from multimodalpfn_amd import _lib
        from multimodalpfn_amd.engine import HipEngine  # noqa: F401  (initialises the runtime as the engine does)

        lib = _lib.load_library()
        _CTX.append((lib, lib.mmpfn_create(0, None)))
    return _CTX[0]


def _way(tap: str) -> C.Way:
    """tap: "fwd<code>", "layer" (mmpfn_item_attention_layer), "layer_f16" (_layer_ex code 5), "cached"."""
    if tap.startswith("fwd"):
        return C.forward_way(int(tap[3:]))
    return C.OLD_F16 if tap == "layer_f16" else C.OLD_BF16


def _case(kind: str, T: int, S: int, N: int, prescaled: bool, state: int, nh: int = C.H) -> dict:
    key = (kind, T, S, N, prescaled, state, nh)
    if key not in _CASES:
        _CASES[key] = (C.selection_case(T, S, N, prescaled, bool(state), nh) if kind == "selection"
                       else C.spread_case(T, S, N, prescaled, state, nh))
    return _CASES[key]


def _operands(kind: str, way: C.Way, form: int, T: int, S: int, N: int, state: int, nh: int) -> dict:
    """The stored operands of a launch: S counts the rows of the form-0 case the others derive from."""
    c = _case(kind, T, S, N, way.prescaled, state, nh)
    if kind == "spread":
        c = C.stored(way, c)
    return C.cached_operands(c) if form == 2 else c


def _ref(kind: str, way: C.Way, form: int, T: int, S: int, N: int, state: int, nh: int = C.H) -> dict:
    key = (kind, way, form, T, S, N, state, nh)
    if key not in _REFS:
        c = _operands(kind, way, form, T, S, N, state, nh)
        _REFS[key] = C.attend(way, form, c["q"], c["k"], c["vt"], N, want_mag=kind == "spread")
    return _REFS[key]


def _launch(tap: str, form: int, c: dict) -> torch.Tensor:
    """One launch on the case's operands; returns out as integers of the output type, [T][S][H * 32]."""
    lib, ctx = _ctx()
    way = _way(tap)
    T, nh, S, _ = c["q"].shape
    N, Npad = c["N"], c["k"].shape[2]
    qk = way.qk or torch.float32
    vdt = torch.bfloat16 if C.is16(way) else torch.float32
    q, k, vt = c["q"].to("cuda", qk), c["k"].to("cuda", qk), c["vt"].to("cuda", vdt)
    assert torch.equal(q.double().cpu(), c["q"]), "the case's q is not exact in the launch's type"
    keep = [t.clone() for t in (q, k, vt)]
    n = T * S * nh * C.HD
    out = torch.full((n + GUARD,), C.SENTINEL[way.out], dtype=C.INT[way.out], device="cuda")
    args = (ctx, q.data_ptr(), k.data_ptr(), vt.data_ptr(), out.data_ptr(), S, T, nh, Npad, N)
    if tap.startswith("fwd"):
        rc = lib.mmpfn_item_attention_forward(*args, form, int(tap[3:]))
    elif tap == "layer":
        assert form == 0
        rc = lib.mmpfn_item_attention_layer(*args)
    elif tap == "layer_f16":
        assert form == 0
        rc = lib.mmpfn_item_attention_layer_ex(*args, 5)
    else:
        assert tap == "cached" and form == 2
        rc = lib.mmpfn_item_attention_cached(*args)
    assert rc == 0, (tap, form, rc, lib.mmpfn_last_error(ctx).decode())
    torch.cuda.synchronize()
    for name, a, b in zip("q k vt".split(), (q, k, vt), keep):
        it = torch.int16 if a.element_size() == 2 else torch.int32
        assert torch.equal(a.view(it), b.view(it)), f"{name} was modified"
    o = out.cpu()
    assert bool((o[n:] == C.SENTINEL[way.out]).all()), "elements behind out were written"
    return o[:n].view(T, S, nh * C.HD)


def _describe(got: torch.Tensor, r: dict) -> str:
    want, w = C.bits(r), r["written"]
    sent = C.SENTINEL[r["out"].dtype]
    bad = got != want
    first = [int(i) for i in bad.nonzero()[0]] if bool(bad.any()) else None
    return (f"{int(bad.sum())} elements differ in bits, first at {first}; {int((bad & ~w).sum())} outside what the form "
            f"stores, {int((w & (got == sent)).sum())} never written")


def _selection(tap: str, form: int, T: int, S: int, N: int, state: int, nh: int = C.H) -> torch.Tensor:
    way = _way(tap)
    got = _launch(tap, form, _operands("selection", way, form, T, S, N, state, nh))
    r = _ref("selection", way, form, T, S, N, state, nh)
    assert C.selection_passes(got, r), f"{tap} form {form} T {T} S {S} N {N} shifted {state} H {nh}: " + _describe(got, r)
    return got


# ---------------------------------------------------------------------------------------------- selection, form 0
@pytest.mark.parametrize("i", range(len(C.N_FULL)), ids=[f"N{n}" for n in C.N_FULL])
@pytest.mark.parametrize("prec", FWD_CODES)
def test_full_layer_selects_the_chosen_key(prec, i):
    N, (qa, qb) = C.N_FULL[i], C.q_pairs(i)
    for state in (0, 1):
        _selection(f"fwd{prec}", 0, 1, N + qa, N, state)
        _selection(f"fwd{prec}", 0, 3, N + qb, N, state)


def test_a_block_count_that_is_no_multiple_of_eight_occurs():
    blocks = lambda T, S, N: T * sum(math.ceil((N + (C.H * (S - N) if g == 0 else 0)) / C.QPB) for g in range(C.H))
    counts = [blocks(T, N + C.q_pairs(i)[j], N) for i, N in enumerate(C.N_FULL) for j, T in ((0, 1), (1, 3))]
    assert any(c % 8 for c in counts) and any(c % 8 == 0 for c in counts), counts


# ---------------------------------------------------------------------------------------------- forms 1 and 2
@pytest.mark.parametrize("i", range(len(C.N_LAST)), ids=[f"N{n}" for n in C.N_LAST])
@pytest.mark.parametrize("prec", FWD_CODES)
def test_last_layers_form_selects_and_equals_the_full_form(prec, i):
    N, T = C.N_LAST[i], 3
    a0, _ = C.own_rows(1, 0, N)
    for nq, state in ((C.Q_LAST[i % 3], 0), (C.Q_LAST[(i + 1) % 3], 1)):
        S = N + nq
        last = _selection(f"fwd{prec}", 1, T, S, N, state)
        full = _selection(f"fwd{prec}", 0, T, S, N, state)
        assert torch.equal(last[:, a0:], full[:, a0:]), "the last layer's stored rows differ from the full layer's"
        sent = C.SENTINEL[_way(f"fwd{prec}").out]
        assert bool((last[:, :a0] == sent).all())


@pytest.mark.parametrize("S,N", C.CACHED)
@pytest.mark.parametrize("prec", FWD_CODES)
def test_cached_form_selects_and_equals_the_full_forms_test_rows(prec, S, N):
    """Bit for bit wherever both launches take the same path for a query.  The shifted state sends queries through a
    re-run that is decided per wave (mode 0: per block), and the cached form packs other queries into a wave than the
    full layer does; the 16-bit selection results are exact on every path, so they stay bit-equal, while modes 0 and 2
    hold each launch to 4 u |v| of the chosen vector there."""
    T = 3
    for state in (0, 1):
        cached = _selection(f"fwd{prec}", 2, T, N + S, N, state)
        full = _selection(f"fwd{prec}", 0, T, N + S, N, state)
        if state == 0 or C.is16(_way(f"fwd{prec}")):
            assert torch.equal(cached, full[:, N:]), "the cached form differs from the full layer's test rows"


@pytest.mark.parametrize("nh", [1, 8])
@pytest.mark.parametrize("prec", FWD_CODES)
def test_one_and_eight_heads(prec, nh):
    for state in (0, 1):
        _selection(f"fwd{prec}", 0, 3, 129 + 43, 129, state, nh)
        _selection(f"fwd{prec}", 1, 3, 321 + 43, 321, state, nh)
        _selection(f"fwd{prec}", 2, 3, 65 + 37, 65, state, nh)


# ---------------------------------------------------------------------------------------------- the older taps
@pytest.mark.parametrize("i", range(len(C.N_FULL)), ids=[f"N{n}" for n in C.N_FULL])
@pytest.mark.parametrize("tap", ["layer", "layer_f16"])
def test_unprescaled_taps_select_the_chosen_key(tap, i):
    N, (qa, qb) = C.N_FULL[i], C.q_pairs(i)
    for state in (0, 1):
        _selection(tap, 0, 1, N + qa, N, state)
        _selection(tap, 0, 3, N + qb, N, state)


@pytest.mark.parametrize("S,N", C.CACHED)
def test_unprescaled_cached_tap_selects_the_chosen_key(S, N):
    for state in (0, 1):
        cached = _selection("cached", 2, 3, N + S, N, state)
        assert torch.equal(cached, _selection("layer", 0, 3, N + S, N, state)[:, N:])


# ---------------------------------------------------------------------------------------------- spread
def _spread(tap: str, form: int, T: int, S: int, N: int, state: int) -> torch.Tensor:
    way = _way(tap)
    got = _launch(tap, form, _operands("spread", way, form, T, S, N, state, C.H))
    r = _ref("spread", way, form, T, S, N, state)
    sent = C.SENTINEL[way.out]
    w = r["written"]
    assert bool((got[~w] == sent).all()), f"{tap} form {form}: stored outside the form's rows"
    vals = got.view(way.out).double()
    worst = C.ratio(vals, r)
    where = f"S {S} N {N} T {T} state {state}"
    print(f"spread {tap} form {form} {where}: kernel / bound {worst:.3f}")
    if not worst <= _WORST.get((tap, form), (-1.0, ""))[0]:
        _WORST[tap, form] = (worst, where)
    assert worst <= 1.0, (tap, form, where, worst)
    return got


SPREAD_CODES = (0, 1, 2, 5)
SPREAD_STATES = (0, 2)  # plain; and the shifted one that holds state 1's shifts and the late +120


@pytest.mark.parametrize("i", range(len(C.N_FULL)), ids=[f"N{n}" for n in C.N_FULL])
@pytest.mark.parametrize("prec", SPREAD_CODES)
def test_full_layer_spread_within_the_derived_bound(prec, i):
    N, (qa, qb) = C.N_FULL[i], C.q_pairs(i)
    for state in SPREAD_STATES:
        _spread(f"fwd{prec}", 0, 1, N + qa, N, state)
        _spread(f"fwd{prec}", 0, 3, N + qb, N, state)


@pytest.mark.parametrize("i", range(len(C.N_LAST)), ids=[f"N{n}" for n in C.N_LAST])
@pytest.mark.parametrize("prec", SPREAD_CODES)
def test_last_layers_form_spread_within_the_bound_and_equal_to_the_full_form(prec, i):
    """Form 1 keeps every query's place in its wave and block: bit-equal to form 0 in every state."""
    N, T = C.N_LAST[i], 3
    a0, _ = C.own_rows(1, 0, N)
    for nq, state in ((C.Q_LAST[i % 3], SPREAD_STATES[0]), (C.Q_LAST[(i + 1) % 3], SPREAD_STATES[1])):
        last = _spread(f"fwd{prec}", 1, T, N + nq, N, state)
        full = _spread(f"fwd{prec}", 0, T, N + nq, N, state)
        assert torch.equal(last[:, a0:], full[:, a0:]), "the last layer's stored rows differ from the full layer's"


@pytest.mark.parametrize("S,N", C.CACHED)
@pytest.mark.parametrize("prec", SPREAD_CODES)
def test_cached_form_spread_within_the_bound_and_equal_to_the_full_forms_test_rows(prec, S, N):
    """Form 2 packs its waves otherwise than form 0, so where a wave re-runs (the shifted state) another query may take
    another path; in state 0 every wave keeps its first pass and the two are bit-equal."""
    for state in SPREAD_STATES:
        cached = _spread(f"fwd{prec}", 2, 3, N + S, N, state)
        if state == 0:
            assert torch.equal(cached, _spread(f"fwd{prec}", 0, 3, N + S, N, state)[:, N:]), \
                "the cached form differs from the full layer's test rows"


# (states 0 and 1: the unprescaled taps' backstop takes q * c unrounded, item_attn_cases)
@pytest.mark.parametrize("i", range(len(C.N_FULL)), ids=[f"N{n}" for n in C.N_FULL])
@pytest.mark.parametrize("tap", ["layer", "layer_f16"])
def test_unprescaled_taps_spread_within_the_derived_bound(tap, i):
    N, (qa, qb) = C.N_FULL[i], C.q_pairs(i)
    for state in (0, 1):
        _spread(tap, 0, 1, N + qa, N, state)
        _spread(tap, 0, 3, N + qb, N, state)


@pytest.mark.parametrize("S,N", C.CACHED)
def test_unprescaled_cached_tap_spread_within_the_derived_bound(S, N):
    for state in (0, 1):
        _spread("cached", 2, 3, N + S, N, state)


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals_launch_nothing():
    from multimodalpfn_amd import _lib

    lib, ctx = _ctx()
    T, S, N, nh, Npad = 3, 70, 33, C.H, 64
    c = _operands("selection", C.forward_way(1), 0, T, S, N, 0, nh)
    q, k, vt = (c[o].to("cuda", torch.bfloat16) for o in ("q", "k", "vt"))
    out = torch.full((T * S * nh * C.HD + GUARD,), C.SENTINEL[torch.bfloat16], dtype=torch.int16, device="cuda")
    before = out.clone()
    p = (q.data_ptr(), k.data_ptr(), vt.data_ptr(), out.data_ptr())
    call = lib.mmpfn_item_attention_forward
    for what, args in [("form", (*p, S, T, nh, Npad, N, 3, 1)),
                       ("form", (*p, S, T, nh, Npad, N, -1, 1)),
                       ("precision", (*p, S, T, nh, Npad, N, 0, 8)),
                       ("precision", (*p, S, T, nh, Npad, N, 0, -1)),
                       ("geometry", (*p, S, 0, nh, Npad, N, 0, 1)),
                       ("geometry", (*p, S, -1, nh, Npad, N, 2, 1)),
                       ("geometry", (*p, 0, T, nh, Npad, N, 2, 1)),
                       ("geometry", (*p, S, T, nh, Npad, 0, 0, 1)),
                       ("geometry", (*p, S, T, nh, Npad, S + 1, 0, 1)),
                       ("geometry", (*p, S, T, nh, Npad, 65, 2, 1)),
                       ("geometry", (*p, S, T, nh, 96, N, 0, 1)),
                       ("geometry", (*p, S, T, 9, Npad, N, 0, 1)),
                       ("geometry", (*p, S, T, 0, Npad, N, 0, 1)),
                       ("test rows", (*p, N, T, nh, Npad, N, 1, 1)),
                       ("test rows", (*p, N, T, nh, Npad, N, 1, 0))]:
        # set a marker first, so that a stale message of the call before cannot pass for this one's
        assert lib.mmpfn_item_attention(ctx, *p, S, T, nh, Npad, 0, N, N, -1, 5) == _lib.MMPFN_ERR_INVALID
        marker = lib.mmpfn_last_error(ctx).decode()
        assert call(ctx, *args) == _lib.MMPFN_ERR_INVALID, (what, args)
        msg = lib.mmpfn_last_error(ctx).decode()
        assert what in msg and msg != marker, (what, msg)
    for i in range(4):  # a null operand, and no context
        a = list(p)
        a[i] = None
        assert call(ctx, *a, S, T, nh, Npad, N, 0, 1) == _lib.MMPFN_ERR_INVALID
    assert call(None, *p, S, T, nh, Npad, N, 0, 1) == _lib.MMPFN_ERR_INVALID
    torch.cuda.synchronize()
    assert torch.equal(out, before), "a refused call wrote to out"
    for prec in FWD_CODES:  # a good call afterwards passes
        _selection(f"fwd{prec}", 0, T, S, N, 0)
