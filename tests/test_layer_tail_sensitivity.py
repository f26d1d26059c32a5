"""CPU: what the bounds of tests/layer_tail_cases.py catch, and what ties its restatement to the oracle.

Each fault below is a mistake ``mlp_rows_kernel`` (mlp_rows.hip) or its weight packing (weight_pack.h) could make,
applied to the float64 restatement itself.  Every one must move some element by at least ten times that element's
bound, on the normal-data case in every mode and on the integer case that targets it.  The erf GELU in place of the
16-bit modes' tanh form is the counter-example: it must stay *below* the bf16 bound on normal data -- the test asserts
what common.h claims (the tanh form, rounded as the mode rounds), not bit-identity.  Measured there: max 3.65e-3 against
q = 5.96e-3 (0.61), RMS 5.0e-4 against 1.35e-3 (0.37).
"""

import pytest
import torch

import layer_tail_cases as L
import oracle.forward as ofw
from helpers import oracle_spec
from test_taps_gpu import TOL

from multimodalpfn_amd.model.spec import ModelConfig

K = ("X", "O", "Wout", "W1", "W2")
ROWS, NHID = 129, 768
_CACHE: dict = {}


def f16_row_perm(r: int) -> int:
    """weight_pack.h: the fp16 mode's output-row order (image row r holds weight row f16_row_perm(r))."""
    f, rho = r >> 4, r & 15
    return 32 * (f >> 1) + 8 * (rho >> 2) + 4 * (f & 1) + (rho & 3)


PERM = [f16_row_perm(r) for r in range(L.E)]
INV = [PERM.index(r) for r in range(L.E)]


def _case(kind: str) -> dict:
    if kind not in _CACHE:
        make = dict(normal=L.normal_case, prologue=L.prologue_case, mlp=L.mlp_case,
                    mlp_light=lambda rows, nhid: L.mlp_case(rows, nhid, light=True))[kind]
        _CACHE[kind] = make(257 if kind == "normal" else ROWS, NHID)
    return _CACHE[kind]


def _ops(c: dict) -> dict:
    return {k: c[k] for k in K}


def _ref(kind: str, mode: int):
    """(reference, per-element bound) of a case in a mode."""
    if (kind, mode) not in _CACHE:
        c = _case(kind)
        r = L.tail(mode, **_ops(c))
        if kind == "normal":
            b = L.normal_bounds(mode, r, L.tail(mode, exact=True, **_ops(c)), TOL)
            bound = L.normal_elem_bound(mode, r, b)
        else:
            bound = L.prologue_bound(mode, r) if kind == "prologue" else L.mlp_bound(mode, r, c["W2"])
        _CACHE[kind, mode] = (r, bound)
    return _CACHE[kind, mode]


def _swap_cols(W: torch.Tensor, a, b) -> torch.Tensor:
    W = W.clone()
    W[:, a], W[:, b] = W[:, b].clone(), W[:, a].clone()
    return W


def _stale_chunk(c: int):
    def f(case):
        W1 = case["W1"].clone()
        W1[32 * c: 32 * c + 32] = case["W1"][32 * (c - 1): 32 * c]
        return dict(W1=W1)
    return f


def _w1_k_swap(case):
    k1 = int(case["W1"][0].nonzero()[0])  # a feature some hidden unit reads
    return dict(W1=_swap_cols(case["W1"], k1, (k1 + 5) % L.E))


def _drop_last(case):
    W2 = case["W2"].clone()
    W2[:, -32:] = 0
    return dict(W2=W2)


def _wout_units(case):
    W = case["Wout"].clone()
    W[37, 0:8], W[37, 8:16] = case["Wout"][37, 8:16], case["Wout"][37, 0:8]
    return dict(Wout=W)


# name -> (the integer case that targets it, changed operands, restatement fault, output fault)
FAULTS = {
    "wout_halves_exchanged": ("prologue", lambda c: dict(Wout=torch.cat([c["Wout"][96:], c["Wout"][:96]])), None),
    "wout_rows_natural_where_f16_perm": ("prologue", lambda c: dict(Wout=c["Wout"][INV]), None),
    "wout_rows_f16_perm_where_natural": ("prologue", lambda c: dict(Wout=c["Wout"][PERM]), None),
    "wout_two_16B_units_exchanged": ("prologue", _wout_units, None),
    "w1_slot_read_one_fill_early_c3": ("mlp", _stale_chunk(3), None),
    "w1_slot_read_one_fill_early_c4": ("mlp", _stale_chunk(4), None),
    "w1_slot_read_one_fill_early_c5": ("mlp", _stale_chunk(5), None),
    "last_hidden_chunk_dropped": ("mlp", _drop_last, None),
    "w2_two_hidden_units_exchanged": ("mlp", lambda c: dict(W2=_swap_cols(c["W2"], 67, 81)), None),
    "w1_two_features_exchanged": ("mlp", _w1_k_swap, None),
    "residual_from_x": ("prologue", lambda c: {}, "residual_x"),
    "operand_unnormalised": ("mlp_light", lambda c: {}, "operand_raw"),
    "row_m1_duplicated_into_m2": ("prologue", lambda c: {}, "row_dup"),
}


def _faulty(kind: str, mode: int, name: str) -> torch.Tensor:
    _, change, fault = FAULTS[name]
    c = _case(kind)
    out = L.tail(mode, **{**_ops(c), **change(c)}, fault=fault if fault != "row_dup" else None)["out"]
    if fault == "row_dup":
        out = out.clone()
        out[-2] = out[-1]
    return out


@pytest.mark.parametrize("mode", L.MODES)
@pytest.mark.parametrize("name", list(FAULTS))
def test_fault_moves_an_element_ten_bounds(name, mode):
    for kind in ("normal", FAULTS[name][0]):
        r, bound = _ref(kind, mode)
        ratio = float(((_faulty(kind, mode, name) - r["pre"]).abs() / bound).max())
        print(f"{name} mode {mode} {kind}: largest move / bound {ratio:.1f}")
        assert ratio >= 10.0, (name, mode, kind, ratio)


def test_f16_row_perm_faults_are_faults():
    """The two row-order faults are distinct permutations, neither the identity."""
    assert PERM != list(range(L.E)) and INV != PERM and sorted(PERM) == list(range(L.E))


@pytest.mark.parametrize("mode", [1, 5])
def test_erf_gelu_stays_below_the_bf16_bound_on_normal_data(mode):
    """The erf form differs from the specified tanh form by less than the mode-1 bound: the GPU test holds the kernel
    to the form common.h states, within the rounding's own effect, and not to bit-identity."""
    c = _case("normal")
    r, _ = _ref("normal", mode)
    b = L.normal_bounds(1, _ref("normal", 1)[0], L.tail(1, exact=True, **_ops(c)), TOL)
    d = L.tail(mode, **_ops(c), gelu=L.gelu_erf)["out"] - r["out"]
    mx, rms = float(d.abs().max()), float(d.pow(2).mean().sqrt())
    print(f"erf for tanh, mode {mode}: max {mx:.3e} / {b['max']:.3e}, rms {rms:.3e} / {b['rms']:.3e}")
    assert 0 < mx < b["max"] and rms < b["rms"]


# ---------------------------------------------------------------------------------------------- the cases themselves
@pytest.mark.parametrize("factor", L.NHID_FACTORS)
@pytest.mark.parametrize("mode", L.MODES)
def test_integer_cases_are_what_their_bounds_assume(mode, factor):
    nhid = L.E * factor
    c = L.mlp_case(ROWS, nhid)
    r = L.tail(mode, **_ops(c))
    L.check_mlp_case(mode, c, r)
    cu = L.mlp_case(ROWS, nhid, unit=True)  # the mmpfn_mlp_ln form: X = +-1 itself
    ru = L.mlp_only(mode, cu["X"], cu["W1"], cu["W2"])
    if L.OP[mode] is not None:
        pre = ru["y"]
        assert ((pre - pre.round()).abs() < 1e-15).all()  # an exact integer in front of the LayerNorm
    c = L.prologue_case(ROWS, nhid)
    L.check_prologue_case(c, L.tail(mode, **_ops(c)))
    for b in (L.mlp_bound(mode, r, L.mlp_case(ROWS, nhid)["W2"]), L.prologue_bound(mode, L.tail(mode, **_ops(c)))):
        assert torch.isfinite(b).all() and float(b.min()) > 0 and float(b.max()) < 0.05


@pytest.mark.parametrize("factor", L.NHID_FACTORS)
def test_normal_case_spreads_the_variance(factor):
    """X, O Wout^T and the MLP term each carry about a third of the variance in front of the last LayerNorm, so a
    fault in any one of them is not hidden behind the other two."""
    shares = L.variance_shares(L.normal_case(257, L.E * factor))
    print(f"nhid {L.E * factor}: variance shares X {shares[0]:.3f}, O.Wout^T {shares[1]:.3f}, MLP {shares[2]:.3f}")
    assert abs(sum(shares) - 1.0) < 1e-12 and all(0.25 <= s <= 0.42 for s in shares)


@pytest.mark.parametrize("mode", [1, 5])
def test_sixteen_bit_bounds_are_the_roundings_own_effect(mode):
    """q is a few 16-bit ulps of an O(1) result: far below the 1e-2 .. 2e-2 of the whole-layer tolerances."""
    c = _case("normal")
    b = L.normal_bounds(mode, _ref("normal", mode)[0], L.tail(mode, exact=True, **_ops(c)), TOL)
    print(f"mode {mode}: q max {b['max']:.3e}, rms {b['rms']:.3e}")
    assert 0 < b["rms"] < b["max"] < (8e-3 if mode == 1 else 2e-3)


# ---------------------------------------------------------------------------------------------- the oracle tie
def _oracle_weights(c: dict) -> dict:
    p = "transformer_encoder.layers.0."
    return {p + "self_attn_between_items._w_out": L.w_out_param(c["Wout"]),
            p + "self_attn_between_items._w_qkv": torch.zeros(3, L.H, L.HD, L.E, dtype=torch.float64),
            p + "mlp.linear1.weight": c["W1"], p + "mlp.linear2.weight": c["W2"]}


def test_mlp_half_is_the_oracles_mlp_sublayer():
    c = L.normal_case(33, 576)
    spec = oracle_spec(ModelConfig(nlayers=1, nhid_factor=3, mixer_type=None))
    ref = ofw.mlp_sublayer(spec, _oracle_weights(c), 0, c["X"])
    got = L.mlp_half(0, c["X"], c["W1"], c["W2"])["out"]
    assert float((got - ref).abs().max()) < 1e-12
    assert float((L.mlp_only(2, c["X"], c["W1"], c["W2"])["out"] - ref).abs().max()) < 1e-12


def test_prologue_is_the_oracles_out_projection_and_layernorm(monkeypatch):
    """``item_sublayer`` with its attention replaced by a given output: what is left are the oracle's own
    out-projection einsum, residual and LayerNorm lines, and with them the O[row][32 h + d] <-> _w_out[h][d][e]
    mapping that ``wout_matrix`` / ``w_out_param`` state."""
    S, T = 7, 5
    c = L.normal_case(S * T, 192)
    spec = oracle_spec(ModelConfig(nlayers=1, nhid_factor=1, mixer_type=None))
    O = c["O"].reshape(S, T, L.H, L.HD)  # row s * T + t
    monkeypatch.setattr(ofw, "_attn", lambda q, k, v, use_sdpa=False: O.permute(1, 2, 0, 3))  # [T, H, S, d]
    ref = ofw.item_sublayer(spec, _oracle_weights(c), 0, c["X"].reshape(S, T, L.E), S)
    got = L.prologue(0, c["X"], c["O"], c["Wout"])["xp"].reshape(S, T, L.E)
    assert float((got - ref).abs().max()) < 1e-12
    assert torch.equal(L.wout_matrix(L.w_out_param(c["Wout"])), c["Wout"])
    whole = L.tail(2, **_ops(c))["out"].reshape(S, T, L.E)
    assert float((whole - ofw.mlp_sublayer(spec, _oracle_weights(c), 0, ref)).abs().max()) < 1e-12
