"""CPU: the bounds of tests/test_modality_kernels_gpu.py would catch a tower kernel that is subtly wrong.

The GEMM tap is held to per-element bounds derived from fp32 summation (tests/modality_kernel_cases.py), the
attention tap to 1e-2 (bf16) of ``rel``.  Those only mean something if the mistakes such kernels can make move the
result by much more.  Each test here applies one such mistake to the float64 reference itself.

GEMM, on the normal-data operands of the towers' shapes (``TOWER_SHAPES``), some element must move by at least
10 x its bound:

* the last 32-wide K slice dropped (a ring stage never waited for);
* two adjacent 16-B chunks (8 bf16) of a K slice of A exchanged (a wrong swizzle slot);
* the outputs of two neighbouring tiles exchanged (the block-to-tile map);
* ``bias`` / ``gamma`` read at ``n0 = 0`` by every tile;
* row M-1 duplicated into row M-2 (the clamped A rows of the last M tile reaching the store).

Attention, at L = 65 (one full key tile and a partial one of one key), the reference must move by at least 5 x the
bf16 bound:

* the last key of the partial tile dropped;
* the finite key bias added to the log2-unit scores without the log2(e) factor.

Also here: the float64 grid check of the tanh-form GELU against the erf form that common.h's comment quotes.
"""

import math

import pytest
import torch

import modality_kernel_cases as mk
from test_modality_gpu import _attn_ref, rel

GEMM_FACTOR = 10.0
ATTN_BF16_BOUND = 1e-2
ATTN_MIN_MOVE = 5 * ATTN_BF16_BOUND

_CASES: dict = {}


def _case(name):
    """Operands, float64 pre-activation, reference and bound of one tower shape (computed once, left unchanged)."""
    if name not in _CASES:
        _, _, _, _, epi, act, with_gamma = next(s for s in mk.TOWER_SHAPES if s[0] == name)
        ops = mk.tower_operands(name)
        gamma = ops["gamma"] if with_gamma else None
        pre = mk.preactivation(ops["A"], ops["W"], ops["bias"])
        ref = mk.expected(pre, epi, act, gamma, ops["c0"])
        bnd = mk.bound(pre, ref, mk.accb(ops), epi, act, gamma)
        _CASES.clear()  # one shape's float64 matrices at a time
        _CASES[name] = (ops, gamma, epi, act, ref, bnd)
    return _CASES[name]


def _worst(wrong, ref, bnd):
    return float(((wrong - ref).abs() / bnd).max())


def _faults(ops, gamma, epi, act):
    """name -> the float64 result a kernel with that fault would produce."""
    A, W, bias, c0 = ops["A"], ops["W"], ops["bias"], ops["c0"]
    K = ops["K"]

    def out(pre, g=gamma):
        return mk.expected(pre, epi, act, g, c0)

    yield "last K slice dropped", out(mk.preactivation(A[:, :K - 32], W[:, :K - 32], bias))
    A2 = A.clone()
    A2[:, 0:8], A2[:, 8:16] = A[:, 8:16], A[:, 0:8]
    yield "16-B chunks 0 and 1 of A's first K slice exchanged", out(mk.preactivation(A2, W, bias))
    good = out(mk.preactivation(A, W, bias))
    sw = good.clone()
    sw[0:256, 0:256], sw[0:256, 256:512] = good[0:256, 256:512], good[0:256, 0:256]
    yield "tiles (0, 0) and (0, 1) exchanged", sw
    reps = ops["N"] // 256
    yield "bias read at n0 = 0", out(mk.preactivation(A, W, bias[:256].repeat(reps)))
    if gamma is not None:
        yield "gamma read at n0 = 0", out(mk.preactivation(A, W, bias), gamma[:256].repeat(reps))
    dup = good.clone()
    dup[-2] = good[-1]
    yield "row M-1 duplicated into row M-2", dup


@pytest.mark.parametrize("name", [s[0] for s in mk.TOWER_SHAPES])
def test_gemm_faults_exceed_the_bounds(name):
    ops, gamma, epi, act, ref, bnd = _case(name)
    for what, wrong in _faults(ops, gamma, epi, act):
        worst = _worst(wrong, ref, bnd)
        print(f"{name}: {what}: worst |d| / bound {worst:.1f}")
        assert worst >= GEMM_FACTOR, (name, what, worst)


def test_gemm_reference_is_inside_its_own_bounds():
    """The float64 reference rounded the way the kernel stores it (fp32, or bf16 of fp32) sits inside the bound:
    the faults above are not measured against a bound that the storage format alone would exceed (bf16's unit
    roundoff is 2^-8: half a spacing of 2^-7 at the bottom of a binade)."""
    for name in ("qkv_bf16", "wide_f32"):
        ops, gamma, epi, act, ref, bnd = _case(name)
        stored = ref.float().bfloat16().double() if epi == mk.EPI_BF16 else ref.float().double()
        assert _worst(stored, ref, bnd) <= 1.0


def _attn_case(bias_scale):
    g = torch.Generator().manual_seed(65)
    B, L, H = 3, 65, 4
    qkv = torch.randn(B, L, 3, H, 64, generator=g).bfloat16().float()
    kb = bias_scale * torch.randn(B, L, generator=g)
    return qkv, kb


def test_attention_dropped_last_key_moves_the_reference():
    qkv, _ = _attn_case(0.0)
    ref = _attn_ref(qkv, None, bf16_q=True)
    kb = torch.zeros(qkv.shape[0], qkv.shape[1])
    kb[:, 64] = -float("inf")  # key 64: the one key of the partial second tile
    move = rel(_attn_ref(qkv, kb, bf16_q=True).numpy(), ref.numpy())
    print(f"L = 65: dropping key 64 moves the attention reference by {move:.3f}")
    assert move >= ATTN_MIN_MOVE


def test_attention_bias_without_log2e_moves_the_reference():
    qkv, kb = _attn_case(2.0)
    ref = _attn_ref(qkv, kb, bf16_q=True)
    # scores in log2 units s log2(e) + b instead of (s + b) log2(e): in natural units the bias is b / log2(e)
    move = rel(_attn_ref(qkv, kb / math.log2(math.e), bf16_q=True).numpy(), ref.numpy())
    print(f"L = 65: a key bias N(0, 2^2) without log2(e) moves the attention reference by {move:.3f}")
    assert move >= ATTN_MIN_MOVE


def test_tanh_gelu_deviation_from_erf_is_4_73e_4():
    """common.h documents gelu_tanh_fast's distance from the erf GELU; in float64 on 2.4 M points of [-12, 12]."""
    x = torch.linspace(-12.0, 12.0, 2_400_001, dtype=torch.float64)
    erf = 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))
    d = (mk.gelu_tanh(x) - erf).abs()
    i = int(d.argmax())
    print(f"tanh-form GELU vs erf: max {float(d[i]):.4e} at x = {float(x[i]):.3f}")
    assert abs(float(d[i]) - 4.73e-4) <= 0.01 * 4.73e-4
    assert abs(abs(float(x[i])) - 2.70) < 0.02
    # the slope bound the GELU epilogue's test uses
    xs = torch.linspace(-12.0, 12.0, 240_001, dtype=torch.float64)
    slope = (mk.gelu_tanh(xs)[1:] - mk.gelu_tanh(xs)[:-1]) / (xs[1:] - xs[:-1])
    assert float(slope.abs().max()) <= mk.GELU_DMAX
