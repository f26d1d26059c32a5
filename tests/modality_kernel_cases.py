"""Seeded operands, float64 references and per-element bounds of the modality towers' GEMM tap
(``mmpfn_enc_linear``), shared by tests/test_modality_kernels_gpu.py (which holds the kernel to them) and
tests/test_modality_kernels_sensitivity.py (which shows on the CPU what they catch).

The kernel multiplies bf16 operands and accumulates in fp32, so the reference is float64 arithmetic on the
same bf16 values.  bf16 x bf16 products are exact in fp32; what is left is the order and rounding of the sums:

  accb = 2 * K * 2^-24 * (sum_k |a_k| |w_k| + |bias|)

is the any-order fp32 summation bound, doubled because the MFMA's internal adder is not documented to round
each partial sum to nearest.  Per epilogue (``bound``):

  fp32 store                       accb
  residual C += gamma (acc + bias)  |gamma| accb + 2^-23 |result|
  bf16 store                       2^-8 |ref| + accb
  bf16 store of the GELU           2^-8 |ref| + 1.13 accb + the fp32 evaluation's allowance (``gelu_allowance``)

None of these comes from a run of the kernel.
"""

from __future__ import annotations

import math

import torch

EPI_BF16, EPI_RESID, EPI_F32 = 0, 1, 2  # MMPFN_ENC_EPI_* (include/mmpfn_modality.h)
GELU_DMAX = 1.13  # max |GELU'| (1.129 at x = 1.5 for the erf and the tanh form alike)
GELU_C = 2.0 * math.sqrt(2.0 / math.pi)

# the towers' own GEMM shapes at 1300 rows (6 M tiles): (name, M, N, K, epilogue, act, with gamma)
TOWER_SHAPES = [
    ("qkv_bf16", 1300, 2304, 768, EPI_BF16, 0, False),
    ("fc2_resid", 1300, 768, 3072, EPI_RESID, 0, False),
    ("fc2_resid_gamma", 1300, 768, 3072, EPI_RESID, 0, True),
    ("fc1_gelu", 1300, 3072, 768, EPI_BF16, 1, False),
    ("wide_f32", 1300, 1024, 4096, EPI_F32, 0, False),
]


def gelu_tanh(x: torch.Tensor) -> torch.Tensor:
    """The tanh-form GELU the bf16 epilogue is specified to compute, x * sigmoid(2 sqrt(2/pi) (x + 0.044715 x^3))."""
    return x / (1.0 + torch.exp(-GELU_C * (x + 0.044715 * x ** 3)))


def gelu_allowance(pre: torch.Tensor, ref: torch.Tensor) -> torch.Tensor:
    """What evaluating the tanh form in fp32 may add (common.h ``gelu_tanh_fast``): g = x / (1 + 2^u) with
    u = x * fma(k c, x^2, k), k = -2 sqrt(2/pi) log2(e).  u takes five roundings (the two constants, x^2, the fma,
    the product) of terms of one sign, so |du| <= 5 * 2^-24 |u| < 3 * |u| * 2^-23.  e = 2^u then carries the
    relative error ln(2) du plus the 1 ulp (2^-23) of v_exp_f32, which moves g by the factor e / (1 + e) < 1 of it;
    the sum 1 + e (2^-24), v_rcp_f32 (1 ulp, 2^-23) and the last product (2^-24) add 2^-22 of g.  Together
      |dg| <= |g| * 2^-23 * (3 ln(2) |u| + 3),
    relative to g itself, and for |x| < 8 (|u| < 72) below 2e-5 |g|: two hundred times less than the bf16 rounding
    term 2^-8 |g| it is added to."""
    u = GELU_C * math.log2(math.e) * (pre + 0.044715 * pre ** 3)
    return ref.abs() * 2.0 ** -23 * (3.0 * math.log(2.0) * u.abs() + 3.0)


def operands(M: int, N: int, K: int, kind: str, seed: int) -> dict:
    """A [M][K], W [N][K] bf16; bias, gamma [N] and the prior C [M][N] fp32.  kind "int": integers in [-3, 3]
    (bias [-4, 4], gamma [-2, 2], prior C [-3, 3]): every product and partial sum is an exact fp32 integer in any
    order for K <= 4096 (|sum| <= 36 864 < 2^24), and so is the residual (< 2 * 36 868 + 3).  kind "normal":
    A ~ N(0, 1), W ~ N(0, 1/K), bias ~ 0.5 N(0, 1), gamma ~ U(0.2, 1), prior C ~ N(0, 1)."""
    g = torch.Generator().manual_seed(seed)
    if kind == "int":
        assert K <= 4096
        A = torch.randint(-3, 4, (M, K), generator=g).bfloat16()
        W = torch.randint(-3, 4, (N, K), generator=g).bfloat16()
        bias = torch.randint(-4, 5, (N,), generator=g).float()
        gamma = torch.randint(-2, 3, (N,), generator=g).float()
        c0 = torch.randint(-3, 4, (M, N), generator=g).float()
    else:
        A = torch.randn(M, K, generator=g).bfloat16()
        W = (torch.randn(N, K, generator=g) / math.sqrt(K)).bfloat16()
        bias = 0.5 * torch.randn(N, generator=g)
        gamma = 0.2 + 0.8 * torch.rand(N, generator=g)
        c0 = torch.randn(M, N, generator=g)
    return dict(M=M, N=N, K=K, A=A, W=W, bias=bias, gamma=gamma, c0=c0)


def tower_operands(name: str) -> dict:
    """The normal-data operands of a ``TOWER_SHAPES`` entry (the two residual entries share theirs)."""
    i, (_, M, N, K, _, _, _) = next((i, s) for i, s in enumerate(TOWER_SHAPES) if s[0] == name.replace("_gamma", ""))
    return operands(M, N, K, "normal", seed=7000 + i)


def preactivation(A: torch.Tensor, W: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    """float64 A . W^T + bias of the operands as given."""
    return A.double() @ W.double().T + bias.double()


def accb(ops: dict) -> torch.Tensor:
    K = ops["K"]
    mag = ops["A"].double().abs() @ ops["W"].double().abs().T + ops["bias"].double().abs()
    return 2.0 * K * 2.0 ** -24 * mag


def expected(pre: torch.Tensor, epi: int, act: int, gamma, c0) -> torch.Tensor:
    """float64 result of an epilogue on the float64 pre-activation (gamma None: 1)."""
    if epi == EPI_BF16:
        return gelu_tanh(pre) if act else pre
    if epi == EPI_F32:
        return pre
    return c0.double() + (pre if gamma is None else gamma.double() * pre)


def bound(pre: torch.Tensor, ref: torch.Tensor, ab: torch.Tensor, epi: int, act: int, gamma) -> torch.Tensor:
    """Per-element bound of |kernel - ref| (module docstring); ab = accb(ops)."""
    if epi == EPI_F32:
        return ab
    if epi == EPI_RESID:
        return (ab if gamma is None else gamma.double().abs() * ab) + 2.0 ** -23 * ref.abs()
    if act:
        return 2.0 ** -8 * ref.abs() + GELU_DMAX * ab + gelu_allowance(pre, ref)
    return 2.0 ** -8 * ref.abs() + ab
