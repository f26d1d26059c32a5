"""Operands, float64 references and bounds of the layer's tail, attention output -> state,

    X <- LN(X' + MLP(X')),   X' = LN(X + O Wout^T),   MLP(x) = GELU(x W1^T) W2^T,

shared by tests/test_layer_tail_gpu.py (which holds ``mmpfn_outproj_mlp_ln`` and ``mmpfn_mlp_ln`` to them) and
tests/test_layer_tail_sensitivity.py (which shows on the CPU what they catch).  No GPU here.

The restatement (``prologue``, ``mlp_half``, ``tail``) is float64 arithmetic that rounds only where the mode rounds:

  modes 0, 2 (fp32)   nothing; erf GELU.
  mode 1 (bf16)       O, Wout, W1, W2 to bf16; X' to bf16 as the up-projection's operand, unrounded as the residual (the
                      kernel keeps it in fp32 registers); the tanh-form GELU to bf16.
  mode 5 (fp16)       the same in fp16, and the state X and the result in fp16.

``exact=True`` keeps the rounded inputs and weights and drops every later rounding.  tests/test_layer_tail_sensitivity.py
ties ``mlp_half`` to ``oracle.forward.mlp_sublayer`` and ``prologue`` to the out-projection + LayerNorm lines of
``oracle.forward.item_sublayer``; ``wout_matrix`` is the oracle's einsum "thsd,hde->ste" written as a matrix,
Wout[e][32 h + d] = _w_out[h][d][e].

Bounds.  None comes from a run of a kernel.  u = 2^-24, E = 192.

``ln_bound(y)`` -- a LayerNorm evaluated in fp32 on exact fp32 inputs y, sums in any order:
  mean      s = fl(sum y): |ds| <= (E - 1) u sum|y|; times fl(1 / E): two more roundings.  |dmean| <= (E + 1) u mean|y| =: dm
  d_i       fl(y_i - mean): |dd_i| <= dm + u |d_i|
  variance  v = fl(sum d_i^2) / E + eps: the squares carry 2 |d_i| dd_i + u d_i^2, the sum (E - 1) u, the scaling and the
            eps two more.  rel(v) <= 2 mean(|d| dd) / v + (E + 3) u =: rv
  inv       1 / sqrt(v): half of rv, and 4 u for the square root and the division (correctly rounded each: 2 u; doubled)
  out_i     fl(d_i inv): |dout_i| <= dd_i / sigma + |out_i| (rv / 2 + 5 u)
``ln_prop(y, dy)`` -- what an input error dy moves a LayerNorm's output by, to first order (the second order is below
  1e-8 for the dy used here): out = d / sigma gives dout_e = (dy_e - mean dy) / sigma - out_e mean(out (dy - mean dy)) / sigma,
  so |dout_e| <= (|dy_e| + m + |out_e| mean(|out| (|dy| + m))) / sigma with m = mean|dy|.

Integer cases (``prologue_case``, ``mlp_case``): everything before the last LayerNorm is exact, or nearly --
  prologue   X, O, Wout integers in [-3, 3], W2 = 0: z = X + O Wout^T is an exact integer (|z| <= 192 * 9 + 3) in every
             mode and order, the MLP adds g * 0 = 0, so the result is LN(LN(z)): ``ln_bound`` of the last LayerNorm,
             doubled for the one before it.
  MLP        O = 0, X rows of 96 x +a and 96 x -a: mean 0 and variance a^2 exactly, X' = +-(1 - 5e-6 / a^2) up to 5 u
             (the fp32 LayerNorm of exact inputs: the variance's scaling, the eps, sqrt, division, product), +-1 as a
             16-bit operand.  W1 rows hold three +-8, so h = 8 (+-1 +-1 +-1) X' is +-8 or +-24 (times 1 - 5e-6 / a^2 in
             the fp32 modes); there every GELU form of common.h returns h for h > 0 and 0 (to 1e-20) for h < 0: erf_fast
             is +-1 exactly beyond |x| = 5.7 (its exponential is below 2^-46), 2^u under- or overflows to 0 / inf in
             the tanh forms.  1e-6 per hidden unit is allowed for it all the same.  W2 integers in [-3, 3]: the sum over
             the hidden units is an integer below 768 * 24 * 3 < 2^24, but the residual X' is not an integer, so the
             accumulation onto it rounds: any order, Fh + 1 terms, 2 (Fh + 1) u sum|terms| (doubled: the MFMA's internal
             adder is not documented to round to nearest), plus 5 u sum|terms| for X' itself.  That dy goes through
             ``ln_prop``, the last LayerNorm adds ``ln_bound``.  With the residual +-1 given directly (``mmpfn_mlp_ln``)
             the pre-LN value is an exact integer and only the GELU allowance remains in dy.
  fp16       the store adds 2^-11 |ref|, half an ulp: the kernel's result is compared with the restatement in front of
             its store (``pre``).  Against the stored restatement a result a hair away can be a whole ulp off.

Normal-data cases (``normal_case``), 16-bit modes: kernel and restatement round at the same points, so they differ by
fp32 summation order and by rounding decisions that fall on different sides.  The kernel is held to q, the distance
between ``tail`` and ``tail(exact=True)`` -- how far the mode's own rounding moves the result -- in max norm and in RMS
(``normal_bounds``, ``normal_ratios``).  Mode 5 evaluates the GELU in packed fp16 arithmetic; its restatement
(``gelu_tanh_f16``) follows common.h's formula step by step, rounding where each fp16 instruction rounds, so q holds
those roundings and no separate term is added for them.  Mode 5's fp16 store is kept out of q and allowed explicitly,
as in the integer cases: two values a hair apart can be stored a whole ulp apart, which a q that itself contains half
an ulp would mistake for a fault.  The kernel's result is compared with the restatement in front of its store, and
2^-11 |result| -- the half ulp its own store may add -- is allowed on top of q: the value the kernel rounds is held to
q.  Modes 0 and 2: the taps' own tolerance (tests/test_taps_gpu.py ``TOL``) against ``tail``, once per sublayer
crossed: 2 TOL max(1, max|ref|).
"""

from __future__ import annotations

import math

import torch

E, H, HD = 192, 6, 32
EPS = 1e-5
U = 2.0 ** -24
MODES = (0, 1, 2, 5)
OP = {0: None, 2: None, 1: torch.bfloat16, 5: torch.float16}
ROWS = (1, 15, 16, 17, 31, 32, 33, 127, 128, 129, 257)  # mlp_rows_kernel's 16-row tile, 32-row wave, 128-row block
NHID_FACTORS = (1, 2, 3, 4, 5)
GELU_C = 2.0 * math.sqrt(2.0 / math.pi)
GELU_DMAX = 1.13  # max |GELU'|
LAYER0 = "transformer_encoder.layers.0."


# ---------------------------------------------------------------------------------------------- the restatement
def _r(t: torch.Tensor, op) -> torch.Tensor:
    """float64 of t rounded to the operand type (None: as it is)."""
    return t.double() if op is None else t.float().to(op).double()


def ln(x: torch.Tensor, eps: float = EPS) -> torch.Tensor:
    d = x - x.mean(-1, keepdim=True)
    return d / torch.sqrt((d * d).mean(-1, keepdim=True) + eps)


def gelu_tanh(x: torch.Tensor) -> torch.Tensor:
    """x * sigmoid(2 sqrt(2/pi) (x + 0.044715 x^3)): the form common.h specifies for the 16-bit modes."""
    return x * torch.sigmoid(GELU_C * (x + 0.044715 * x ** 3))


def gelu_erf(x: torch.Tensor) -> torch.Tensor:
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def _h(t: torch.Tensor) -> torch.Tensor:
    return t.float().half().double()


def gelu_tanh_f16(h: torch.Tensor) -> torch.Tensor:
    """The tanh form as mode 5 evaluates it (common.h ``gelu_tanh_h2x2_f32``): every step of
    x * rcp(1 + exp2(x * fma(kc, x * x, kk))) in fp16, each rounded to nearest -- the conversion of h, the square, the
    fma (one rounding), the product, v_exp_f16, the sum, v_rcp_f16, the last product.  2^u overflowing fp16 gives
    rcp(inf) = 0.  (The two transcendentals are taken as correctly rounded; where the hardware's differ by an ulp the
    kernel differs from this as it does for a rounding that falls on the other side.)"""
    k = torch.tensor(-2.0, dtype=torch.float32) * torch.tensor(0.7978845608028654, dtype=torch.float32) \
        * torch.tensor(1.4426950408889634, dtype=torch.float32)
    kk, kc = _h(k), _h(k * torch.tensor(0.044715, dtype=torch.float32))
    x = _h(h)
    u = _h(x * _h(kc * _h(x * x) + kk))
    return _h(x * _h(1.0 / _h(_h(torch.exp2(u)) + 1.0)))


def wout_matrix(w_out: torch.Tensor) -> torch.Tensor:
    """``_w_out`` [H][d][E] -> Wout [E][H d] with O[row][32 h + d]: the oracle's einsum "thsd,hde->ste"."""
    return w_out.reshape(H * HD, E).T.contiguous()


def w_out_param(Wout: torch.Tensor) -> torch.Tensor:
    return Wout.T.reshape(H, HD, E).contiguous()


def state_in(mode: int, X: torch.Tensor) -> torch.Tensor:
    """The state as the kernels read it: fp32, or fp16 in mode 5."""
    return X.float().half().double() if mode == 5 else X.float().double()


def prologue(mode: int, X, O, Wout, eps: float = EPS) -> dict:
    """X' = LN(X + O Wout^T); z is the pre-LN value."""
    op = OP[mode]
    z = state_in(mode, X) + _r(O, op) @ _r(Wout, op).T
    return dict(z=z, xp=ln(z, eps))


def mlp_half(mode: int, xp, W1, W2, eps: float = EPS, exact: bool = False, gelu=None, operand=None, residual=None) -> dict:
    """LN(X' + GELU(X' W1^T) W2^T) on an unrounded X'.  ``gelu``, ``operand``, ``residual`` replace the GELU form, the
    up-projection's operand and the residual (tests/test_layer_tail_sensitivity.py's faults)."""
    op = OP[mode]
    ri = (lambda t: t) if exact or op is None else (lambda t: _r(t, op))
    if gelu is None:
        gelu = gelu_erf if op is None else gelu_tanh_f16 if mode == 5 and not exact else gelu_tanh
    h = ri(xp if operand is None else operand) @ _r(W1, op).T
    g = ri(gelu(h))
    y = (xp if residual is None else residual) + g @ _r(W2, op).T
    pre = ln(y, eps)
    out = pre.float().half().double() if mode == 5 and not exact else pre
    return dict(h=h, g=g, y=y, pre=pre, out=out)  # pre: the result in front of mode 5's fp16 store


def tail(mode: int, X, O, Wout, W1, W2, eps: float = EPS, exact: bool = False, fault: str | None = None, gelu=None) -> dict:
    """The whole step.  fault "residual_x": the MLP's residual taken from X; "operand_raw": its up-projection fed
    X + O Wout^T unnormalised."""
    p = prologue(mode, X, O, Wout, eps)
    m = mlp_half(mode, p["xp"], W1, W2, eps, exact, gelu,
                 operand=p["z"] if fault == "operand_raw" else None,
                 residual=state_in(mode, X) if fault == "residual_x" else None)
    return {**p, **m}


def mlp_only(mode: int, X, W1, W2, eps: float = EPS) -> dict:
    """``mmpfn_mlp_ln``: the MLP half on the state itself."""
    return mlp_half(mode, state_in(mode, X), W1, W2, eps)


# ---------------------------------------------------------------------------------------------- bounds
def _stats(y: torch.Tensor, eps: float):
    d = y - y.mean(-1, keepdim=True)
    v = (d * d).mean(-1, keepdim=True) + eps
    sigma = torch.sqrt(v)
    return d, v, sigma, d / sigma


def ln_bound(y: torch.Tensor, eps: float = EPS) -> torch.Tensor:
    """Per-element bound of an fp32 LayerNorm of exact inputs, any summation order (module docstring)."""
    d, v, sigma, out = _stats(y, eps)
    dm = (E + 1) * U * y.abs().mean(-1, keepdim=True)
    dd = dm + U * d.abs()
    rv = 2.0 * (d.abs() * dd).mean(-1, keepdim=True) / v + (E + 3) * U
    return dd / sigma + out.abs() * (rv / 2.0 + 5.0 * U)


def ln_prop(y: torch.Tensor, dy: torch.Tensor, eps: float = EPS) -> torch.Tensor:
    """First-order bound of what the input error dy moves LN(y) by (module docstring)."""
    _, _, sigma, out = _stats(y, eps)
    dc = dy.abs() + dy.abs().mean(-1, keepdim=True)
    return (dc + out.abs() * (out.abs() * dc).mean(-1, keepdim=True)) / sigma


def store_bound(mode: int, ref: torch.Tensor) -> torch.Tensor:
    return 2.0 ** -11 * ref.abs() if mode == 5 else torch.zeros_like(ref)


def prologue_bound(mode: int, r: dict) -> torch.Tensor:
    """Integer prologue case, against r["pre"]: two LayerNorms (the last one's bound, doubled) and the fp16 store."""
    return 2.0 * ln_bound(r["y"]) + store_bound(mode, r["pre"])


def mlp_bound(mode: int, r: dict, W2: torch.Tensor, exact_residual: bool = False) -> torch.Tensor:
    """Integer MLP case, against r["pre"]: the accumulation onto the non-integer residual, the GELU allowance, the
    last LayerNorm, the fp16 store."""
    w2a = W2.double().abs()
    dy = 1e-6 * w2a.sum(-1).expand_as(r["y"])
    if not exact_residual:
        terms = (r["y"] - r["g"] @ W2.double().T).abs() + r["g"].abs() @ w2a.T
        dy = dy + (2.0 * (W2.shape[1] + 1) + 5.0) * U * terms
    return ln_prop(r["y"], dy) + ln_bound(r["y"]) + store_bound(mode, r["pre"])


def normal_bounds(mode: int, r: dict, x: dict, tol: dict) -> dict:
    """Bounds of a normal-data case: r = ``tail``, x = ``tail(exact=True)``.  16-bit: max norm and RMS of the
    rounding's own effect q, in front of mode 5's store; fp32: 2 tol max(1, max|ref|) in max norm (``rms``: None)."""
    if OP[mode] is None:
        return dict(max=2.0 * tol[mode] * max(1.0, float(r["out"].abs().max())), rms=None)
    q = r["pre"] - x["out"]
    return dict(max=float(q.abs().max()), rms=float(q.pow(2).mean().sqrt()))


def normal_elem_bound(mode: int, r: dict, b: dict) -> torch.Tensor:
    """The max-norm bound per element: q, and mode 5's store."""
    return b["max"] + store_bound(mode, r["pre"])


def normal_ratios(mode: int, got: torch.Tensor, r: dict, b: dict) -> tuple[float, float | None]:
    """(max-norm, RMS) distance of a kernel's result from the restatement over its bound.  Mode 5: from the
    restatement in front of its store, less the kernel's own store rounding of at most half an ulp, 2^-11 |got| --
    in RMS by the triangle inequality, rms(got - pre) <= q_rms + rms(2^-11 |got|)."""
    d = (got - r["pre"]).abs()
    half = store_bound(mode, got)
    mx = float((d - half).clamp(min=0).max()) / b["max"]
    if b["rms"] is None:
        return mx, None
    return mx, float(d.pow(2).mean().sqrt()) / (b["rms"] + float(half.pow(2).mean().sqrt()))


# ---------------------------------------------------------------------------------------------- operands
def _gen(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(seed)


def _randint(g, shape) -> torch.Tensor:
    return torch.randint(-3, 4, shape, generator=g).double()


def prologue_case(rows: int, nhid: int, seed: int = 0) -> dict:
    """Integer X, O, Wout in [-3, 3], W2 = 0 (W1: N(0, 1/E), of no consequence)."""
    g = _gen(9100 + seed)
    Wout, W1 = _randint(g, (E, E)), torch.randn(nhid, E, generator=g).double() / math.sqrt(E)
    gx = _gen(9200 + 7 * rows + seed)
    c = dict(kind="prologue", X=_randint(gx, (rows, E)), O=_randint(gx, (rows, E)), Wout=Wout, W1=W1,
             W2=torch.zeros(E, nhid, dtype=torch.float64))
    assert float((c["X"].abs() + c["O"].abs() @ Wout.abs().T).max()) <= 192 * 9 + 3
    return c


def balanced_rows(rows: int, seed: int, unit: bool = False) -> torch.Tensor:
    """Rows of 96 x +a and 96 x -a in a seeded order, a in {1, 2, 3} per row (``unit``: a = 1)."""
    g = _gen(9300 + 7 * rows + seed)
    sign = torch.ones(rows, E, dtype=torch.float64)
    for r in range(rows):
        sign[r, torch.randperm(E, generator=g)[: E // 2]] = -1.0
    a = torch.ones(rows, 1, dtype=torch.float64) if unit else torch.randint(1, 4, (rows, 1), generator=g).double()
    return sign * a


def mlp_case(rows: int, nhid: int, seed: int = 0, unit: bool = False, light: bool = False) -> dict:
    """O = 0 (Wout integers all the same), balanced X, W1 rows of three +-8, W2 integers differing in every column.
    ``light``: W2 keeps one entry in 256, so that the MLP term (about 30) does not swamp the residual (1) in front of
    the scale-free LayerNorm -- the case for a fault that scales a whole row's MLP term (an unnormalised operand)."""
    g = _gen(9400 + nhid + seed)
    W1 = torch.zeros(nhid, E, dtype=torch.float64)
    for j in range(nhid):
        W1[j, torch.randperm(E, generator=g)[:3]] = 8.0 * (2.0 * torch.randint(0, 2, (3,), generator=g).double() - 1.0)
    W2 = _randint(g, (E, nhid))
    assert len({tuple(col) for col in W2.T.tolist()}) == nhid, "W2 columns must differ"
    assert ((W1 != 0).sum(-1) == 3).all()
    if light:
        W2 = W2 * (torch.randint(0, 256, W2.shape, generator=g) == 0)
    return dict(kind="mlp", X=balanced_rows(rows, seed, unit), O=torch.zeros(rows, E, dtype=torch.float64),
                Wout=_randint(g, (E, E)), W1=W1, W2=W2)


def check_mlp_case(mode: int, c: dict, r: dict) -> None:
    """The properties the MLP case's bound rests on; a generator that breaks one fails here, on the CPU."""
    X = c["X"]
    assert (X.sum(-1) == 0).all() and ((X * X).mean(-1) == X[:, 0] ** 2).all()  # mean 0, variance a^2
    a2 = X[:, :1] ** 2
    assert torch.allclose(r["xp"], X / X.abs() * (1.0 - 5e-6 / a2), rtol=0, atol=1e-9)
    if OP[mode] is not None:
        assert (_r(r["xp"], OP[mode]) == X.sign()).all()  # +-1 exactly as a 16-bit operand
        assert ((r["h"].abs() == 8) | (r["h"].abs() == 24)).all()
        assert ((r["g"] - torch.where(r["h"] > 0, r["h"], torch.zeros_like(r["h"]))).abs() < 1e-18).all()
        pre = r["g"] @ c["W2"].T
        assert ((pre - pre.round()).abs() < 1e-15).all() and float(pre.abs().max()) < 2 ** 24
    else:
        k = r["h"] / (8.0 * (1.0 - 5e-6 / a2))
        assert ((k - k.round()).abs() < 1e-9).all() and (k.round().abs() >= 1).all() and (k.round().abs() <= 3).all()
        assert ((r["g"] - torch.where(r["h"] > 0, r["h"], torch.zeros_like(r["h"]))).abs() < 1e-6).all()


def check_prologue_case(c: dict, r: dict) -> None:
    assert (r["z"] == r["z"].round()).all() and float(r["z"].abs().max()) <= 192 * 9 + 3
    assert (r["y"] == r["xp"]).all()  # W2 = 0: the MLP adds nothing


def normal_case(rows: int, nhid: int, seed: int = 0) -> dict:
    """X, O ~ N(0, 1), Wout ~ N(0, 1/E), W1 ~ N(0, 1/E), W2 ~ N(0, s^2 / nhid) with s chosen so that the MLP term
    carries half the variance of X' -- X, O Wout^T and the MLP term then each hold about a third of the variance in
    front of the last LayerNorm (``variance_shares``)."""
    g = _gen(9500 + nhid + seed)
    Wout = torch.randn(E, E, generator=g).double() / math.sqrt(E)
    W1 = torch.randn(nhid, E, generator=g).double() / math.sqrt(E)
    W2 = torch.randn(E, nhid, generator=g).double() / math.sqrt(nhid)
    gx = _gen(9600 + 7 * rows + seed)
    X, O = torch.randn(rows, E, generator=gx).double(), torch.randn(rows, E, generator=gx).double()
    probe = gelu_erf(ln(torch.randn(512, E, generator=_gen(9700)).double()) @ W1.T) @ W2.T
    W2 = W2 * math.sqrt(0.5 / float(probe.var()))
    f32 = lambda t: t.float().double()  # what the engine is given: fp32 values
    return dict(kind="normal", X=f32(X), O=f32(O), Wout=f32(Wout), W1=f32(W1), W2=f32(W2))


def variance_shares(c: dict) -> tuple[float, float, float]:
    """Shares of X, O Wout^T and the MLP term in the variance in front of the last LayerNorm (float64, unrounded;
    X' splits its unit variance between X and O Wout^T in proportion to theirs)."""
    ow = c["O"] @ c["Wout"].T
    xp = ln(c["X"] + ow)
    m = gelu_erf(xp @ c["W1"].T) @ c["W2"].T
    vx, vo, vm = float(c["X"].var()), float(ow.var()), float(m.var())
    tot = 1.0 + vm
    return vx / (vx + vo) / tot, vo / (vx + vo) / tot, vm / tot


def state_dict_with(sd: dict, c: dict) -> dict:
    """sd with the case's weights written into layer 0 (numpy float32, as the checkpoint ABI takes them)."""
    sd = dict(sd)
    sd[LAYER0 + "self_attn_between_items._w_out"] = w_out_param(c["Wout"]).float().numpy()
    sd[LAYER0 + "mlp.linear1.weight"] = c["W1"].float().numpy()
    sd[LAYER0 + "mlp.linear2.weight"] = c["W2"].float().numpy()
    return sd
