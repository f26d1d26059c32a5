"""Operands, float64 restatement and bounds of the attention-between-features sublayer,

    X <- LN(X + concat_h(softmax(Q_h K_h^T / sqrt(32)) V_h) Wout^T),   Q_h, K_h, V_h = X Wq_h^T, X Wk_h^T, X Wv_h^T

over the T tokens of one table row, shared by tests/test_feat_block_gpu.py (which holds ``mmpfn_feature_attention_ex`` to
them) and tests/test_feat_block_sensitivity.py (which shows on the CPU what they catch).  No GPU here.  States are in
the engine's order, X [M][T][S][E]; weights Wq, Wk, Wv [H][32][E] and Wout [E][32 h + d] (``layer_tail_cases.wout_matrix``).

The restatement (``feat_block``) is float64 arithmetic that rounds only where the mode rounds.  The 16-bit modes at
T <= 64 run ``feat_rows_kernel`` (featrow.hip; weights packed by weight_pack.h ``pack_feat_rows``):
  X, Wk, Wv, Wout    to the operand type (bf16 in mode 1, fp16 in mode 5; mode 5's state is fp16 already)
  Wq                 times fl32(log2(e) / sqrt(32)) in fp32, then to the operand type (the scores are in log2 units)
  Q, K, V            to the operand type (``cat8`` of the fp32 accumulators)
  P = exp2(s - max)  to the operand type, unnormalised; the row sum is taken over the unrounded exponentials in fp32
  O = (P V) / sum    to the operand type
  z = X + O Wout^T   on the fp32 state (mode 1) or the fp16 state (mode 5), fp32 LayerNorm, fp16 store in mode 5
Mode 5 at T > 64 is mode 1 (capi.cpp ``decode_prec``).  Modes 0 and 2 round nothing.  Mode 1 at T > 64 takes the general
path, whose rounding points differ (gemm.hip's projection, attention.hip ``attn_item_kernel<1>``), restated where
``is_general``: Q is rounded, multiplied by the fp32 scale and rounded again; the softmax's reference is the first 64-key
tile's maximum (the later tiles' maxima must stay within the kernel's rescale threshold of it, asserted); the row sum is
taken over the rounded P (an MFMA against ones).  ``exact=True`` keeps the rounded inputs and weights and drops every
later rounding.  tests/test_feat_block_sensitivity.py ties modes 0 and 2 to ``oracle.forward.feat_sublayer``.

``fault`` injects one of ``FAULTS`` into the restatement, each what a kernel bug of that name would compute:
  pad_joins      one zero padding token (K = V = 0, score 0) joins the softmax as a key
  mask_last      the last valid key is masked
  pad_v          the padding key that joins carries token 0's V (what a padding lane loads: its address is clamped to
                 token 0) instead of zero.  Behind a right mask a padding V meets P = 0 and is no fault; it is one with
                 the weight a padding key gets, so the two are injected together
  qk_perm        Wk's rows carry pack_feat_rows' permutation and Wq's do not (omitted on both the dot product is
                 unchanged: it would be no fault)
  swap_pair_v    keys 1 and 17 (one of each tile of a pair; keys 0 and 1 where T < 18) swapped in V only
  heads_swapped  heads 0 and 1 swapped at the out-projection
  no_res_perm    mode 5: Wout's rows not in ``f16_row_perm`` order while the residual and the store are
  park_head      32 < T <= 48, full form: head 1's tile-2 fragment replaced by head 0's
  member_row     member m > 0 reads member m - 1's row
  no_scale       the softmax scale log2(e) / sqrt(32) is missing

Bounds.  None comes from a run of a kernel.  ``ln_bound`` and ``ln_prop`` are layer_tail_cases' (its docstring derives
them); u = 2^-24.

Selection case (T <= 64).  All 192 features are three one-hot blocks of 64: block 0 the token's own id t, blocks 1 and
2 target ids pi_A(t), pi_B(t), permutations of [0, T) drawn per (member, row).  Per head h: Wk_h[d][j] = c_h(j)[d] on
block 0 with a +-1 code book c_h of 64 codes of 32 dimensions; Wq_h[d][64 b + j] = 16 c_h(j)[d] on block b = 1 (even
heads) or 2 (odd heads); Wv_h[d][j] = v_h(j)[d] on block 0, integers in [-3, 3]; Wout integers in [-3, 3].  So
Q = 16 fl(scale) c_h(target), K = c_h(t), the score of key j is 16 scale c_h(target) . c_h(j): 32 for the target, less
for every other key.  ``check_selection`` asserts that the target leads every other key by >= 40 log2 units in the mode's
own scores (the seed of the code books is chosen so that it holds: about 49 in every mode) and that the unrounded O
is within 64 * 3 * 2^-40 of v_h(target), rounded or not.  Then P is 1 for the target and <= 2^-40 for the rest, O rounds
to the integer v_h(target) in the 16-bit modes (beside v = 0, bf16 keeps the losers' 2^-40), and z = X + O Wout^T is an
integer (|z| <= 1 + 192 * 9) in every mode and order, but for the losers' weight.
The losers' weight is allowed explicitly: dO = 64 * 3 * 2^-40 per element, dz = dO sum_k |Wout[e][k]|, through
``ln_prop``; the LayerNorm adds ``ln_bound``, mode 5's store half an ulp of the result.

Uniform case (T <= 255).  Wq = 0; Wk integers in [-3, 3]; Wv_h[d] a single +-1 at feature f(h, d), f a permutation of
the 192 features; Wout integers in [-3, 3]; X = T * {-1, 0, 1}, exact in bf16 and fp16.  The scores are exactly 0, every
exponential exactly 1, the row sum exactly T, P V = T n with n = sum_t {-1, 0, 1} an integer, |n| <= T.  The 16-bit
kernels compute fl32(T n * rcp(T)) = n (1 + 2 u) and round it to the operand type: n.  z is an exact integer
(|z| <= T + 192 * 3 * T < 2^24).  The fp32 modes keep O = n (1 + d), |d| <= 4 u (the division 1 / T or its reciprocal, 2.5
ulp at most, and the product), and accumulate it onto X in fp32 in any order: dz = (4 + 2 (E + 1)) u (|X| + |O| |Wout|^T),
the accumulation's factor doubled as in layer_tail_cases' MLP case.  A padding key that joins, or a valid key that is
masked, turns n into n T / (T +- 1).  Read from the sources: the general path keeps the case exact too -- gemm.hip /
rowgemm3.hip project integer operands exactly (fp32 accumulation below 2^24; the split-bf16 low planes are zero),
attn_item_kernel's first-tile reference is max 0 = 0 and never rescaled, its P = exp2(0) = 1, its row sum T (VALU adds,
or the ones-MFMA in bf16), O = fl(T n * fl(1 / T)), in bf16 rounded to n.

Normal case.  randn X and N(0, 1 / 192) weights (synth's scale), Wout scaled so that O Wout^T carries the residual's
variance (``variance_shares``).  16-bit modes: kernel and restatement round at the same points, so the kernel is held
to q = |restatement - restatement(exact)| in max norm and RMS, in front of mode 5's store, whose half ulp is allowed on
top -- ``layer_tail_cases.normal_ratios``, see that module's docstring.  Modes 0 and 2: the taps' own tolerance
(tests/test_taps_gpu.py ``TOL``) times max(1, max|ref|), once: one sublayer.
"""

from __future__ import annotations

import math

import torch

from layer_tail_cases import E, EPS, H, HD, MODES, OP, U, _r, ln, ln_bound, ln_prop, state_in, store_bound, w_out_param

T_EDGES = (1, 2, 15, 16, 17, 31, 32, 33, 36, 47, 48, 49, 63, 64)  # featrow's 16-token tiles, NT = 1 .. 4
S_EDGES = (1, 4, 5)  # less than a 4-row block, one, one and a row
MS = ((2, 3), (3, 3), (2, 4))  # (M, S): a member boundary inside a block (twice), and on a block's edge
T_GENERAL = (65, 127, 128, 129)  # the general path: its 64-key tiles
LAYER0 = "transformer_encoder.layers.0.self_attn_between_features."
FAULTS = ("pad_joins", "mask_last", "pad_v", "qk_perm", "swap_pair_v", "heads_swapped", "no_res_perm", "park_head",
          "member_row", "no_scale")
A_SEL = 16.0
MARGIN = 40.0
D_LOSERS = 64 * 3 * 2.0 ** -40
IA_TAU = 8.0  # attention.hip: the general path's lazy-rescale threshold
C32 = torch.tensor(1.4426950408889634, dtype=torch.float32) / torch.sqrt(torch.tensor(32.0, dtype=torch.float32))
C64 = math.log2(math.e) / math.sqrt(32.0)


def pack_row_perm() -> torch.Tensor:
    """pack_feat_rows: image row 16 f + rho of a head's Q or K holds head dim 8 (rho >> 2) + 4 f + (rho & 3)."""
    return torch.tensor([8 * ((r & 15) >> 2) + 4 * (r >> 4) + (r & 3) for r in range(HD)])


def f16_row_perm() -> torch.Tensor:
    """weight_pack.h ``f16_row_perm``: image row r of mode 5's out-projection holds Wout row perm(r)."""
    return torch.tensor([32 * ((r >> 4) >> 1) + 8 * ((r & 15) >> 2) + 4 * ((r >> 4) & 1) + (r & 3) for r in range(E)])


# ---------------------------------------------------------------------------------------------- the restatement
def is_general(mode: int, T: int) -> bool:
    return OP[mode] is None or T > 64


def feat_block(mode: int, X: torch.Tensor, W: dict, eps: float = EPS, exact: bool = False, fault: str | None = None,
               last: bool = False) -> dict:
    """The sublayer on X [M][T][S][E] (module docstring).  ``pre`` is the result in front of mode 5's store, ``out``
    behind it; ``last``: the pruned form, tokens other than T - 1 come back as the state holds them."""
    assert fault is None or fault in FAULTS
    M, T, S, _ = X.shape
    if mode == 5 and T > 64:
        mode = 1  # decode_prec
    op, general = OP[mode], is_general(mode, T)
    ri = (lambda t: t) if exact or op is None else (lambda t: _r(t, op))
    xs = state_in(mode, X)  # the state: the residual
    if fault == "member_row" and M > 1:
        xs = torch.cat([xs[:1], xs[:-1]])
    x = _r(xs, op).permute(0, 2, 1, 3)  # [M][S][T][E], as an operand
    scale = 1.0 if fault == "no_scale" else None
    Wq, Wk, Wv = W["Wq"].double(), W["Wk"].double(), W["Wv"].double()
    if fault == "qk_perm":
        Wk = Wk[:, pack_row_perm()]
    proj = lambda w: torch.einsum("mste,hde->mshtd", x, w)
    if op is None:
        Q = proj(Wq) * (C64 if scale is None else scale)
    elif general:
        c = float(C32) if scale is None else scale
        Q = ri((ri(proj(_r(Wq, op))).float() * c).double()) if not exact else proj(_r(Wq, op)) * c
    else:
        Q = ri(proj(_r((Wq.float() * (C32 if scale is None else scale)).float(), op)))
    K, V = ri(proj(_r(Wk, op))), ri(proj(_r(Wv, op)))
    if fault == "swap_pair_v" and T >= 2:
        a, b = (1, 17) if T >= 18 else (0, 1)
        idx = torch.arange(T)
        idx[a], idx[b] = b, a
        V = V[..., idx, :]
    s = Q @ K.transpose(-1, -2)  # [M][S][H][query][key], log2 units
    if fault == "mask_last" and T > 1:
        s = s.clone()
        s[..., T - 1] = -math.inf
    if fault in ("pad_joins", "pad_v"):
        s = torch.cat([s, torch.zeros_like(s[..., :1])], -1)
        V = torch.cat([V, V[..., :1, :] if fault == "pad_v" else torch.zeros_like(V[..., :1, :])], -2)
    if general and op is not None:
        m = s[..., :64].max(-1, keepdim=True).values
        assert float((s.max(-1, keepdim=True).values - m).max()) <= IA_TAU, "a later tile would rescale"
    else:
        m = s.max(-1, keepdim=True).values
    e = torch.exp2(s - m)
    P = ri(e)
    total = (P if general and op is not None else e).sum(-1, keepdim=True)
    O = ri((P @ V) / total)  # [M][S][H][T][d]
    if fault == "heads_swapped":
        O = O[:, :, [1, 0, 2, 3, 4, 5]]
    if fault == "park_head" and 32 < T <= 48 and not last:
        O = O.clone()
        O[:, :, 1, 32:] = O[:, :, 0, 32:]
    Oc = O.permute(0, 3, 1, 2, 4).reshape(M, T, S, H * HD)  # [M][T][S][32 h + d]
    attn = Oc @ _r(W["Wout"], op).T
    if fault == "no_res_perm" and mode == 5 and not general:
        moved = torch.empty_like(attn)
        moved[..., f16_row_perm()] = attn
        attn = moved
    z = xs + attn
    pre = ln(z, eps)
    out = pre.float().half().double() if mode == 5 and not exact else pre
    if last and not general:
        keep = torch.ones(T, dtype=torch.bool)
        keep[T - 1] = False
        pre, out = pre.clone(), out.clone()
        pre[:, keep], out[:, keep] = xs[:, keep], xs[:, keep]
    return dict(s=s, O=Oc, z=z, y=z, pre=pre, out=out, x=xs)


# ---------------------------------------------------------------------------------------------- operands
def _gen(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(seed)


def _randint(g, shape) -> torch.Tensor:
    return torch.randint(-3, 4, shape, generator=g).double()


SEL_SEED = 7700  # the code books' seed: chosen so that ``check_selection``'s margin holds (asserted there)


def selection_weights() -> dict:
    g = _gen(SEL_SEED)
    code = 2.0 * torch.randint(0, 2, (H, 64, HD), generator=g).double() - 1.0  # c_h(j)[d]
    val = _randint(g, (H, 64, HD))  # v_h(j)[d]
    Wq, Wk, Wv = (torch.zeros(H, HD, E, dtype=torch.float64) for _ in range(3))
    for h in range(H):
        b = 64 * (1 + h % 2)
        Wk[h, :, :64] = code[h].T
        Wq[h, :, b:b + 64] = A_SEL * code[h].T
        Wv[h, :, :64] = val[h].T
    return dict(kind="selection", Wq=Wq, Wk=Wk, Wv=Wv, Wout=_randint(g, (E, E)), val=val)


def uniform_weights() -> dict:
    g = _gen(7800)
    Wv = torch.zeros(H * HD, E, dtype=torch.float64)
    Wv[torch.arange(E), torch.randperm(E, generator=g)] = 2.0 * torch.randint(0, 2, (E,), generator=g).double() - 1.0
    return dict(kind="uniform", Wq=torch.zeros(H, HD, E, dtype=torch.float64), Wk=_randint(g, (H, HD, E)),
                Wv=Wv.reshape(H, HD, E), Wout=_randint(g, (E, E)))


def normal_weights() -> dict:
    """N(0, 1 / 192) weights; Wout scaled so that O Wout^T has the variance of a randn state at T = 36."""
    g = _gen(7900)
    f32 = lambda t: t.float().double()  # what the engine is given: fp32 values
    W = {k: f32(torch.randn(H, HD, E, generator=g).double() / math.sqrt(E)) for k in ("Wq", "Wk", "Wv")}
    W["Wout"] = torch.randn(E, E, generator=g).double() / math.sqrt(E)
    probe = torch.randn(1, 36, 8, E, generator=_gen(7901)).double()
    r = feat_block(0, probe, W)
    W["Wout"] = f32(W["Wout"] * math.sqrt(float(probe.var()) / float((r["z"] - probe).var())))
    W["kind"] = "normal"
    return W


WEIGHTS = dict(selection=selection_weights, uniform=uniform_weights, normal=normal_weights)


def selection_state(M: int, S: int, T: int, seed: int = 0) -> dict:
    assert 1 <= T <= 64
    g = _gen(8000 + 1009 * M + 101 * S + T + seed)
    X = torch.zeros(M, T, S, E, dtype=torch.float64)
    tgt = torch.empty(2, M, S, T, dtype=torch.long)
    t = torch.arange(T)
    for m in range(M):
        for s in range(S):
            X[m, t, s, t] = 1.0
            for b in range(2):
                tgt[b, m, s] = torch.randperm(T, generator=g)
                X[m, t, s, 64 * (b + 1) + tgt[b, m, s]] = 1.0
    return dict(kind="selection", X=X, tgt=tgt)


def uniform_state(M: int, S: int, T: int, seed: int = 0) -> dict:
    assert 1 <= T <= 255
    g = _gen(8100 + 1009 * M + 101 * S + T + seed)
    return dict(kind="uniform", X=float(T) * torch.randint(-1, 2, (M, T, S, E), generator=g).double())


def normal_state(M: int, S: int, T: int, seed: int = 0) -> dict:
    g = _gen(8200 + 1009 * M + 101 * S + T + seed)
    return dict(kind="normal", X=torch.randn(M, T, S, E, generator=g).float().double())


STATES = dict(selection=selection_state, uniform=uniform_state, normal=normal_state)


def variance_shares(W: dict, X: torch.Tensor) -> tuple[float, float]:
    """Shares of X and of the attention term O Wout^T in the variance in front of the LayerNorm (float64, unrounded)."""
    a = feat_block(0, X, W)["z"] - X
    vx, va = float(X.var()), float(a.var())
    return vx / (vx + va), va / (vx + va)


def state_dict_with(sd: dict, W: dict) -> dict:
    """sd with the weight set written into layer 0's feature attention (numpy float32, as the checkpoint ABI takes
    them: ``_w_qkv`` [3][H][32][E], ``_w_out`` [H][32][E])."""
    sd = dict(sd)
    sd[LAYER0 + "_w_qkv"] = torch.stack([W["Wq"], W["Wk"], W["Wv"]]).float().numpy()
    sd[LAYER0 + "_w_out"] = w_out_param(W["Wout"]).float().numpy()
    return sd


# ---------------------------------------------------------------------------------------------- checks and bounds
def selection_margin(r: dict, c: dict) -> float:
    """The least lead, in log2 units, of a query's target key over its other keys (inf at T = 1)."""
    s, tgt = r["s"], c["tgt"]  # s [M][S][H][q][k]
    lead = math.inf
    for h in range(H):
        sh = s[:, :, h]
        win = torch.gather(sh, -1, tgt[h % 2].unsqueeze(-1))
        rest = sh.scatter(-1, tgt[h % 2].unsqueeze(-1), -math.inf).max(-1, keepdim=True).values
        lead = min(lead, float((win - rest).min()))
    return lead


def check_selection(mode: int, W: dict, c: dict, r: dict) -> None:
    """What the selection case's bound rests on; a generator that breaks it fails here, on the CPU."""
    assert selection_margin(r, c) >= MARGIN, selection_margin(r, c)
    M, T, S, _ = c["X"].shape
    want = torch.empty(M, T, S, H, HD, dtype=torch.float64)
    for h in range(H):
        want[:, :, :, h] = W["val"][h][c["tgt"][h % 2]].permute(0, 2, 1, 3)  # [M][S][T][d] -> [M][T][S][d]
    want = want.reshape(M, T, S, H * HD)
    O = feat_block(mode, c["X"], W, exact=True)["O"]
    assert float((O - want).abs().max()) <= D_LOSERS
    assert float((r["O"] - want).abs().max()) <= D_LOSERS  # (bf16 keeps the losers' 2^-40 beside an integer 0)
    zi = c["X"] + want @ W["Wout"].T
    assert float((r["z"] - zi).abs().max()) <= D_LOSERS * 3 * E and float(zi.abs().max()) <= 1 + E * 9


def check_uniform(mode: int, W: dict, c: dict, r: dict) -> None:
    T = c["X"].shape[1]
    assert float(r["s"].abs().max()) == 0.0
    assert torch.equal(r["O"], r["O"].round()) and float(r["O"].abs().max()) <= T
    assert torch.equal(r["z"], r["z"].round()) and float(r["z"].abs().max()) < 2 ** 24
    if OP[mode] is not None:
        assert torch.equal(_r(c["X"], OP[mode]), c["X"])


def selection_bound(mode: int, W: dict, r: dict) -> torch.Tensor:
    """Against r["pre"]: the losers' weight through Wout and the LayerNorm, the LayerNorm itself, the fp16 store."""
    dz = (D_LOSERS * W["Wout"].abs().sum(-1)).expand_as(r["z"])
    return ln_prop(r["z"], dz) + ln_bound(r["z"]) + store_bound(mode, r["pre"])


def uniform_bound(mode: int, W: dict, r: dict) -> torch.Tensor:
    """Against r["pre"]: the fp32 modes' unrounded O = n (1 + 4 u) accumulated onto X in fp32 (the 16-bit modes: exact),
    the LayerNorm, the fp16 store."""
    b = ln_bound(r["z"]) + store_bound(mode, r["pre"])
    if OP[mode] is None:
        dz = (4.0 + 2.0 * (E + 1)) * U * (r["x"].abs() + r["O"].abs() @ W["Wout"].abs().T)
        b = b + ln_prop(r["z"], dz)
    return b


INT_BOUND = dict(selection=selection_bound, uniform=uniform_bound)
INT_CHECK = dict(selection=check_selection, uniform=check_uniform)


def normal_bounds(mode: int, r: dict, x: dict, tol: dict) -> dict:
    """r = ``feat_block``, x = ``feat_block(exact=True)``.  16-bit: max norm and RMS of the rounding's own effect q, in
    front of mode 5's store; fp32: tol max(1, max|ref|) in max norm (``rms``: None)."""
    if OP[mode] is None:
        return dict(max=tol[mode] * max(1.0, float(r["out"].abs().max())), rms=None)
    q = r["pre"] - x["out"]
    return dict(max=float(q.abs().max()), rms=float(q.pow(2).mean().sqrt()))


def int_ratio(got: torch.Tensor, r: dict, bound: torch.Tensor) -> float:
    return float(((got - r["pre"]).abs() / bound).max())
