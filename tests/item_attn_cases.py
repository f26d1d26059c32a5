"""Operands, float64 restatement, bounds and faults of the item attention itself,

    O[b][s][h] = softmax(Q[b][h][s] K[b][g]^T / sqrt(32)) V[b][g]   over the N train rows (keys) of token column b,
                                                                      g = h for a train row, g = 0 for a test row,

shared by tests/test_item_attn_gpu.py (which holds ``mmpfn_item_attention_forward`` and the older attention taps to them)
and tests/test_item_attn_sensitivity.py (which shows on the CPU what they catch).  No GPU here.  Layouts are the
kernels': q [T][H][S][32], k [T][H][Npad][32], vt [T][H][32][Npad], out [T][S][H * 32]; Npad = N rounded up to 64, K
rows and V^T columns [N, Npad) NaN on input.  The kernels: attention_pipe.hip ``attn_pipe_kernel`` (16-bit),
attention.hip ``attn_item3_kernel`` (mode 0) and ``attn_item_kernel<0, 4>`` (mode 2).

A ``Way`` says how a launch takes its operands.  ``forward_way(precision)`` is the forwards' (capi.cpp
``item_attn_args``, through ``mmpfn_item_attention_forward``): the 16-bit codes read bf16 Q that already carries
fl32(log2(e) / sqrt(32)) (``feat_block_cases.C32``) and bf16 K, and store bf16 (codes 1, 3, 4) or fp16 (5, 6, 7); modes 0
and 2 read plain fp32 Q.  ``OLD_BF16`` / ``OLD_F16`` are the older taps' (``mmpfn_item_attention_layer``,
``mmpfn_item_attention_cached``; ``mmpfn_item_attention_layer_ex`` code 5): Q unprescaled, in bf16 / fp16.

Forms: 0 a full layer (rows [0, N) own heads, rows [N, S) head 0's K / V); 1 the pruned last layer (own-head rows
[a0, N) only, a0 = N - N % 256; rows [0, a0) of out are not written); 2 a cache predict (every row a test row, k / vt
hold one head: [T][1][Npad][32], [T][1][32][Npad]).

The restatement (``attend``) is float64 arithmetic on the operands as stored.  It rounds only where the source rounds:
  Q        unprescaled ways: (QT)((float)q * c) (attention_pipe.hip, the Q load); modes 0 and 2: fl32(q c), in mode 0 then
           split hi = bf16(x), lo = bf16(x - hi) (common.h ``split_bf16``); K and V^T of mode 0 split the same way, three
           products per contraction (lo x lo dropped)
  P        exp2(s) to bf16 in the 16-bit ways (``expc``); ``pre`` carries it, ``exact`` does not
  store    to the way's output type
``exact`` is the value with P unrounded; the spread case's bound is on |kernel - exact| and *contains* P's half ulp,
because the kernel's P is rounded from a score with its own accumulation error (and, on the re-run, relative to
another reference), so kernel and restatement need not round the same number.  For the same reason the fault
``p_not_rounded`` (which turns ``pre`` into ``exact``) is invisible to the bound: it is listed, and the sensitivity test
asserts that it is *not* seen.  ``bits`` gives what the caller's sentinel-filled out buffer holds afterwards.

Selection case (``selection_case``), bitwise.  nb = bit length of N - 1 code dimensions hold +-1 codes of a key's index
(XORed with a per-(column, kv head) mask, so every K sequence differs), nb further dimensions hold 1 in K and -A in Q
(the bias: spread over nb dimensions rather than one, so that in the unprescaled ways, where the kernel rounds q c, every
term has the same magnitude r = round(A c) and the chosen key's score is r (nb - nb) = 0 exactly), dimension 30 holds 1 in
K and a per-query shift in Q (``shifted``: +110 / -80 log2 units on some queries of every wave, which sends their waves
through the first-tile re-run and, where the chosen key is 128 units above the first tile's best, the exact backstop).
A = 32 prescaled, 128 unprescaled (r = 32.6): every other key scores <= -64 log2 units.  V^T holds +-(8 + m) / 8 2^e,
m in [0, 8), e in [-2, 2): 4 significant bits, exact in bf16, fp16 and e4m3.  Then P is 1 (or one rounded number p) for the
chosen key and <= 2^-64 p for the rest, the row sum is p, O = fl(p v) fl(1 / p) rounds to v in every 16-bit output type: the
comparison is on bits, in the fp8 kernels' kept pass (P' a power of two or one e4m3 number, V^T exact) as in their re-run.
Modes 0 and 2: |got - v| <= 4 u |v| (the product, the row sum, the correctly rounded division, the last product).
pi steps 65 keys (or the next number coprime to N) per query of a K sequence, in the order the kernels number its
queries: every key is chosen wherever a sequence has N queries, consecutive queries choose keys of different tiles.
``check_selection_operands`` asserts representability, distinct V vectors, the score gap and pi's coverage.

Spread case (``spread_case``), bounded per element.  K, V ~ N(0, 1), Q ~ N(0, g^2) with g such that a score's standard
deviation is 3 log2 units: a handful of comparable dominant keys per query, anywhere.  State 1 shifts every score of
some queries by +110 or -80 log2 units (dimension 30: the first-tile re-run) and of some by -12 (a row sum of about
2^-3, far below the padded tile's cancelled ones and still above the re-run's threshold), state 2 also the scores of
keys >= 64 of some queries by +120 (dimension 31: the re-run's reference, the first tile's max, is then 120 too low:
the backstop).  Per element, with
u = 2^-24, L = sum p, w = sum p |v| / L, dev = sum p |v - O| / L and, per query, mag = max_k sum |q k|, smax = max_k |s|:
  d     relative error of one p:  ln 2 * 2 (Ks + 1) u (mag + smax)   fp32 accumulation of s over Ks products (32; mode 0:
                                    96; mode 2: 64, its products are rounded too), doubled as the other suites double
                                    MFMA accumulation; + smax: the re-run's s - mref, mode 2's accumulator start -mref
                                  + 4 u                                v_exp_f32 (1 ulp) and exp2f's range scaling
                                  + eP                                 P's half ulp: 2^-8 of it (bf16: 8 significant
                                                                       bits); mode 0: 2^-16, what P's hi + lo leaves,
                                                                       in P.V and in the row sum alike; mode 2: 0
        the same d sits in numerator and denominator: it moves O by d * dev
  ao    P.V accumulation: 2 (Ko + 1) u w, Ko = N (mode 0: 3 N; mode 2: 2 N), plus, mode 2, 4 u per lazy rescale (<= tiles),
        plus, mode 0, 2^-16 w: the V lo x P lo product that attention.hip's three P.V MFMAs (vl ph, vh pl, vh ph) leave
        out, |vl| <= 2^-8 |v| and pl <= 2^-8 p.  It is in the numerator only (the row sum has no V), so it weighs on w,
        not on dev: with one key dev is 0 and this term is all but the whole error
  al    row sum: 2 (Kl + 1) u |O|, Kl = N (mode 0: 2 N), plus the padded tile's cancelled ones (16-bit): the row sum
        starts at -npad and the partial tile adds npad ones, 64 additions at magnitude <= npad: 2 * 65 u npad / L0, L0 the
        sum at reference 0, at least 2^-12 npad or the wave re-runs (attention_pipe.hip ``padsum * padv * 0x1p-12f``);
        a row whose L0 is below that, or out of [2^-60, 2^100), re-runs on tiles that mask the padded keys: no term
  4 u |O|    the reciprocal and the product
  store      half an ulp of the output type (bf16 2^-8 of the value, fp16 2^-11 and 2^-25 below its normal range)
bound = (d dev + (ao + al + 4 u |O|) (1 + d)) / (1 - d - al / |O|), then the store of |exact| + that.  None of it comes
from a run.  The backstop of mode 0 (attention.hip ``attn_item3_kernel``'s ``exact_rows(p, Kg, Vg, qrow, orow, ..., c)``
on the unsplit fp32 q c, K and V^T) computes a more exact quantity than the split kernel: each operand's hi + lo leaves
2^-16 of it and the kernel drops lo x lo (2^-8 * 2^-8), so its score is up to 3 * 2^-16 sum |q k| away and its V up to
2^-16 |v|.  A mode-0 launch that holds a query whose re-run overflows (``lead``: its later tiles' max less its first
tile's, at least 100 - log2 N - 1) gets ln 2 * 3 * 2^-16 mag added to d and 2^-16 w to ao, for every query: the backstop
is taken per 32-query chain and state 2 puts such a query into nearly every chain.
The unprescaled 16-bit taps do not run state 2: their backstop takes (float)q * c unrounded (attention_pipe.hip
``exact_rows(..., p.q_prescaled ? 1.0f : c)``) where the kernel's score MFMAs take it rounded to bf16 / fp16, 2^-8 /
2^-11 of every product away -- a term of ln 2 * 2^-8 mag, about 10 % of p at state 2's magnitudes, would hold the
backstop to nothing; its addressing is held on bits by the shifted selection case, which reaches it in those taps too.

``fault`` injects one of ``FAULTS`` (module constant; ``applies`` says where each is a fault at all).
"""

from __future__ import annotations

import math
from typing import NamedTuple

import torch

from feat_block_cases import C32
from item_qkv_cases import INT as _INT, SENTINEL as _SENTINEL
from layer_tail_cases import H, HD, U, _r, store_bound

QPB = 256  # kernels.h ATTN_ITEM_QPB
KT = 64
FAULTS = ("last_key_dropped", "pad_key_counted", "k_perm_on_v", "test_rows_own_head", "head_div_qpb", "col_prev",
          "cache_full_stride", "no_prescale", "double_prescale", "last_from_row0", "clamp_stored", "out_row_shift",
          "p_not_rounded")
SENTINEL = {**_SENTINEL, torch.float16: 0x7E55}  # a quiet NaN with a payload in each output type
INT = {**_INT, torch.float16: torch.int16}

N_FULL = (1, 63, 64, 65, 127, 128, 129, 192, 193, 255, 256, 257, 321, 705)
Q_EDGES = (0, 1, 43, 130)
N_LAST = (1, 255, 256, 257, 321, 705)
Q_LAST = (1, 43, 130)
CACHED = ((1, 1), (37, 65), (129, 193), (300, 705))  # (S, N)


def q_pairs(i: int) -> tuple[int, int]:
    """The two test-row counts the i-th train-row count is paired with (``item_qkv_cases.q_pairs``' scheme)."""
    return (Q_EDGES[0], Q_EDGES[2]) if i % 2 == 0 else (Q_EDGES[1], Q_EDGES[3])


class Way(NamedTuple):
    mode: int  # 0, 2: the fp32 kernels; 1, 5: attn_pipe_kernel storing bf16 / fp16
    prescaled: bool
    qk: object  # Q / K element type (None: fp32)
    out: object


OLD_BF16 = Way(1, False, torch.bfloat16, torch.bfloat16)
OLD_F16 = Way(5, False, torch.float16, torch.float16)


def forward_way(prec: int) -> Way:
    base = {3: 1, 4: 1, 6: 5, 7: 5}.get(prec, prec)
    if base in (0, 2):
        return Way(base, False, None, torch.float32)
    return Way(base, True, torch.bfloat16, torch.bfloat16 if base == 1 else torch.float16)


def is16(way: Way) -> bool:
    return way.mode in (1, 5)


def own_rows(form: int, S: int, N: int) -> tuple[int, int]:
    """(a0, na): the own-head rows of a form (capi.cpp ``item_attn_args``)."""
    if form == 2:
        return 0, 0
    if form == 1:
        return N - N % QPB, N % QPB
    return 0, N


def applies(fault: str, way: Way, form: int, T: int, S: int, N: int, nheads: int = H) -> bool:
    """Whether the fault changes anything for this way, form and shape."""
    nb = S if form == 2 else S - N
    a0, na = own_rows(form, S, N)
    if fault == "last_key_dropped":
        return N > 1
    if fault == "pad_key_counted":
        return N % KT != 0
    if fault == "k_perm_on_v":
        return N > 4
    if fault == "test_rows_own_head":
        return form != 2 and nb > 0 and nheads > 1
    if fault == "head_div_qpb":
        return nb > 0 and nb != QPB and nheads > 1
    if fault == "col_prev":
        return T > 1
    if fault == "cache_full_stride":
        return form == 2 and T > 1 and nheads > 1
    if fault == "no_prescale":
        return not way.prescaled
    if fault == "last_from_row0":
        return form == 1 and a0 > 0 and na > 0
    if fault == "clamp_stored":
        # (where the unclamped lanes' stores certainly land in the buffer on other values: an own-head sequence's onto
        # head 0's test rows, the cached form's onto the next row with the next column's q)
        return (form != 2 and na % KT != 0 and nb > 0 and nheads > 1) or (form == 2 and (nheads * nb) % KT != 0 and T > 1)
    if fault == "p_not_rounded":
        return is16(way)
    return True  # double_prescale, out_row_shift


# ---------------------------------------------------------------------------------------------- the restatement
def _bf(t: torch.Tensor) -> torch.Tensor:
    return t.float().to(torch.bfloat16).double()


def _split(x: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    hi = _bf(x)
    return hi, _bf((x.float() - hi.float()).double())


def q_operand(way: Way, q: torch.Tensor, fault: str | None = None) -> torch.Tensor:
    """Q as the score MFMAs read it (mode 0: hi + lo)."""
    times = (0 if way.prescaled else 1) - (fault == "no_prescale") + (fault == "double_prescale")
    x = q.double()
    for _ in range(times):
        x = (x.float() * C32).double()  # one fp32 multiply
        if is16(way):
            x = _r(x, way.qk)
    return x


def _perm23(n: int) -> torch.Tensor:
    i = torch.arange(n)
    return (i & ~12) | ((i & 4) << 1) | ((i & 8) >> 1)


class _Seq:
    """One K / V sequence as the kernels read it: keys [0, nk), the mode's operand planes."""

    def __init__(self, way: Way, k: torch.Tensor, vt: torch.Tensor, nk: int, fault: str | None):
        n = nk - 1 if fault == "last_key_dropped" and nk > 1 else nk
        v = torch.nan_to_num(vt.double(), nan=0.0)  # (the kernels zero V^T at keys >= nk)
        if fault == "k_perm_on_v":
            p = _perm23(v.shape[1])
            v = torch.where((p < nk)[None], v[:, p], torch.zeros_like(v))
        self.k, self.v, self.n = k[:n].double(), v[:, :n], n
        self.way = way
        self.extra = 1.0 if fault == "pad_key_counted" and nk % KT else 0.0  # one padded key: s = 0, p = 1, V = 0

    def scores(self, qop: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
        """(s, sum |q k|) [rows][keys] in log2 units."""
        if self.way.mode == 0:
            qh, ql = _split(qop)
            kh, kl = _split(self.k)
            s = qh @ kl.T + ql @ kh.T + qh @ kh.T
            m = qh.abs() @ kl.abs().T + ql.abs() @ kh.abs().T + qh.abs() @ kh.abs().T
            return s, m
        return qop @ self.k.T, qop.abs() @ self.k.abs().T

    def values(self) -> torch.Tensor:
        if self.way.mode == 0:
            vh, vl = _split(self.v)
            return vh + vl
        return self.v


def _soft(seq: _Seq, qop: torch.Tensor, want_mag: bool, round_p: bool) -> dict:
    """softmax(s) V of the rows qop [n][32] against one sequence: ``pre`` (P rounded where the way rounds it), ``exact``
    and, ``want_mag``, the bound's magnitudes."""
    s, mag = seq.scores(qop)
    v = seq.values()  # [32][keys]
    mi = torch.floor(s.max(1).values)  # an integer reference: 2^mi commutes with every rounding
    e = torch.exp2(s - mi[:, None])
    pad = seq.extra * torch.exp2(-mi)
    L = e.sum(1) + pad
    exact = (e @ v.T) / L[:, None]
    if is16(seq.way) and round_p:
        p = _bf(e)
        pre = (p @ v.T) / (p.sum(1) + pad)[:, None]
    else:
        pre = exact
    r = dict(pre=pre, exact=exact)
    if want_mag:
        r["w"] = (e @ v.abs().T) / L[:, None]
        dev = torch.empty_like(exact)
        for i in range(0, e.shape[0], 64):
            dev[i:i + 64] = (e[i:i + 64, :, None] * (v.T[None] - exact[i:i + 64, None, :]).abs()).sum(1)
        r["dev"] = dev / L[:, None]
        r["mag"] = mag.max(1).values
        r["smax"] = s.abs().max(1).values
        r["log2L0"] = torch.log2(L) + mi  # the row sum at reference 0
        first = s[:, :KT].max(1).values  # the re-run's reference: the first tile's max
        r["lead"] = (s[:, KT:].max(1).values - first) if s.shape[1] > KT else torch.full_like(first, -math.inf)
    return r


_PER_ELEM = ("pre", "exact", "w", "dev")
_PER_QUERY = ("mag", "smax", "log2L0", "lead")


def attend(way: Way, form: int, q: torch.Tensor, k: torch.Tensor, vt: torch.Tensor, N: int, fault: str | None = None,
           want_mag: bool = False) -> dict:
    """The attention of a form on stored operands (module docstring).  Returns ``pre``, ``exact``, ``out`` and
    ``written`` in out's layout [T][S][H * 32] and, ``want_mag``, ``w``, ``dev`` (same layout) and ``mag``, ``smax``,
    ``log2L0`` per query [T][S][H]."""
    assert fault is None or fault in FAULTS
    T, nh, S, _ = q.shape
    Hk, Npad = k.shape[1], k.shape[2]
    assert Hk == (1 if form == 2 else nh) and Npad % KT == 0 and 0 < N <= Npad and (form == 2 or N <= S)
    a0, na = own_rows(form, S, N)
    b0, nb = (0, S) if form == 2 else (N, S - N)
    qop = q_operand(way, q, fault)
    names = _PER_ELEM + _PER_QUERY if want_mag else ("pre", "exact")
    res = {n: torch.zeros(T, S, nh, HD if n in _PER_ELEM else 1, dtype=torch.float64) for n in names}
    written = torch.zeros(T, S, nh, HD, dtype=torch.bool)

    def column(b: int) -> int:
        if fault == "col_prev":
            return max(b - 1, 0)
        if fault == "cache_full_stride" and form == 2:
            return min(b * nh, T - 1)  # (past the buffer's end: the last column stands for what lies there)
        return b

    seqs: dict = {}

    def seq(b: int, g: int) -> _Seq:
        if (b, g) not in seqs:
            seqs[b, g] = _Seq(way, k[column(b), g], vt[column(b), g], N, fault)
        return seqs[b, g]

    def put(b: int, h: int, rows: slice, r: dict) -> None:
        for n in names:
            t = r[n]
            res[n][b, rows, h] = t if t.dim() == 2 else t[:, None]
        written[b, rows, h] = True

    rp = fault != "p_not_rounded"
    for b in range(T):
        for h in range(nh):
            if na > 0:
                rows = slice(0, na) if fault == "last_from_row0" else slice(a0, a0 + na)
                put(b, h, rows, _soft(seq(b, h), qop[b, h, rows], want_mag, rp))
            if nb > 0:
                g = h if fault == "test_rows_own_head" and form != 2 else 0
                put(b, h, slice(b0, b0 + nb), _soft(seq(b, g), qop[b, h, b0:b0 + nb], want_mag, rp))

    if fault == "head_div_qpb" and nb > 0:
        # query jj of the shared sequence taken as head jj / 256, row b0 + jj % nb: those (head, row) pairs get their
        # own (right) results, the others are never stored
        jj = torch.arange(nh * nb)
        hf, sf = jj // QPB, b0 + jj % nb
        keep = torch.zeros(S, nh, dtype=torch.bool)
        keep[sf[hf < nh], hf[hf < nh]] = True
        written[:, b0:b0 + nb] &= keep[None, b0:b0 + nb, :, None]
    if fault == "clamp_stored":
        # lanes j in [cnt, cnt rounded up to the wave) of every K sequence run unclamped, through attn_item.h
        # ``item_query``'s second branch: query jj = j - na as head jj / nb, row b0 + jj % nb (no test rows: row a0 + j of
        # head g), both as flat indices into q and out
        qflat = qop.reshape(T * nh * S, HD)
        for b in range(T):
            for g in range(nh if form != 2 else 1):
                cnt = na + (nh * nb if g == 0 else 0)
                if cnt == 0:
                    continue
                for j in range(cnt, (cnt + KT - 1) // KT * KT):
                    if nb > 0:
                        jj = j - na
                        hq, sq = jj // nb, b0 + jj % nb
                    else:
                        hq, sq = g, a0 + j
                    qi, oi = (b * nh + hq) * S + sq, (b * S + sq) * nh + hq
                    if qi >= T * nh * S or oi >= T * S * nh:
                        continue
                    r = _soft(seq(b, g), qflat[qi:qi + 1], want_mag, rp)
                    for n in names:
                        res[n].reshape(T * S * nh, -1)[oi] = r[n].reshape(-1)
                    written.reshape(T * S * nh, HD)[oi] = True
    if fault == "out_row_shift":
        idx = torch.clamp(torch.arange(S) + 1, max=S - 1)
        for n in names:  # row s holds row s + 1's result (the last row its own)
            res[n] = res[n][:, idx]
    out = {n: (t.reshape(T, S, nh * HD) if n in _PER_ELEM else t.reshape(T, S, nh)) for n, t in res.items()}
    out["written"] = written.reshape(T, S, nh * HD)
    out["out"] = out["pre"].float().to(way.out)
    out.update(way=way, form=form, N=N, npad=Npad - N if N % KT else 0)
    return out


def bits(r: dict) -> torch.Tensor:
    """What the caller's sentinel-filled out buffer holds after the launch, as integers."""
    t = r["out"]
    s = torch.full(t.shape, SENTINEL[t.dtype], dtype=INT[t.dtype])
    return torch.where(r["written"], t.contiguous().view(INT[t.dtype]), s)


def selection_passes(got_bits: torch.Tensor, r: dict) -> bool:
    """The selection case's comparison of a buffer (integers of the output type) with the restatement r: on bits in
    the 16-bit ways; in modes 0 and 2 the sentinels on bits and the stored values within 4 u |v|."""
    want = bits(r)
    if is16(r["way"]):
        return torch.equal(got_bits, want)
    w = r["written"]
    if not torch.equal(got_bits[~w], want[~w]):
        return False
    got, ref = got_bits.view(torch.float32).double()[w], r["exact"][w]
    return bool(((got - ref).abs() <= 4 * U * ref.abs()).all())  # (a NaN fails)


# ---------------------------------------------------------------------------------------------- bounds
def elem_bound(r: dict) -> torch.Tensor:
    """The spread case's per-element bound of |stored - exact| (module docstring); r from ``attend(want_mag=True)``."""
    way, N = r["way"], r["N"]
    ks, ko, kl, ep = {0: (96, 3 * N, 2 * N, 2.0 ** -16), 2: (64, 2 * N, N, 0.0)}.get(way.mode, (32, N, N, 2.0 ** -8))
    tiles = (N + KT - 1) // KT
    d = (math.log(2.0) * 2 * (ks + 1) * U * (r["mag"] + r["smax"]) + 4 * U + ep)[..., None]  # per query
    # mode 0's backstop: a launch that holds a query whose re-run overflows (its later tiles lead the first tile's max
    # by 100 log2 units, less the log2 of the key count and one for the sum's rounding) may send any of its queries there
    backstop = way.mode == 0 and float(r["lead"].max()) >= 100.0 - math.log2(N) - 1.0
    if backstop:
        d = d + (math.log(2.0) * 3 * 2.0 ** -16 * r["mag"])[..., None]
    O, w, dev = r["exact"].abs(), r["w"], r["dev"]
    shape = O.shape
    q = lambda t: t.reshape(*shape[:2], -1, HD)  # [T][S][H][32]
    lolo = 2.0 ** -16 if way.mode == 0 else 0.0  # the dropped V lo x P lo; the backstop: what V's hi + lo leaves
    ao = (2 * (ko + 1) * U + (4 * U * tiles if way.mode == 2 else 0.0) + lolo + (2.0 ** -16 if backstop else 0.0)) * q(w)
    rl = torch.full_like(d, 2 * (kl + 1) * U + (4 * U * tiles if way.mode == 2 else 0.0))  # relative, of the row sum
    if is16(way) and r["npad"]:
        # only a wave that keeps its first pass has them: a row sum below 2^-12 npad (computed to 130 u npad: 2^-5 of
        # slack on the threshold is ample) or out of [2^-60, 2^100) re-runs, on tiles that mask the padded keys
        lg = r["log2L0"][..., None]
        kept = (lg >= math.log2(2.0 ** -12 * r["npad"] * (1 - 2.0 ** -5))) & (lg < 100.01)
        l0 = torch.exp2(torch.clamp(lg, min=-100.0, max=101.0))
        rl = rl + torch.where(kept, 2 * (KT + 1) * U * r["npad"] / l0, torch.zeros_like(l0))
    b0 = (d * q(dev) + (ao + (rl + 4 * U) * q(O)) * (1 + d)) / (1 - d - rl)
    b0 = b0.reshape(shape)
    if way.out is torch.float32:
        return b0
    top = O + b0
    if way.out is torch.float16:
        return b0 + store_bound(5, top) + 2.0 ** -25
    return b0 + 8.0 * store_bound(5, top)  # bf16: 8 significant bits


def ratio(got: torch.Tensor, r: dict) -> float:
    """Worst |got - exact| / bound over the written elements."""
    w = r["written"]
    d = (got.double() - r["exact"]).abs()[w]
    return float((d / elem_bound(r)[w]).max())


# ---------------------------------------------------------------------------------------------- operands
def _gen(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(seed)


def _pad(k: torch.Tensor, v: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """k [T][H][N][32], v [T][H][N][32] -> k [T][H][Npad][32], vt [T][H][32][Npad] with NaN padding."""
    T, nh, N, _ = k.shape
    Npad = (N + KT - 1) // KT * KT
    kp = torch.full((T, nh, Npad, HD), float("nan"), dtype=torch.float64)
    vt = torch.full((T, nh, HD, Npad), float("nan"), dtype=torch.float64)
    kp[:, :, :N], vt[:, :, :, :N] = k, v.transpose(2, 3)
    return kp, vt


def cached_operands(c: dict) -> dict:
    """Form 2's operands of a form-0 case: its test rows' q, head 0's K / V^T."""
    N = c["N"]
    d = dict(c, q=c["q"][:, :, N:].contiguous(), k=c["k"][:, :1].contiguous(), vt=c["vt"][:, :1].contiguous(),
             S=c["S"] - N)
    if "pi" in c:
        d["pi"] = c["pi"][:, :, N:]
    return d


def _stride(nk: int) -> int:
    s = min(65, nk)
    while math.gcd(s, nk) != 1:
        s += 1
    return s


def selection_case(T: int, S: int, N: int, prescaled: bool, shifted: bool = False, nheads: int = H) -> dict:
    """Form 0's operands of the selection case (module docstring): q, k, vt as float64 holding the stored values, and
    pi [T][H][S], the key every query selects."""
    nbits = max(1, (N - 1).bit_length())
    assert 2 * nbits <= 30
    A = 32.0 if prescaled else 128.0
    code = lambda idx: (2 * ((idx[..., None] >> torch.arange(nbits)) & 1) - 1).double()
    b, h = torch.arange(T)[:, None], torch.arange(nheads)[None, :]
    xmask = ((b * nheads + h) * 37) % (1 << nbits)  # [T][H]
    keys = torch.arange(N)
    k = torch.zeros(T, nheads, N, HD, dtype=torch.float64)
    k[..., :nbits] = code(keys[None, None, :] ^ xmask[..., None])
    k[..., nbits:2 * nbits] = 1.0
    k[..., 30] = 1.0
    # pi by position in the K sequence, as the kernels number its queries: own rows j = s of (b, h); test rows
    # j = N + h (S - N) + (s - N) of (b, 0)
    s = torch.arange(S)[None, None, :]
    own = s < N
    j = torch.where(own, s, N + h[..., None] * (S - N) + (s - N)).expand(T, nheads, S)
    g = torch.where(own, h[..., None], torch.zeros_like(h[..., None])).expand(T, nheads, S)
    bb = b[..., None].expand(T, nheads, S)
    pi = (_stride(N) * j + 17 * bb + 5 * g) % N
    q = torch.zeros(T, nheads, S, HD, dtype=torch.float64)
    q[..., :nbits] = A * code(pi ^ xmask[bb, g])
    q[..., nbits:2 * nbits] = -A
    if shifted:
        up, down = (110.0, -80.0) if prescaled else (448.0, -320.0)
        srow = torch.arange(S)
        shift = torch.zeros(S, dtype=torch.float64)
        shift[srow % 5 == 2], shift[srow % 5 == 4] = up, down
        q[..., 30] = shift
    gen = _gen(8100 + 7 * T + 3 * N + nheads)
    m = torch.randint(0, 8, (T, nheads, N, HD), generator=gen).double()
    e = torch.randint(-2, 2, (T, nheads, N, HD), generator=gen).double()
    sign = 2.0 * torch.randint(0, 2, (T, nheads, N, HD), generator=gen).double() - 1.0
    v = sign * (8.0 + m) / 8.0 * torch.exp2(e)
    kp, vt = _pad(k, v)
    return dict(q=q, k=kp, vt=vt, pi=pi, T=T, S=S, N=N, H=nheads, prescaled=prescaled, shifted=shifted)


def check_selection_operands(c: dict, way: Way) -> None:
    """What the selection case's bitwise claim rests on; a generator that breaks one of them fails here, on the CPU."""
    T, S, N, nh = c["T"], c["S"], c["N"], c["H"]
    assert way.prescaled == c["prescaled"]
    q, k, v = c["q"], c["k"][:, :, :N], c["vt"][:, :, :, :N]
    for name, t in (("q", q), ("k", k), ("vt", v)):
        for ty in (torch.bfloat16, torch.float16):
            assert torch.equal(_r(t, ty), t), f"{name} is not exact in {ty}"
        hi, lo = _split(t)
        assert torch.equal(hi, t) and not bool(lo.any()), f"{name} has a lo plane"
    a = v.abs()
    ex = torch.floor(torch.log2(a))
    assert bool((a * torch.exp2(3 - ex) == torch.round(a * torch.exp2(3 - ex))).all()), "V: more than 4 significant bits"
    assert float(a.min()) >= 2.0 ** -6 and float(a.max()) <= 448.0, "V outside e4m3's normal range"
    vecs = v.permute(0, 1, 3, 2).reshape(-1, HD)
    n = len({tuple(x) for x in vecs.tolist()})
    assert n == vecs.shape[0], f"{n} of {vecs.shape[0]} V vectors distinct"
    # the score gap in the way's own Q operand, the shift (dimension 30, the same for every key) taken out
    qop = q_operand(way, q)
    own = torch.arange(S) < N
    for b in range(T):
        for h in range(nh):
            for rows, g in ((own, h), (~own, 0)):
                if not bool(rows.any()):
                    continue
                seq = _Seq(way, c["k"][b, g], c["vt"][b, g], N, None)
                sc, _ = seq.scores(qop[b, h, rows])
                sc = sc - (qop[b, h, rows, 30] * 1.0)[:, None]
                chosen = sc.gather(1, c["pi"][b, h, rows][:, None])[:, 0]
                tol = 0.0 if is16(way) else 2.0 ** -10
                assert float(chosen.abs().max()) <= tol, (b, h, float(chosen.abs().max()))
                rest = sc.scatter(1, c["pi"][b, h, rows][:, None], -1e9)
                assert N == 1 or float(rest.max()) <= -64.0 + tol, (b, h, float(rest.max()))
    # coverage: every key of a sequence with at least N queries is chosen; consecutive queries, other tiles
    for b in range(T):
        for g in range(nh):
            chosen = c["pi"][b, g, :N]
            if g == 0:
                chosen = torch.cat([chosen] + [c["pi"][b, h, N:] for h in range(nh)])
            assert len(set(chosen.tolist())) == N, (b, g)
            if N >= 193:
                assert bool((chosen[1:] // KT != chosen[:-1] // KT).all()), (b, g)


def spread_case(T: int, S: int, N: int, prescaled: bool, state: int = 0, nheads: int = H) -> dict:
    """Form 0's operands of the spread case (module docstring), as float64 of fp32 values (a launch rounds them to its
    own operand types; ``stored`` does the same for the restatement)."""
    gen = _gen(8200 + 13 * T + 5 * S + N + nheads)
    draw = lambda *shape: torch.randn(*shape, generator=gen).float().double()
    c64 = math.log2(math.e) / math.sqrt(HD)
    gq = 3.0 / math.sqrt(HD - 2) / (1.0 if prescaled else c64)
    q, k, v = gq * draw(T, nheads, S, HD), draw(T, nheads, N, HD), draw(T, nheads, N, HD)
    q[..., 30:] = 0.0
    k[..., 30] = 1.0
    k[..., 31] = (torch.arange(N) >= KT).double()
    if state:
        unit = 1.0 if prescaled else 1.0 / c64
        s = torch.arange(S)
        shift = torch.zeros(S, dtype=torch.float64)
        shift[s % 7 == 3], shift[s % 7 == 5], shift[s % 7 == 1] = 110.0, -80.0, -12.0
        q[..., 30] = shift * unit
        if state == 2:
            q[..., 31] = (s % 11 == 4).double() * 120.0 * unit
    kp, vt = _pad(k, v)
    return dict(q=q.float().double(), k=kp, vt=vt, T=T, S=S, N=N, H=nheads, prescaled=prescaled, state=state)


def stored(way: Way, c: dict) -> dict:
    """The case's operands as a launch of this way stores them: Q / K in the way's type, V^T in bf16 (fp32 ways: fp32)."""
    if not is16(way):
        return dict(c, q=c["q"].float().double(), k=c["k"].float().double(), vt=c["vt"].float().double())
    return dict(c, q=_r(c["q"], way.qk), k=_r(c["k"], way.qk), vt=_r(c["vt"], torch.bfloat16))
