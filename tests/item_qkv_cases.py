"""Operands, float64 restatement and bounds of the item attention's projection,

    Q = X Wq^T,  K = X Wk^T,  V^T = (X Wv^T)^T   per token column, train rows [0, N) through q|k|v, test rows [N, S)
                                                  through the test rows' q,

shared by tests/test_item_qkv_gpu.py (which holds ``mmpfn_item_qkv`` to them) and tests/test_item_qkv_sensitivity.py
(which shows on the CPU what they catch).  No GPU here.  States are in the engine's order, X [M][T][S][E]; a weight set
is ``Wtr`` [576][192] (rows 192 j + 32 h + d of q, k, v: ``_w_qkv`` [3][H][32][E] flattened) and ``Wte`` [192][192], the
test rows' q (``Wtr[:192]`` unless the model has ``two_sets_of_queries``: then ``_w_q[0]`` | ``_w_kv`` and ``_w_q[1]``).
Outputs are in the attention's layouts, q [TM][H][S][32], k [TM][H][Npad][32], vt [TM][H][32][Npad] with TM = M T token
columns (``last``: column T - 1 of every member alone, TM = M) and Npad = N rounded up to 64; N = 0 is the train-KV
cache's predict form, every row through ``Wte``, nothing stored to k / vt.

The restatement (``project``) is float64 arithmetic that rounds only where the mode rounds, read from the sources:
  mode 1 (bf16)   X to bf16 (rowgemm.hip ``qkv2_tile``); W to bf16, its q rows first multiplied in fp32 by
                  fl32(log2(e) / sqrt(32)) (weight_pack.h ``prescale_item_q``; ``feat_block_cases.C32``); fp32
                  accumulation; Q, K, V^T stored in bf16.
  mode 5 (fp16)   X is fp16 already (the state), W to fp16 after the same prescale; Q, K and V^T stored in bf16 all the
                  same (the item attention's S runs on bf16 MFMA in every 16-bit mode).  At T > 64 it is mode 1 (``decode_prec``).
  mode 0 (fp32)   W split as weight_pack.h ``split_bf16`` splits it, hi = bf16(w), lo = bf16(w - hi); X split the same
                  way in registers (rowgemm3.hip ``split_rows3``); three products per element, w_lo x_hi + w_hi x_lo +
                  w_hi x_hi, the lo x lo one dropped; q not prescaled; fp32 stores.
  mode 2          nothing is rounded (gemm.hip on the fp32-input MFMA); q not prescaled.
``pre`` is the float64 value in front of the store, ``out`` the stored one, ``mag`` the sum of the magnitudes of the
products that ``pre`` sums.  ``bits`` turns a result into what the caller's buffers hold afterwards as integers: the
stored element's bit pattern where the kernels store, the caller's sentinel elsewhere -- K rows and V^T columns
[N, Npad), and everything the restatement marks unwritten.

``fault`` injects one of ``FAULTS``, each what a kernel or host bug of that name would compute:
  row_shift          position p of a column holds row p + 1 (the last row twice)
  col_prev           column c reads column c - 1 (column 0 itself)
  member_prev        member m reads member m - 1 (member 0 itself)
  heads_swapped      heads 0 and 1 swapped in q, k and vt
  test_q_from_train  the test rows through the train rows' q weights (a fault on a ``two_sets_of_queries`` model only)
  no_prescale        the 16-bit modes' q without log2(e) / sqrt(32)
  last_wrong_col     ``last`` projects column 0
  kv_tail_missing    the last N % 8 keys of K and V^T are not written
  vt_not_transposed  V stored [pos][d] where V^T [d][Npad] belongs
  drop_lo_hi         mode 0 without the x_lo w_hi product

Address case (``address_state``), bitwise in every mode.  Every state row is 2^a e_j, one non-zero feature, j = r % 192
and a = (r // 192) % 4 with r the row's index in the [M][T][S] order.  Every projected element is then one product with
exact zeros around it, 2^a W[n][j] in the mode's operand form (mode 0: 2^a (hi + lo)): exact in fp32 in any order of
accumulation, so the kernel must equal the restatement bit for bit -- in the 16-bit modes after the one bf16 rounding
of the store, which is deterministic (exact in mode 1, where the operand is bf16 already).  Weights (``address_weights``)
are N(0, 1 / 192), synth's scale, with |w| raised to at least 2^-10 so that no operand, product or store is subnormal
in any type.  ``check_address_weights`` asserts what this rests on: fl32(hi + lo) == hi + lo for every weight, no
subnormal operand, and that all 32-dim output vectors W[32 b .. 32 b + 31][j] (every 32-row block b of ``Wtr`` and
``Wte``, every feature j), times every 2^a, are distinct in the mode's form, so that a row, a column, a member, a head or
a weight set taken wrongly shows as a different bit pattern.

Normal case (``normal_state``, ``normal_weights``), bounded per element; u = 2^-24, K = 192.  None of the bounds comes
from a run of a kernel.
  mode 2     |got - pre| <= 2 (K + 1) u mag: K products and K - 1 additions in fp32, any order, gamma_{K+1} to first
             order; doubled, as ``layer_tail_cases`` doubles its accumulation bounds: the MFMA's internal adder is not
             documented to round to nearest.
  mode 0     pre is the float64 sum of the three products; 3 K terms: 2 (3 K + 1) u mag.
  1 and 5    the same accumulation bound a, and the bf16 store: the kernel rounds a value within a of pre, half an ulp
             of bf16 (8 significant bits) is at most 2^-8 of it: a + 2^-8 (|pre| + a).  ``layer_tail_cases.store_bound``
             is that half ulp for fp16's 11 bits; bf16's is 2^3 times it.
This is the case that sees X's lo plane (the x_lo w_hi product) and the k-step order; the address case's X has no lo part.
"""

from __future__ import annotations

import math

import torch

from feat_block_cases import C32
from layer_tail_cases import E, H, HD, MODES, OP, U, _r, state_in, store_bound

LAYER0 = "transformer_encoder.layers.0.self_attn_between_items."
FAULTS = ("row_shift", "col_prev", "member_prev", "heads_swapped", "test_q_from_train", "no_prescale",
          "last_wrong_col", "kv_tail_missing", "vt_not_transposed", "drop_lo_hi")
WMIN = 2.0 ** -10
# sentinels: a quiet NaN with a payload, as the element type's integer -- no store of a finite projection equals it
SENTINEL = {torch.float32: 0x7FC5A5A5, torch.bfloat16: 0x7FE5}
INT = {torch.float32: torch.int32, torch.bfloat16: torch.int16}

N_EDGES = (1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 127, 128, 129, 160)
Q_EDGES = (0, 1, 33, 130)
CACHE_S = (1, 37, 129)


def q_pairs(i: int) -> tuple[int, int]:
    """The two test-row counts that the i-th train-row count of ``N_EDGES`` is paired with; over two consecutive i every
    count of ``Q_EDGES`` occurs."""
    return (Q_EDGES[0], Q_EDGES[2]) if i % 2 == 0 else (Q_EDGES[1], Q_EDGES[3])


def decode(mode: int, T: int) -> int:
    """capi.cpp ``decode_prec`` on the base modes: the fp16 mode holds a row's tokens as up to four 16-token tiles."""
    return 1 if mode == 5 and T > 64 else mode


def out_dtype(mode: int):
    return torch.float32 if OP[mode] is None else torch.bfloat16


def applies(fault: str, mode: int, two: bool) -> bool:
    """Whether the fault changes anything in this mode on this kind of model."""
    if fault == "no_prescale":
        return OP[mode] is not None
    if fault == "drop_lo_hi":
        return mode == 0
    if fault == "test_q_from_train":
        return two
    return True


# ---------------------------------------------------------------------------------------------- the restatement
def _bf(t: torch.Tensor) -> torch.Tensor:
    return t.float().to(torch.bfloat16).double()


def _terms(mode: int, x: torch.Tensor, w: torch.Tensor, prescale: bool, fault: str | None) -> list:
    """The (x, w) operand pairs whose products the mode sums for x [.., E] (the state as the kernel reads it) and the
    fp32 weight rows w [n][E]."""
    op = OP[mode]
    if mode == 2:
        return [(x, w.double())]
    if mode == 0:
        wh, xh = _bf(w), _bf(x)
        wl, xl = _bf(w - wh), _bf(x - xh)  # (an fp32 value less its bf16 rounding is exact, in fp32 as in float64)
        t = [(xh, wl), (xh, wh)]
        if fault != "drop_lo_hi" and bool((xl != 0).any()):
            t.insert(1, (xl, wh))
        return t
    if prescale and fault != "no_prescale":
        w = (w.float() * C32).double()
    return [(_r(x, op), _r(w, op))]


def _heads(y: torch.Tensor) -> torch.Tensor:
    """[TM][rows][192] -> [TM][H][rows][32]."""
    return y.reshape(y.shape[0], y.shape[1], H, HD).permute(0, 2, 1, 3)


def project(mode: int, X: torch.Tensor, W: dict, N: int, last: bool = False, fault: str | None = None,
            want_mag: bool = False) -> dict:
    """The projection of X [M][T][S][E] with N train rows (module docstring).  Returns per output o in q, k, vt:
    ``pre[o]``, ``out[o]``, ``mag[o]`` (``want_mag``) and ``written[o]``, a mask of the elements the kernels store."""
    assert fault is None or fault in FAULTS
    M, T, S, _ = X.shape
    assert 0 <= N <= S
    mode = decode(mode, T)
    xs = state_in(mode, X)
    if fault == "member_prev":
        xs = torch.cat([xs[:1], xs[:-1]])
    if last:
        xs = xs[:, :1] if fault == "last_wrong_col" else xs[:, T - 1:]
    TM = xs.shape[0] * xs.shape[1]
    cols = xs.reshape(TM, S, E)
    if fault == "col_prev":
        cols = torch.cat([cols[:1], cols[:-1]])
    if fault == "row_shift":
        cols = torch.cat([cols[:, 1:], cols[:, -1:]], dim=1)
    Npad = (N + 63) // 64 * 64
    Wtr, Wte = W["Wtr"], W["Wte"]
    wq_test = Wtr[:E] if fault == "test_q_from_train" else Wte

    def gemm(x, w, prescale):
        terms = _terms(mode, x, w, prescale, fault)
        return (sum(x @ w.T for x, w in terms),
                sum(x.abs() @ w.abs().T for x, w in terms) if want_mag else None)

    zeros = lambda *shape: torch.zeros(shape, dtype=torch.float64)
    pre = dict(q=zeros(TM, H, S, HD), k=zeros(TM, H, Npad, HD), vt=zeros(TM, H, HD, Npad))
    mag = {o: torch.zeros_like(t) for o, t in pre.items()} if want_mag else None
    written = {o: torch.zeros(t.shape, dtype=torch.bool) for o, t in pre.items()}
    written["q"][:] = True

    if N > 0:
        for name, rows, prescale in (("q", Wtr[:E], True), ("k", Wtr[E:2 * E], False), ("v", Wtr[2 * E:], False)):
            p, g = gemm(cols[:, :N], rows, prescale)
            for dst, val in ((pre, p), (mag, g)):
                if val is None:
                    continue
                v = _heads(val)  # [TM][H][N][32]
                if name == "q":
                    dst["q"][:, :, :N] = v
                elif name == "k":
                    dst["k"][:, :, :N] = v
                elif fault == "vt_not_transposed":
                    dst["vt"].reshape(TM, H, HD * Npad)[:, :, :N * HD] = v.reshape(TM, H, N * HD)
                else:
                    dst["vt"][:, :, :, :N] = v.transpose(2, 3)
        nw = N - N % 8 if fault == "kv_tail_missing" else N
        written["k"][:, :, :nw] = True
        if fault == "vt_not_transposed":
            written["vt"].reshape(TM, H, HD * Npad)[:, :, :nw * HD] = True
        else:
            written["vt"][:, :, :, :nw] = True
    if N < S:
        p, g = gemm(cols[:, N:], wq_test, True)
        pre["q"][:, :, N:] = _heads(p)
        if want_mag:
            mag["q"][:, :, N:] = _heads(g)
    if fault == "heads_swapped":
        for d in (pre, mag, written):
            if d is not None:
                for o in d:
                    d[o] = torch.cat([d[o][:, 1:2], d[o][:, :1], d[o][:, 2:]], dim=1)
    odt = out_dtype(mode)
    out = {o: t.float().to(odt) for o, t in pre.items()}
    return dict(mode=mode, pre=pre, out=out, mag=mag, written=written, TM=TM, Npad=Npad)


def bits(r: dict) -> dict:
    """What the caller's sentinel-filled q, k and vt hold after the projection r, as integers."""
    res = {}
    for o, t in r["out"].items():
        s = torch.full(t.shape, SENTINEL[t.dtype], dtype=INT[t.dtype])
        res[o] = torch.where(r["written"][o], t.contiguous().view(INT[t.dtype]), s)
    return res


def same_bits(a: dict, b: dict) -> bool:
    return all(torch.equal(a[o], b[o]) for o in ("q", "k", "vt"))


# ---------------------------------------------------------------------------------------------- bounds
def elem_bound(r: dict, o: str) -> torch.Tensor:
    """The normal case's per-element bound of |stored - pre| (module docstring); r from ``project(want_mag=True)``."""
    mode = r["mode"]  # (decoded)
    k = 3 * E if mode == 0 else E
    a = 2.0 * (k + 1) * U * r["mag"][o]
    if OP[mode] is None:
        return a
    return a + 8.0 * store_bound(5, r["pre"][o].abs() + a)


def ratios(got: dict, r: dict) -> dict:
    """Worst |got - pre| / bound over the written elements of each output (0 where nothing is written)."""
    res = {}
    for o in ("q", "k", "vt"):
        w = r["written"][o]
        if not bool(w.any()):
            res[o] = 0.0
            continue
        d = (got[o].double() - r["pre"][o]).abs()[w]
        res[o] = float((d / elem_bound(r, o)[w]).max())
    return res


# ---------------------------------------------------------------------------------------------- operands
def _gen(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(seed)


def _weights(seed: int, two: bool, floor: float) -> dict:
    g = _gen(seed)
    f32 = lambda t: t.float().double()  # what the engine is given: fp32 values
    draw = lambda n: torch.randn(n, E, generator=g).double() / math.sqrt(E)
    Wtr, Wte = draw(3 * E), draw(E)
    if floor:
        Wtr, Wte = (torch.where(w.abs() < floor, floor * torch.where(w < 0, -1.0, 1.0), w) for w in (Wtr, Wte))
    Wtr = f32(Wtr)
    return dict(Wtr=Wtr, Wte=f32(Wte) if two else Wtr[:E].clone(), two=two)


def address_weights(two: bool) -> dict:
    return _weights(7100 + int(two), two, WMIN)


def normal_weights(two: bool) -> dict:
    return _weights(7200 + int(two), two, 0.0)


def address_state(M: int, T: int, S: int) -> torch.Tensor:
    """X [M][T][S][E]: row r = (m T + t) S + s is 2^((r // 192) % 4) e_(r % 192)."""
    r = torch.arange(M * T * S)
    X = torch.zeros(M * T * S, E, dtype=torch.float64)
    X[r, r % E] = 2.0 ** ((r // E) % 4).double()
    return X.reshape(M, T, S, E)


def normal_state(M: int, T: int, S: int, seed: int = 0) -> torch.Tensor:
    return torch.randn(M, T, S, E, generator=_gen(7300 + 1009 * M + 101 * S + T + seed)).float().double()


def operand_forms(mode: int, W: dict) -> torch.Tensor:
    """Every weight row as an address-case result of scale 1 sees it: [576 or 768][192] (``Wtr``, and ``Wte`` where it is a set of its own), float64."""
    eye = torch.eye(E, dtype=torch.float64)
    rows = []
    for w, prescale in ((W["Wtr"][:E], True), (W["Wtr"][E:], False)) + (((W["Wte"], True),) if W["two"] else ()):
        rows.append(sum(x @ v.T for x, v in _terms(mode, eye, w, prescale, None)).T)
    return torch.cat(rows)


def check_address_weights(W: dict) -> None:
    """The properties the address case's bitwise claim rests on; a generator that breaks one fails here, on the CPU."""
    both = torch.cat([W["Wtr"], W["Wte"]])
    assert float(both.abs().min()) >= WMIN
    hi = _bf(both)
    lo = _bf((both.float() - hi.float()).double())
    assert torch.equal((hi + lo).float().double(), hi + lo), "hi + lo must be exact in fp32"
    assert float(lo[lo != 0].abs().min()) >= 2.0 ** -126 and float((both.float() * C32).abs().min()) >= 2.0 ** -14
    for mode in MODES:
        f = operand_forms(mode, W)
        assert float(f.abs().min()) >= (2.0 ** -14 if mode == 5 else 2.0 ** -126)
        stored = f.float().to(out_dtype(mode)).double()
        vec = stored.reshape(-1, HD, E).permute(0, 2, 1).reshape(-1, HD)  # [blocks * 192 features][32]
        scaled = torch.cat([vec * 2.0 ** a for a in range(4)])
        n = len({tuple(v) for v in scaled.tolist()})
        assert n == scaled.shape[0], f"mode {mode}: {n} of {scaled.shape[0]} output vectors distinct"


def state_dict_with(sd: dict, W: dict) -> dict:
    """sd with the weight set written into layer 0's item attention (numpy float32, as the checkpoint ABI takes them:
    ``_w_qkv`` [3][H][32][E], or ``_w_q`` [2][H][32][E] (train, test) and ``_w_kv`` [2][H][32][E])."""
    sd = dict(sd)
    Wtr = W["Wtr"].float()
    if W["two"]:
        sd[LAYER0 + "_w_q"] = torch.stack([Wtr[:E], W["Wte"].float()]).reshape(2, H, HD, E).numpy()
        sd[LAYER0 + "_w_kv"] = Wtr[E:].reshape(2, H, HD, E).contiguous().numpy()
    else:
        sd[LAYER0 + "_w_qkv"] = Wtr.reshape(3, H, HD, E).contiguous().numpy()
    return sd
