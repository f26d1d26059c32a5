// Row-resident attention-between-features sublayer for gfx950 (bf16 performance mode):
//   X <- LayerNorm(X + MHA_features(X))        (layer.py:332-339,437-455; multi_head_attention.py:547-736)
//
// One wave owns one table row (its T <= 16*NT tokens) for the whole sublayer and never
// moves the row's data through LDS: every MFMA result is, lane for lane, the operand of the
// next MFMA (v_mfma_f32_16x16x32_bf16; lane l = (g = l>>4, n = l&15)):
//   X^T fragments     xf[tt][ks]  lane holds X[token 16tt+n][32ks+8g .. +7]            (B / A operand)
//   Q^T, K^T tiles    = W_{q,k} . X^T, W rows permuted so that tile f row 4g+i is head dim 8g+4f+i:
//                      the two tiles of a token tile concatenate into the lane's Q[token][8g..8g+7]
//                      -- the B operand (Q^T) and the A operand (K) of S^T = K Q^T
//   V tiles           = X . Wv^T (untransposed): lane holds V[token 16kt+4g+i][d = 16mt+n], two key
//                      tiles concatenate into the A operand V^T[d][keys] of O^T = V^T P^T, in the
//                      same permuted key order as P^T taken from the S^T accumulators
//   O^T tiles         lane holds O^T[d 16mt+4g+i][query n]; concatenated over mt they are the B
//                      operand (K-step h) of Y^T = Wout . O^T with Wout's columns permuted alike;
//                      the six heads' fragments are kept (6*NT regs) and the out-projection runs
//                      once after the last head, so no 192-wide accumulator lives across heads
//   Y^T accumulators  lane holds Y^T[feature 16f+4g+i][token n]: residual + LayerNorm per token
//                      with the 48 features of a lane reduced across the 4 lane groups.
// The softmax scale log2(e)/sqrt(32) is folded into Wq (exp2 on the scores).
// Only the weights move: they are stored as LDS images (capi.cpp pack_feat_rows: 416-B rows,
// so conflict-free ds_read_b128) and copied global -> LDS by LDS-DMA (global_load_lds, 1 KB
// per wave-instruction, no staging registers) in groups of 32 rows (13 KB: a head's Q, K or V rows, a sixth of the
// out-projection image) through a ring of 13-KB slots.  Six slots (78 KB) where nothing else needs LDS: the next
// head's Q | K | V in flight during the current head, one barrier per head, the 78 KB out-projection image whole at
// the end.  The three-tile full form, the one short of registers, keeps the last tile's finished O^T fragments in
// LDS (24 KB) instead, beside a three-slot ring (39 KB) handed on twice per head and once per out-projection group.
// The out-projection runs two token tiles per Wout fragment read.  <= 79872 B of LDS and <= 256 VGPRs per 4-row
// block, no scratch: two blocks per CU (NT = 4: one wave per SIMD).  Resources (VGPRs, LDS): NT = 3 full form 246 /
// 250 (fp16 / bf16), 64512 B; its last-layer form 184 / 182, 79872 B; tests/test_featrow_nospill_codegen.py.
// Per row: 6*(18*NT + NT^2 + 2*NT*ceil(NT/2)) + 72*NT MFMAs; HBM traffic = X read + written once (measured 0.99x).
//
// F16 (PREC_F16: the state X is fp16, the reference's autocast dtype): the row's X^T fragments are
// loaded as they are stored (16-B loads, no conversion) and are the exact residual, so X is read once;
// the out-projection image's rows are permuted (capi.cpp: pack_feat_rows res_perm) so that Y^T tile f
// row 4g+i is feature 32(f>>1) + 8g + 4(f&1) + i -- the features of the lane's X fragments -- and
// the normalised row is stored as 16-B pieces of 8 features.
#include <type_traits>

#include "common.h"
#include "kernels.h"
#include "lds_dma.h"

namespace mmpfn {

namespace {

constexpr int FR_E = 192;                        // model width
constexpr int FR_H = 6;                          // heads
constexpr int FR_ST = FEAT_IMG_STRIDE;           // bf16 row stride of every LDS image (416 B)
constexpr int FR_GRP = 32 * FR_ST;               // one image group = one ring slot: 32 rows, 6656 bf16 = 13 KB
constexpr int FR_GPIECES = FR_GRP * 2 / 1024;    // 1-KB DMA pieces per group (13)
constexpr int FR_QKV_GRPS = 3 * FR_H;            // groups 0 .. 17: head h's Q | K | V at 3 h + {0, 1, 2}; then Wout's
constexpr int FR_FRAG = 512;                     // one parked fragment of a wave: 64 lanes x 16 B (in bf16 elements)

// Where the finished O^T fragment of (head h, query tile t) waits for the out-projection: a parking place in LDS
// (the wave's own, lane-linear: each lane writes and later reads back its own 16 B, no conflicts), or -1 = in
// registers.  Only the three-tile full form is short of registers (two waves per SIMD: 256): it spilled 32 (fp16) /
// 16 (bf16) of them to scratch, which reached HBM.  Its tile 2 runs alone in the out-projection's second pass, so
// tile 2's six fragments are parked: the fewest that leave no spill in either form (parking tiles 0 and 1 of the
// first one or two heads as well measured the same, profiles/r08/INDEX.md).
template <int NT, bool LAST>
constexpr int fr_park(int h, int t) {
  return NT == 3 && !LAST && t == 2 ? h : -1;
}
template <int NT, bool LAST>
constexpr int FR_NPARK = NT == 3 && !LAST ? FR_H : 0;

template <typename X8>
__device__ __forceinline__ X8 cat8(const f32x4& a, const f32x4& b, float s = 1.0f) {
  typedef decltype(X8{}[0]) T;
  X8 r;
#pragma unroll
  for (int i = 0; i < 4; ++i) r[i] = (T)(a[i] * s), r[4 + i] = (T)(b[i] * s);
  return r;
}

typedef __attribute__((address_space(3))) void lds_void;

// LAST: the form of a forward's pruned last layer (capi.cpp last_layer_tail), which reads this sublayer's output at
// the target token T-1 only: K and V of every token tile as ever, but Q, the softmax, P.V and the out-projection
// for the one query tile that holds token T-1 (the last tile: T > 16 (NT - 1)), and the store for that token alone.
// A tile's MFMA chains do not depend on the other tiles', so token T-1 comes out bit for bit as in the full form.
template <int NT, bool F16, bool LAST = false>
__global__ __launch_bounds__(256, NT <= 3 ? 2 : 1) void feat_rows_kernel(void* __restrict__ Xv,
                                                                         const void* __restrict__ packv, int S, int T,
                                                                         int M, float eps) {
  constexpr int Q0 = LAST ? NT - 1 : 0;  // first query tile
  typedef typename Op16<F16>::x8 X8;
  typedef std::conditional_t<F16, f16, float> XT;  // state element
  typedef typename Op16<F16>::t WT;
  const WT* __restrict__ pack = (const WT*)packv;
  constexpr int NPARK = FR_NPARK<NT, LAST>;
  // The weight images move through a ring of 13-KB slots, item i (image group i; the out-projection's groups again
  // for a second pass of the short ring) in slot i % NSLOT.  Six slots hold two heads' Q | K | V, or the whole
  // out-projection image: one barrier per head, as two 39-KB buffers.  The form that parks fragments has room for
  // three slots only and hands them on twice per head and once per out-projection group (below).
  constexpr int NSLOT = NPARK ? 3 : 6;
  __shared__ __attribute__((aligned(1024))) WT wbuf[NSLOT * FR_GRP + 4 * NPARK * FR_FRAG];  // ring | parking
  // (wave in an SGPR: the LDS-DMA piece addresses below are then a scalar base + the lane's 16-B offset, the
  // saddr form, instead of one 64-bit VGPR address per piece -- ~19 VGPRs at the peak)
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n = lane & 15, g = lane >> 4;
  const int row = blockIdx.x * 4 + wave;  // row over the batch: member row / S, table row row % S
  const bool rowok = row < M * S;  // wave-uniform; a wave past the last row recomputes it and stores nothing
  const int rc = rowok ? row : M * S - 1;
  const int mem = rc / S, sr = rc - mem * S;
  const int64_t SE = (int64_t)S * FR_E;
  XT* __restrict__ X = (XT*)Xv + (int64_t)mem * T * SE;

  // LDS-DMA of image group grp (13 KB of the pack) into its ring slot, KB piece p by wave p % 4
  // (non-dependent pointer types: a builtin call on a template-dependent type is checked at instantiation,
  // where the host pass cannot resolve it, and the kernel's host stub is then silently dropped)
  const uint32_t dvoff = lane * 16;
  auto lds_u32 = [](const void* p) { return (unsigned)(uintptr_t)(lds_void*)p; };
  auto dma_piece = [&](int item, int p) {
    const int grp = item < FR_QKV_GRPS + 6 ? item : item - 6;  // (the short ring's second pass over Wout)
    const char* src = (const char*)(pack + grp * FR_GRP);
    const unsigned dst = lds_u32(wbuf + (item % NSLOT) * FR_GRP);
    lds_dma16(dvoff, src + p * 1024, __builtin_amdgcn_readfirstlane(dst + p * 1024));
  };
  // three slots: a group's 13 pieces are three per wave (dma_part i = 0 .. 2, branch-free) and the 13th by wave 0
  // (dma_tail)
  auto dma_part = [&](int item, int i) { dma_piece(item, wave + 4 * i); };
  auto dma_tail = [&](int item) {
    if (wave == 0) dma_piece(item, FR_GPIECES - 1);
  };
  auto dma_grp = [&](int item) {
#pragma unroll
    for (int i = 0; i < 3; ++i) dma_part(item, i);
    dma_tail(item);
  };
  // Six slots: three consecutive items (a head's Q | K | V, a half of Wout) are one 39-KB image in three consecutive
  // slots and move as the double buffer moved them: 39 pieces, ten per wave (dma_img_part i = 0 .. 9, clamped to the
  // last piece so that the call is branch-free: a clamped piece rewrites the last piece's bytes with the same data)
  // (dma_img leaves the address arithmetic to dma_piece: with the two bases hoisted out of its loop by hand the fp16
  // four-tile form came out with its O^T array in scratch, 400 B per lane; tests/test_featrow_nospill_codegen.py)
  auto dma_img = [&](int item0) {
    for (int p = wave; p < 3 * FR_GPIECES; p += 4) dma_piece(item0, p);
  };
  auto dma_img_part = [&](int item0, int i) { dma_piece(item0, min(wave + 4 * i, 3 * FR_GPIECES - 1)); };
  // SPREAD: an item's dma_part issues go one per k-step into the projection phase that follows its barrier instead of
  // all at the barrier (an LDS-DMA's issue cost grows with the other issues of its phase, MI355X_MICROARCH.md; the
  // fp16 form: 102.8 against 106.7 us when measured, profiles/r04/ab_feat_rows_dma_spread.txt; the bf16 form, not
  // measured with it, issues at the barrier)
  constexpr bool SPREAD = F16;
  auto dma_start = [&](int item) {  // at the barrier: the whole item, or its tail with the parts to follow
    if constexpr (SPREAD) dma_tail(item);
    else dma_grp(item);
  };
  // The asm DMA issues are invisible to the compiler's waitcnt pass, so each barrier that publishes a group waits
  // for this wave's pieces itself (vmcnt counts them with the wave's other global accesses; loads return in order).
  // sync_all: everything this wave issued has landed.  sync_but_last: everything but the group issued last -- at
  // most 3 accesses stay outstanding, the youngest group's (wave 0, with four pieces, waits for one of them too; a
  // younger store or load only makes the wait longer).  Both also retire the wave's LDS reads of the slot that the
  // next DMA overwrites.  This is the counted-vmcnt idiom of LDS-DMA rings: an LDS-DMA is a load on the VM counter,
  // loads retire in issue order, so vmcnt(N) with N = the pieces of the groups left in flight means every older
  // group has landed; a reader may touch it only after a barrier that follows that wait.
  auto sync_all = []() {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  };
  auto sync_but_last = []() { asm volatile("s_waitcnt vmcnt(3) lgkmcnt(0)\n\ts_barrier" ::: "memory"); };

  if constexpr (NSLOT == 6) dma_img(0);  // head 0's Q | K | V
  else dma_grp(0), dma_grp(1), dma_grp(2);
  // row addresses: a wave-uniform row base and a 32-bit lane offset per token tile (the saddr form: one VGPR per
  // tile where a 64-bit address per tile, live to the final stores, cost spills); lane offset = token t, features 8 g
  const char* const xrow = (const char*)(X + (int64_t)sr * FR_E);
  uint32_t xoff[NT];
#pragma unroll
  for (int tt = 0; tt < NT; ++tt) {
    const int t = 16 * tt + n;
    xoff[tt] = (uint32_t)(((tt == NT - 1 && t >= T ? 0 : t) * SE + 8 * g) * sizeof(XT));
  }
  // ---- the row's tokens as bf16 fragments (padding tokens t >= T are zero)
  X8 xf[NT][FR_E / 32];
#pragma unroll
  for (int tt = 0; tt < NT; ++tt) {
    const int t = 16 * tt + n;
    const bool pad = tt == NT - 1 && t >= T;  // only the last tile holds padding (T > 16 (NT - 1))
#pragma unroll
    for (int ks = 0; ks < FR_E / 32; ++ks) {
      if constexpr (F16) {
        xf[tt][ks] = *(const f16x8*)(xrow + xoff[tt] + 64 * ks);
        if (pad) xf[tt][ks] = f16x8{};
      } else {
        const char* xr = xrow + xoff[tt] + 128 * ks;
        f32x4 lo = *(const f32x4*)xr, hi = *(const f32x4*)(xr + 16);
        if (pad) lo = hi = f32x4{0.f, 0.f, 0.f, 0.f};
        xf[tt][ks] = cat8<X8>(lo, hi);
      }
    }
  }
  sync_all();
  if constexpr (NSLOT == 6 && !SPREAD) dma_img(3);  // head 1's, in flight during head 0

  constexpr int NTQ = NT - Q0;  // query tiles
  // the wave's parking places (fragment s at + s FR_FRAG) and the fragments that stay in registers
  WT* const park = wbuf + 3 * FR_GRP + wave * (NPARK * FR_FRAG) + lane * 8;
  X8 of[FR_H][NTQ];  // O^T fragments of every head (K-step h of the out-projection), query tiles Q0 ..
#pragma unroll
  for (int h = 0; h < FR_H; ++h) {
    // Items 3 h + {0, 1, 2} are this head's Q, K, V rows, [32][FR_ST] each, read in that order; items 18 .. are
    // the out-projection image's groups.  Six slots: the end-of-head barrier publishes the next head's three items
    // and frees this head's slots for the items of the head after the next.  Three slots: two barriers per head
    // hand them on -- after the K phase slots 0 and 1 take the next head's Q and K (they land during the V phase
    // and the attention; the end-of-head barrier publishes them), after the head slot 2 takes the next head's V
    // (it lands during the next head's Q and K phases, whose barrier publishes it).
    // ---- Q^T, K^T (C^T tiles) of the row, K = 192 in 6 steps (V after, to bound live registers)
    const WT* wimg = wbuf + ((3 * h) % NSLOT) * FR_GRP;  // [96][FR_ST]: Q (permuted) | K (permuted) | V, a slot each
    X8 qf[NT], kf[NT];
    // Q then K, one set of 2 NT accumulators live at a time (both at once: 54 / 44 spills in the fp16 / bf16
    // forms vs 46 / 24, and 2.5 / 4.5 % slower, profiles/r04/ab_feat_rows_qk_split.txt)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      f32x4 qa[2][NT];
#pragma unroll
      for (int f = 0; f < 2; ++f)
#pragma unroll
        for (int tt = 0; tt < NT; ++tt) qa[f][tt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < FR_E / 32; ++ks) {
        X8 wqf[2];
#pragma unroll
        for (int f = 0; f < 2; ++f) wqf[f] = *(const X8*)(wimg + (32 * j + 16 * f + n) * FR_ST + 32 * ks + 8 * g);
#pragma unroll
        for (int tt = 0; tt < NT; ++tt) {
          if (j == 0 && tt < Q0) continue;  // (Q of the query tiles only)
#pragma unroll
          for (int f = 0; f < 2; ++f) qa[f][tt] = mfma16x(wqf[f], xf[tt][ks], qa[f][tt]);
        }
        if constexpr (SPREAD) {
          // six slots: the ten parts of the next head's image after the Q and K k-steps 0 .. 4 of each
          if (NSLOT == 6 && ks < 5) dma_img_part(3 * h + 3, j * 5 + ks);
          if (NSLOT == 3 && j == 0 && ks < 3 && h > 0) dma_part(3 * h + 2, ks);  // three: this head's V
        }
      }
#pragma unroll
      for (int tt = 0; tt < NT; ++tt) (j == 0 ? qf[tt] : kf[tt]) = cat8<X8>(qa[0][tt], qa[1][tt]);
      __builtin_amdgcn_sched_barrier(0);
    }
    if constexpr (NSLOT == 3) {
      sync_all();  // this head's V landed; slots 0 and 1 are free
      dma_start(3 * h + 3), dma_start(3 * h + 4);
    }
    __builtin_amdgcn_sched_barrier(0);  // phases in order: bounds the live registers (2 waves / SIMD)
    // ---- V (C tiles: lane = head dim, 4 consecutive tokens) -> V^T A fragments per key-tile pair
    constexpr int NKP = (NT + 1) / 2;  // key-tile pairs (K = 32 keys per P.V MFMA)
    X8 vfr[2][NKP];
    {
      f32x4 va[2][NT];
#pragma unroll
      for (int f = 0; f < 2; ++f)
#pragma unroll
        for (int tt = 0; tt < NT; ++tt) va[f][tt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < FR_E / 32; ++ks) {
        X8 wvf[2];
#pragma unroll
        for (int f = 0; f < 2; ++f) wvf[f] = *(const X8*)(wimg + (64 + 16 * f + n) * FR_ST + 32 * ks + 8 * g);
#pragma unroll
        for (int tt = 0; tt < NT; ++tt)
#pragma unroll
          for (int f = 0; f < 2; ++f) va[f][tt] = mfma16x(xf[tt][ks], wvf[f], va[f][tt]);
        if constexpr (SPREAD && NSLOT == 3) dma_part(3 * h + 3 + ks / 3, ks % 3);  // the next Q and K (Wout's 0, 1)
      }
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int kp = 0; kp < NKP; ++kp)
          vfr[mt][kp] = cat8<X8>(va[mt][2 * kp], 2 * kp + 1 < NT ? va[mt][2 * kp + 1] : f32x4{0.f, 0.f, 0.f, 0.f});
    }
    __builtin_amdgcn_sched_barrier(0);

    // ---- per query tile: S^T[key][query] = K Q^T (log2 units), softmax over keys, O^T = V^T P^T
#pragma unroll
    for (int qt = Q0; qt < NT; ++qt) {
      f32x4 st[NT];
#pragma unroll
      for (int kt = 0; kt < NT; ++kt) st[kt] = mfma16x(kf[kt], qf[qt], f32x4{0.f, 0.f, 0.f, 0.f});
#pragma unroll
      for (int i = 0; i < 4; ++i)  // only the last key tile holds padding keys (T > 16*(NT-1))
        if (16 * (NT - 1) + 4 * g + i >= T) st[NT - 1][i] = -INFINITY;
      float m = -INFINITY;
#pragma unroll
      for (int kt = 0; kt < NT; ++kt)
#pragma unroll
        for (int i = 0; i < 4; ++i) m = fmaxf(m, st[kt][i]);
      m = max_rows4(m);
      float sum = 0.f;
#pragma unroll
      for (int kt = 0; kt < NT; ++kt)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float e = __builtin_amdgcn_exp2f(st[kt][i] - m);
          st[kt][i] = e;
          sum += e;
        }
      const float inv = __builtin_amdgcn_rcpf(sum_rows4(sum));
      f32x4 oa[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
      for (int kp = 0; kp < NKP; ++kp) {
        const X8 pb = cat8<X8>(st[2 * kp], 2 * kp + 1 < NT ? st[2 * kp + 1] : f32x4{0.f, 0.f, 0.f, 0.f});
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) oa[mt] = mfma16x(vfr[mt][kp], pb, oa[mt]);
      }
      const int ps = fr_park<NT, LAST>(h, qt);
      if (ps >= 0) *(X8*)(park + ps * FR_FRAG) = cat8<X8>(oa[0], oa[1], inv);
      else of[h][qt - Q0] = cat8<X8>(oa[0], oa[1], inv);
      __builtin_amdgcn_sched_barrier(0);
    }
    sync_all();  // the next items landed (three slots: all but V's, which goes into slot 2 now)
    if constexpr (NSLOT == 3) {
      if (h + 1 < FR_H) dma_start(3 * h + 5);  // the next V: its parts ride in the next head's Q phase
      else dma_grp(3 * h + 5);                 // Wout's group 2
    } else {
      // the head after the next (head 4: Wout's first half), unless it rides in the next head's projections;
      // after head 5 Wout's second half, with nothing to ride in
      if (h + 1 == FR_H || !SPREAD) dma_img(3 * h + 6);
    }
  }
  if constexpr (NSLOT == 6) sync_all();  // the image's second half landed

  // ---- Y^T = Wout . O^T over K = 192 (K-step h = head h), then residual + LayerNorm per token (lane = token n,
  //      48 of its 192 features).  Two token tiles per pass share every Wout fragment read from LDS (one
  //      ds_read_b128 per two MFMAs; a tile's own chain runs over h = 0 .. 5 as ever).  The image [192][FR_ST] is
  //      read in its six 32-row groups (Y^T tiles 2 gr, 2 gr + 1).  Six slots hold all of it.  Through three slots it
  //      streams once per pass, item 18 + 6 pass + gr: the first three are under way (above); the barrier after an
  //      item's MFMAs publishes the next item and frees the slot for the item three on, so a group has two steps to
  //      land.  (A three-tile row so reads the image twice, 156 KB per block instead of 78 KB, out of L2.)
  //      The four-tile form (one wave per SIMD, accumulators in AGPRs) keeps one tile per pass, as it was.
  constexpr int TPP = NT == 4 ? 1 : 2;  // token tiles per pass
  constexpr int NPASS = (NTQ + TPP - 1) / TPP, NITEM = FR_QKV_GRPS + 6 * (NSLOT == 3 ? NPASS : 1);
#pragma unroll
  for (int pass = 0; pass < NPASS; ++pass) {
    const int t0 = Q0 + TPP * pass, nt = NT - t0 < TPP ? NT - t0 : TPP;  // the pass's tiles t0 .. t0 + nt - 1
    if constexpr (NPARK > 0) {  // the pass's parked fragments back into registers
#pragma unroll
      for (int h = 0; h < FR_H; ++h)
#pragma unroll
        for (int k = 0; k < nt; ++k) {
          const int ps = fr_park<NT, LAST>(h, t0 + k);
          if (ps >= 0) of[h][t0 + k - Q0] = *(const X8*)(park + ps * FR_FRAG);
        }
    }
    f32x4 y[TPP][FR_E / 16];
#pragma unroll
    for (int f = 0; f < FR_E / 16; ++f) {
      const int item = FR_QKV_GRPS + (NSLOT == 3 ? 6 * pass : 0) + f / 2;  // (image group f / 2, rows 16 (f % 2) ..)
      const int wrow = 32 * (item % NSLOT) + 16 * (f % 2);  // its first row in the ring (six slots: 16 f)
#pragma unroll
      for (int k = 0; k < nt; ++k) y[k][f] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int h = 0; h < FR_H; ++h) {
        const X8 w = *(const X8*)(wbuf + (wrow + n) * FR_ST + 32 * h + 8 * g);
#pragma unroll
        for (int k = 0; k < nt; ++k) y[k][f] = mfma16x(w, of[h][t0 + k - Q0], y[k][f]);
      }
      if (NSLOT == 3 && f % 2 == 1 && item + 1 < NITEM) {  // the group is read
        if (item + 2 < NITEM) sync_but_last();
        else sync_all();
        if (item + 3 < NITEM) dma_grp(item + 3);
      }
    }
    // (bf16 form: its residual loads stay behind the out-projection, which bounds the live registers)
    if constexpr (!F16) __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int k = 0; k < nt; ++k) {
      const int tt = t0 + k;
      const int t = 16 * tt + n;
      const bool pad = tt == NT - 1 && t >= T;
      const bool valid = rowok && !pad && (!LAST || t == T - 1);
      // fp32 state: the residual / output pieces are 4 features at 16 f + 4 g (the Y^T rows of the lane)
      char* const xr = (char*)xrow + xoff[tt] - 16 * g;
      float sm = 0.f;
      if constexpr (F16) {  // the residual is the lane's own X fragments (image rows permuted to match)
#pragma unroll
        for (int f = 0; f < FR_E / 16; ++f)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            y[k][f][i] += (float)xf[tt][f >> 1][4 * (f & 1) + i];
            sm += y[k][f][i];
          }
      } else {
#pragma unroll
        for (int f = 0; f < FR_E / 16; ++f) {
          const f32x4 xv = *(const f32x4*)(xr + 64 * f);
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            y[k][f][i] += xv[i];
            sm += y[k][f][i];
          }
        }
      }
      const float mean = sum_rows4(sm) * (1.0f / FR_E);
      float q = 0.f;
#pragma unroll
      for (int f = 0; f < FR_E / 16; ++f)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float dl = y[k][f][i] - mean;
          q += dl * dl;
        }
      const float rs = 1.0f / sqrtf(sum_rows4(q) * (1.0f / FR_E) + eps);
      if (valid) {
        if constexpr (F16) {  // features 32k + 8g .. +7 from tiles 2k, 2k+1: one 16-B store each
#pragma unroll
          for (int c = 0; c < FR_E / 32; ++c) {
            f16x8 ov;
#pragma unroll
            for (int i = 0; i < 4; ++i)
              ov[i] = (f16)((y[k][2 * c][i] - mean) * rs), ov[4 + i] = (f16)((y[k][2 * c + 1][i] - mean) * rs);
            *(f16x8*)(xrow + xoff[tt] + 64 * c) = ov;
          }
        } else {
#pragma unroll
          for (int f = 0; f < FR_E / 16; ++f) {
            f32x4 ov;
#pragma unroll
            for (int i = 0; i < 4; ++i) ov[i] = (y[k][f][i] - mean) * rs;
            *(f32x4*)(xr + 64 * f) = ov;
          }
        }
      }
    }
  }
}

template <bool F16, bool LAST>
hipError_t launch_fr(void* X, const void* pk, int S, int T, int M, float eps, hipStream_t st) {
  const dim3 grid((M * S + 3) / 4), block(256);
  if (T <= 16) hipLaunchKernelGGL((feat_rows_kernel<1, F16, LAST>), grid, block, 0, st, X, pk, S, T, M, eps);
  else if (T <= 32) hipLaunchKernelGGL((feat_rows_kernel<2, F16, LAST>), grid, block, 0, st, X, pk, S, T, M, eps);
  else if (T <= 48) hipLaunchKernelGGL((feat_rows_kernel<3, F16, LAST>), grid, block, 0, st, X, pk, S, T, M, eps);
  else hipLaunchKernelGGL((feat_rows_kernel<4, F16, LAST>), grid, block, 0, st, X, pk, S, T, M, eps);
  return hipGetLastError();
}
}  // namespace

hipError_t launch_feat_rows(void* X, const void* pack, int S, int T, int M, int E, int H, float eps, hipStream_t st,
                            DType x_t, bool last) {
  if (S <= 0 || M <= 0) return hipSuccess;
  if (E != FR_E || H != FR_H || T < 1 || T > 64 || x_t == DType::BF16) return hipErrorInvalidValue;
  if (last)
    return x_t == DType::F16 ? launch_fr<true, true>(X, pack, S, T, M, eps, st)
                             : launch_fr<false, true>(X, pack, S, T, M, eps, st);
  return x_t == DType::F16 ? launch_fr<true, false>(X, pack, S, T, M, eps, st)
                           : launch_fr<false, false>(X, pack, S, T, M, eps, st);
}

}  // namespace mmpfn
