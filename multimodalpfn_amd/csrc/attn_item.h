// The seam between attention.hip (launch_attn_layer builds the task map; attn_item3_kernel, the parity mode's item
// attention) and attention_pipe.hip (attn_pipe_kernel, the 16-bit modes'), and nothing else's: the operands and
// task map (as data) of the sample-axis attention kernels, the query map on it, and the kernels' exact backstop.
// There is no block -> (b, g, chunk) helper here: that scan of tstart stays written out in both kernels, and the
// query map in attn_item3_kernel too, because the shared forms changed those kernels' register allocation (see the
// notes at the copies; profiles/r09).
#pragma once
#include "common.h"
#include "kernels.h"

namespace mmpfn {

// task map + operands, by value.  The queries that read KV sequence (column b, kv head g) are the own-head rows
// [a0, a0+na) of head g, then, for g == kvb, rows [b0, b0+nb) of all H heads, cut into tasks of ATTN_ITEM_QPB
struct Attn2Args {
  const __bf16* q;  // [B][H][S][32]
  const __bf16* k;  // [B][H][Npad][32]
  const __bf16* vt; // [B][H][32][Npad]
  __bf16* o;        // row b*S + s, element row*H*32 + h*32 + d
  int S, H, Npad, nk;
  int a0, na;          // own-head query rows
  int b0, nb, kvb;     // shared-KV query rows (all heads) against kv head kvb
  int tasks_per_b, nblocks;
  int tstart[9];       // task prefix per kv head inside one column
  int64_t kv_bstride;  // elements between the K (V^T) blocks of consecutive columns: H*Npad*32, or
                       // Npad*32 for a head-0-only train-KV cache
  int q_prescaled;     // Q already carries log2(e)/sqrt(32) (folded into the engine's bf16 Q weights)
  const unsigned char* vt8;  // f8 != 0: V^T in e4m3, the layout of vt
  int f8;              // P.V on fp8 MFMA: 0 off (bf16), 1 P in e4m3, 2 P in e5m2 (attention_pipe.hip)
  int qk_f16;          // q, k and o hold fp16 (S on f16 MFMA; the fp16 tap); vt stays bf16
  int o_f16;           // PREC_F16's forward: q, k bf16, o fp16 (every MFMA a bf16 one)
};
hipError_t launch_attn_pipe(const Attn2Args& a, hipStream_t st);

// queries of (b, g)
__device__ __forceinline__ int item_count(const Attn2Args& p, int g) { return p.na + (g == p.kvb ? p.H * p.nb : 0); }

// query j of the cnt = item_count(p, g) of kv head g -> its head and table row; j >= cnt: the last query's, !ok
struct ItemQuery {
  int h, s;
  bool ok;
};
__device__ __forceinline__ ItemQuery item_query(const Attn2Args& p, int g, int cnt, int j) {
  const int jc = min(j, cnt - 1);
  ItemQuery q;
  q.ok = j < cnt;
  if (jc < p.na) {
    q.h = g, q.s = p.a0 + jc;
  } else {
    const int jj = jc - p.na;
    q.h = jj / p.nb, q.s = p.b0 + jj % p.nb;
  }
  return q;
}

// exact two-pass softmax for one query per lane, K / V^T straight from global memory: the backstop of a row sum
// that overflowed both the reference-free pass and the re-run (out of line: it is never on the hot path)
template <typename QT, typename VT, typename OT>
static __device__ __attribute__((noinline)) void exact_rows(const Attn2Args& p, const QT* Kg, const VT* Vg,
                                                            const QT* qrow, OT* orow, bool valid, float c) {
  float q[32], o[32];
#pragma unroll
  for (int d = 0; d < 32; ++d) q[d] = (float)qrow[d] * c, o[d] = 0.f;
  float m = -INFINITY;
  for (int k = 0; k < p.nk; ++k) {
    float s = 0.f;
#pragma unroll
    for (int d = 0; d < 32; ++d) s = fmaf(q[d], (float)Kg[(int64_t)k * 32 + d], s);
    m = fmaxf(m, s);
  }
  float l = 0.f;
  for (int k = 0; k < p.nk; ++k) {
    float s = 0.f;
#pragma unroll
    for (int d = 0; d < 32; ++d) s = fmaf(q[d], (float)Kg[(int64_t)k * 32 + d], s);
    const float e = exp2f(s - m);
    l += e;
#pragma unroll
    for (int d = 0; d < 32; ++d) o[d] = fmaf(e, (float)Vg[(int64_t)d * p.Npad + k], o[d]);
  }
  if (valid) {
    const float inv = 1.0f / l;
#pragma unroll
    for (int d = 0; d < 32; ++d) orow[d] = (OT)(o[d] * inv);
  }
}

}  // namespace mmpfn
