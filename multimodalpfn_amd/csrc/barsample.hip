// Draws from bar distributions (FullSupportBarDistribution.sample, bar_distribution.py:577-585, with the icdf of
// :256-283): n draws per row of any logits [Q][B], each one level, one binary search in the row's cumulative sums and
// one interpolation.  The row is finished by barhead.h's front end, as the scores' kernel has it; the levels are the
// caller's or come from Philox4x32-10 keyed by the seed and counted by (row, draw).  Always fp32.
#include "barhead.h"

namespace mmpfn {
namespace {

// Philox4x32-10 (Salmon et al., SC'11; Random123's philox4x32_R(10, ...)): the four output words of a counter and key.
struct Philox4 {
  uint32_t w[4];
};
__device__ __forceinline__ Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                                 uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    if (r > 0) k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
  }
  return Philox4{{c0, c1, c2, c3}};
}

constexpr float kBarLevelMin = 0x1p-24f, kBarLevelMax = 1.0f - 0x1p-24f;  // the levels' range: never 0 or 1

// The level of draw J of row q: word J & 3 of the Philox block (counter (J >> 2, q, 0), key the seed), its top 23
// bits as the odd multiple (2 m + 1) 2^-24 -- exact in float32, inside [kBarLevelMin, kBarLevelMax].
__device__ __forceinline__ float bar_draw_level(uint64_t seed, int q, uint64_t J) {
  const uint64_t blk = J >> 2;
  const Philox4 r = philox4x32_10((uint32_t)blk, (uint32_t)(blk >> 32), (uint32_t)q, 0u, (uint32_t)seed,
                                  (uint32_t)(seed >> 32));
  const int w = (int)(J & 3);
  const uint32_t x = w == 0 ? r.w[0] : w == 1 ? r.w[1] : w == 2 ? r.w[2] : r.w[3];
  return (float)(2u * (x >> 9) + 1u) * 0x1p-24f;
}

// The position at level u in (0, 1) of a finished row (p_s, c_s as bar_finish_row leaves them): the icdf of
// bar_head_kernel's last stage (bar_distribution.py:256-283) with the level kept at or below the row's rounded total --
// so the bar found is the first whose inclusive sum reaches it, never a trailing bar of weight zero -- and the share
// of the bar kept in [0, 1], so a draw cannot leave its bucket by rounding.  HALFNORMAL: in the two end buckets the
// share is a level of the half-normal that forward / pi / ei put there (scales ends[kEndS0], ends[kEndSL]).
// Contraction is pinned: a draw is one sequence of roundings wherever it is computed.
__device__ __forceinline__ float bar_draw_at(const float* p_s, const float* c_s, const float* borders,
                                             const float* ends, int B, bool halfnormal, float u) {
#pragma clang fp contract(off)
  const float lv = fminf(u, c_s[B - 1]);
  int lo = 0, hi = B;  // lower bound of lv in c_s[0 .. B)
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (c_s[mid] < lv) lo = mid + 1;
    else hi = mid;
  }
  const int j = lo < B - 1 ? lo : B - 1;
  const float rest = lv - (j > 0 ? c_s[j - 1] : 0.0f);
  const float share = fminf(fmaxf(rest / p_s[j], 0.0f), 1.0f);
  if (halfnormal && j == B - 1)
    return borders[B - 1] + ends[kEndSL] * 1.4142135624f * erfinvf(fminf(share, kBarLevelMax));
  if (halfnormal && j == 0)
    return borders[1] - ends[kEndS0] * 1.4142135624f * erfinvf(fminf(1.0f - share, kBarLevelMax));
  const float left = borders[j], right = borders[j + 1];
  return left + (right - left) * share;
}

// n draws from each row's distribution: block (q, chunk) finishes row q as bar_score_kernel does and serves draws
// [chunk * kBarSampleChunk, ...) of it, thread t the draws t, t + 256, ... of the chunk.  A draw depends on its
// level alone, and a generated level on (seed, q, first_draw + j) alone: not on n, the chunking or the launch.
// A NaN level gives a NaN draw; a row whose total is not a positive number gives NaN draws throughout.
template <int NV>
__global__ __launch_bounds__(kBarThreads) void bar_sample_kernel(const BarSampleArgs a) {
  extern __shared__ __attribute__((aligned(16))) float bar_lds[];
  __shared__ float red[4];
  const int B = a.B, q = blockIdx.x;
  const int ldp = (B + 3) & ~3;
  float* const p_s = bar_lds;
  float* const c_s = bar_lds + ldp;
  const float total = bar_finish_row<NV>(a.logits + (int64_t)q * B, B, a.inv_temp, p_s, c_s, red);
  const bool dead = !(total > 0.0f);  // NaN included
  const int64_t j0 = (int64_t)blockIdx.y * kBarSampleChunk;
  const int64_t j1 = j0 + kBarSampleChunk < a.n ? j0 + kBarSampleChunk : a.n;
  const float nanv = __builtin_nanf("");
  for (int64_t j = j0 + threadIdx.x; j < j1; j += kBarThreads) {
    const int64_t o = (int64_t)q * a.n + j;
    float u = a.uniforms ? a.uniforms[o] : bar_draw_level(a.seed, q, a.first_draw + (uint64_t)j);
    const bool isnan_u = u != u;
    u = isnan_u ? nanv : fminf(fmaxf(u, kBarLevelMin), kBarLevelMax);
    if (a.u_out) a.u_out[o] = u;
    const float y = bar_draw_at(p_s, c_s, a.borders, a.ends, B, a.tails != 0, isnan_u ? 0.5f : u);
    a.out[o] = dead || isnan_u ? nanv : y;
  }
}

template <int NV>
hipError_t bar_sample_launch(const BarSampleArgs& a, int Q, hipStream_t st) {
  const size_t lds = (size_t)2 * ((a.B + 3) & ~3) * sizeof(float);
  static std::atomic<uint64_t> opted{0};
  const hipError_t e = bar_lds_optin(opted, bar_sample_kernel<NV>, lds);
  if (e != hipSuccess) return e;
  const unsigned chunks = (unsigned)((a.n + kBarSampleChunk - 1) / kBarSampleChunk);
  hipLaunchKernelGGL(bar_sample_kernel<NV>, dim3(Q, chunks), dim3(kBarThreads), lds, st, a);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_bar_sample(const BarSampleArgs& a, int Q, hipStream_t st) {
  if (Q <= 0 || a.n == 0) return hipSuccess;
  if (a.B < 2 || a.B > kBarHeadMaxBars || a.n < 0 || a.n > kBarSampleMaxDraws || !a.logits || !a.borders || !a.out ||
      (a.tails != 0 && a.tails != 1) || (a.tails == 1 && !a.ends) || !(a.inv_temp > 0.f))
    return hipErrorInvalidValue;
  if (a.B <= 1024) return bar_sample_launch<1>(a, Q, st);
  if (a.B <= 2048) return bar_sample_launch<2>(a, Q, st);
  if (a.B <= 5120) return bar_sample_launch<5>(a, Q, st);
  return bar_sample_launch<8>(a, Q, st);
}

}  // namespace mmpfn
