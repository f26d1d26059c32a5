// Bar-distribution head of the regression ensemble (regressor.py:691-706 with utils.py:659-700, then the
// renormalised criterion's mean / mode / icdf, bar_distribution.py:239-332,588-597): M members' logits over B bars
// -> one predictive distribution per test row and its point estimates, in one pass over the logits.  Always fp32.
// Scoring of a finished row (bar_score_row: the negative log density, CDF, probability of improvement and expected
// improvement at up to kBarScoreMaxTargets targets per row, and the mean of squares; bar_distribution.py:59-97,
// 487-571,600-675,706-758) runs from the head itself (bar_head_kernel<NV, true>) or over any logits [Q][B]
// (bar_score_kernel).  The pieces shared with the draws' kernel (barsample.hip) are in barhead.h.
#include "barhead.h"

namespace mmpfn {
namespace {

// Half-normal pieces of the two end buckets (bar_distribution.py:677-703): EI of a half-normal of scale s over an
// incumbent at u * s (u <= 0 is minus the position in the tail), 2 s (phi(u) + u Phi(u)).
__device__ __forceinline__ float bar_halfnormal_ei(float s, float u) {
  const float phi = expf(-0.5f * (u * u)) * 0.3989422804f;
  const float Phi = 0.5f * erfcf(-u * 0.7071067812f);
  return (2.0f * s) * (phi + u * Phi);
}

// Scores of a finished row: p_s [ldp] holds the row's probabilities (zero beyond B) and c_s their inclusive
// cumulative sums, as bar_head_kernel's last stage leaves them, both visible to every thread (a barrier lies between
// their stores and this call).  m_s [ldp] is scratch for the one extra scan the expected improvement needs.
// Per row O(B): the mean of squares and the scan of p_b * (mid_b - centre) over the interior buckets (the centre is
// one of the borders, so borders far from zero cost nothing: every term is as small as the borders' span).  Per
// target O(log B): thread j < J finds the bucket of ys[j] as searchsorted(borders, y) - 1 does (left side, clamped:
// the first border >= y; equal borders of a zero-width bucket are fine) and reads what it needs at that bucket.
// The two end buckets carry the half-normal tails in nll / pi / ei and the piecewise-linear form in cdf, as the
// reference has them.  A NaN target scores nll 0 and cdf / pi / ei NaN.  Every output pointer may be null.
// Contraction is pinned: both callers must round alike.
template <int NV>
__device__ __forceinline__ void bar_score_row(const float* p_s, const float* c_s, float* m_s, float* red,
                                              const BarScoreArgs& s, int B, int q) {
#pragma clang fp contract(off)
  const bool want_ei = s.ei != nullptr && s.J > 0;
  if (want_ei || s.mean_of_square) {  // block-uniform
    float g[NV][4], x[NV][4];
    float sq = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int j0 = bar_index<NV>(i);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int b = j0 + k;
        const float p = b < B ? p_s[b] : 0.f;
        g[i][k] = b < B && want_ei ? p * s.ei_mids[b] : 0.f;
        if (b < B && s.mean_of_square) sq += p * s.mean_squares[b];
      }
    }
    if (want_ei) {
      bar_block_scan<NV>(g, x, red);
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const int j0 = bar_index<NV>(i);
        if (j0 < B)
          *reinterpret_cast<f32x4*>(m_s + j0) =
              f32x4{x[i][0] + g[i][0], x[i][1] + g[i][1], x[i][2] + g[i][2], x[i][3] + g[i][3]};
      }
    }
    if (s.mean_of_square) {
      sq = bar_block_sum(sq, red);
      if (threadIdx.x == 0) s.mean_of_square[q] = sq;
    }
    __syncthreads();  // m_s before the targets read it
  }
  const int j = threadIdx.x;
  if (j >= s.J) return;
  const float y = s.ys[(int64_t)q * s.J + j];
  const bool isnan_y = y != y;
  int lo = 0, hi = B + 1;  // lower bound of y in borders[0 .. B]
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (s.borders[mid] < y) lo = mid + 1;
    else hi = mid;
  }
  const int b = lo - 1 < 0 ? 0 : lo - 1 > B - 1 ? B - 1 : lo - 1;
  const float L = s.borders[b], R = s.borders[b + 1], w = s.widths[b], p = p_s[b];
  const float p0 = p_s[0], pl = p_s[B - 1];
  const float b1 = s.borders[1], bl = s.borders[B - 1];
  const float nanv = __builtin_nanf("");
  const int64_t o = (int64_t)q * s.J + j;
  if (s.nll) {
    float lp = logf(p) - s.log_widths[b];
    if (b == 0) {
      const float t = fmaxf(b1 - y, 1e-8f);
      lp += s.ends[kEndK0] - (t * t) * s.ends[kEndInv2Var0];
    }
    if (b == B - 1) {
      const float t = fmaxf(y - bl, 1e-8f);
      lp += s.ends[kEndKL] - (t * t) * s.ends[kEndInv2VarL];
    }
    s.nll[o] = isnan_y ? 0.f : -lp;
  }
  const float share = fminf(fmaxf((y - L) / w, 0.0f), 1.0f);
  if (s.cdf) {
    float cd = (b > 0 ? c_s[b - 1] : 0.f) + p * share;
    if (y <= s.borders[0]) cd = 0.f;
    if (y >= s.borders[B]) cd = 1.f;
    s.cdf[o] = isnan_y ? nanv : fminf(fmaxf(cd, 0.0f), 1.0f);
  }
  // the interior buckets (1 .. B - 2) wholly right of the target, and its own bucket when that is an interior one
  const bool inner = b >= 1 && b <= B - 2;
  const float pint = b <= B - 2 ? c_s[B - 2] - c_s[b] : 0.f;
  const float pos0 = fmaxf(b1 - y, 0.f), posl = fmaxf(y - bl, 0.f);  // positions in the two half-normals
  if (s.pi) {
    const float f0 = pos0 > 0.f ? erff(pos0 * s.ends[kEndInvS0] * 0.7071067812f) : 0.f;
    const float fl = posl > 0.f ? erfcf(posl * s.ends[kEndInvSL] * 0.7071067812f) : 1.f;
    const float v = (p0 * f0 + pl * fl) + (pint + (inner ? p * (1.0f - share) : 0.f));
    s.pi[o] = isnan_y ? nanv : v;
  }
  if (s.ei) {
    const float gint = b <= B - 2 ? m_s[B - 1] - m_s[b] : 0.f;
    const float d = R - y;
    const float part = inner ? p * ((d * d) / (2.0f * w)) : 0.f;
    const float s0 = s.ends[kEndS0], sl = s.ends[kEndSL];
    const float e0 = bar_halfnormal_ei(s0, 0.f) - bar_halfnormal_ei(s0, -pos0 * s.ends[kEndInvS0]);
    const float el = bar_halfnormal_ei(sl, -posl * s.ends[kEndInvSL]);
    const float v = (p0 * e0 + pl * el) + ((gint - (y - s.ends[kEndCentre]) * pint) + part);
    s.ei[o] = isnan_y ? nanv : v;
  }
}

struct BarHeadArgs {
  const float* logits;          // [M][Q][B]
  const unsigned char* cancel;  // [M][ldc] or null
  const int* idx;               // [M][ldt]: source bucket, -1: CDF forced to 0, -2: forced to 1
  const float* share;           // [M][ldt]
  const float* borders;         // [B + 1] renormalised criterion
  const float* means;           // [B] bucket means with the half-normal ends
  const float* mode_means;      // [B] plain bucket means
  const float* widths;          // [B]
  const float* levels;          // [K]
  float* out_logits;            // [Q][B] or null
  float* mean;                  // [Q]
  float* mode;                  // [Q]
  float* quantiles;             // [K][Q]
  int M, Q, B, K;
  float inv_temp;
  int avg_before;
  int ldt, ldc;      // row strides of the tables (>= B + 1) and of the cancel mask (>= B)
  int tvec, cvec;    // the strides and bases allow 16-byte table loads / 4-byte mask loads (padded rows)
};

// SCORE: the scores of the finished row as well (bar_score_row, one more LDS array); without it `s` is not read.
template <int NV, bool SCORE>
__global__ __launch_bounds__(kBarThreads) void bar_head_kernel(const BarHeadArgs a, const BarScoreArgs s) {
  extern __shared__ __attribute__((aligned(16))) float bar_lds[];
  __shared__ float red[4];
  __shared__ int red_i[4];
  const int B = a.B, q = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ldp = (B + 3) & ~3;
  float* const p_s = bar_lds;        // [ldp] a member's bucket probabilities, then the final ones
  float* const c_s = bar_lds + ldp;  // [ldp] their exclusive prefix sums, then the final inclusive ones

  float acc[NV][4];
#pragma unroll
  for (int i = 0; i < NV; ++i)
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[i][k] = 0.f;

  // a member's row as its softmax reads it, before the temperature: cancelled bars and the padding beyond B at -inf
  auto load_row = [&](int m, float (&v)[NV][4]) {
    const float* row = a.logits + ((int64_t)m * a.Q + q) * B;
    const unsigned char* cm = a.cancel ? a.cancel + (int64_t)m * a.ldc : nullptr;
    const bool vec = (reinterpret_cast<uintptr_t>(row) & 15) == 0;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int j0 = bar_index<NV>(i);
      if (vec && j0 + 3 < B) {
        const f32x4 r = *reinterpret_cast<const f32x4*>(row + j0);
#pragma unroll
        for (int k = 0; k < 4; ++k) v[i][k] = r[k];
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[i][k] = j0 + k < B ? row[j0 + k] : -INFINITY;
      }
      if (cm && j0 < B) {
        if (a.cvec) {  // the group's four mask bytes in one load (a padded row: ldc >= B rounded up to 4)
          const uint32_t w = *reinterpret_cast<const uint32_t*>(cm + j0);
#pragma unroll
          for (int k = 0; k < 4; ++k)
            if (j0 + k < B && ((w >> (8 * k)) & 0xffu)) v[i][k] = -INFINITY;
        } else {
#pragma unroll
          for (int k = 0; k < 4; ++k)
            if (j0 + k < B && cm[j0 + k]) v[i][k] = -INFINITY;
        }
      }
    }
  };

  // The members one after the other.  What a member reads from global memory is asked for a phase ahead of its
  // use -- the next member's row while this one's softmax runs, this member's border tables before its softmax --
  // since a block's phases are serial and only two or three blocks share a CU.
  float nxt[NV][4];
  load_row(0, nxt);
  for (int m = 0; m < a.M; ++m) {
    float e[NV][4], c[NV][4];
    float mx = -INFINITY;
#pragma unroll
    for (int i = 0; i < NV; ++i)
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        e[i][k] = nxt[i][k] * a.inv_temp;  // (-inf stays -inf: inv_temp > 0)
        mx = fmaxf(mx, e[i][k]);
      }
    if (m + 1 < a.M) load_row(m + 1, nxt);
    const int* ix = a.idx + (int64_t)m * a.ldt;
    const float* sh = a.share + (int64_t)m * a.ldt;
    int tix[NV][4];  // the tables at the thread's own borders; beyond the last border the CDF is 1
    float tsh[NV][4];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int j0 = bar_index<NV>(i);
      if (a.tvec && j0 <= B) {  // 16-byte pieces of a padded row (ldt >= B + 1 rounded up to 4)
        typedef __attribute__((ext_vector_type(4))) int i32x4;
        const i32x4 t = *reinterpret_cast<const i32x4*>(ix + j0);
        const f32x4 u = *reinterpret_cast<const f32x4*>(sh + j0);
#pragma unroll
        for (int k = 0; k < 4; ++k) tix[i][k] = j0 + k <= B ? t[k] : -2, tsh[i][k] = j0 + k <= B ? u[k] : 0.f;
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int j = j0 + k;
          tix[i][k] = j <= B ? ix[j] : -2;
          tsh[i][k] = j <= B ? sh[j] : 0.f;
        }
      }
    }
    mx = bar_block_max(mx, red);
#pragma unroll
    for (int i = 0; i < NV; ++i)
#pragma unroll
      for (int k = 0; k < 4; ++k) e[i][k] = expf(e[i][k] - mx);
    const float inv = 1.0f / bar_block_scan<NV>(e, c, red);
    // the previous member's gather is done with p_s / c_s: bar_block_scan's barriers lie in between
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int j0 = bar_index<NV>(i);
      if (j0 < B) {
        *reinterpret_cast<f32x4*>(p_s + j0) = f32x4{e[i][0], e[i][1], e[i][2], e[i][3]} * inv;
        *reinterpret_cast<f32x4*>(c_s + j0) = f32x4{c[i][0], c[i][1], c[i][2], c[i][3]} * inv;
      }
    }
    __syncthreads();
    // CDF of the member's distribution at a target border (utils.py:659-677,696-698) from its table entries
    auto cdf_of = [&](int s, float share) -> float {
      if (s < 0) return s == -1 ? 0.0f : 1.0f;
      s = s < B ? s : B - 1;  // a table entry beyond the bars must not index past the row
      return fminf(fmaxf(c_s[s] + p_s[s] * share, 0.0f), 1.0f);
    };
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int j0 = bar_index<NV>(i);
      float cd[5];
#pragma unroll
      for (int k = 0; k < 4; ++k) cd[k] = cdf_of(tix[i][k], tsh[i][k]);
      cd[4] = __shfl_down(cd[0], 1, 64);
      if (lane == 63) cd[4] = j0 + 4 <= B ? cdf_of(ix[j0 + 4], sh[j0 + 4]) : 1.0f;  // the next group's first border
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float bar = fmaxf(cd[k + 1] - cd[k], 0.0f);
        acc[i][k] += a.avg_before ? logf(bar) : bar;
      }
    }
  }

  // ensemble mean (regressor.py:699-703), then log and the criterion's own softmax (:706, bar_distribution.py:241)
  const float invM = 1.0f / (float)a.M;
  float e[NV][4], c[NV][4];
  if (a.avg_before) {
    float mx = -INFINITY;
#pragma unroll
    for (int i = 0; i < NV; ++i)
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        acc[i][k] = bar_index<NV>(i) + k < B ? acc[i][k] * invM : -INFINITY;
        mx = fmaxf(mx, acc[i][k]);
      }
    mx = bar_block_max(mx, red);
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i)
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        acc[i][k] = expf(acc[i][k] - mx);
        s += acc[i][k];
      }
    const float inv = 1.0f / bar_block_sum(s, red);
#pragma unroll
    for (int i = 0; i < NV; ++i)
#pragma unroll
      for (int k = 0; k < 4; ++k) acc[i][k] *= inv;
  } else {
#pragma unroll
    for (int i = 0; i < NV; ++i)
#pragma unroll
      for (int k = 0; k < 4; ++k) acc[i][k] = bar_index<NV>(i) + k < B ? acc[i][k] * invM : 0.f;
  }
  float mx = -INFINITY;
#pragma unroll
  for (int i = 0; i < NV; ++i)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      acc[i][k] = logf(acc[i][k]);  // the final log-probabilities; -inf beyond B
      mx = fmaxf(mx, acc[i][k]);
    }
  if (a.out_logits) {
    float* out = a.out_logits + (int64_t)q * B;
    const bool vec = (reinterpret_cast<uintptr_t>(out) & 15) == 0;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int j0 = bar_index<NV>(i);
      if (vec && j0 + 3 < B) {
        *reinterpret_cast<f32x4*>(out + j0) = f32x4{acc[i][0], acc[i][1], acc[i][2], acc[i][3]};
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (j0 + k < B) out[j0 + k] = acc[i][k];
      }
    }
  }
  mx = bar_block_max(mx, red);
#pragma unroll
  for (int i = 0; i < NV; ++i)
#pragma unroll
    for (int k = 0; k < 4; ++k) e[i][k] = expf(acc[i][k] - mx);
  const float inv = 1.0f / bar_block_scan<NV>(e, c, red);

  // mean, mode (first bucket of the largest density), and p / inclusive cumulative sums for the quantiles
  float msum = 0.f, best = -INFINITY;
  int best_j = 0x7fffffff;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int j0 = bar_index<NV>(i);
    float pk[4], ck[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      pk[k] = e[i][k] * inv;
      ck[k] = (c[i][k] + e[i][k]) * inv;
      if (j0 + k < B) {
        msum += pk[k] * a.means[j0 + k];
        const float dens = pk[k] / a.widths[j0 + k];
        if (dens > best) best = dens, best_j = j0 + k;  // ascending j within a thread: the first maximum stays
      }
    }
    if (j0 < B) {
      *reinterpret_cast<f32x4*>(p_s + j0) = f32x4{pk[0], pk[1], pk[2], pk[3]};
      *reinterpret_cast<f32x4*>(c_s + j0) = f32x4{ck[0], ck[1], ck[2], ck[3]};
    }
  }
  msum = bar_block_sum(msum, red);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ob = __shfl_xor(best, o, 64);
    const int oj = __shfl_xor(best_j, o, 64);
    if (ob > best || (ob == best && oj < best_j)) best = ob, best_j = oj;
  }
  __syncthreads();
  if (lane == 0) red[wave] = best, red_i[wave] = best_j;
  __syncthreads();  // also orders the p_s / c_s stores before the quantile search
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; ++w)
      if (red[w] > best || (red[w] == best && red_i[w] < best_j)) best = red[w], best_j = red_i[w];
    a.mean[q] = msum;
    a.mode[q] = a.mode_means[best_j < B ? best_j : 0];
  }
  // icdf (bar_distribution.py:256-283): first bucket whose inclusive cumulative sum reaches the level
  for (int k = threadIdx.x; k < a.K; k += kBarThreads) {
    const float lv = a.levels[k];
    int lo = 0, hi = B;  // lower bound of lv in c_s[0 .. B)
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (c_s[mid] < lv) lo = mid + 1;
      else hi = mid;
    }
    const int j = lo < B - 1 ? lo : B - 1;
    const float rest = lv - (j > 0 ? c_s[j - 1] : 0.0f);
    const float left = a.borders[j], right = a.borders[j + 1];
    a.quantiles[(int64_t)k * a.Q + q] = left + (right - left) * rest / p_s[j];
  }
  if constexpr (SCORE) bar_score_row<NV>(p_s, c_s, bar_lds + 2 * ldp, red, s, B, q);
}

// Scores of any logits [Q][B]: bar_finish_row, then bar_score_row.
template <int NV>
__global__ __launch_bounds__(kBarThreads) void bar_score_kernel(const float* logits, int B, float inv_temp,
                                                                const BarScoreArgs s) {
  extern __shared__ __attribute__((aligned(16))) float bar_lds[];
  __shared__ float red[4];
  const int q = blockIdx.x;
  const int ldp = (B + 3) & ~3;
  float* const p_s = bar_lds;
  float* const c_s = bar_lds + ldp;
  bar_finish_row<NV>(logits + (int64_t)q * B, B, inv_temp, p_s, c_s, red);
  bar_score_row<NV>(p_s, c_s, bar_lds + 2 * ldp, red, s, B, q);
}

template <int NV, bool SCORE>
hipError_t bar_head_launch(const BarHeadArgs& a, const BarScoreArgs& s, hipStream_t st) {
  const size_t lds = (size_t)(SCORE ? 3 : 2) * ((a.B + 3) & ~3) * sizeof(float);
  static std::atomic<uint64_t> opted{0};
  const hipError_t e = bar_lds_optin(opted, bar_head_kernel<NV, SCORE>, lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((bar_head_kernel<NV, SCORE>), dim3(a.Q), dim3(kBarThreads), lds, st, a, s);
  return hipGetLastError();
}

template <int NV>
hipError_t bar_score_launch(const float* logits, int Q, int B, float inv_temp, const BarScoreArgs& s, hipStream_t st) {
  const size_t lds = (size_t)3 * ((B + 3) & ~3) * sizeof(float);
  static std::atomic<uint64_t> opted{0};
  const hipError_t e = bar_lds_optin(opted, bar_score_kernel<NV>, lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(bar_score_kernel<NV>, dim3(Q), dim3(kBarThreads), lds, st, logits, B, inv_temp, s);
  return hipGetLastError();
}

// What both scoring entry points refuse; `s.J` is set to 0 where no per-target output is asked for.
bool bar_score_args_ok(BarScoreArgs& s, int B) {
  const bool per_target = s.nll || s.cdf || s.pi || s.ei;
  if (B < 2 || B > kBarHeadMaxBars || s.J < 0 || s.J > kBarScoreMaxTargets || (per_target && !s.ys)) return false;
  if (!s.borders || !s.widths || !s.log_widths || !s.mean_squares || !s.ei_mids || !s.ends) return false;
  if (!per_target) s.J = 0;
  return true;
}

}  // namespace

hipError_t launch_bar_head(const float* logits, int M, int Q, int B, const unsigned char* cancel, int ldc,
                           const int* idx, const float* share, int ldt, float inv_temp, int avg_before, const float* borders,
                           const float* means, const float* mode_means, const float* widths, const float* levels,
                           int K, float* out_logits, float* mean, float* mode, float* quantiles, hipStream_t st,
                           const BarScoreArgs* score) {
  if (Q <= 0) return hipSuccess;
  if (M <= 0 || M > kBarHeadMaxMembers || B < 1 || B > kBarHeadMaxBars || K < 0 || K > kBarHeadMaxLevels ||
      ldt < B + 1 || (cancel && ldc < B))
    return hipErrorInvalidValue;
  const int tvec = ldt % 4 == 0 && ldt >= ((B + 4) & ~3) && (reinterpret_cast<uintptr_t>(idx) & 15) == 0 &&
                   (reinterpret_cast<uintptr_t>(share) & 15) == 0;
  const int cvec = cancel && ldc % 4 == 0 && ldc >= ((B + 3) & ~3) && (reinterpret_cast<uintptr_t>(cancel) & 3) == 0;
  const BarHeadArgs a{logits, cancel,  idx,  share, borders, means, mode_means, widths,   levels,
                      out_logits, mean, mode, quantiles, M,  Q,  B,  K,  inv_temp, avg_before, ldt, ldc, tvec, cvec};
  if (!score) {
    const BarScoreArgs none{};
    if (B <= 1024) return bar_head_launch<1, false>(a, none, st);
    if (B <= 2048) return bar_head_launch<2, false>(a, none, st);
    if (B <= 5120) return bar_head_launch<5, false>(a, none, st);
    return bar_head_launch<8, false>(a, none, st);
  }
  BarScoreArgs s = *score;
  s.borders = borders;
  s.widths = widths;
  if (!bar_score_args_ok(s, B)) return hipErrorInvalidValue;
  if (B <= 1024) return bar_head_launch<1, true>(a, s, st);
  if (B <= 2048) return bar_head_launch<2, true>(a, s, st);
  if (B <= 5120) return bar_head_launch<5, true>(a, s, st);
  return bar_head_launch<8, true>(a, s, st);
}

hipError_t launch_bar_score(const float* logits, int Q, int B, float inv_temp, const BarScoreArgs& score, hipStream_t st) {
  if (Q <= 0) return hipSuccess;
  BarScoreArgs s = score;
  if (!bar_score_args_ok(s, B)) return hipErrorInvalidValue;
  if (B <= 1024) return bar_score_launch<1>(logits, Q, B, inv_temp, s, st);
  if (B <= 2048) return bar_score_launch<2>(logits, Q, B, inv_temp, s, st);
  if (B <= 5120) return bar_score_launch<5>(logits, Q, B, inv_temp, s, st);
  return bar_score_launch<8>(logits, Q, B, inv_temp, s, st);
}

}  // namespace mmpfn
