// Building blocks of the bar-distribution kernels (barhead.hip: the head and the scores; barsample.hip: the draws):
// the thread-to-bar mapping, the block-wide reductions and scan, the front end that finishes a row of logits, and
// the dynamic-LDS opt-in of their launches.  One definition each: what the kernels share must round alike.
#pragma once
#include "common.h"
#include "kernels.h"

namespace mmpfn {

constexpr int kBarThreads = 256;  // 4 waves

// Block-wide helpers on `red` (4 floats).  The leading barrier frees `red` from the previous use.
__device__ __forceinline__ float bar_block_max(float v, float* red) {
  v = wave_max(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}
__device__ __forceinline__ float bar_block_sum(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

__device__ __forceinline__ float wave_inclusive_scan(float x, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const float y = __shfl_up(x, d, 64);
    if (lane >= d) x += y;
  }
  return x;
}

// A thread's bars: NV groups of 4 consecutive bars; wave w owns bars [w * 256 NV, (w + 1) * 256 NV), group i of lane l
// starts at bar w * 256 NV + 256 i + 4 l, so a wave instruction covers 256 consecutive bars (1 KiB).
template <int NV>
__device__ __forceinline__ int bar_index(int i) {
  return (threadIdx.x >> 6) * (256 * NV) + 256 * i + 4 * (threadIdx.x & 63);
}

// Exclusive prefix sums of the block's values e (>= 0, zero beyond B) in bar order, and their total.  Lane-local
// sums of 4, a wave scan per group with a running carry, then the lower waves' totals.
template <int NV>
__device__ __forceinline__ float bar_block_scan(const float (&e)[NV][4], float (&c)[NV][4], float* red) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float carry = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const float t = (e[i][0] + e[i][1]) + (e[i][2] + e[i][3]);
    const float inc = wave_inclusive_scan(t, lane);
    float ex = __shfl_up(inc, 1, 64);
    if (lane == 0) ex = 0.f;
    float base = carry + ex;
    c[i][0] = base;
    base += e[i][0];
    c[i][1] = base;
    base += e[i][1];
    c[i][2] = base;
    base += e[i][2];
    c[i][3] = base;
    carry += __shfl(inc, 63, 64);
  }
  __syncthreads();
  if (lane == 0) red[wave] = carry;
  __syncthreads();
  const float t0 = red[0], t1 = red[1], t2 = red[2], t3 = red[3];
  const float off = wave == 0 ? 0.f : wave == 1 ? t0 : wave == 2 ? t0 + t1 : (t0 + t1) + t2;
#pragma unroll
  for (int i = 0; i < NV; ++i)
#pragma unroll
    for (int k = 0; k < 4; ++k) c[i][k] += off;
  return ((t0 + t1) + t2) + t3;
}

// A row of any logits [B] as a finished row: temperature, softmax and scan as bar_head_kernel's last stage has them
// (-inf logits are bars of weight zero), the probabilities in p_s and their inclusive cumulative sums in c_s, visible
// to every thread on return.  Returns the sum of exp(logit - max): NaN for a row without a finite maximum.
template <int NV>
__device__ __forceinline__ float bar_finish_row(const float* row, int B, float inv_temp, float* p_s, float* c_s,
                                                float* red) {
  const bool vec = (reinterpret_cast<uintptr_t>(row) & 15) == 0;
  float acc[NV][4], e[NV][4], c[NV][4];
  float mx = -INFINITY;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int j0 = bar_index<NV>(i);
    if (vec && j0 + 3 < B) {
      const f32x4 r = *reinterpret_cast<const f32x4*>(row + j0);
#pragma unroll
      for (int k = 0; k < 4; ++k) acc[i][k] = r[k];
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) acc[i][k] = j0 + k < B ? row[j0 + k] : -INFINITY;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      acc[i][k] = acc[i][k] * inv_temp;
      mx = fmaxf(mx, acc[i][k]);
    }
  }
  mx = bar_block_max(mx, red);
#pragma unroll
  for (int i = 0; i < NV; ++i)
#pragma unroll
    for (int k = 0; k < 4; ++k) e[i][k] = expf(acc[i][k] - mx);
  const float total = bar_block_scan<NV>(e, c, red);
  const float inv = 1.0f / total;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int j0 = bar_index<NV>(i);
    float pk[4], ck[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      pk[k] = e[i][k] * inv;
      ck[k] = (c[i][k] + e[i][k]) * inv;
    }
    if (j0 < B) {
      *reinterpret_cast<f32x4*>(p_s + j0) = f32x4{pk[0], pk[1], pk[2], pk[3]};
      *reinterpret_cast<f32x4*>(c_s + j0) = f32x4{ck[0], ck[1], ck[2], ck[3]};
    }
  }
  __syncthreads();
  return total;
}

// Dynamic LDS of a block: 2 arrays of B floats (3 with the scores), 64 KiB (96 KiB) at B = 8192 beside the static words
template <typename Kernel>
hipError_t bar_lds_optin(std::atomic<uint64_t>& opted, Kernel fn, size_t lds) {
  if (lds + 64 <= 64 * 1024) return hipSuccess;
  return lds_optin(opted, (const void*)fn, lds <= 64 * 1024 ? 64 * 1024 : 96 * 1024);
}

}  // namespace mmpfn
