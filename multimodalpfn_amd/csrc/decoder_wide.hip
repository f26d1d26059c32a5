// Decoder of a value-target (regression) model, n_out = the bar distribution's buckets (5000 in the reference's
// checkpoints; transformer.py:388-403,850-853): two GEMMs with the M and N edges guarded,
//   hidden = GELU(X W1^T + b1)  [M Q][Fh]   in the mode's operand type, into a workspace
//   logits = hidden W2^T + b2   [M][Q][n_out] fp32
// on fp32-input MFMA (the fp32 modes: exact fp32 fma chains) or bf16 / fp16 MFMA with fp32 accumulation (the 16-bit
// modes; the bf16 mode's fp32 state is rounded to bf16 as it is loaded).  The fused decoders of encoder.hip stop at
// n_out <= 16 (MFMA form) or need (nhid / 32 + 1) Q n_out floats of scratch (fp32 form); a classifier keeps them.
#include "common.h"
#include "kernels.h"

namespace mmpfn {
namespace {

// operand fragments of one 16-row tile and one K step: lane l holds row l & 15, K elements KL (l >> 4) .. + KL
template <typename T> struct WideOp;
template <> struct WideOp<float> {
  typedef f32x4 frag;  // 4 K steps of mfma 16x16x4: step j takes element j of every lane (K 4 (l >> 4) + j)
  static constexpr int KS = 16;
};
template <> struct WideOp<bf16> {
  typedef bf16x8 frag;
  static constexpr int KS = 32;
};
template <> struct WideOp<_Float16> {
  typedef f16x8 frag;
  static constexpr int KS = 32;
};

__device__ __forceinline__ f32x4 wide_load(const float* p, float) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ bf16x8 wide_load(const bf16* p, bf16) { return *reinterpret_cast<const bf16x8*>(p); }
__device__ __forceinline__ f16x8 wide_load(const _Float16* p, _Float16) { return *reinterpret_cast<const f16x8*>(p); }
__device__ __forceinline__ bf16x8 wide_load(const float* p, bf16) {  // fp32 state -> bf16 operands
  const f32x4 lo = *reinterpret_cast<const f32x4*>(p), hi = *reinterpret_cast<const f32x4*>(p + 4);
  bf16x8 r;
#pragma unroll
  for (int j = 0; j < 4; ++j) r[j] = (bf16)lo[j], r[4 + j] = (bf16)hi[j];
  return r;
}

__device__ __forceinline__ void wide_mma(f32x4 a, f32x4 b, f32x4& c) {
#pragma unroll
  for (int j = 0; j < 4; ++j) c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], b[j], c, 0, 0, 0);
}
__device__ __forceinline__ void wide_mma(bf16x8 a, bf16x8 b, f32x4& c) { c = mfma16x(a, b, c); }
__device__ __forceinline__ void wide_mma(f16x8 a, f16x8 b, f32x4& c) { c = mfma16x(a, b, c); }

// C[z][m][n] = act(sum_k A[z][m][k] W[n][k] + bias[n]); a 64 x 64 tile per block, 32 x 32 per wave as 2 x 2 MFMA
// tiles, operands straight from global memory (16 B per lane and fragment; W and a block row of A stay in L2).
// Rows >= M and columns >= N load the last valid row (no read beyond the matrices) and store nothing.
template <typename T, typename TA, typename TC, int ACT>
__global__ __launch_bounds__(256) void dec_wide_kernel(const TA* __restrict__ A, int64_t lda, int64_t a_z,
                                                       const T* __restrict__ W, const float* __restrict__ bias,
                                                       TC* __restrict__ C, int64_t ldc, int64_t c_z, int M, int N, int K) {
  constexpr int KS = WideOp<T>::KS, KL = KS / 4;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
  const int m0 = blockIdx.y * 64 + (wave >> 1) * 32, n0 = blockIdx.x * 64 + (wave & 1) * 32;
  if (m0 >= M || n0 >= N) return;
  A += (int64_t)blockIdx.z * a_z;
  C += (int64_t)blockIdx.z * c_z;
  const TA* ap[2];
  const T* wp[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    ap[i] = A + (int64_t)min(m0 + 16 * i + r, M - 1) * lda + KL * g;
    wp[i] = W + (int64_t)min(n0 + 16 * i + r, N - 1) * K + KL * g;
  }
  f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int k = 0; k < K; k += KS) {
    typename WideOp<T>::frag a[2], b[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) a[i] = wide_load(ap[i] + k, T{}), b[i] = wide_load(wp[i] + k, T{});
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) wide_mma(a[i], b[j], acc[i][j]);
  }
  // C fragment: column l & 15, rows 4 (l >> 4) + rr
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int col = n0 + 16 * j + r;
    if (col >= N) continue;
    const float bv = bias[col];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const int row = m0 + 16 * i + 4 * g + rr;
        if (row >= M) continue;
        float v = acc[i][j][rr] + bv;
        if (ACT == ACT_GELU) v = gelu_erf(v);
        C[(int64_t)row * ldc + col] = (TC)v;
      }
  }
}

template <typename T, typename TA>
hipError_t decoder_wide_t(const void* X, int Q, int64_t xm, int M, const void* W1, const float* b1, int Fh,
                          const void* W2, const float* b2, int n_out, void* hidden, float* out, int E, hipStream_t st) {
  T* H = (T*)hidden;
  hipLaunchKernelGGL((dec_wide_kernel<T, TA, T, ACT_GELU>), dim3((Fh + 63) / 64, (Q + 63) / 64, M), dim3(256), 0, st,
                     (const TA*)X, (int64_t)E, xm, (const T*)W1, b1, H, (int64_t)Fh, (int64_t)Q * Fh, Q, Fh, E);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const int64_t rows = (int64_t)M * Q;
  hipLaunchKernelGGL((dec_wide_kernel<T, T, float, ACT_NONE>), dim3((n_out + 63) / 64, (unsigned)((rows + 63) / 64), 1),
                     dim3(256), 0, st, (const T*)H, (int64_t)Fh, (int64_t)0, (const T*)W2, b2, out, (int64_t)n_out,
                     (int64_t)0, (int)rows, n_out, Fh);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_decoder_wide(const void* X, DType x_t, int Q, int64_t xm, int M, const void* W1, const float* b1,
                               int Fh, const void* W2, const float* b2, int n_out, DType op_t, void* hidden, float* out,
                               int E, hipStream_t st) {
  if (Q <= 0 || M <= 0) return hipSuccess;
  if (!X || !W1 || !b1 || !W2 || !b2 || !hidden || !out || n_out <= 0 || E % 32 != 0 || Fh % 32 != 0 ||
      (int64_t)M * Q > 0x7fffffff || (Q + 63) / 64 > 65535 || ((int64_t)M * Q + 63) / 64 > 65535 || M > 65535)
    return hipErrorInvalidValue;
  if (x_t == DType::F32 && op_t == DType::F32)
    return decoder_wide_t<float, float>(X, Q, xm, M, W1, b1, Fh, W2, b2, n_out, hidden, out, E, st);
  if (x_t == DType::F32 && op_t == DType::BF16)
    return decoder_wide_t<bf16, float>(X, Q, xm, M, W1, b1, Fh, W2, b2, n_out, hidden, out, E, st);
  if (x_t == DType::F16 && op_t == DType::F16)
    return decoder_wide_t<_Float16, _Float16>(X, Q, xm, M, W1, b1, Fh, W2, b2, n_out, hidden, out, E, st);
  return hipErrorInvalidValue;
}

}  // namespace mmpfn
