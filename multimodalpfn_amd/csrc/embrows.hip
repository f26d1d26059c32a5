// Row embeddings out of the state: the target token's final state of a range of rows, as fp32.
//
// The state is X [M][T][S][E] (token-major, fp32 or -- PREC_F16 -- fp16); the row embeddings of the reference's
// forward (transformer.py:850-864) are column T-1 of it: rows [0, N) the train rows', rows [N, S) the test rows' (the
// decoder's input).  launch_target_rows copies rows [r0, r0 + n) of that column of every member to a compact fp32
// [M][n][E].  One thread moves 16 bytes of the state: four fp32 values, or eight fp16 values widened to two 16-byte
// stores (fp16 -> fp32 is exact, so the output is the state's own values either way).  No LDS, no atomics.
#include "common.h"
#include "kernels.h"

namespace mmpfn {

namespace {
// V: the 16-byte piece of a state row (f32x4 or f16x8); pr: pieces per row; member m's column T-1 starts at
// X + m * xm + col (elements of the state's type), so piece i of the output -- row i / pr of [M * n] -- is piece
// i % pr of state row r0 + (i / pr) % n
template <typename V>
__global__ __launch_bounds__(256) void target_rows_kernel(const V* __restrict__ X, int64_t xm_pieces, int64_t n,
                                                          int pr, int64_t total, f32x4* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int64_t row = i / pr, m = row / n;
  const int p = (int)(i - row * pr);
  const V v = X[m * xm_pieces + (row - m * n) * pr + p];
  if constexpr (std::is_same<V, f32x4>::value) {
    out[i] = v;
  } else {
    f32x4 lo, hi;
#pragma unroll
    for (int k = 0; k < 4; ++k) lo[k] = (float)v[k], hi[k] = (float)v[4 + k];
    out[2 * i] = lo, out[2 * i + 1] = hi;
  }
}
}  // namespace

hipError_t launch_target_rows(const void* X, DType x_t, int S, int T, int E, int M, int r0, int n, float* out,
                              hipStream_t st) {
  if (n <= 0 || M <= 0) return hipSuccess;
  if (!X || !out || x_t == DType::BF16 || S <= 0 || T <= 0 || E <= 0 || E % 8 != 0 || r0 < 0 || r0 > S - n ||
      ((uintptr_t)X | (uintptr_t)out) % 16 != 0)
    return hipErrorInvalidValue;
  const int64_t xm = (int64_t)T * S * E, first = ((int64_t)(T - 1) * S + r0) * E;  // elements of the state's type
  const int per = x_t == DType::F16 ? 8 : 4, pr = E / per;                          // elements / pieces of a row
  const int64_t total = (int64_t)M * n * pr, blocks = (total + 255) / 256;
  if (blocks > 0x7fffffff) return hipErrorInvalidValue;
  if (x_t == DType::F16)
    hipLaunchKernelGGL((target_rows_kernel<f16x8>), dim3((unsigned)blocks), dim3(256), 0, st,
                       (const f16x8*)((const f16*)X + first), xm / per, (int64_t)n, pr, total, (f32x4*)out);
  else
    hipLaunchKernelGGL((target_rows_kernel<f32x4>), dim3((unsigned)blocks), dim3(256), 0, st,
                       (const f32x4*)((const float*)X + first), xm / per, (int64_t)n, pr, total, (f32x4*)out);
  return hipGetLastError();
}

}  // namespace mmpfn
