// Member preprocessing of the test rows (model/preprocessing.py's fitted steps as preprocessing.py:416-473 chains them):
// one launch runs a member's compiled program (device_transform.py: a flat op list plus an int and a double blob) over
// all Q rows in float64 and writes the member's float32 table.  Rows are independent: a block takes `rows` of them,
// keeps each one's working row in LDS twice (ping-pong, stride `width` doubles) and walks the op list with one barrier
// per op, a thread per output cell.  The work is a few hundred cells per row, so the kernel is one short launch and
// nothing more; every search is a binary search per cell and the hash a serial chain per row.
// Every index the kernel forms was checked against the blobs when the program was made (capi.cpp xform_refusal).
#include "common.h"
#include "kernels.h"

namespace mmpfn {
namespace {

__device__ __forceinline__ uint64_t xf_bits(double x) { return (uint64_t)__double_as_longlong(x); }
__device__ __forceinline__ double xf_double(uint64_t b) { return __longlong_as_double((long long)b); }

// float32 -> float64 as the host converts it: exact, a NaN keeping its sign and payload with the quiet bit set
__device__ __forceinline__ double xf_widen(float v) {
  if (v != v) {
    const uint32_t b = __float_as_uint(v);
    return xf_double(((uint64_t)(b >> 31) << 63) | 0x7FF8000000000000ull | ((uint64_t)(b & 0x7FFFFFu) << 29));
  }
  return (double)v;
}

// float64 -> float32, round to nearest even (astype(np.float32)); a NaN keeps its sign and the payload's top bits
__device__ __forceinline__ float xf_narrow(double v) {
  if (v != v) {
    const uint64_t b = xf_bits(v);
    return __uint_as_float((uint32_t)(b >> 63) << 31 | 0x7FC00000u | (uint32_t)((b >> 29) & 0x3FFFFFu));
  }
  return (float)v;
}

// np.interp (numpy's arr_interp) at a non-NaN x over xp = q, fp = r, or with NEG over xp = -q[::-1], fp = -r[::-1]:
// j is the LAST index with xp[j] <= x -- inside a run of tied quantiles that choice is the result.
template <bool NEG>
__device__ __forceinline__ double xf_interp(double x, const double* q, const double* r, int n) {
#pragma clang fp contract(off)
  auto xp = [&](int i) { return NEG ? -q[n - 1 - i] : q[i]; };
  auto fp = [&](int i) { return NEG ? -r[n - 1 - i] : r[i]; };
  if (x > xp(n - 1)) return fp(n - 1);
  if (x < xp(0)) return fp(0);
  int lo = 0, hi = n;  // the first index whose xp exceeds x
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (xp(mid) <= x) lo = mid + 1;
    else hi = mid;
  }
  const int j = lo - 1;  // >= 0: x >= xp(0)
  const double xj = xp(j), fj = fp(j);
  if (j == n - 1 || xj == x) return fj;
  const double x1 = xp(j + 1), f1 = fp(j + 1);
  const double slope = (f1 - fj) / (x1 - xj);
  double res = slope * (x - xj) + fj;
  if (res != res) {
    res = slope * (x - x1) + f1;
    if (res != res && fj == f1) res = fj;
  }
  return res;
}

// QuantileTransformer._transform_col, output_distribution="uniform": both interpolation directions halved, exact hits
// on the two bounds, NaN passed through with its bits
__device__ __forceinline__ double xf_quantile(double x, const double* q, const double* r, int n) {
#pragma clang fp contract(off)
  if (x != x) return x;
  double y = 0.5 * (xf_interp<false>(x, q, r, n) - xf_interp<true>(-x, q, r, n));
  if (x == q[n - 1]) y = 1.0;
  if (x == q[0]) y = 0.0;
  return y;
}

// exact match in the sorted categories -> its value; none -> unseen; NaN -> miss.  p: [unseen, miss, cats[n], values[n]]
__device__ __forceinline__ double xf_lookup(double x, const double* p, int n) {
  if (x != x) return p[1];
  const double* cats = p + 2;
  int lo = 0, hi = n;  // the first index whose category is not below x
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (cats[mid] < x) lo = mid + 1;
    else hi = mid;
  }
  return lo < n && cats[lo] == x ? cats[n + lo] : p[0];
}

// make_standard_scaler_safe: inf -> NaN -> pre, (x - mean) / scale as a true division, inf -> NaN -> post
__device__ __forceinline__ double xf_scale(double x, const double* p) {
#pragma clang fp contract(off)
  if (x != x || fabs(x) == INFINITY) x = p[0];
  double y = (x - p[1]) / p[2];
  if (y != y || fabs(y) == INFINITY) y = p[3];
  return y;
}

__device__ __forceinline__ uint64_t xf_rotl(uint64_t x, int r) { return (x << r) | (x >> (64 - r)); }
__device__ __forceinline__ void xf_sipround(uint64_t& v0, uint64_t& v1, uint64_t& v2, uint64_t& v3) {
  v0 += v1, v1 = xf_rotl(v1, 13) ^ v0, v0 = xf_rotl(v0, 32);
  v2 += v3, v3 = xf_rotl(v3, 16) ^ v2;
  v0 += v3, v3 = xf_rotl(v3, 21) ^ v0;
  v2 += v1, v1 = xf_rotl(v1, 17) ^ v2, v2 = xf_rotl(v2, 32);
}

// AddFingerprintFeaturesStep's test form: SipHash-2-4 with the zero key (model/_siphash.py) over the w float64 cells
// of (x + salt) + salt, -1 mapped to -2, then mod 10^12 / 10^12.  A NaN cell is not sent through the adder: the host's
// adder keeps its sign and payload and sets the quiet bit, and that is written out here.
__device__ double xf_fingerprint(const double* row, int w, double salt) {
#pragma clang fp contract(off)
  uint64_t v0 = 0x736F6D6570736575ull, v1 = 0x646F72616E646F6Dull, v2 = 0x6C7967656E657261ull,
           v3 = 0x7465646279746573ull;
  for (int j = 0; j < w; ++j) {
    const double x = row[j];
    const uint64_t m = x != x ? (xf_bits(x) | 0x0008000000000000ull) : xf_bits((x + salt) + salt);
    v3 ^= m;
    xf_sipround(v0, v1, v2, v3);
    xf_sipround(v0, v1, v2, v3);
    v0 ^= m;
  }
  const uint64_t last = (uint64_t)((8 * (int64_t)w) & 0xFF) << 56;
  v3 ^= last;
  xf_sipround(v0, v1, v2, v3);
  xf_sipround(v0, v1, v2, v3);
  v0 ^= last;
  v2 ^= 0xFF;
  for (int k = 0; k < 4; ++k) xf_sipround(v0, v1, v2, v3);
  int64_t h = (int64_t)(v0 ^ v1 ^ v2 ^ v3);
  if (h == -1) h = -2;
  int64_t rem = h % 1000000000000ll;
  if (rem < 0) rem += 1000000000000ll;
  return (double)rem / 1e12;
}

template <bool X64>
__global__ __launch_bounds__(kXformThreads) void xform_kernel(const XformArgs a) {
  extern __shared__ __attribute__((aligned(16))) double xf_lds[];
  const int W = a.width, tid = threadIdx.x;
  const int r0 = blockIdx.x * a.rows;
  const int nr = a.Q - r0 < a.rows ? a.Q - r0 : a.rows;
  double* cur = xf_lds;
  double* nxt = xf_lds + (size_t)a.rows * W;

  bool inf = false;
  for (int cell = tid; cell < nr * a.n_in; cell += kXformThreads) {
    const int r = cell / a.n_in, j = cell - r * a.n_in;
    const int64_t o = (int64_t)(r0 + r) * a.ldx + j;
    const double v = X64 ? ((const double*)a.x)[o] : xf_widen(((const float*)a.x)[o]);
    inf |= fabs(v) == INFINITY;
    cur[r * W + j] = v;
  }
  if (inf) atomicOr(a.flag, kXformInfFlag);
  __syncthreads();

  for (int k = 0; k < a.n_ops; ++k) {
    const int32_t* op = a.ops + k * kXformOpInts;
    const int code = op[0], w_in = op[1], w_out = op[2];
    const int32_t* ints = a.ints + op[3];
    if (code == kXformGather) {
      for (int cell = tid; cell < nr * w_out; cell += kXformThreads) {
        const int r = cell / w_out, j = cell - r * w_out;
        nxt[r * W + j] = cur[r * W + ints[j]];
      }
    } else if (code == kXformMap) {
      for (int cell = tid; cell < nr * w_out; cell += kXformThreads) {
        const int r = cell / w_out, j = cell - r * w_out;
        const int32_t* c = ints + j * kXformMapInts;
        const double x = cur[r * W + c[0]];
        const double* p = a.dbl + c[2];
        const int kind = c[1];
        nxt[r * W + j] = kind == kXformPass     ? x
                         : kind == kXformLookup ? xf_lookup(x, p, c[3])
                         : kind == kXformQuantile ? xf_quantile(x, p, a.dbl + c[4], c[3])
                                                  : xf_scale(x, p);
      }
    } else if (code == kXformSvd) {
      const int n_pass = op[5], nz = op[6];
      const double* comps = a.dbl + op[4];
      for (int cell = tid; cell < nr * w_out; cell += kXformThreads) {
#pragma clang fp contract(off)
        const int r = cell / w_out, j = cell - r * w_out;
        const double* z = cur + r * W + n_pass;
        double acc = cur[r * W + (j < n_pass ? j : 0)];
        if (j >= n_pass) {
          const double* cj = comps + (size_t)(j - n_pass) * nz;
          acc = 0.0;
          for (int i = 0; i < nz; ++i) acc = acc + z[i] * cj[i];  // index order, product and sum rounded apart
        }
        nxt[r * W + j] = acc;
      }
    } else {  // kXformFingerprint
      for (int cell = tid; cell < nr * w_in; cell += kXformThreads) {
        const int r = cell / w_in, j = cell - r * w_in;
        nxt[r * W + j] = cur[r * W + j];
      }
      if (tid < nr) nxt[tid * W + w_in] = xf_fingerprint(cur + tid * W, w_in, a.dbl[op[4]]);
    }
    __syncthreads();
    double* t = cur;
    cur = nxt, nxt = t;
  }

  for (int cell = tid; cell < nr * a.n_out; cell += kXformThreads) {
    const int r = cell / a.n_out, j = cell - r * a.n_out;
    const double v = cur[r * W + j];
    a.out32[(int64_t)(r0 + r) * a.ld32 + j] = xf_narrow(v);
    if (a.out64) a.out64[(int64_t)(r0 + r) * a.ld64 + j] = v;
  }
}

}  // namespace

int xform_rows_per_block(int width) {
  const int r = kXformMaxWidth / (width > 0 ? width : 1);
  return r < 1 ? 1 : r > kXformMaxRows ? kXformMaxRows : r;
}

hipError_t launch_xform(const XformArgs& args, hipStream_t st) {
  XformArgs a = args;
  if (a.Q <= 0) return hipSuccess;
  if (!a.ops || !a.x || !a.out32 || !a.flag || a.n_ops < 0 || a.n_in < 1 || a.n_out < 1 || a.width < a.n_in ||
      a.width < a.n_out || a.width > kXformMaxWidth || a.ldx < a.n_in || a.ld32 < a.n_out ||
      (a.out64 && a.ld64 < a.n_out))
    return hipErrorInvalidValue;
  a.rows = xform_rows_per_block(a.width);
  const size_t lds = (size_t)2 * a.rows * a.width * sizeof(double);  // <= 64 KiB: rows * width <= kXformMaxWidth
  const unsigned blocks = (unsigned)((a.Q + a.rows - 1) / a.rows);
  if (a.x_f64) hipLaunchKernelGGL(xform_kernel<true>, dim3(blocks), dim3(kXformThreads), lds, st, a);
  else hipLaunchKernelGGL(xform_kernel<false>, dim3(blocks), dim3(kXformThreads), lds, st, a);
  return hipGetLastError();
}

}  // namespace mmpfn
