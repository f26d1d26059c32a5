// Image front end (SURVEY.md 8(f)4'): raw RGB uint8 pixels of any size -> the patch-embedding GEMM's A operand.
//
// The reference resizes every decoded picture on the host in front of its image tower
// (mmpfn/datasets/pad_ufes_20.py:53-61, cbis_ddsm.py:71-81, petfinder.py:85-95:
//   np.array(img.resize((img_size, img_size), Image.BILINEAR), dtype=np.float32); images /= 255.0).
// This kernel does that resize on the device with Pillow's own integers (img_coeffs.h builds the tables on the
// host), horizontal pass first, uint8 between the passes, and writes the im2col rows im2col_kernel
// (modality.hip) would write from the resized fp32 image: row (b, py, px), column c * P * P + ky * P + kx, zero
// from 3 * P * P to Kpad.  No fp32 image and no intermediate reaches HBM.
//
// One block per (band of P output rows, tile of <= 384 output pixels, image); one launch serves a ragged batch.
// A thread owns one output pixel column of the tile (its three channels share the horizontal coefficients):
//   * the tile's horizontal coefficients are copied to LDS once, tap-major (lane t reads word x * 384 + t: no bank
//     conflict), when the batch's longest row of taps fits; else they are read from the table in global memory;
//   * the band's source rows stream once through LDS in chunks (16-B loads, each row at its own 16-B skew);
//   * per source row the thread resamples its pixel horizontally (clipped to uint8 as Pillow clips its
//     intermediate) and adds it, times the row's vertical coefficient, to the int32 accumulators of the output
//     rows the source row feeds -- registers, P <= 16 -- so a band's height in source rows is unbounded;
//   * the clipped band is staged in LDS as uint8 [P][pixels][3], and every A row leaves as contiguous 16-B stores
//     of table-scaled values (float32(v) / float32(255), divided on the host).
// Optional second output: the resized uint8 [B][oh][ow][3] image.
#include <algorithm>

#include "common.h"
#include "modality.h"

namespace mmpfn {

namespace {

constexpr int IP_THREADS = 384;                // = output pixels per tile
constexpr int IP_BCOLS = IP_THREADS * 3;       // band staging row: (pixel, channel)
constexpr int IP_ROWS = 16;                    // source rows per LDS chunk, at most
constexpr int IP_STAGE = 24576;                // bytes of the row stage, unless one row needs more
constexpr int IP_KH_TAPS = 24;                 // horizontal taps kept in LDS, at most (shrink factors to 11.5)
constexpr int IP_TAIL = IMGPREP_PMAX * IP_BCOLS + 256 * 4;  // band staging + scale table

template <typename TO> struct Vec16;
template <> struct Vec16<float> { typedef f32x4 t; };
template <> struct Vec16<bf16> { typedef bf16x8 t; };

__device__ __forceinline__ int clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// LDS: [row stage: stage_bytes][horizontal taps: kh_taps * 384 * 4][band: 16 * 1152][scale table: 1024]
template <typename TO>
__global__ __launch_bounds__(IP_THREADS) void imgprep_kernel(
    const uint8_t* __restrict__ pixels, const ImgPrepDesc* __restrict__ desc, const int32_t* __restrict__ tab,
    const float* __restrict__ lut, int oh, int ow, int P, int Kpad, int tpx, int stage_bytes, int kh_taps,
    uint8_t* __restrict__ resized, TO* __restrict__ patches) {
  extern __shared__ __attribute__((aligned(16))) unsigned char ip_smem[];
  uint8_t* stage = ip_smem;                          // [rows][stride], row r's bytes from its skew on
  int32_t* khs = (int32_t*)(ip_smem + stage_bytes);  // [tap][IP_THREADS]
  uint8_t* band = ip_smem + stage_bytes + kh_taps * IP_THREADS * 4;  // [IMGPREP_PMAX][IP_BCOLS]
  float* slut = (float*)(band + IMGPREP_PMAX * IP_BCOLS);
  const int t = threadIdx.x;
  const int py = blockIdx.x, b = blockIdx.z;
  const ImgPrepDesc d = desc[b];
  const int gh = oh / P, gw = ow / P;
  const int px0 = blockIdx.y * tpx, npx = min(tpx, gw - px0);
  const int ox0 = px0 * P, npix = npx * P;
  const int32_t* kh = tab + d.kh + (int64_t)ox0 * d.ksh;
  const int32_t* hb = tab + d.hb + 2 * ox0;
  const int32_t* kv = tab + d.kv + (int64_t)py * P * d.ksv;
  const int32_t* vb = tab + d.vb + 2 * py * P;
  if (t < 256) slut[t] = lut[t];
  const bool kh_lds = d.ksh <= kh_taps;  // the block's own taps fit what the launch reserved
  if (kh_lds)
    for (int u = t; u < npix * d.ksh; u += IP_THREADS) {
      const int p = u / d.ksh, x = u - p * d.ksh;
      khs[x * IP_THREADS + p] = kh[u];
    }

  // the tile's source columns [x0, x1) and the band's source rows [y0, y1): bounds are monotone in the index
  const int x0 = hb[0], x1 = hb[2 * (npix - 1)] + hb[2 * (npix - 1) + 1];
  const int y0 = vb[0], y1 = vb[2 * (P - 1)] + vb[2 * (P - 1) + 1];
  const int n = (x1 - x0) * 3;                 // bytes of a source row the tile reads
  const int stride = (n + 15 + 15) & ~15;      // skew (<= 15) + n, in whole 16-B words
  const int nws = stride >> 4;
  const int R = min(IP_ROWS, stage_bytes / stride);  // >= 1: the launcher sizes the stage for the widest image
  const uint8_t* gimg = pixels + d.pix_off + (int64_t)x0 * 3;
  const int64_t rowb = (int64_t)d.W * 3;

  const bool live = t < npix;
  const int rel = live ? (hb[2 * t] - x0) * 3 : 0;  // the pixel's first tap, bytes into the staged row
  const int cnt = live ? hb[2 * t + 1] : 0;
  const int32_t* kp = kh + (int64_t)(live ? t : 0) * d.ksh;
  // vertical pass: source row y feeds the output rows [r_lo, r_hi) (the bounds are monotone), row r with the
  // coefficient kv[voff[r] + y]; all of it is the same in every lane and stays in scalar registers
  int voff[IMGPREP_PMAX];
#pragma unroll
  for (int r = 0; r < IMGPREP_PMAX; ++r)
    voff[r] = __builtin_amdgcn_readfirstlane(r * d.ksv - vb[2 * min(r, P - 1)]);
  int r_lo = 0, r_hi = 0;
  int acc[3][IMGPREP_PMAX];
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int r = 0; r < IMGPREP_PMAX; ++r) acc[c][r] = 0;

  for (int yc = y0; yc < y1; yc += R) {
    const int nr = min(R, y1 - yc);
    __syncthreads();  // the previous chunk has been read (first pass: khs and slut are written)
    for (int u = t; u < nr * nws; u += IP_THREADS) {
      const int rr = u / nws, w = u - rr * nws;
      const uint8_t* g = gimg + (int64_t)(yc + rr) * rowb;  // n bytes from here
      const int skew = (int)((uintptr_t)g & 15);
      const int lo = 16 * w, hi = lo + 16, end = skew + n;  // the row occupies [skew, end) of its stage row
      if (lo >= end) continue;
      uint8_t* l = stage + rr * stride;
      const uint8_t* ga = g - skew;  // 16-B aligned; only bytes [skew, end) of it are read
      if (lo >= skew && hi <= end) {
        *(u32x4*)(l + lo) = *(const u32x4*)(ga + lo);
      } else {
        for (int q = max(lo, skew); q < min(hi, end); ++q) l[q] = ga[q];
      }
    }
    __syncthreads();
    for (int rr = 0; rr < nr; ++rr) {
      const int y = yc + rr;
      const int skew = (int)((uintptr_t)(gimg + (int64_t)y * rowb) & 15);
      const uint8_t* s = stage + rr * stride + skew + rel;
      int h0 = 1 << 21, h1 = 1 << 21, h2 = 1 << 21;
      // 24-bit multiplies: a byte times a coefficient of at most 2^22 + 2
      if (kh_lds) {
        // every tap of the table: those past the pixel's count are zero, and the bytes they meet lie inside the
        // block's LDS (at most 3 * IP_KH_TAPS past the row stage), so the trip count is the same in every lane
        const int32_t* kq = khs + t;
        for (int x = 0; x < d.ksh; ++x) {
          const int k = kq[x * IP_THREADS];
          h0 += __mul24((int)s[3 * x], k);
          h1 += __mul24((int)s[3 * x + 1], k);
          h2 += __mul24((int)s[3 * x + 2], k);
        }
      } else {
        for (int x = 0; x < cnt; ++x) {
          const int k = kp[x];
          h0 += __mul24((int)s[3 * x], k);
          h1 += __mul24((int)s[3 * x + 1], k);
          h2 += __mul24((int)s[3 * x + 2], k);
        }
      }
      h0 = clip8(h0 >> 22), h1 = clip8(h1 >> 22), h2 = clip8(h2 >> 22);
      while (r_hi < P && vb[2 * r_hi] <= y) ++r_hi;
      while (r_lo < r_hi && vb[2 * r_lo] + vb[2 * r_lo + 1] <= y) ++r_lo;
      const unsigned open = ((1u << r_hi) - 1u) & ~((1u << r_lo) - 1u);
#pragma unroll
      for (int r = 0; r < IMGPREP_PMAX; ++r) {
        if (open >> r & 1u) {
          const int kvv = kv[voff[r] + y];
          acc[0][r] += __mul24(h0, kvv);
          acc[1][r] += __mul24(h1, kvv);
          acc[2][r] += __mul24(h2, kvv);
        }
      }
    }
  }

  // clip the band, stage it (and write the resized image)
  if (live) {
#pragma unroll
    for (int r = 0; r < IMGPREP_PMAX; ++r) {
      if (r < P) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const uint8_t v = (uint8_t)clip8((acc[c][r] + (1 << 21)) >> 22);
          band[r * IP_BCOLS + 3 * t + c] = v;
          if (resized) resized[(((int64_t)b * oh + py * P + r) * ow + ox0 + t) * 3 + c] = v;
        }
      }
    }
  }
  __syncthreads();
  if (!patches) return;
  // A rows: 16 contiguous bytes per lane, consecutive lanes along the row
  constexpr int V = 16 / (int)sizeof(TO);
  const int vpr = Kpad / V, K0 = 3 * P * P;
  for (int u = t; u < npx * vpr; u += IP_THREADS) {
    const int pxl = u / vpr, k0 = (u - pxl * vpr) * V;
    int c = k0 / (P * P), ky = (k0 - c * P * P) / P, kx = k0 - c * P * P - ky * P;
    typename Vec16<TO>::t vals;
#pragma unroll
    for (int e = 0; e < V; ++e) {
      float f = 0.f;
      if (k0 + e < K0) {
        f = slut[band[ky * IP_BCOLS + (pxl * P + kx) * 3 + c]];
        if (++kx == P) {
          kx = 0;
          if (++ky == P) ky = 0, ++c;
        }
      }
      vals[e] = from_f32<TO>(f);
    }
    const int64_t row = ((int64_t)b * gh + py) * gw + px0 + pxl;
    *(typename Vec16<TO>::t*)(patches + row * Kpad + k0) = vals;
  }
}

std::atomic<uint64_t> ip_opted32{0}, ip_opted16{0};

int stage_bytes_for(int max_w) {
  const int widest = (3 * max_w + 15 + 15) & ~15;  // one whole source row at the worst skew
  return std::max(widest, std::min(IP_ROWS * widest, IP_STAGE));
}

}  // namespace

hipError_t launch_imgprep(const uint8_t* pixels, const ImgPrepDesc* desc, const int32_t* tab, const float* lut, int B,
                          int max_w, int max_ksh, int oh, int ow, int P, int Kpad, uint8_t* resized, void* patches,
                          bool out_f32, hipStream_t st) {
  if (B <= 0) return hipSuccess;
  if (B > 65535 || P <= 0 || P > IMGPREP_PMAX || oh <= 0 || ow <= 0 || oh % P || ow % P || oh / P > 65535 ||
      Kpad < 3 * P * P || Kpad % 32 || max_w <= 0 || max_w > 16384 || max_ksh <= 0 || ((uintptr_t)patches & 15))
    return hipErrorInvalidValue;
  const int tpx = IP_THREADS / P;  // whole patches per tile
  const int gw = ow / P;
  const dim3 grid(oh / P, (gw + tpx - 1) / tpx, B);
  const int stage = stage_bytes_for(max_w);
  const int kh_taps = max_ksh <= IP_KH_TAPS ? max_ksh : 0;  // longer rows of taps stay in global memory
  const int lds = stage + kh_taps * IP_THREADS * 4 + IP_TAIL;
  const int lds_max = stage_bytes_for(16384) + IP_KH_TAPS * IP_THREADS * 4 + IP_TAIL;  // opt-in: per device, set once
  if (out_f32) {
    hipError_t e = lds_optin(ip_opted32, (const void*)imgprep_kernel<float>, lds_max);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(imgprep_kernel<float>, grid, dim3(IP_THREADS), lds, st, pixels, desc, tab, lut, oh, ow, P, Kpad,
                       tpx, stage, kh_taps, resized, (float*)patches);
  } else {
    hipError_t e = lds_optin(ip_opted16, (const void*)imgprep_kernel<bf16>, lds_max);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(imgprep_kernel<bf16>, grid, dim3(IP_THREADS), lds, st, pixels, desc, tab, lut, oh, ow, P, Kpad,
                       tpx, stage, kh_taps, resized, (bf16*)patches);
  }
  return hipGetLastError();
}

}  // namespace mmpfn
