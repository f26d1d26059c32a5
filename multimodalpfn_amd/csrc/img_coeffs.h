// Coefficient tables of Pillow's 8-bit bilinear resize (Image.resize(size, Image.BILINEAR) on an RGB image,
// libImaging/Resample.c: precompute_coeffs + normalize_coeffs_8bpc), restated for the image front end
// (imgprep.hip).  The reference resizes every picture with it in front of its image tower
// (mmpfn/datasets/pad_ufes_20.py:53-61, cbis_ddsm.py:71-81, petfinder.py:85-95).
//
// Host only, IEEE double in Pillow's order of operations, no HIP: the device reads these integers and never
// recomputes them, so bit equality with Pillow does not depend on a device compiler's contraction choices.
//
// Per axis, in_size -> out_size:
//   scale = in / out; fs = max(scale, 1); support = 1.0 * fs; ksize = (int)ceil(support) * 2 + 1
//   for output index xx: center = (xx + 0.5) * scale; ss = 1 / fs
//     xmin = max((int)(center - support + 0.5), 0); xmax = min((int)(center + support + 0.5), in) - xmin
//     w[x] = max(0, 1 - |(x + xmin - center + 0.5) * ss|), x < xmax; ww = their left-to-right sum; w[x] /= ww
//     k[x] = (int)(0.5 + w[x] * 2^22)        (bilinear weights are never negative)
//   out = clamp((2^21 + sum pixel[xmin + x] * k[x]) >> 22, 0, 255), int32 accumulator
// The integers of one output index sum to 2^22 +- 2; they are not renormalised.  in == out gives the identity
// (k = {2^22, 0, 0}), which is what Pillow's skipping of that pass computes.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

namespace mmpfn {

constexpr int RESIZE_PRECISION_BITS = 32 - 8 - 2;  // Pillow's PRECISION_BITS
constexpr int RESIZE_MAX_SIDE = 16384;

inline int resize_ksize(int in_size, int out_size) {
  const double scale = (double)in_size / (double)out_size;
  const double fs = scale < 1.0 ? 1.0 : scale;
  const double support = 1.0 * fs;
  return (int)std::ceil(support) * 2 + 1;
}

// k [out_size][ksize] (zero past an index's xmax), bounds [out_size][2] = (xmin, xmax)
inline void resize_coeffs(int in_size, int out_size, int32_t* k, int32_t* bounds) {
#pragma clang fp contract(off)
  const double scale = (double)in_size / (double)out_size;
  const double fs = scale < 1.0 ? 1.0 : scale;
  const double support = 1.0 * fs;
  const int ksize = (int)std::ceil(support) * 2 + 1;
  const double ss = 1.0 / fs;
  std::vector<double> w(ksize);
  for (int xx = 0; xx < out_size; ++xx) {
    const double center = (xx + 0.5) * scale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in_size) xmax = in_size;
    xmax -= xmin;
    double ww = 0.0;
    for (int x = 0; x < xmax; ++x) {
      double a = (x + xmin - center + 0.5) * ss;
      if (a < 0.0) a = -a;
      const double v = a < 1.0 ? 1.0 - a : 0.0;
      w[x] = v;
      ww += v;
    }
    for (int x = 0; x < xmax; ++x)
      if (ww != 0.0) w[x] /= ww;
    int32_t* kk = k + (int64_t)xx * ksize;
    for (int x = 0; x < ksize; ++x) kk[x] = x < xmax ? (int32_t)(0.5 + w[x] * (double)(1 << RESIZE_PRECISION_BITS)) : 0;
    bounds[2 * xx] = xmin;
    bounds[2 * xx + 1] = xmax;
  }
}

// what the tower is handed for a byte: float32(v) / float32(255), one correctly rounded fp32 division
// (v * (1 / 255.f) differs for some v)
inline void pixel_scale_table(float* out256) {
  for (int v = 0; v < 256; ++v) {
    volatile float num = (float)v, den = 255.0f;
    out256[v] = num / den;
  }
}

}  // namespace mmpfn
