// Host-side helpers shared by the two C-ABI translation units (capi.cpp, capi_modality.cpp): the owning device
// buffer, weight upload, and the error-return macros.  A handle (mmpfn_ctx, mmpfn_enc) is any struct with
// `std::string err` and the host weight map `host`; every helper leaves its error text in the handle it is given.
#pragma once
#include <hip/hip_runtime.h>

#include <map>
#include <string>
#include <vector>

#include "../../include/mmpfn_hip.h"
#include "kernels.h"
#include "weight_pack.h"

namespace mmpfn {

// device allocation, freed when the buffer (or the struct that holds it) goes away; move-only
struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr, o.bytes = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) {
      reset();
      p = o.p, bytes = o.bytes;
      o.p = nullptr, o.bytes = 0;
    }
    return *this;
  }
  ~DevBuf() { reset(); }
  void reset() {  // teardown: an error here has no caller to report to
    if (p) (void)hipFree(p);
    p = nullptr, bytes = 0;
  }
};

// One weight in the forms the kernels read it in; a form the model or its shape does not have is an empty buffer.
// The forms of one weight need not share a matrix order: whoever fills them says which order each has.
struct Weight {
  enum Form : unsigned { F32 = 1, BF16 = 2, F16 = 4, SPLIT = 8, GEMM = F32 | BF16 | SPLIT };  // GEMM: launch_gemm's
  DevBuf f32, bf16, f16;
  DevBuf split;       // the parity mode's bf16 planes (split_bf16): hi, and lo `numel` elements on
  int64_t numel = 0;  // elements of one split plane
  // the operand of a 16-bit mode's kernel, t = DType::F16 or DType::BF16
  const void* op16(DType t) const { return t == DType::F16 ? f16.p : bf16.p; }
  // the weight operand of launch_gemm in mode prec: PREC_BF16, PREC_F32 (split planes) or PREC_F32_MFMA
  void gemm_operand(GemmArgs& a, int prec) const {
    a.W = prec == PREC_BF16 ? bf16.p : prec == PREC_F32 ? split.p : f32.p;
    a.w_lo_off = prec == PREC_F32 ? numel : 0;
  }
};

template <typename H>
int fail(H* h, int code, const std::string& msg) {
  if (h) h->err = msg;
  return code;
}

// return the error of a HIP call / of a nested step from the enclosing function (h: the handle)
#define HIPCHK_ON(h, expr)                                                                                  \
  do {                                                                                                      \
    hipError_t e_ = (expr);                                                                                 \
    if (e_ != hipSuccess) return fail((h), MMPFN_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)
#define RC(expr)                     \
  do {                               \
    int rc_ = (expr);                \
    if (rc_ != MMPFN_OK) return rc_; \
  } while (0)

template <typename H>
int ensure(H* h, DevBuf& b, size_t bytes) {
  if (b.bytes >= bytes && b.p) return MMPFN_OK;
  b.reset();
  bytes = (bytes + 255) & ~size_t(255);
  HIPCHK_ON(h, hipMalloc(&b.p, bytes));
  b.bytes = bytes;
  return MMPFN_OK;
}

// v as fp32, or rounded to bf16 / fp16
template <typename H>
int upload(H* h, DevBuf& b, const std::vector<float>& v, DType t = DType::F32) {
  if (t == DType::F32) {
    RC(ensure(h, b, v.size() * 4));
    HIPCHK_ON(h, hipMemcpy(b.p, v.data(), v.size() * 4, hipMemcpyHostToDevice));
    return MMPFN_OK;
  }
  std::vector<uint16_t> r(v.size());
  for (size_t i = 0; i < v.size(); ++i) r[i] = t == DType::BF16 ? f2bf(v[i]) : f2h(v[i]);
  RC(ensure(h, b, r.size() * 2));
  HIPCHK_ON(h, hipMemcpy(b.p, r.data(), r.size() * 2, hipMemcpyHostToDevice));
  return MMPFN_OK;
}

// the matrix v into the given forms of w (a mask of Weight::Form)
template <typename H>
int fill(H* h, Weight& w, const std::vector<float>& v, unsigned forms) {
  if (forms & Weight::F32) RC(upload(h, w.f32, v));
  if (forms & Weight::BF16) RC(upload(h, w.bf16, v, DType::BF16));
  if (forms & Weight::F16) RC(upload(h, w.f16, v, DType::F16));
  if (forms & Weight::SPLIT) {
    const std::vector<uint16_t> planes = split_bf16(v);
    RC(ensure(h, w.split, planes.size() * 2));
    w.numel = (int64_t)v.size();
    HIPCHK_ON(h, hipMemcpy(w.split.p, planes.data(), planes.size() * 2, hipMemcpyHostToDevice));
  }
  return MMPFN_OK;
}

template <typename H>
const std::vector<float>* getw(H* h, const std::string& name, size_t numel) {
  auto it = h->host.find(name);
  if (it == h->host.end()) {
    h->err = "missing weight: " + name;
    return nullptr;
  }
  if (it->second.size() != numel) {
    h->err = "weight " + name + " has " + std::to_string(it->second.size()) + " elements, expected " +
             std::to_string(numel);
    return nullptr;
  }
  return &it->second;
}

#define GETW_ON(h, var, name, n)                          \
  const std::vector<float>* var = getw((h), (name), (n)); \
  if (!var) return MMPFN_ERR_WEIGHT;

}  // namespace mmpfn
