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
  size_t n = 0;  // elements (split weight planes: elements per plane)
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p(o.p), bytes(o.bytes), n(o.n) { o.p = nullptr, o.bytes = o.n = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) {
      reset();
      p = o.p, bytes = o.bytes, n = o.n;
      o.p = nullptr, o.bytes = o.n = 0;
    }
    return *this;
  }
  ~DevBuf() { reset(); }
  void reset() {  // teardown: an error here has no caller to report to
    if (p) (void)hipFree(p);
    p = nullptr, bytes = n = 0;
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
