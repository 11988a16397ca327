// The host side of a launch with more than 64 KB of dynamic LDS, shared by the row-panel kernels (row_panel.h) and the GEMM family (gemm_kernel.h).  Host only.
#pragma once
#include <mutex>

#include "fyc_common.h"

namespace rp {

// Dynamic LDS above 64 KB needs hipFuncAttributeMaxDynamicSharedMemorySize on the kernel once per device; one process may drive
// several GPUs from several threads.  One object per launch site, as a function-local static (so a templated launcher keeps one
// per instantiation): `if (int rc = attr.set("fyc_x", LDS_BYTES, kernel<a>, kernel<b>)) return rc;`
class LdsAttr {
 public:
  template <typename... K>
  int set(const char* name, int bytes, K*... kernels) {
    const void* ks[] = {reinterpret_cast<const void*>(kernels)...};
    int dev = 0;
    (void)hipGetDevice(&dev);
    return set_on(dev, name, bytes, ks, (int)sizeof...(K),
                  [](const void* k, int b) { return hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, b); });
  }
  // the logic behind set(), with the device index and the attribute call handed in (tests/lds_attr_harness.hip passes fakes).
  // A device index outside [0, MAX_DEV) is served, but not remembered: its attribute is set at every launch.
  template <typename Setter>
  int set_on(int dev, const char* name, int bytes, const void* const* kernels, int n, Setter setter) {
    const bool tracked = dev >= 0 && dev < MAX_DEV;
    std::lock_guard<std::mutex> lk(mu_);
    if (tracked && done_[dev]) return 0;
    hipError_t e = hipSuccess;
    for (int i = 0; i < n && e == hipSuccess; ++i) e = setter(kernels[i], bytes);
    if (e != hipSuccess) FYC_FAIL(-3, "%s: %d bytes of dynamic LDS refused: %s", name, bytes, hipGetErrorString(e));
    if (tracked) done_[dev] = true;            // only after success: a failed call is retried at the next launch
    return 0;
  }

 private:
  static constexpr int MAX_DEV = 64;
  std::mutex mu_;
  bool done_[MAX_DEV] = {};
};

}  // namespace rp
