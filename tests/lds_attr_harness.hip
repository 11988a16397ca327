// rp::LdsAttr (csrc/row_panel.h) on the CPU (tests/test_lds_attr.py): the "set the dynamic-LDS attribute once per device, retry after a
// failure, mark the device done only after success" logic that a passing GPU run never exercises.  LdsAttr::set_on takes the device
// index and the attribute call from its caller; this program passes fakes that count their calls and fail on demand.  No GPU is used
// and no kernel is launched: the only HIP call reached is hipGetErrorString.  Built with the host sanitizers
// (-Xarch_host -fsanitize=address,undefined) and run as a program of its own.  Exit status 0 and "ok" = every check held; otherwise one
// line per failed check and status 1.
#include <stdio.h>
#include <string.h>

#include <string>

#include "../followyourclick_amd/csrc/row_panel.h"

thread_local char g_fyc_err[512];          // (csrc/api.hip owns it in the library)

namespace {
int g_failed = 0;
#define CHECK(cond) do { if (!(cond)) { printf("line %d: %s\n", __LINE__, #cond); ++g_failed; } } while (0)

struct Fake {                              // the attribute call: counts, remembers its last arguments, fails from call `fail_from` on
  int calls = 0, fail_from = 1 << 30, last_bytes = 0;
  const void* last_kernel = nullptr;
  hipError_t operator()(const void* k, int bytes) {
    last_kernel = k; last_bytes = bytes;
    return ++calls >= fail_from ? hipErrorInvalidValue : hipSuccess;
  }
};
const char k_a = 0, k_b = 0;               // stand-ins for two kernels' addresses
const void* const KERNELS[2] = {&k_a, &k_b};
}  // namespace

int main() {
  const std::string refused = std::string("fyc_x: 4096 bytes of dynamic LDS refused: ") + hipGetErrorString(hipErrorInvalidValue);
  {  // a failing setter: -3, the formatted message, and it is called again at the next launch - until it succeeds, then never again
    rp::LdsAttr attr;
    Fake f; f.fail_from = 1;
    auto call = [&](int dev) { return attr.set_on(dev, "fyc_x", 4096, KERNELS, 2, [&](const void* k, int b) { return f(k, b); }); };
    g_fyc_err[0] = 0;
    CHECK(call(0) == -3);
    CHECK(refused == g_fyc_err);
    CHECK(f.calls == 1 && f.last_kernel == &k_a && f.last_bytes == 4096);     // the second kernel is not tried after the first one failed
    g_fyc_err[0] = 0;
    CHECK(call(0) == -3 && f.calls == 2 && refused == g_fyc_err);             // retried
    f.fail_from = 4;                                                           // call 3 (first kernel) passes, call 4 (second kernel) fails
    CHECK(call(0) == -3 && f.calls == 4 && f.last_kernel == &k_b);            // a failure of the second kernel is a failure too
    f.fail_from = 1 << 30;
    g_fyc_err[0] = 0;
    CHECK(call(0) == 0 && f.calls == 6 && g_fyc_err[0] == 0);                 // both kernels set: the device is done
    CHECK(call(0) == 0 && f.calls == 6);
    CHECK(call(1) == 0 && f.calls == 8);                                      // another device has its own flag
  }
  {  // a succeeding setter: once per kernel and device index, never again
    rp::LdsAttr attr;
    Fake f;
    auto call = [&](int dev) { return attr.set_on(dev, "fyc_x", 4096, KERNELS, 2, [&](const void* k, int b) { return f(k, b); }); };
    for (int round = 0; round < 3; ++round)
      for (int dev = 0; dev < 64; ++dev) CHECK(call(dev) == 0);
    CHECK(f.calls == 2 * 64);
    // device indices outside [0, 64): served, not remembered - the setter runs at every launch
    const int before = f.calls;
    CHECK(call(64) == 0 && call(64) == 0 && call(-1) == 0 && call(-1) == 0 && call(1 << 20) == 0);
    CHECK(f.calls == before + 2 * 5);
    f.fail_from = 0;
    CHECK(call(64) == -3 && refused == g_fyc_err);                            // ... and its failure is reported like any other
    CHECK(call(63) == 0);                                                     // (a tracked device stays done)
  }
  {  // two objects (two launch sites, or two instantiations of a templated launcher) share nothing
    rp::LdsAttr a, b;
    Fake f;
    auto set = [&](const void* k, int bytes) { return f(k, bytes); };
    CHECK(a.set_on(0, "fyc_x", 4096, KERNELS, 1, set) == 0 && f.calls == 1);
    CHECK(b.set_on(0, "fyc_x", 4096, KERNELS, 1, set) == 0 && f.calls == 2);
    CHECK(a.set_on(0, "fyc_x", 4096, KERNELS, 1, set) == 0 && b.set_on(0, "fyc_x", 4096, KERNELS, 1, set) == 0 && f.calls == 2);
  }
  {  // the alignment predicate of the FYC_REQUIREs: null counts as aligned, any one misaligned pointer fails it
    alignas(16) static char buf[64];
    const float* none = nullptr;
    CHECK(rp::aligned16(buf, buf + 16, none, (const double*)(buf + 32)));
    CHECK(!rp::aligned16(buf, buf + 8) && !rp::aligned16(buf + 4) && !rp::aligned16(buf, none, buf + 17));
  }
  if (g_failed == 0) printf("ok\n");
  return g_failed ? 1 : 0;
}
