// engine_internal.hpp -- what engine.cpp (models, densities, samplers, lowering) and draws.cpp (the calls over device-resident draws)
// share.  Not part of the C ABI.
#ifndef RH_ENGINE_INTERNAL_HPP
#define RH_ENGINE_INTERNAL_HPP

#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <functional>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/rainier_hip.h"
#include "rir.hpp"

struct Fail { int code; std::string msg; };
#define HIPCHK(expr)                                                                                   \
  do {                                                                                                 \
    hipError_t e_ = (expr);                                                                            \
    if (e_ != hipSuccess) throw Fail{RH_E_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_)}; \
  } while (0)

// device allocation released on scope exit (also when a HIP call throws)
struct DevBuf {
  void *p = nullptr;
  explicit DevBuf(size_t bytes) { hipError_t e = hipMalloc(&p, bytes ? bytes : 8); if (e != hipSuccess) throw Fail{RH_E_DEVICE, std::string("hipMalloc: ") + hipGetErrorString(e)}; }
  ~DevBuf() { if (p) (void)hipFree(p); }
  DevBuf(const DevBuf &) = delete;
  DevBuf &operator=(const DevBuf &) = delete;
};

// ---- defined in engine.cpp ----
extern const char *const kSharedSrc, *const kPreludeSrc;   // device/rh_shared.h, device/rh_prelude.hip.h as text
std::string &thread_err();                                 // what rh_last_error(NULL) reports on this thread
int guard(rh_model *m, const std::function<void()> &fn);   // Fail -> return code, the message to thread_err() and to m->err
std::vector<char> build_source(const std::string &arch, const std::string &source, const std::string &extra = std::string(), const char *suffix = ".hsaco");
enum { KH_ABSENT = 0, KH_OK = 1, KH_BAD = 2 };
int kernel_health(const std::vector<char> &code, const std::string &name, std::string *why = nullptr);
// what draws.cpp needs of a sampler; draws: device pointer, [chains][iterations][nvars], iterations: the buffer's allocated extent
struct DrawsView { const void *draws; int device; hipStream_t stream; int chains, it_done, nvars; long long iterations; std::mutex *mu; std::string *err; rh_model *model; };
DrawsView sampler_draws(rh_sampler *s);

// ---- one copy each of what every call over a device needs ----
inline void launch(hipFunction_t f, unsigned grid, unsigned block, hipStream_t s, void **args) {
  HIPCHK(hipModuleLaunchKernel(f, grid, 1, 1, block, 1, 1, 0, s, args, nullptr));
}
inline std::string device_arch(int dev) {
  hipDeviceProp_t prop;
  HIPCHK(hipGetDeviceProperties(&prop, dev));
  const std::string arch = prop.gcnArchName;
  return arch.substr(0, arch.find(':'));
}
// compute units of a device (4 SIMDs each)
inline int device_cus(int dev) {
  int cus = 0;
  HIPCHK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  return cus;
}
// -1: the current device; makes the device current and returns its ordinal
inline int use_device(int device, const char *fn) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) throw Fail{RH_E_DEVICE, "no HIP device available: the engine has no CPU fallback"};
  if (device < 0) HIPCHK(hipGetDevice(&device));
  if (device >= ndev) throw Fail{RH_E_INVALID, std::string(fn) + ": no such device"};
  HIPCHK(hipSetDevice(device));
  return device;
}
// every kernel of `kernels` is in `code`, passes kernel_health, spills nothing and uses no scratch; `what` opens the message
inline void require_clean(const std::vector<char> &code, const std::vector<std::string> &kernels, const std::string &what) {
  for (const std::string &k : kernels) {
    std::string why;
    if (kernel_health(code, k, &why) != KH_OK) throw Fail{RH_E_UNSUPPORTED, what + (why.empty() ? k + " is missing" : why)};
    rh::KernelMeta km;
    if (!rh::kernel_meta(code, k, km) || km.vgpr_spills != 0 || km.sgpr_spills != 0 || km.scratch_bytes != 0 || rh::kernel_touches_scratch(code, k) != 0)
      throw Fail{RH_E_UNSUPPORTED, what + k + ": spilled registers or scratch memory"};
  }
}
// a malloc'ed copy of a code object for the caller (freed with rh_free)
inline void copy_out(const std::vector<char> &code, void **out, size_t *size) {
  if (size) *size = code.size();
  if (out) { *out = std::malloc(code.size()); std::memcpy(*out, code.data(), code.size()); }
}
#endif
