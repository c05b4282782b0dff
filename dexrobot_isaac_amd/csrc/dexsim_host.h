// dexsim_host.h -- what the host code of libdexsim's two translation units (dexsim.hip, dexsim_queries.hip) shares: the handle,
// the guards of an entry point and the error record.  Internal to the library; the ABI is include/dexsim.h.
#pragma once
#include "dexsim_device.h"

// The error record: one thread_local string, defined in dexsim.hip with these two functions (hidden: not part of the ABI).
// fail: store `what` as the thread's last error, return `code`.
__attribute__((visibility("hidden"))) int fail(int code, const char* what);
// fail_hip: store "<expr>: <HIP's error string>", return DEXSIM_ERR_HIP (HIP_TRY's failure branch).
__attribute__((visibility("hidden"))) int fail_hip(const char* expr, hipError_t e);

#define HIP_TRY(expr)                                  \
  do {                                                 \
    hipError_t _e = (expr);                            \
    if (_e != hipSuccess) return fail_hip(#expr, _e);  \
  } while (0)

struct DexSim {
  DexSimConfig cfg;
  DexHandModel model;
  int device;
  int N;  // real envs
  int NS; // padded to a multiple of 64: arena stride, every lane of every wavefront owns an env
  DevParams* d_params;
  Arena arena;
  ApiPtrs api;
  bool bound;
  bool model_struct;           // the model has the structure of the specialised chain forms: the MS step kernels (dexsim_create)
  hipEvent_t ev0, ev1;
  const float* last_actions;   // device pointer of the last dexsim_step (DEXSIM_STAGE_STEP re-launches the same kernel)
  hipEvent_t tev[128];         // dexsim_step_timing: ring of 64 (start, stop) pairs
  int timing;                  // 0 = off, else 1 + number of steps recorded since it was switched on
};

inline int padded(int n) { return (n + 63) / 64 * 64; }

// Every entry point runs on the handle's device whatever the caller's current device is, and restores the caller's.
struct DeviceGuard {
  int prev = -1; bool switched = false;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) == hipSuccess && prev != dev) switched = hipSetDevice(dev) == hipSuccess;
  }
  ~DeviceGuard() { if (switched) (void)hipSetDevice(prev); }
};

#define NEED_BOUND(h)                                                        \
  if (!(h)) return fail(DEXSIM_ERR_ARG, "null handle");                      \
  if (!(h)->bound) return fail(DEXSIM_ERR_NOT_BOUND, "dexsim_bind has not been called"); \
  DeviceGuard _device_guard((h)->device)
#define LAUNCH_CHECK() HIP_TRY(hipGetLastError())
