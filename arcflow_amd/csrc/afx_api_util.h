// Error plumbing shared by the extern "C" translation units.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/arcflow_hip.h"

extern thread_local char afx_g_err[512];
int afx_fail(int code, const char* fmt, ...);
#define fail afx_fail

#define HIP_TRY(expr)                                                                           \
  do {                                                                                          \
    hipError_t e_ = (expr);                                                                     \
    if (e_ != hipSuccess) return fail(AFX_E_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
  } while (0)

#define AFX_TRY(expr) do { const int rc_ = (expr); if (rc_ != AFX_OK) return rc_; } while (0)

// [a, a + an) and [b, b + bn) share a byte (a null range shares nothing)
static inline bool ranges_overlap(const void* a, int64_t an, const void* b, int64_t bn) {
  if (a == nullptr || b == nullptr) return false;
  const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
  return pa < pb + (uintptr_t)bn && pb < pa + (uintptr_t)an;
}
