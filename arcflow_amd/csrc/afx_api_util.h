// Error plumbing and entry helpers shared by the extern "C" translation units.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <initializer_list>

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

// one of the pointers (NULL ones pass) is not 16-byte aligned
static inline bool misaligned16(std::initializer_list<const void*> ptrs) {
  uintptr_t bits = 0;
  for (const void* p : ptrs) bits |= (uintptr_t)p;
  return (bits & 15) != 0;
}

// Launch of a streaming step kernel (the teacher-sampler steps, afx_sampler.hip, and the edit blend, afx_edit.hip): one lane per chunk of
// 8 consecutive elements, 256 lanes per work-group, grid-stride over `batch` samples of n elements; the kernel's last two parameters are
// (chunks_per_sample, chunks).  max_blocks > 0 caps the grid; the default cap of 2048 is 8 work-groups per CU (256 CUs), which hide the
// load latency of a streaming pass -- more only add launch work.
template <typename... P, typename... A>
static int launch_step(void (*kernel)(P...), int32_t batch, int64_t n, int32_t max_blocks, void* stream, A... args) {
  const int64_t cps = n / 8, chunks = cps * batch;
  const int64_t cap = max_blocks > 0 ? max_blocks : 2048;
  const unsigned grid = (unsigned)std::min<int64_t>((chunks + 255) / 256, cap);
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, args..., cps, chunks);
  HIP_TRY(hipGetLastError());
  return AFX_OK;
}

// work-groups of 256 lanes that cover n units of work
static inline unsigned blocks_for(int64_t n) { return (unsigned)((n + 255) / 256); }

// Launch of a kernel with one lane per unit of work: n units on blocks_for(n) work-groups of 256; n == 0 launches nothing.
template <typename... P, typename... A>
static int launch_flat(void (*kernel)(P...), int64_t n, void* stream, A... args) {
  if (n == 0) return AFX_OK;
  hipLaunchKernelGGL(kernel, dim3(blocks_for(n)), dim3(256), 0, (hipStream_t)stream, args...);
  HIP_TRY(hipGetLastError());
  return AFX_OK;
}

// ... and of one on a grid the entry lays out itself (a row per wave or per work-group, 2-D tiles), work-groups of 256
template <typename... P, typename... A>
static int launch_grid(void (*kernel)(P...), dim3 grid, void* stream, A... args) {
  hipLaunchKernelGGL(kernel, grid, dim3(256), 0, (hipStream_t)stream, args...);
  HIP_TRY(hipGetLastError());
  return AFX_OK;
}

// The LoRA-dropout constants of a drop probability 0 <= p < 1: an element is kept where its hash (lora_drop_keep, afx_common.h) is at
// least thresh, and kept elements are scaled by inv_keep
struct DropConsts { uint32_t thresh; float inv_keep; };
static inline DropConsts drop_consts(float p) { return {(uint32_t)((double)p * 4294967296.0), 1.0f / (1.0f - p)}; }

// The value of a *_ws_bytes entry: `batch` samples x `parts` slots of K doubles, or the refusal (negative) by the entry's name.
static inline int64_t ws_bytes_or_fail(const char* name, bool bad, const char* rule, int32_t batch, int64_t parts, int K) {
  if (bad) return (int64_t)fail(AFX_E_INVALID, "bad argument to %s%s", name, rule);
  if (parts > INT32_MAX) return (int64_t)fail(AFX_E_INVALID, "%s: more than 2^31 - 1 tiles per sample", name);
  return (int64_t)batch * parts * K * (int64_t)sizeof(double);
}
