// What the handle engines (flux_engine.hip, vae_engine.hip, text_engine.hip, grid_engine.hip) share: error reporting, the workspace carve-up, stream
// capture and the run of a captured plan.  Host code only, for those four files alone (each gets its own internal copy): no
// kernel translation unit includes it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <algorithm>
#include <vector>
#include "../../include/vcloze_hip.h"
#include "plan_cache.h"

namespace {

struct Err {
  char* buf; int len;
};
#define FAIL(code, ...)                         \
  do {                                          \
    snprintf(e.buf, e.len, __VA_ARGS__);        \
    return code;                                \
  } while (0)
#define TRY(x)                \
  do {                        \
    int rc_ = (x);            \
    if (rc_ != VC_OK) return rc_; \
  } while (0)
#define HIP(x, what)                                                        \
  do {                                                                      \
    hipError_t he_ = (x);                                                   \
    if (he_ != hipSuccess) FAIL(VC_ERR_HIP, what ": %s", hipGetErrorString(he_)); \
  } while (0)
// the prologue of an ABI entry point (void* handle, ..., char* err, int errlen): `Err e` and the handle as `Type& var`
#define HANDLE(Type, var, prefix)                                        \
  Err e{err, errlen};                                                    \
  if (!handle) FAIL(VC_ERR_ARG, prefix ": null handle");                 \
  Type& var = *(Type*)handle

inline int64_t align256(int64_t v) { return (v + 255) & ~(int64_t)255; }
inline int pad_to(int n, int m) { return (n + m - 1) / m * m; }
inline bool aligned256(const void* p) { return p && !((uintptr_t)p & 255); }

// the carve-up of a workspace into 256-byte aligned buffers; a null base only adds up the sizes
struct Carver {
  char* base; int64_t off = 0;
  template <class T> T* take(int64_t count) {
    T* p = base ? (T*)(base + off) : nullptr;
    off += align256(count * (int64_t)sizeof(T));
    return p;
  }
  char* bytes(int64_t n) {   // an empty buffer has no address
    char* p = take<char>(n);
    return n ? p : nullptr;
  }
};

// capture what `issue` launches on `s` into an instantiated graph; *nodes (where given): the number of nodes of that graph
template <class F> int capture(hipStream_t s, hipGraphExec_t& out, Err e, F issue, int* nodes = nullptr) {
  HIP(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal), "hipStreamBeginCapture");
  const int rc = issue();
  hipGraph_t g = nullptr;
  hipError_t he = hipStreamEndCapture(s, &g);
  if (rc != VC_OK) { if (g) (void)hipGraphDestroy(g); return rc; }
  HIP(he, "hipStreamEndCapture");
  if (nodes) {
    size_t n = 0;
    if (hipGraphGetNodes(g, nullptr, &n) != hipSuccess) n = 0;
    *nodes = (int)n;
  }
  he = hipGraphInstantiate(&out, g, nullptr, nullptr, 0);
  (void)hipGraphDestroy(g);
  HIP(he, "hipGraphInstantiate");
  return VC_OK;
}
struct DropExec {
  void operator()(hipGraphExec_t ge) const { if (ge) (void)hipGraphExecDestroy(ge); }
};

// run `issue` as the plan of `key` (a PlanCache of hipGraphExec_t): un-captured on the default stream for a null stream, else ONE
// launch of its captured graph.  `warmed`: the plan shapes that have run un-captured once on this handle - the run that sets the
// kernels' attributes is needed once per set of launches, not once per set of argument pointers
template <class Cache, class Key, class Shape, class F>
int run_captured(Cache& cache, std::vector<Shape>& warmed, const Key& key, const Shape& shape, Err e, F issue) {
  if (!key.s) return issue();
  if (hipGraphExec_t* hit = cache.find(key)) {
    HIP(hipGraphLaunch(*hit, key.s), "hipGraphLaunch");
    return VC_OK;
  }
  if (std::find(warmed.begin(), warmed.end(), shape) == warmed.end()) {   // outside capture first: kernel attributes are set on a kernel's first launch
    TRY(issue());
    warmed.push_back(shape);
  }
  hipGraphExec_t ge = nullptr;
  TRY(capture(key.s, ge, e, issue));
  cache.insert(key, ge);
  HIP(hipGraphLaunch(ge, key.s), "hipGraphLaunch");
  return VC_OK;
}

}  // namespace
