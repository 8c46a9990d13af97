// vc_resample_u8: separable resampling of an 8-bit [H, W, 3] image with a bicubic or Lanczos-3 filter in fixed point - the rule of
// include/vcloze_hip.h (the resampling section), which is what Pillow's Image.resize does for 8-bit images, so a resized photograph
// leaves here with Pillow's bytes.  Two parts:
//   host    the coefficient tables of one axis (xmin, len, integer weights per output index), built in double with libm and staged
//           through pinned memory into the caller's `tmp` on the caller's stream (vc_resample_coeffs is the same builder, host-only);
//   device  one thread per output pixel, three int32 accumulators; the horizontal pass writes an 8-bit intermediate [H, w, 3], the
//           vertical pass reads it.  Memory-bound and tiny next to a model evaluation: plain integer C++, no LDS, not tuned.
// The host part restates double arithmetic operation by operation: no multiply-add may be contracted (Makefile: RULES_FLAGS).
#include "common.h"
#include "vcloze_internal.h"
#include <math.h>
#include <string.h>
#include <mutex>
#include <vector>

#pragma STDC FP_CONTRACT OFF

namespace {

constexpr int PRECISION_BITS = 32 - 8 - 2;     // 22: an 8-bit pixel times a weight of magnitude < 2 fits int32 with room for the sum

double bicubic_filter(double x) {
#pragma clang fp contract(off)
  const double a = -0.5;
  if (x < 0.0) x = -x;
  if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
  if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
  return 0.0;
}
double sinc_filter(double x) {
#pragma clang fp contract(off)
  if (x == 0.0) return 1.0;
  x = x * M_PI;
  return sin(x) / x;
}
double lanczos_filter(double x) {
#pragma clang fp contract(off)
  if (-3.0 <= x && x < 3.0) return sinc_filter(x) * sinc_filter(x / 3);
  return 0.0;
}

bool filter_ok(int filter) { return filter == VC_FILTER_BICUBIC || filter == VC_FILTER_LANCZOS; }
bool size_ok(int n) { return n >= 1 && n <= 65535; }

struct Axis {
  double scale, filterscale, support;
  int kmax;
};
Axis axis_of(int in, int out, int filter) {
#pragma clang fp contract(off)
  Axis a;
  a.scale = (double)in / out;
  a.filterscale = a.scale < 1.0 ? 1.0 : a.scale;
  a.support = (filter == VC_FILTER_LANCZOS ? 3.0 : 2.0) * a.filterscale;
  a.kmax = (int)ceil(a.support) * 2 + 1;
  return a;
}

// the tables of one axis: xmin[out], len[out], ki[out][kmax] (entries past len are 0)
void build_tables(int in, int out, int filter, int32_t* xmin, int32_t* len, int32_t* ki) {
#pragma clang fp contract(off)
  const Axis a = axis_of(in, out, filter);
  const double ss = 1.0 / a.filterscale;
  std::vector<double> k((size_t)a.kmax);
  for (int xx = 0; xx < out; ++xx) {
    const double center = (xx + 0.5) * a.scale;
    int lo = (int)(center - a.support + 0.5);
    if (lo < 0) lo = 0;
    int hi = (int)(center + a.support + 0.5);
    if (hi > in) hi = in;
    const int n = hi - lo;
    double ww = 0.0;
    for (int x = 0; x < n; ++x) {
      const double arg = (x + lo - center + 0.5) * ss;
      const double w = filter == VC_FILTER_LANCZOS ? lanczos_filter(arg) : bicubic_filter(arg);
      k[x] = w;
      ww += w;
    }
    int32_t* row = ki + (size_t)xx * a.kmax;
    for (int x = 0; x < a.kmax; ++x) {
      if (x >= n) { row[x] = 0; continue; }
      const double v = ww != 0.0 ? k[x] / ww : k[x];
      row[x] = v < 0 ? (int32_t)(-0.5 + v * (1 << PRECISION_BITS)) : (int32_t)(0.5 + v * (1 << PRECISION_BITS));
    }
    xmin[xx] = lo;
    len[xx] = n;
  }
}

int64_t up256(int64_t v) { return (v + 255) & ~(int64_t)255; }
int64_t table_bytes(int in, int out, int filter) {       // 0 for a pass that is skipped
  return in == out ? 0 : up256(((int64_t)2 * out + (int64_t)out * axis_of(in, out, filter).kmax) * 4);
}

// Pinned staging for the table uploads.  A buffer serves again once the copy that read it has finished (its event says so), so a
// call never waits for the stream unless VC_STAGES uploads are all still in flight.
// Lifetime: at most VC_STAGES buffers (64 KiB each, or the largest table set asked for) per PROCESS, allocated on first use, kept
// until the process ends and never handed out of this file; g_stage_mu guards them, so calls from several threads serialise on the
// table build.  Several devices: a slot remembers the device its event was recorded on and is taken for another device only when no
// slot is empty or ready for the caller's - after waiting for its copy - and is then freed and allocated again under the current
// device, so an event is only ever recorded on a stream of the device it was created on.  (A pinned allocation per call would
// need no ring, but hipHostMalloc / hipHostFree cost more than the whole resample and the free waits for the device.)
constexpr int VC_STAGES = 8;
struct Stage {
  void* p = nullptr;
  size_t cap = 0;
  hipEvent_t ev = nullptr;
  int dev = -1;
};
std::mutex g_stage_mu;
Stage g_stage[VC_STAGES];
unsigned g_stage_next = 0;

hipError_t stage_acquire(size_t bytes, Stage** out) {
  const int dev = vc_device_index();
  Stage* pick = nullptr;
  for (int i = 0; i < VC_STAGES && !pick; ++i) {
    Stage& s = g_stage[i];
    if (!s.p) pick = &s;
    else if (s.dev == dev && hipEventQuery(s.ev) == hipSuccess) pick = &s;
  }
  if (!pick) {                                  // all in flight: wait for the oldest
    pick = &g_stage[g_stage_next++ % VC_STAGES];
    hipError_t e = hipEventSynchronize(pick->ev);
    if (e != hipSuccess) return e;
  }
  (void)hipGetLastError();                      // hipEventQuery's hipErrorNotReady is no error of ours
  if (pick->p && (pick->cap < bytes || pick->dev != dev)) {
    (void)hipHostFree(pick->p);
    (void)hipEventDestroy(pick->ev);
    *pick = Stage{};
  }
  if (!pick->p) {
    const size_t cap = bytes < 65536 ? 65536 : bytes;
    hipError_t e = hipHostMalloc(&pick->p, cap, hipHostMallocDefault);
    if (e != hipSuccess) { *pick = Stage{}; return e; }
    e = hipEventCreateWithFlags(&pick->ev, hipEventDisableTiming);
    if (e != hipSuccess) { (void)hipHostFree(pick->p); *pick = Stage{}; return e; }
    pick->cap = cap;
    pick->dev = dev;
  }
  *out = pick;
  return hipSuccess;
}

// HORIZONTAL: dst [rows, out_w, 3] from src [rows, in_w, 3]; consecutive threads take consecutive output columns of a row, so their
// table rows are consecutive.  VERTICAL: dst [out_h, cols, 3] from src [in_h, cols, 3]; a wave shares one table row.
template <bool VERTICAL>
__global__ void resample_kernel(const unsigned char* __restrict__ src, unsigned char* __restrict__ dst, int in_n, int out_n, int other,
                                const int32_t* __restrict__ xmin, const int32_t* __restrict__ len, const int32_t* __restrict__ ki, int kmax) {
  const long total = (long)out_n * other;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  int o, line;                                   // o: index along the resampled axis; line: index along the other one
  long base, stride;                             // byte address of the first tap and the step between taps
  if (VERTICAL) {
    o = (int)(i / other);
    line = (int)(i % other);
    base = ((long)xmin[o] * other + line) * 3;
    stride = (long)other * 3;
  } else {
    line = (int)(i / out_n);
    o = (int)(i % out_n);
    base = ((long)line * in_n + xmin[o]) * 3;
    stride = 3;
  }
  const int n = len[o];                          // xmin + len <= in_n by construction: every tap lies inside src
  const int32_t* k = ki + (long)o * kmax;
  int32_t s0 = 1 << (PRECISION_BITS - 1), s1 = s0, s2 = s0;
  for (int t = 0; t < n; ++t) {
    const unsigned char* p = src + base + t * stride;
    const int32_t w = k[t];
    s0 += (int32_t)p[0] * w;
    s1 += (int32_t)p[1] * w;
    s2 += (int32_t)p[2] * w;
  }
  s0 >>= PRECISION_BITS;                         // arithmetic shift
  s1 >>= PRECISION_BITS;
  s2 >>= PRECISION_BITS;
  unsigned char* q = dst + i * 3;                // both layouts: output pixel i of a dense [.., .., 3] array
  q[0] = (unsigned char)(s0 < 0 ? 0 : s0 > 255 ? 255 : s0);
  q[1] = (unsigned char)(s1 < 0 ? 0 : s1 > 255 ? 255 : s1);
  q[2] = (unsigned char)(s2 < 0 ? 0 : s2 > 255 ? 255 : s2);
}

bool overlap(const void* a, int64_t an, const void* b, int64_t bn) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + (uintptr_t)bn && y < x + (uintptr_t)an;
}

}  // namespace

int vc_resample_kmax_impl(int in, int out, int filter, char* err, int errlen) {
  if (!size_ok(in) || !size_ok(out)) { snprintf(err, errlen, "resample_kmax: sizes %d -> %d must lie in 1..65535", in, out); return VC_ERR_ARG; }
  if (!filter_ok(filter)) { snprintf(err, errlen, "resample_kmax: unknown filter %d (VC_FILTER_BICUBIC, VC_FILTER_LANCZOS)", filter); return VC_ERR_ARG; }
  return axis_of(in, out, filter).kmax;
}

int vc_resample_coeffs_impl(int in, int out, int filter, int32_t* xmin, int32_t* len, int32_t* ki, int kmax, char* err, int errlen) {
  if (!xmin || !len || !ki) { snprintf(err, errlen, "resample_coeffs: null pointer"); return VC_ERR_ARG; }
  const int need = vc_resample_kmax_impl(in, out, filter, err, errlen);
  if (need < 0) return need;
  if (kmax != need) { snprintf(err, errlen, "resample_coeffs: kmax = %d, vc_resample_kmax(%d, %d, %d) = %d expected", kmax, in, out, filter, need); return VC_ERR_ARG; }
  build_tables(in, out, filter, xmin, len, ki);
  return VC_OK;
}

int64_t vc_resample_tmp_bytes_impl(int H, int W, int h, int w, int filter, char* err, int errlen) {
  if (!size_ok(H) || !size_ok(W) || !size_ok(h) || !size_ok(w)) {
    snprintf(err, errlen, "resample: sizes %dx%d -> %dx%d (height x width) must lie in 1..65535", H, W, h, w);
    return VC_ERR_ARG;
  }
  if (!filter_ok(filter)) { snprintf(err, errlen, "resample: unknown filter %d (VC_FILTER_BICUBIC, VC_FILTER_LANCZOS)", filter); return VC_ERR_ARG; }
  const int64_t inter = (W != w && H != h) ? up256((int64_t)H * w * 3) : 0;
  const int64_t n = table_bytes(W, w, filter) + table_bytes(H, h, filter) + inter;
  return n ? n : 256;                           // never 0: the caller always has something to pass
}

int vc_resample_u8_launch(const void* src, int H, int W, void* dst, int h, int w, int filter, void* tmp, int64_t tmp_bytes, hipStream_t s,
                          char* err, int errlen) {
  if (!src || !dst || !tmp) { snprintf(err, errlen, "resample_u8: null pointer"); return VC_ERR_ARG; }
  const int64_t need = vc_resample_tmp_bytes_impl(H, W, h, w, filter, err, errlen);
  if (need < 0) return (int)need;
  if (tmp_bytes < need) { snprintf(err, errlen, "resample_u8: tmp too small (%lld < %lld bytes)", (long long)tmp_bytes, (long long)need); return VC_ERR_ARG; }
  if ((uintptr_t)tmp & 255) { snprintf(err, errlen, "resample_u8: tmp must be 256-byte aligned"); return VC_ERR_ARG; }
  const int64_t sb = (int64_t)H * W * 3, db = (int64_t)h * w * 3;
  if (overlap(src, sb, dst, db) || overlap(src, sb, tmp, tmp_bytes) || overlap(dst, db, tmp, tmp_bytes)) {
    snprintf(err, errlen, "resample_u8: src, dst and tmp must not overlap");
    return VC_ERR_ARG;
  }
#define VC_RS_HIP(x, what)                                                                     \
  do {                                                                                         \
    hipError_t he_ = (x);                                                                      \
    if (he_ != hipSuccess) { snprintf(err, errlen, what ": %s", hipGetErrorString(he_)); return VC_ERR_HIP; } \
  } while (0)
  if (H == h && W == w) {
    VC_RS_HIP(hipMemcpyAsync(dst, src, (size_t)sb, hipMemcpyDeviceToDevice, s), "resample_u8 hipMemcpyAsync");
    return VC_OK;
  }
  const bool hor = W != w, ver = H != h;
  const int64_t hb = table_bytes(W, w, filter), vb = table_bytes(H, h, filter);
  char* base = (char*)tmp;
  unsigned char* inter = (unsigned char*)(base + hb + vb);
  {
    std::lock_guard<std::mutex> lock(g_stage_mu);
    Stage* st = nullptr;
    VC_RS_HIP(stage_acquire((size_t)(hb + vb), &st), "resample_u8 pinned staging");
    char* host = (char*)st->p;
    if (hor) { int32_t* t = (int32_t*)host; build_tables(W, w, filter, t, t + w, t + 2 * (size_t)w); }
    if (ver) { int32_t* t = (int32_t*)(host + hb); build_tables(H, h, filter, t, t + h, t + 2 * (size_t)h); }
    VC_RS_HIP(hipMemcpyAsync(base, host, (size_t)(hb + vb), hipMemcpyHostToDevice, s), "resample_u8 hipMemcpyAsync(tables)");
    VC_RS_HIP(hipEventRecord(st->ev, s), "resample_u8 hipEventRecord");
  }
  const dim3 block(256);
  if (hor) {
    const int32_t* t = (const int32_t*)base;
    unsigned char* out = ver ? inter : (unsigned char*)dst;
    const long total = (long)H * w;
    hipLaunchKernelGGL((resample_kernel<false>), dim3((unsigned)((total + 255) / 256)), block, 0, s, (const unsigned char*)src, out, W, w, H, t,
                       t + w, t + 2 * (size_t)w, axis_of(W, w, filter).kmax);
  }
  if (ver) {
    const int32_t* t = (const int32_t*)(base + hb);
    const unsigned char* in = hor ? inter : (const unsigned char*)src;
    const long total = (long)h * w;
    hipLaunchKernelGGL((resample_kernel<true>), dim3((unsigned)((total + 255) / 256)), block, 0, s, in, (unsigned char*)dst, H, h, w, t, t + h,
                       t + 2 * (size_t)h, axis_of(H, h, filter).kmax);
  }
#undef VC_RS_HIP
  return vc_launch_status("resample_u8 launch", err, errlen);
}
