// The numerics monitor (vc_tensor_stats, vc_flux_set_monitor): per sample of a strided [B][rows][cols] tensor, bf16 or f32, the number
// of non-finite elements, the number of elements, max |x| and sum x^2 over the finite ones.  A read-once streaming pass: HBM-bound,
// 16-byte loads where the geometry allows, a capped grid.  There is no reference for it - the reference has no such check.
//
// The order of the sum (include/vcloze_hip.h states it too) is the two-pass reduction of block_reduce.h.  A row is cut into UNITS of
// E consecutive elements (E = 8 for bf16, 4 for f32 - 16 bytes; the last unit of a row is shorter where cols % E != 0), numbered row
// by row.  A thread adds s = s + x * x with the product rounded to f32 on its own (no fused multiply-add), a non-finite x skipped.
// The 16-byte and the element-wise path - the same units, loaded differently - give the same bits.  max |x| and the two counts do
// not depend on any order.
#include "common.h"
#include "vcloze_internal.h"
#include "block_reduce.h"
#include "monitor_sites.h"

namespace {

constexpr int MON_THREADS = 256;                      // = VC_MONITOR_MAX_BLOCKS: pass 2 reduces one partial per thread
static_assert(sizeof(VcStat) == 16, "a VcStat is one 16-byte store");

struct Acc { float mx, ss; uint32_t bad, cnt; };      // (no initialisers: it lives in LDS too)
struct AccOp {
  VC_DEV Acc operator()(Acc x, Acc y) const { return Acc{fmaxf(x.mx, y.mx), x.ss + y.ss, x.bad + y.bad, x.cnt + y.cnt}; }
};
VC_DEV void take(Acc& a, float v) {
#pragma clang fp contract(off)
  ++a.cnt;
  if ((__builtin_bit_cast(uint32_t, v) & 0x7f800000u) == 0x7f800000u) { ++a.bad; return; }     // inf / NaN: exponent all ones
  a.mx = fmaxf(a.mx, fabsf(v));
  const float sq = v * v;
  a.ss = a.ss + sq;
}

// pass 1: grid (nblk, B).  VEC: every unit is one aligned 16-byte load (cols % E == 0, the strides and the base allow it)
template <bool F32, bool VEC>
__global__ __launch_bounds__(MON_THREADS) void tensor_stats_kernel(const void* __restrict__ x, long bstride, long ld, int cols, uint32_t upr,
                                                                   uint32_t units, uint32_t* __restrict__ partial) {
  constexpr int E = F32 ? 4 : 8;
  __shared__ Acc l[MON_THREADS];
  const uint32_t nblk = gridDim.x, b = blockIdx.y;
  Acc a = {0.0f, 0.0f, 0u, 0u};
  for (uint64_t u64 = (uint64_t)blockIdx.x * MON_THREADS + threadIdx.x; u64 < units; u64 += (uint64_t)nblk * MON_THREADS) {
    const uint32_t u = (uint32_t)u64, row = u / upr, c0 = (u - row * upr) * E;
    const long off = (long)b * bstride + (long)row * ld + c0;
    if constexpr (VEC) {
      const u32x4 w = *(const u32x4*)((const char*)x + off * (F32 ? 4 : 2));
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const uint32_t wi = w[i];          // (a copy: __builtin_bit_cast of the vector element itself reads element 0 every time)
        if constexpr (F32) take(a, __builtin_bit_cast(float, wi));
        else { take(a, lo_bf(wi)); take(a, hi_bf(wi)); }
      }
    } else {
      const int n = (int)c0 + E <= cols ? E : cols - (int)c0;
      for (int i = 0; i < n; ++i) take(a, F32 ? ((const float*)x)[off + i] : bf2f(((const bf16_t*)x)[off + i]));
    }
  }
  a = block_tree(l, a, AccOp());
  if (threadIdx.x == 0) {
    uint32_t* p = partial + ((long)b * nblk + blockIdx.x) * 4;
    p[0] = __builtin_bit_cast(uint32_t, a.mx); p[1] = __builtin_bit_cast(uint32_t, a.ss); p[2] = a.bad; p[3] = a.cnt;
  }
}

// pass 2: grid (B); the sample's nblk <= 256 partials -> out[row * out_stride + b], row = *row_ptr (0 without one); a row outside
// [0, capacity) writes nothing
__global__ __launch_bounds__(MON_THREADS) void tensor_stats_finish_kernel(const uint32_t* __restrict__ partial, int nblk, u32x4* __restrict__ out,
                                                                          long out_stride, const int* __restrict__ row_ptr, int capacity) {
  __shared__ Acc l[MON_THREADS];
  const int b = blockIdx.x;
  Acc a = {0.0f, 0.0f, 0u, 0u};
  if ((int)threadIdx.x < nblk) {
    const uint32_t* p = partial + ((long)b * nblk + threadIdx.x) * 4;
    a.mx = __builtin_bit_cast(float, p[0]); a.ss = __builtin_bit_cast(float, p[1]); a.bad = p[2]; a.cnt = p[3];
  }
  a = block_tree(l, a, AccOp());
  if (threadIdx.x != 0) return;
  const int row = row_ptr ? *row_ptr : 0;
  if (row < 0 || row >= capacity) return;
  u32x4 o;
  o[0] = __builtin_bit_cast(uint32_t, a.mx); o[1] = __builtin_bit_cast(uint32_t, a.ss); o[2] = a.bad; o[3] = a.cnt;     // VcStat's fields in order
  out[(long)row * out_stride + b] = o;
}

// ONE block over the n entries of a log [evaluations][n_sites][B]: the entry with nonfinite != 0 that was WRITTEN first - evaluation by
// evaluation, within one the sites in the order of vcmon::site_rank (monitor_sites.h: the tap sites, then v, then x), then the samples
// - as its rank (evaluation * n_sites + site_rank) * B + sample -> out[0], or -1
__global__ __launch_bounds__(MON_THREADS) void first_bad_kernel(const u32x4* __restrict__ log, int n, int n_sites, int B, int* __restrict__ out) {
  __shared__ int l[MON_THREADS];
  int first = 0x7fffffff;
  for (int i = threadIdx.x; i < n; i += MON_THREADS) {
    if (log[i][2] == 0) continue;
    const int b = i % B, site = i / B % n_sites, ev = i / B / n_sites;
    first = min(first, (ev * n_sites + vcmon::site_rank(site, n_sites)) * B + b);
  }
  first = block_tree(l, first, [](int x, int y) { return min(x, y); });
  if (threadIdx.x == 0) out[0] = first == 0x7fffffff ? -1 : first;
}

}  // namespace

int vc_tensor_stats_launch(const void* x, int x_is_f32, int64_t bstride, int64_t ld, int B, int64_t rows, int cols, VcStat* out, int64_t out_stride,
                           const int32_t* row_ptr, int capacity, float* scratch, hipStream_t s, char* err, int errlen) {
  if (!x || !out || !scratch) { snprintf(err, errlen, "tensor_stats: null x / out / scratch"); return VC_ERR_ARG; }
  if (B <= 0 || B > 65535 || rows <= 0 || cols <= 0 || capacity <= 0 || bstride < 0) {
    snprintf(err, errlen, "tensor_stats: B = %d (1..65535), rows = %lld, cols = %d, capacity = %d must be positive, bstride = %lld not negative", B,
             (long long)rows, cols, capacity, (long long)bstride);
    return VC_ERR_ARG;
  }
  if (ld < cols) { snprintf(err, errlen, "tensor_stats: ld = %lld is smaller than cols = %d", (long long)ld, cols); return VC_ERR_ARG; }
  if (out_stride < B) { snprintf(err, errlen, "tensor_stats: out_stride = %lld is smaller than B = %d", (long long)out_stride, B); return VC_ERR_ARG; }
  const int esize = x_is_f32 ? 4 : 2, E = 16 / esize;
  if ((uintptr_t)out & 15) { snprintf(err, errlen, "tensor_stats: out must be 16-byte aligned (a VcStat is one 16-byte store)"); return VC_ERR_ARG; }
  if ((uintptr_t)x % esize || (uintptr_t)scratch & 3) { snprintf(err, errlen, "tensor_stats: x / scratch are not aligned to their elements"); return VC_ERR_ARG; }
  const int64_t upr = (cols + E - 1) / E, units = rows * upr;
  if (units > 0x7fffffff || rows * (int64_t)cols > 0xffffffffLL) {
    snprintf(err, errlen, "tensor_stats: rows = %lld x cols = %d per sample exceeds the 32-bit counts of a VcStat", (long long)rows, cols);
    return VC_ERR_ARG;
  }
  const bool vec = cols % E == 0 && ld % E == 0 && bstride % E == 0 && ((uintptr_t)x & 15) == 0;
  const int nblk = vc_reduce_blocks<MON_THREADS, VC_MONITOR_MAX_BLOCKS>(units);
  auto kernel = x_is_f32 ? (vec ? tensor_stats_kernel<true, true> : tensor_stats_kernel<true, false>)
                         : (vec ? tensor_stats_kernel<false, true> : tensor_stats_kernel<false, false>);
  hipLaunchKernelGGL(kernel, dim3(nblk, B), dim3(MON_THREADS), 0, s, x, (long)bstride, (long)ld, cols, (uint32_t)upr, (uint32_t)units,
                     (uint32_t*)scratch);
  hipLaunchKernelGGL(tensor_stats_finish_kernel, dim3(B), dim3(MON_THREADS), 0, s, (const uint32_t*)scratch, nblk, (u32x4*)out, (long)out_stride,
                     (const int*)row_ptr, capacity);
  return vc_launch_status("tensor_stats launch", err, errlen);
}

int vc_monitor_first_bad_launch(const VcStat* log, int64_t n, int n_sites, int B, int32_t* out, hipStream_t s, char* err, int errlen) {
  if (!log || !out || n_sites < 2 || B <= 0 || n <= 0 || n > 0x7fffffff || ((uintptr_t)log & 15)) { snprintf(err, errlen, "monitor_first_bad: bad args"); return VC_ERR_ARG; }
  hipLaunchKernelGGL(first_bad_kernel, dim3(1), dim3(MON_THREADS), 0, s, (const u32x4*)log, (int)n, n_sites, B, (int*)out);
  return vc_launch_status("monitor_first_bad launch", err, errlen);
}
