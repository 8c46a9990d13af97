// The flow-matching loss of ONE model evaluation (include/vcloze_hip.h: vc_fm_plan, vc_fm_loss) - Transport.training_losses
// (transport.py:132-176) for the Linear path and velocity prediction, forward only: the path sample in front of the evaluation and the
// masked squared error behind it.  Two read-once streaming passes over B * rows * cols elements: HBM-bound, 16-byte accesses where
// the geometry allows, capped grids.
//   fm_plan   x_t = t x1 + (1 - t) x0 -> bf16, straight into the first `cols` columns of the model-input rows (the cond columns beside
//             them are the caller's);  u_t = x1 - x0 -> f32.  x0 is a tensor, or drawn in place from THE STREAM (rng_device.h): no
//             draw launch, no stored x0.  f32 arithmetic, one operation after the other, no fused multiply-add.
//   fm_loss   loss[b] = sum over the first valid[b] rows and all cols of ((-out) - u_t)^2 / (valid[b] * cols), summed in f32 in the
//             FIXED ORDER of block_reduce.h, over the units of vc_tensor_stats (monitor.hip): a row is cut into units of 8
//             consecutive elements (the last unit of a row is shorter where cols % 8 != 0); the units of the sample's VALID rows,
//             numbered row by row, are the ones summed, while nblk comes from ALL rows (one grid serves every sample); a thread
//             adds s = s + d * d with the product rounded on its own.  The 16-byte and the element-wise path give the same bits.
#include "common.h"
#include "vcloze_internal.h"
#include "block_reduce.h"
#include "rng_device.h"

namespace {

constexpr int FM_THREADS = 256;
constexpr int FM_PLAN_MAX_BLOCKS = 2048;      // 8 workgroups of 256 per CU of a 256-CU device; the grid-stride loop takes the rest

struct FmPair { float xt, ut; };
// one element, f32, one operation after the other: t * x1.float() + (1 - t) * x0.float() and x1.float() - x0.float() in torch
VC_DEV FmPair fm_element(float t, float omt, float x1, float x0) {
#pragma clang fp contract(off)
  const float a = t * x1;
  const float c = omt * x0;
  return FmPair{a + c, x1 - x0};
}

// VEC: work item = 8 consecutive elements of a row (every base and stride allows 16-byte accesses, cols % 8 == 0); else one element.
// F32: x1 (and a caller's x0) are f32, else bf16.  DRAW: x0 is drawn in place - element i (flat index over [B, rows, cols]) is the
// VC_RNG_F32 value at stream position offset + i, rounded to bf16 for a bf16 x1 (the VC_RNG_BF16 value)
template <bool F32, bool VEC, bool DRAW>
__global__ __launch_bounds__(FM_THREADS) void fm_plan_kernel(const void* __restrict__ x1, long x1_bstride, long x1_ld, const float* __restrict__ t,
                                                             const void* __restrict__ x0, uint64_t seed, uint64_t offset, bf16_t* __restrict__ xt,
                                                             long xt_ld, float* __restrict__ ut, long rows, int cols, long total) {
#pragma clang fp contract(off)
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  const long per_row = VEC ? cols / 8 : cols;
  for (long wi = blockIdx.x * (long)FM_THREADS + threadIdx.x; wi < total; wi += gridDim.x * (long)FM_THREADS) {
    const long g = wi / per_row, b = g / rows, r = g - b * rows;
    const int c0 = (int)(wi - g * per_row) * (VEC ? 8 : 1);
    const long src = b * x1_bstride + r * x1_ld + c0, flat = g * cols + c0, dst = g * xt_ld + c0;
    const float tb = t[b], omt = 1.0f - tb;
    if constexpr (VEC) {
      float a[8], z[8];
      if constexpr (F32) {
        const f32x4 lo = *(const f32x4*)((const float*)x1 + src), hi = *(const f32x4*)((const float*)x1 + src + 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) { a[e] = lo[e]; a[4 + e] = hi[e]; }
      } else {
        const u32x4 w = *(const u32x4*)((const bf16_t*)x1 + src);
#pragma unroll
        for (int e = 0; e < 4; ++e) { const uint32_t we = w[e]; a[2 * e] = lo_bf(we); a[2 * e + 1] = hi_bf(we); }
      }
      if constexpr (DRAW) {
        const uint64_t p = offset + (uint64_t)flat;
        switch ((uint32_t)p & 3u) {
          case 0: normals8<0>(p, k0, k1, z); break;
          case 1: normals8<1>(p, k0, k1, z); break;
          case 2: normals8<2>(p, k0, k1, z); break;
          default: normals8<3>(p, k0, k1, z); break;
        }
        if constexpr (!F32) {
#pragma unroll
          for (int e = 0; e < 8; ++e) z[e] = rbf(z[e]);
        }
      } else if constexpr (F32) {
        const f32x4 lo = *(const f32x4*)((const float*)x0 + flat), hi = *(const f32x4*)((const float*)x0 + flat + 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) { z[e] = lo[e]; z[4 + e] = hi[e]; }
      } else {
        const u32x4 w = *(const u32x4*)((const bf16_t*)x0 + flat);
#pragma unroll
        for (int e = 0; e < 4; ++e) { const uint32_t we = w[e]; z[2 * e] = lo_bf(we); z[2 * e + 1] = hi_bf(we); }
      }
      f32x4 u[2];
      float xo[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const FmPair o = fm_element(tb, omt, a[e], z[e]);
        xo[e] = o.xt; u[e >> 2][e & 3] = o.ut;
      }
      u32x4 w;
#pragma unroll
      for (int e = 0; e < 4; ++e) w[e] = pack2bf(xo[2 * e], xo[2 * e + 1]);
      *(u32x4*)(xt + dst) = w;
      *(f32x4*)(ut + flat) = u[0];
      *(f32x4*)(ut + flat + 4) = u[1];
    } else {
      const float a = F32 ? ((const float*)x1)[src] : bf2f(((const bf16_t*)x1)[src]);
      float z;
      if constexpr (DRAW) {
        z = normal_at(offset + (uint64_t)flat, k0, k1);
        if (!F32) z = rbf(z);
      } else {
        z = F32 ? ((const float*)x0)[flat] : bf2f(((const bf16_t*)x0)[flat]);
      }
      const FmPair o = fm_element(tb, omt, a, z);
      xt[dst] = f2bf(o.xt);
      ut[flat] = o.ut;
    }
  }
}

// host counts travel by value: a launch has no device memory of its own
struct FmCounts { int use; int v[VC_FM_MAX_HOST_COUNTS]; };
VC_DEV long fm_valid(const FmCounts& hc, const int* __restrict__ dev, int b, long rows) {
  long v = dev ? (long)dev[b] : hc.use ? (long)hc.v[b] : rows;
  return v < 0 ? 0 : v > rows ? rows : v;          // a device count outside [0, rows] reads nothing outside the sample
}

VC_DEV void fm_take(float& s, float o, float u) {
#pragma clang fp contract(off)
  const float d = (0.0f - o) - u;      // (-out) - u_t: the negation is exact
  const float sq = d * d;
  s = s + sq;
}

// pass 1: grid (nblk, B)
template <bool VEC>
__global__ __launch_bounds__(FM_THREADS) void fm_loss_kernel(const bf16_t* __restrict__ out, long out_ld, const float* __restrict__ ut, FmCounts hc,
                                                             const int* __restrict__ valid_dev, long rows, int cols, uint32_t upr,
                                                             float* __restrict__ partial) {
  __shared__ float l[FM_THREADS];
  const uint32_t nblk = gridDim.x, b = blockIdx.y;
  const uint64_t units = (uint64_t)fm_valid(hc, valid_dev, (int)b, rows) * upr;
  float s = 0.0f;
  for (uint64_t u64 = (uint64_t)blockIdx.x * FM_THREADS + threadIdx.x; u64 < units; u64 += (uint64_t)nblk * FM_THREADS) {
    const uint32_t u = (uint32_t)u64, row = u / upr, c0 = (u - row * upr) * 8;
    const long g = (long)b * rows + row, oo = g * out_ld + c0, uo = g * cols + c0;
    if constexpr (VEC) {
      const u32x4 w = *(const u32x4*)(out + oo);
      const f32x4 lo = *(const f32x4*)(ut + uo), hi = *(const f32x4*)(ut + uo + 4);
      float uu[8];
#pragma unroll
      for (int i = 0; i < 4; ++i) { uu[i] = lo[i]; uu[4 + i] = hi[i]; }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const uint32_t wi = w[i];          // (a copy, as in monitor.hip)
        fm_take(s, lo_bf(wi), uu[2 * i]);
        fm_take(s, hi_bf(wi), uu[2 * i + 1]);
      }
    } else {
      const int n = (int)c0 + 8 <= cols ? 8 : cols - (int)c0;
      for (int i = 0; i < n; ++i) fm_take(s, bf2f(out[oo + i]), ut[uo + i]);
    }
  }
  s = block_tree(l, s, VcAddOp());
  if (threadIdx.x == 0) partial[(long)b * nblk + blockIdx.x] = s;
}

// pass 2: grid (B); the sample's nblk <= 256 partials -> loss[b] = total / f32(valid * cols) (0 / 0 = NaN for a device count of 0)
__global__ __launch_bounds__(FM_THREADS) void fm_loss_finish_kernel(const float* __restrict__ partial, int nblk, FmCounts hc,
                                                                    const int* __restrict__ valid_dev, long rows, int cols, float* __restrict__ loss) {
  __shared__ float l[FM_THREADS];
  const int b = blockIdx.x;
  const float total = block_tree(l, (int)threadIdx.x < nblk ? partial[(long)b * nblk + threadIdx.x] : 0.0f, VcAddOp());
  if (threadIdx.x == 0) loss[b] = total / (float)(fm_valid(hc, valid_dev, b, rows) * (long)cols);
}

template <bool F32, bool VEC>
void fm_plan_issue(bool draw, int grid, hipStream_t s, const void* x1, long x1_bstride, long x1_ld, const float* t, const void* x0, uint64_t seed,
                   uint64_t offset, bf16_t* xt, long xt_ld, float* ut, long rows, int cols, long total) {
  if (draw) hipLaunchKernelGGL((fm_plan_kernel<F32, VEC, true>), dim3(grid), dim3(FM_THREADS), 0, s, x1, x1_bstride, x1_ld, t, x0, seed, offset, xt, xt_ld, ut, rows, cols, total);
  else hipLaunchKernelGGL((fm_plan_kernel<F32, VEC, false>), dim3(grid), dim3(FM_THREADS), 0, s, x1, x1_bstride, x1_ld, t, x0, seed, offset, xt, xt_ld, ut, rows, cols, total);
}

}  // namespace

int vc_fm_plan_launch(const void* x1, int x1_is_f32, int64_t x1_bstride, int64_t x1_ld, const float* t, const void* x0, uint64_t seed,
                      uint64_t offset, void* xt, int64_t xt_ld, float* ut, int B, int64_t rows, int cols, hipStream_t s, char* err, int errlen) {
  if (!x1 || !t || !xt || !ut) { snprintf(err, errlen, "fm_plan: null x1 / t / xt / ut"); return VC_ERR_ARG; }
  if (B <= 0 || rows <= 0 || cols <= 0 || x1_bstride < 0) {
    snprintf(err, errlen, "fm_plan: B = %d, rows = %lld, cols = %d must be positive, x1_bstride = %lld not negative", B, (long long)rows, cols,
             (long long)x1_bstride);
    return VC_ERR_ARG;
  }
  if (x1_ld < cols || xt_ld < cols) {
    snprintf(err, errlen, "fm_plan: x1_ld = %lld / xt_ld = %lld is smaller than cols = %d", (long long)x1_ld, (long long)xt_ld, cols);
    return VC_ERR_ARG;
  }
  const int es = x1_is_f32 ? 4 : 2, E = 16 / es;
  if ((uintptr_t)x1 % es || (x0 && (uintptr_t)x0 % es) || (uintptr_t)xt & 1 || ((uintptr_t)ut | (uintptr_t)t) & 3) {
    snprintf(err, errlen, "fm_plan: every buffer must be aligned to its elements (x1 / x0: %d bytes, xt: 2, ut / t: 4)", es);
    return VC_ERR_ARG;
  }
  const unsigned __int128 n128 = (unsigned __int128)(uint64_t)B * (uint64_t)rows * (uint64_t)cols;
  if (n128 > (unsigned __int128)INT64_MAX / 8) { snprintf(err, errlen, "fm_plan: B * rows * cols does not fit a 64-bit byte offset"); return VC_ERR_ARG; }
  const int64_t n = (int64_t)n128;
  if (!x0 && (uint64_t)n - 1 > UINT64_MAX - offset) {
    snprintf(err, errlen, "fm_plan: offset + B * rows * cols wraps the 64-bit stream position (offset=%llu n=%lld)", (unsigned long long)offset,
             (long long)n);
    return VC_ERR_ARG;
  }
  const bool vec = cols % 8 == 0 && x1_ld % E == 0 && x1_bstride % E == 0 && xt_ld % 8 == 0 &&
                   !(((uintptr_t)x1 | (uintptr_t)x0 | (uintptr_t)xt | (uintptr_t)ut) & 15);      // (a NULL x0 counts as aligned)
  const long total = vec ? (long)(n / 8) : (long)n;
  const long want = (total + FM_THREADS - 1) / FM_THREADS;
  const int grid = (int)(want < FM_PLAN_MAX_BLOCKS ? want : FM_PLAN_MAX_BLOCKS);
  const bool draw = x0 == nullptr;
#define FM_PLAN_ARGS draw, grid, s, x1, (long)x1_bstride, (long)x1_ld, t, x0, seed, offset, (bf16_t*)xt, (long)xt_ld, ut, (long)rows, cols, total
  if (x1_is_f32) { if (vec) fm_plan_issue<true, true>(FM_PLAN_ARGS); else fm_plan_issue<true, false>(FM_PLAN_ARGS); }
  else { if (vec) fm_plan_issue<false, true>(FM_PLAN_ARGS); else fm_plan_issue<false, false>(FM_PLAN_ARGS); }
#undef FM_PLAN_ARGS
  return vc_launch_status("fm_plan launch", err, errlen);
}

int vc_fm_loss_launch(const void* out, int64_t out_ld, const float* ut, const int32_t* valid_rows, int valid_on_host, float* loss, float* scratch,
                      int B, int64_t rows, int cols, hipStream_t s, char* err, int errlen) {
  if (!out || !ut || !loss || !scratch) { snprintf(err, errlen, "fm_loss: null out / ut / loss / scratch"); return VC_ERR_ARG; }
  if (B <= 0 || B > 65535 || rows <= 0 || cols <= 0) {
    snprintf(err, errlen, "fm_loss: B = %d (1..65535), rows = %lld, cols = %d must be positive", B, (long long)rows, cols);
    return VC_ERR_ARG;
  }
  if (out_ld < cols) { snprintf(err, errlen, "fm_loss: out_ld = %lld is smaller than cols = %d", (long long)out_ld, cols); return VC_ERR_ARG; }
  if ((uintptr_t)out & 1 || ((uintptr_t)ut | (uintptr_t)loss | (uintptr_t)scratch | (uintptr_t)valid_rows) & 3) {
    snprintf(err, errlen, "fm_loss: every buffer must be aligned to its elements (out: 2 bytes, ut / loss / scratch / valid_rows: 4)");
    return VC_ERR_ARG;
  }
  const int64_t upr = ((int64_t)cols + 7) / 8, units = rows * upr;
  if (rows > 0x7fffffff / upr) { snprintf(err, errlen, "fm_loss: rows = %lld x cols = %d per sample is more than 2^31 - 1 units", (long long)rows, cols); return VC_ERR_ARG; }
  FmCounts hc;
  hc.use = 0;
  if (valid_rows && valid_on_host) {
    if (B > VC_FM_MAX_HOST_COUNTS) {
      snprintf(err, errlen, "fm_loss: host counts serve at most %d samples (B = %d): pass them in device memory", VC_FM_MAX_HOST_COUNTS, B);
      return VC_ERR_ARG;
    }
    hc.use = 1;
    for (int b = 0; b < B; ++b) {
      if (valid_rows[b] <= 0 || valid_rows[b] > rows) {
        snprintf(err, errlen, "fm_loss: valid_rows[%d] = %d outside [1, rows = %lld] (a sample without a valid row has no loss)", b, valid_rows[b],
                 (long long)rows);
        return VC_ERR_ARG;
      }
      hc.v[b] = valid_rows[b];
    }
  }
  const int* dev = valid_rows && !valid_on_host ? valid_rows : nullptr;
  const bool vec = cols % 8 == 0 && out_ld % 8 == 0 && !(((uintptr_t)out | (uintptr_t)ut) & 15);
  const int nblk = vc_reduce_blocks<FM_THREADS, VC_FM_LOSS_MAX_BLOCKS>(units);
  if (vec) hipLaunchKernelGGL(fm_loss_kernel<true>, dim3(nblk, B), dim3(FM_THREADS), 0, s, (const bf16_t*)out, (long)out_ld, ut, hc, dev, (long)rows, cols, (uint32_t)upr, scratch);
  else hipLaunchKernelGGL(fm_loss_kernel<false>, dim3(nblk, B), dim3(FM_THREADS), 0, s, (const bf16_t*)out, (long)out_ld, ut, hc, dev, (long)rows, cols, (uint32_t)upr, scratch);
  hipLaunchKernelGGL(fm_loss_finish_kernel, dim3(B), dim3(FM_THREADS), 0, s, (const float*)scratch, nblk, hc, dev, (long)rows, cols, loss);
  return vc_launch_status("fm_loss launch", err, errlen);
}
