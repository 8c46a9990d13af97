// First-block step cache of the fused Euler loop ("the step cache"): the three elementwise passes the rule needs.
// The rule is this library's own - the reference evaluates every block at every step.
//   residual_change   r = bf16(f32(h1) - f32(h0)) -> HBM, and per sample (sum |f32(r) - f32(P)|, sum |f32(P)|) in f32
//   residual_sub/add  out = bf16(f32(a) -/+ f32(b)) on per-sample contiguous rows (R = hE - h1; X_img = h1 + R)
// All HBM-bound, 16-byte accesses, bf16 storage, f32 math.  The sums are the two-pass reduction of block_reduce.h over 16-byte
// chunks: a FIXED order, no atomics, so a repeated run gives the same bits.
#include "common.h"
#include "vcloze_internal.h"
#include "block_reduce.h"

namespace {

constexpr int RC_THREADS = 256;                       // = VC_RESIDUAL_CHANGE_MAX_BLOCKS: pass 2 reduces one partial per thread

// (sum |r - P|, sum |P|): one tree carries both
struct RcPair { float s0, s1; };
struct RcAdd { VC_DEV RcPair operator()(RcPair x, RcPair y) const { return RcPair{x.s0 + y.s0, x.s1 + y.s1}; } };

// pass 1: grid (nblk, B); sample b's n8 16-byte chunks are dealt to the nblk * 256 threads round-robin
__global__ __launch_bounds__(RC_THREADS) void residual_change_kernel(const u32x4* __restrict__ h0, const u32x4* __restrict__ h1,
                                                                     const u32x4* __restrict__ p, u32x4* __restrict__ r,
                                                                     float* __restrict__ partial, long n8) {
  __shared__ RcPair l[RC_THREADS];
  const int nblk = gridDim.x, b = blockIdx.y;
  const long base = (long)b * n8;
  float s0 = 0.0f, s1 = 0.0f;
  for (long c = (long)blockIdx.x * RC_THREADS + threadIdx.x; c < n8; c += (long)nblk * RC_THREADS) {
    const u32x4 a0 = h0[base + c], a1 = h1[base + c], pp = p[base + c];
    u32x4 o;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float rl = rbf(lo_bf(a1[i]) - lo_bf(a0[i])), rh = rbf(hi_bf(a1[i]) - hi_bf(a0[i]));
      const float pl = lo_bf(pp[i]), ph = hi_bf(pp[i]);
      s0 += fabsf(rl - pl); s1 += fabsf(pl);
      s0 += fabsf(rh - ph); s1 += fabsf(ph);
      o[i] = pack2bf(rl, rh);
    }
    r[base + c] = o;
  }
  const RcPair t = block_tree(l, RcPair{s0, s1}, RcAdd());
  if (threadIdx.x == 0) {
    partial[((long)b * nblk + blockIdx.x) * 2] = t.s0;
    partial[((long)b * nblk + blockIdx.x) * 2 + 1] = t.s1;
  }
}

// pass 2: ONE block; per sample the nblk <= 256 partials -> sums[b] = (sum |r - P|, sum |P|); metric = max_b of their ratio
// (a NaN ratio - no P: 0 / 0 - stays NaN, so that a host comparing `metric < threshold` never reuses on it)
__global__ __launch_bounds__(RC_THREADS) void residual_change_finish_kernel(const float* __restrict__ partial, float* __restrict__ sums,
                                                                            float* __restrict__ metric, int B, int nblk) {
  __shared__ RcPair l[RC_THREADS];
  float m = 0.0f;
  for (int b = 0; b < B; ++b) {
    RcPair t = {0.0f, 0.0f};
    if ((int)threadIdx.x < nblk) {
      t.s0 = partial[((long)b * nblk + threadIdx.x) * 2];
      t.s1 = partial[((long)b * nblk + threadIdx.x) * 2 + 1];
    }
    t = block_tree(l, t, RcAdd());
    const float mb = t.s0 / t.s1;
    if (b == 0 || mb > m || mb != mb) m = (m != m) ? m : mb;
    if (threadIdx.x == 0 && sums) { sums[2 * b] = t.s0; sums[2 * b + 1] = t.s1; }
  }
  if (threadIdx.x == 0 && metric) *metric = m;
}

// grid (ceil(n8 / 256), B): out[b][c] = bf16(a[b][c] +/- b[b][c]) per 16-byte chunk; the strides count chunks
template <bool ADD>
__global__ __launch_bounds__(256) void residual_op_kernel(const u32x4* __restrict__ a, long a_bs, const u32x4* __restrict__ b, long b_bs,
                                                          u32x4* __restrict__ out, long o_bs, long n8) {
  const long c = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n8) return;
  const int s = blockIdx.y;
  const u32x4 x = a[s * a_bs + c], y = b[s * b_bs + c];
  u32x4 o;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float yl = ADD ? lo_bf(y[i]) : -lo_bf(y[i]), yh = ADD ? hi_bf(y[i]) : -hi_bf(y[i]);
    o[i] = pack2bf(lo_bf(x[i]) + yl, hi_bf(x[i]) + yh);
  }
  out[s * o_bs + c] = o;
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

int vc_residual_change_launch(const void* h0, const void* h1, const void* p, void* r, float* sums, float* metric, float* scratch,
                              int32_t B, int64_t n, hipStream_t s, char* err, int errlen) {
  if (!h0 || !h1 || !p || !r || !scratch || (!sums && !metric) || B <= 0 || B > 65535 || n <= 0) {
    snprintf(err, errlen, "residual_change: bad args");
    return VC_ERR_ARG;
  }
  if (n % 8 || !aligned16(h0) || !aligned16(h1) || !aligned16(p) || !aligned16(r)) {
    snprintf(err, errlen, "residual_change: n must be a multiple of 8 and every base 16-byte aligned");
    return VC_ERR_ARG;
  }
  const long n8 = n / 8;
  const int nblk = vc_reduce_blocks<RC_THREADS, VC_RESIDUAL_CHANGE_MAX_BLOCKS>(n8);
  hipLaunchKernelGGL(residual_change_kernel, dim3(nblk, B), dim3(RC_THREADS), 0, s, (const u32x4*)h0, (const u32x4*)h1, (const u32x4*)p,
                     (u32x4*)r, scratch, n8);
  hipLaunchKernelGGL(residual_change_finish_kernel, dim3(1), dim3(RC_THREADS), 0, s, (const float*)scratch, sums, metric, (int)B, nblk);
  return vc_launch_status("residual_change launch", err, errlen);
}

int vc_residual_op_launch(int add, const void* a, int64_t a_bstride, const void* b, int64_t b_bstride, void* out, int64_t out_bstride,
                          int32_t B, int64_t n, hipStream_t s, char* err, int errlen) {
  const char* name = add ? "residual_add" : "residual_sub";
  if (!a || !b || !out || B <= 0 || B > 65535 || n <= 0 || a_bstride < 0 || b_bstride < 0 || out_bstride < (B > 1 ? n : 0)) {
    snprintf(err, errlen, "%s: bad args", name);
    return VC_ERR_ARG;
  }
  if (n % 8 || a_bstride % 8 || b_bstride % 8 || out_bstride % 8 || !aligned16(a) || !aligned16(b) || !aligned16(out)) {
    snprintf(err, errlen, "%s: n and the sample strides must be multiples of 8 and every base 16-byte aligned", name);
    return VC_ERR_ARG;
  }
  const long n8 = n / 8;
  const dim3 grid((unsigned)((n8 + 255) / 256), B), block(256);
  if (add) hipLaunchKernelGGL(residual_op_kernel<true>, grid, block, 0, s, (const u32x4*)a, (long)(a_bstride / 8), (const u32x4*)b,
                              (long)(b_bstride / 8), (u32x4*)out, (long)(out_bstride / 8), n8);
  else hipLaunchKernelGGL(residual_op_kernel<false>, grid, block, 0, s, (const u32x4*)a, (long)(a_bstride / 8), (const u32x4*)b,
                          (long)(b_bstride / 8), (u32x4*)out, (long)(out_bstride / 8), n8);
  return vc_launch_status(add ? "residual_add launch" : "residual_sub launch", err, errlen);
}
