// The adaptive solve's kernels: embedded Runge-Kutta pairs, tableau-driven, the ONE implementation behind vc_rk_* and vc_dopri5_*
// ("the adaptive solve").  f(t, y) = -model(bf16(y) || cond, 1 - f32(t)); every k is stored in bf16 (the
// model's output dtype), the state y is f32; every sum is taken left to right over the NON-ZERO coefficients, one f32 operation after
// the other with floating-point contraction off; every coefficient is a double rounded ONCE to f32.  A torch f32 expression of the
// same shape (transport.rk_step / rk_error_ratio / rk_hermite / dopri5_interp) gives the same bits.
//   rk_stage        k[stage] = -v and the next stage's input state (or y1 behind the last-but-one evaluation)
//   rk_error_ratio  the mixed-tolerance RMS norm of the embedded error estimate, and the three norms of the initial step size
//   rk_dense        the dense output of the pair: the quartic through (y0, f0, y_mid, y1, f1) for Dormand-Prince, the Hermite cubic
//                   through (y0, f0, y1, f1) for bosh3 / adaptive_heun
//   dopri5_load     the caller's state -> the f32 state and its bf16 shadow (every solver with an f32 state of its own starts here)
// vc_dopri5_stage / _error_ratio / _interp are these launchers at VC_RK_DOPRI5 under their own names (api.hip).
// The methods (a method of S stages evaluates k1..kS per step; kS = f(t1, y1) is the next step's k1: first same as last):
//   VC_RK_DOPRI5 = 0         Dormand & Prince 1980 5(4) (SciPy's RK45.C / .A / .B / .E), S = 7, order 5
//     c    0, 1/5, 3/10, 4/5, 8/9, 1, 1
//     a2   1/5
//     a3   3/40, 9/40
//     a4   44/45, -56/15, 32/9
//     a5   19372/6561, -25360/2187, 64448/6561, -212/729
//     a6   9017/3168, -355/33, 46732/5247, 49/176, -5103/18656
//     b    35/384, 0, 500/1113, 125/192, -2187/6784, 11/84                       (5th order: y1; also the row a7)
//     e    -71/57600, 0, 71/16695, -71/1920, 17253/339200, -22/525, 1/40         (b - b^, the 4th-order companion)
//     DPS_C_MID  6025192743/30085553152/2, 0, 51252292925/65400821598/2, -2691868925/45128329728/2,
//                187940372067/1594534317056/2, -1776094331/19743644256/2, 11237099/235043384/2        (y at t0 + dt/2: torchdiffeq's)
//   VC_RK_BOSH3 = 1          Bogacki-Shampine 3(2) (SciPy's RK23.C / .A / .B / .E), S = 4, order 3
//     c 0, 1/2, 3/4, 1;  a2 1/2;  a3 0, 3/4;  a4 = b 2/9, 1/3, 4/9;  e 5/72, -1/12, -1/9, 1/8
//   VC_RK_ADAPTIVE_HEUN = 2  Heun-Euler 2(1), S = 3, order 2
//     c 0, 1, 1;  a2 1;  a3 = b 1/2, 1/2;  e 1/2, -1/2, 0
// The Hermite cubic, as ONE sequence of f32 operations (x = theta, d = y1 - y0, f0 = k1, f1 = kS):
//   c0 = 1 - x; c1 = x - 1; c2 = 1 - 2 x; w = x c1; h0 = c1 dt; h1 = x dt
//   y(x) = (c0 y0 + x y1) + w ((c2 d + h0 f0) + h1 f1)                          theta = 0 / 1: the bits of y0 / y1
// For bosh3 this is SciPy's RK23 dense output (its P rows are this cubic expanded).  The controller around these kernels
// (flux_sample.hip, transport.rk_integrate / dopri5_integrate) is torchdiffeq's AS RECALLED - the package was not available to check
// against: "unpinned against real torchdiffeq" - and pinned to SciPy's RK45 / RK23 in the tableaus and in single steps
// (tests/test_dopri5_cpu.py, tests/test_rk_embedded_cpu.py).
// Memory: elementwise passes over n elements with 2..7 k planes.  The W = 8 kernels move 16 bytes per access - eight bf16 of a k
// plane, four f32 of the state - wherever the address allows it (plane j starts at element j n: 16-byte aligned for every j only
// where n % 8 == 0, which every [B, N, 64] state is); the last n % 8 elements, and every element where a base is not 16-byte
// aligned (the launcher picks W = 1), run one by one through the SAME per-element expression.  The norm deals single elements to
// threads: its summation order is part of its result (block_reduce.h, transport._rk_norm).  The quartic and the load run one element
// per thread.
#include "common.h"
#include "vcloze_internal.h"
#include "block_reduce.h"

#pragma clang fp contract(off)

namespace {

constexpr int RK_THREADS = 256;                        // = VC_DOPRI5_MAX_BLOCKS: pass 2 reduces one partial per thread
constexpr int RK_PROBE = 7;                            // the probe stage of every method
constexpr int RK_E = 6;                                // the row of e

// [method]: rows 0..S-3 feed the evaluations behind stages 0..S-3 (a2..), row S-2 is b (forms y1), row 6 is e
__constant__ float RK_ROWS[3][7][7] = {
    {{(float)(1.0 / 5.0), 0, 0, 0, 0, 0, 0},
     {(float)(3.0 / 40.0), (float)(9.0 / 40.0), 0, 0, 0, 0, 0},
     {(float)(44.0 / 45.0), (float)(-56.0 / 15.0), (float)(32.0 / 9.0), 0, 0, 0, 0},
     {(float)(19372.0 / 6561.0), (float)(-25360.0 / 2187.0), (float)(64448.0 / 6561.0), (float)(-212.0 / 729.0), 0, 0, 0},
     {(float)(9017.0 / 3168.0), (float)(-355.0 / 33.0), (float)(46732.0 / 5247.0), (float)(49.0 / 176.0), (float)(-5103.0 / 18656.0), 0, 0},
     {(float)(35.0 / 384.0), 0, (float)(500.0 / 1113.0), (float)(125.0 / 192.0), (float)(-2187.0 / 6784.0), (float)(11.0 / 84.0), 0},
     {(float)(-71.0 / 57600.0), 0, (float)(71.0 / 16695.0), (float)(-71.0 / 1920.0), (float)(17253.0 / 339200.0), (float)(-22.0 / 525.0),
      (float)(1.0 / 40.0)}},
    {{(float)(1.0 / 2.0), 0, 0, 0, 0, 0, 0},
     {0, (float)(3.0 / 4.0), 0, 0, 0, 0, 0},
     {(float)(2.0 / 9.0), (float)(1.0 / 3.0), (float)(4.0 / 9.0), 0, 0, 0, 0},
     {0, 0, 0, 0, 0, 0, 0},
     {0, 0, 0, 0, 0, 0, 0},
     {0, 0, 0, 0, 0, 0, 0},
     {(float)(5.0 / 72.0), (float)(-1.0 / 12.0), (float)(-1.0 / 9.0), (float)(1.0 / 8.0), 0, 0, 0}},
    {{1.0f, 0, 0, 0, 0, 0, 0},
     {(float)(1.0 / 2.0), (float)(1.0 / 2.0), 0, 0, 0, 0, 0},
     {0, 0, 0, 0, 0, 0, 0},
     {0, 0, 0, 0, 0, 0, 0},
     {0, 0, 0, 0, 0, 0, 0},
     {0, 0, 0, 0, 0, 0, 0},
     {(float)(1.0 / 2.0), (float)(-1.0 / 2.0), 0, 0, 0, 0, 0}},
};
// DPS_C_MID: the weights of y at t0 + dt / 2, which the quartic dense output of Dormand-Prince goes through
__constant__ float DP_MID[7] = {
    (float)(6025192743.0 / 30085553152.0 / 2.0), 0, (float)(51252292925.0 / 65400821598.0 / 2.0),
    (float)(-2691868925.0 / 45128329728.0 / 2.0), (float)(187940372067.0 / 1594534317056.0 / 2.0),
    (float)(-1776094331.0 / 19743644256.0 / 2.0), (float)(11237099.0 / 235043384.0 / 2.0)};

// ---- W consecutive elements at p: one 16-byte access (two for f32) where W = 8 and the address allows it, else one by one
template <int W> VC_DEV void ld_bf(const bf16_t* __restrict__ p, float (&out)[W]) {
  if constexpr (W == 8) {
    if (((uintptr_t)p & 15) == 0) {
      const u32x4 w = *(const u32x4*)p;
#pragma unroll
      for (int e = 0; e < 4; ++e) { out[2 * e] = lo_bf(w[e]); out[2 * e + 1] = hi_bf(w[e]); }
      return;
    }
  }
#pragma unroll
  for (int e = 0; e < W; ++e) out[e] = bf2f(p[e]);
}
template <int W> VC_DEV void st_bf(bf16_t* __restrict__ p, const float (&v)[W]) {
  if constexpr (W == 8) {
    if (((uintptr_t)p & 15) == 0) {
      u32x4 w;
#pragma unroll
      for (int e = 0; e < 4; ++e) w[e] = pack2bf(v[2 * e], v[2 * e + 1]);
      *(u32x4*)p = w;
      return;
    }
  }
#pragma unroll
  for (int e = 0; e < W; ++e) p[e] = f2bf(v[e]);
}
template <int W> VC_DEV void ld_f(const float* __restrict__ p, float (&out)[W]) {
  if constexpr (W == 8) {
    if (((uintptr_t)p & 15) == 0) {
      const f32x4 a = *(const f32x4*)p, b = *(const f32x4*)(p + 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) { out[e] = a[e]; out[4 + e] = b[e]; }
      return;
    }
  }
#pragma unroll
  for (int e = 0; e < W; ++e) out[e] = p[e];
}
template <int W> VC_DEV void st_f(float* __restrict__ p, const float (&v)[W]) {
  if constexpr (W == 8) {
    if (((uintptr_t)p & 15) == 0) {
      f32x4 a, b;
#pragma unroll
      for (int e = 0; e < 4; ++e) { a[e] = v[e]; b[e] = v[4 + e]; }
      *(f32x4*)p = a; *(f32x4*)(p + 4) = b;
      return;
    }
  }
#pragma unroll
  for (int e = 0; e < W; ++e) p[e] = v[e];
}

// sum over the non-zero coefficients of `row`, left to right: ((c_a k_a + c_b k_b) + c_c k_c) + ...
template <int W> VC_DEV void rk_combine(const float* __restrict__ row, const bf16_t* __restrict__ k, long n, long i, float (&acc)[W]) {
  bool first = true;
#pragma unroll
  for (int e = 0; e < W; ++e) acc[e] = 0.0f;
  for (int j = 0; j < 7; ++j) {
    const float c = row[j];
    if (c == 0.0f) continue;
    float kv[W];
    ld_bf<W>(k + (long)j * n + i, kv);
#pragma unroll
    for (int e = 0; e < W; ++e) {
      const float term = c * kv[e];
      acc[e] = first ? term : acc[e] + term;
    }
    first = false;
  }
}

// elements i .. i + W - 1 of one stage (stage in 0..S-1, or RK_PROBE)
template <int W>
VC_DEV void rk_stage_elems(int method, int stage, int S, const float* __restrict__ y0, bf16_t* __restrict__ k, const bf16_t* __restrict__ v,
                           const float* __restrict__ dt_ptr, float* __restrict__ y_stage, bf16_t* __restrict__ y_in, long n, long i) {
  if (v && stage != RK_PROBE) {                         // the drift is -model(...): exact
    float vv[W];
    ld_bf<W>(v + i, vv);
#pragma unroll
    for (int e = 0; e < W; ++e) vv[e] = -vv[e];
    st_bf<W>(k + (long)stage * n + i, vv);
  }
  if (stage == S - 1) return;                           // the last stage stores k alone
  const float dt = *dt_ptr;
  float acc[W], ys[W];
  if (stage == RK_PROBE) ld_bf<W>(k + i, acc);
  else rk_combine<W>(RK_ROWS[method][stage], k, n, i, acc);
  ld_f<W>(y0 + i, ys);
#pragma unroll
  for (int e = 0; e < W; ++e) ys[e] = ys[e] + dt * acc[e];
  if (y_stage) st_f<W>(y_stage + i, ys);
  if (y_in) st_bf<W>(y_in + i, ys);
}

// stage 0..S-3: y_s = y0 + dt * (a row), stage S-2: y1 = y0 + dt * (b row), stage S-1: kS alone, stage 7 (no v): the probe state
// y0 + dt * k1 of the initial step size.  v null: k[stage] is in place already.  A thread owns W consecutive elements
template <int W>
__global__ __launch_bounds__(RK_THREADS) void rk_stage_kernel(int method, int stage_arg, const float* __restrict__ y0, bf16_t* __restrict__ k,
                                                              const bf16_t* __restrict__ v, const float* __restrict__ dt_ptr,
                                                              const int* __restrict__ eval_ptr, float* __restrict__ y_stage,
                                                              bf16_t* __restrict__ y_in, long n) {
  const long i = ((long)blockIdx.x * RK_THREADS + threadIdx.x) * W;
  if (i >= n) return;
  const int stage = stage_arg >= 0 ? stage_arg : *eval_ptr;
  const int S = vc_rk_stages_of(method);
  if (stage < 0 || (stage >= S && stage != RK_PROBE)) return;        // a counter outside the method's stages: nothing is read or written
  if (i + W <= n) rk_stage_elems<W>(method, stage, S, y0, k, v, dt_ptr, y_stage, y_in, n, i);
  else
    for (long t = i; t < n; ++t) rk_stage_elems<1>(method, stage, S, y0, k, v, dt_ptr, y_stage, y_in, n, t);
}

// pass 1: the n elements are dealt to the nblk * 256 threads round-robin, a thread adds its q^2 in ascending order.
//   mode 0  q = dt * (e row) / (atol + rtol * max(|y0|, |y1|))        the error ratio of a step
//   mode 1  q = y0 / (atol + rtol * |y0|)                              d0 of the initial step size
//   mode 2  q = k1 / (atol + rtol * |y0|)                              d1
//   mode 3  q = (k2 - k1) / (atol + rtol * |y0|)                       d2 * h0 (k2 holds the probe evaluation)
__global__ __launch_bounds__(RK_THREADS) void rk_norm_kernel(int method, int mode, const float* __restrict__ y0, const float* __restrict__ y1,
                                                             const bf16_t* __restrict__ k, const float* __restrict__ dt_ptr, float rtol,
                                                             float atol, float* __restrict__ partial, long n) {
  __shared__ float l[RK_THREADS];
  const float dt = mode == 0 ? *dt_ptr : 0.0f;
  float s = 0.0f;
  for (long i = (long)blockIdx.x * RK_THREADS + threadIdx.x; i < n; i += (long)gridDim.x * RK_THREADS) {
    const float a0 = fabsf(y0[i]);
    float num, mag = a0;
    if (mode == 0) {
      float acc[1];
      rk_combine<1>(RK_ROWS[method][RK_E], k, n, i, acc);
      num = dt * acc[0];
      mag = fmaxf(a0, fabsf(y1[i]));
    } else if (mode == 1) num = y0[i];
    else if (mode == 2) num = bf2f(k[i]);
    else num = bf2f(k[n + i]) - bf2f(k[i]);
    const float q = num / (atol + rtol * mag);
    s = s + q * q;
  }
  s = block_tree(l, s, VcAddOp());
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// pass 2: ONE block; the nblk <= 256 partials -> out[0] = sqrt(sum / n)
__global__ __launch_bounds__(RK_THREADS) void rk_norm_finish_kernel(const float* __restrict__ partial, float* __restrict__ out, int nblk, long n) {
  __shared__ float l[RK_THREADS];
  const float s = block_tree(l, (int)threadIdx.x < nblk ? partial[threadIdx.x] : 0.0f, VcAddOp());
  if (threadIdx.x == 0) out[0] = sqrtf(s / (float)n);
}

// the Hermite cubic of the header comment at elements i .. i + W - 1; kl: the plane of the last k
template <int W, bool BF16>
VC_DEV void rk_hermite_elems(const float* __restrict__ y0, const float* __restrict__ y1, const bf16_t* __restrict__ k,
                             const bf16_t* __restrict__ kl, float dt, float x, void* __restrict__ out, long i) {
  float a0[W], a1[W], r[W];
  ld_f<W>(y0 + i, a0);
  ld_f<W>(y1 + i, a1);
  if (x == 0.0f) {
#pragma unroll
    for (int e = 0; e < W; ++e) r[e] = a0[e];
  } else if (x == 1.0f) {
#pragma unroll
    for (int e = 0; e < W; ++e) r[e] = a1[e];
  } else {
    float f0[W], f1[W];
    ld_bf<W>(k + i, f0);
    ld_bf<W>(kl + i, f1);
    const float c0 = 1.0f - x, c1 = x - 1.0f, c2 = 1.0f - 2.0f * x;
    const float w = x * c1, h0 = c1 * dt, h1 = x * dt;
#pragma unroll
    for (int e = 0; e < W; ++e) {
      const float d = a1[e] - a0[e];
      const float inner = (c2 * d + h0 * f0[e]) + h1 * f1[e];
      r[e] = (c0 * a0[e] + x * a1[e]) + w * inner;
    }
  }
  if constexpr (BF16) st_bf<W>((bf16_t*)out + i, r);
  else st_f<W>((float*)out + i, r);
}

template <int W, bool BF16>
__global__ __launch_bounds__(RK_THREADS) void rk_hermite_kernel(int last, const float* __restrict__ y0, const float* __restrict__ y1,
                                                                const bf16_t* __restrict__ k, const float* __restrict__ dt_ptr, float x,
                                                                void* __restrict__ out, long n) {
  const long i = ((long)blockIdx.x * RK_THREADS + threadIdx.x) * W;
  if (i >= n) return;
  const float dt = *dt_ptr;
  const bf16_t* kl = k + (long)last * n;
  if (i + W <= n) rk_hermite_elems<W, BF16>(y0, y1, k, kl, dt, x, out, i);
  else
    for (long t = i; t < n; ++t) rk_hermite_elems<1, BF16>(y0, y1, k, kl, dt, x, out, t);
}

// Dormand-Prince's dense output - torchdiffeq's _interp_fit / _interp_evaluate, operation by operation; theta = 0 and theta = 1 hand
// back y0 and y1 themselves
template <bool BF16>
__global__ __launch_bounds__(RK_THREADS) void dopri5_interp_kernel(const float* __restrict__ y0, const float* __restrict__ y1,
                                                                   const bf16_t* __restrict__ k, const float* __restrict__ dt_ptr, float x,
                                                                   void* __restrict__ out, long n) {
  const long i = (long)blockIdx.x * RK_THREADS + threadIdx.x;
  if (i >= n) return;
  const float a0 = y0[i], a1 = y1[i];
  float r;
  if (x == 0.0f) r = a0;
  else if (x == 1.0f) r = a1;
  else {
    const float dt = *dt_ptr;
    const float f0 = bf2f(k[i]), f1 = bf2f(k[6 * n + i]);
    float mid[1];
    rk_combine<1>(DP_MID, k, n, i, mid);
    const float ym = a0 + dt * mid[0];
    const float two_dt = 2.0f * dt;
    const float ca = (two_dt * (f1 - f0) - 8.0f * (a1 + a0)) + 16.0f * ym;
    const float cb = ((dt * (5.0f * f0 - 3.0f * f1) + 18.0f * a0) + 14.0f * a1) - 32.0f * ym;
    const float cc = ((dt * (f1 - 4.0f * f0) - 11.0f * a0) - 5.0f * a1) + 16.0f * ym;
    const float cd = dt * f0;
    float xp = x;
    r = a0 + xp * cd;
    xp = xp * x; r = r + xp * cc;
    xp = xp * x; r = r + xp * cb;
    xp = xp * x; r = r + xp * ca;
  }
  if constexpr (BF16) ((bf16_t*)out)[i] = f2bf(r);
  else ((float*)out)[i] = r;
}

// the caller's state -> the f32 state and its bf16 shadow (what img_in reads)
template <bool BF16>
__global__ __launch_bounds__(RK_THREADS) void dopri5_load_kernel(const void* __restrict__ x, float* __restrict__ y0, bf16_t* __restrict__ y_in,
                                                                 long n) {
  const long i = (long)blockIdx.x * RK_THREADS + threadIdx.x;
  if (i >= n) return;
  const float v = BF16 ? bf2f(((const bf16_t*)x)[i]) : ((const float*)x)[i];
  y0[i] = v;
  y_in[i] = f2bf(v);
}

// a grid of ceil(n / 256) blocks must fit the x dimension
inline bool rk_n_ok(int64_t n) { return n > 0 && n <= (int64_t)0x7fffffff * RK_THREADS; }
inline unsigned rk_blocks(int64_t n, int W) { return (unsigned)(((n + W - 1) / W + RK_THREADS - 1) / RK_THREADS); }
// null counts as aligned: a buffer the call does not use
inline bool rk_aligned16(std::initializer_list<const void*> ps) {
  for (const void* p : ps) if ((uintptr_t)p & 15) return false;
  return true;
}

}  // namespace

// `what`: the entry point's name, known at run time only (an alias)
static int rk_launch_status(const char* what, char* err, int errlen) {
  char prefix[64];
  snprintf(prefix, sizeof(prefix), "%s launch", what);
  return vc_launch_status(prefix, err, errlen);
}

// `alias` (all three launchers): the vc_dopri5_* entry point the call serves - its name stands in the messages, which then name no method
int vc_rk_stage_launch(int method, int stage, const float* y0, void* k, const void* v, const float* dt_ptr, const int32_t* eval_ptr,
                       float* y_stage, void* y_in, int64_t n, hipStream_t s, char* err, int errlen, const char* alias) {
  const char* what = alias ? alias : "rk_stage";
  const int S = vc_rk_stages_of(method);
  if (!S) { snprintf(err, errlen, "%s: unknown method %d (VC_RK_DOPRI5, VC_RK_BOSH3, VC_RK_ADAPTIVE_HEUN)", what, method); return VC_ERR_ARG; }
  if (!y0 || !k || !dt_ptr || !rk_n_ok(n) || (stage >= S && stage != RK_PROBE) || (stage < 0 && !eval_ptr) || (stage == S - 1 && !v) ||
      (stage == RK_PROBE && v) || (stage != S - 1 && !y_stage && !y_in)) {
    char of[32] = "";
    if (!alias) snprintf(of, sizeof(of), "method %d: ", method);
    snprintf(err, errlen, "%s: bad args (%sstage 0..%d, or < 0 with the evaluation counter; stage 7, the probe state, takes no v)", what, of,
             S - 1);
    return VC_ERR_ARG;
  }
  if (rk_aligned16({y0, k, v, y_stage, y_in}))
    hipLaunchKernelGGL(rk_stage_kernel<8>, dim3(rk_blocks(n, 8)), dim3(RK_THREADS), 0, s, method, stage, y0, (bf16_t*)k, (const bf16_t*)v, dt_ptr,
                       (const int*)eval_ptr, y_stage, (bf16_t*)y_in, (long)n);
  else
    hipLaunchKernelGGL(rk_stage_kernel<1>, dim3(rk_blocks(n, 1)), dim3(RK_THREADS), 0, s, method, stage, y0, (bf16_t*)k, (const bf16_t*)v, dt_ptr,
                       (const int*)eval_ptr, y_stage, (bf16_t*)y_in, (long)n);
  return rk_launch_status(what, err, errlen);
}

int vc_rk_error_ratio_launch(int method, int mode, const float* y0, const float* y1, const void* k, const float* dt_ptr, float rtol, float atol,
                             float* out, float* scratch, int64_t n, hipStream_t s, char* err, int errlen, const char* alias) {
  const char* what = alias ? alias : "rk_error_ratio";
  if (!vc_rk_stages_of(method)) {
    snprintf(err, errlen, "%s: unknown method %d (VC_RK_DOPRI5, VC_RK_BOSH3, VC_RK_ADAPTIVE_HEUN)", what, method);
    return VC_ERR_ARG;
  }
  if (mode < 0 || mode > 3 || !y0 || !out || !scratch || !rk_n_ok(n) || (mode == 0 && (!y1 || !dt_ptr)) || (mode != 1 && !k)) {
    snprintf(err, errlen, "%s: bad args (mode 0..3; mode 0 needs y1, k and dt, modes 2 and 3 need k)", what);
    return VC_ERR_ARG;
  }
  if (!(rtol >= 0.0f) || !(atol >= 0.0f) || !(rtol + atol > 0.0f) || !(rtol + atol - (rtol + atol) == 0.0f)) {
    snprintf(err, errlen, "%s: rtol = %g and atol = %g must be finite, non-negative and not both zero", what, rtol, atol);
    return VC_ERR_ARG;
  }
  const int nblk = vc_reduce_blocks<RK_THREADS, VC_DOPRI5_MAX_BLOCKS>(n);
  hipLaunchKernelGGL(rk_norm_kernel, dim3(nblk), dim3(RK_THREADS), 0, s, method, mode, y0, y1, (const bf16_t*)k, dt_ptr, rtol, atol, scratch,
                     (long)n);
  hipLaunchKernelGGL(rk_norm_finish_kernel, dim3(1), dim3(RK_THREADS), 0, s, (const float*)scratch, out, nblk, (long)n);
  return rk_launch_status(what, err, errlen);
}

// the dense output of the pair: the quartic for Dormand-Prince, the Hermite cubic for the others
int vc_rk_dense_launch(int method, const float* y0, const float* y1, const void* k, const float* dt_ptr, float theta, void* out,
                       int out_is_bf16, int64_t n, hipStream_t s, char* err, int errlen, const char* alias) {
  const char* what = alias ? alias : "rk_interp";
  const int S = vc_rk_stages_of(method);
  if (!S) { snprintf(err, errlen, "%s: unknown method %d (VC_RK_DOPRI5, VC_RK_BOSH3, VC_RK_ADAPTIVE_HEUN)", what, method); return VC_ERR_ARG; }
  if (!y0 || !y1 || !k || !dt_ptr || !out || !rk_n_ok(n)) { snprintf(err, errlen, "%s: bad args", what); return VC_ERR_ARG; }
  if (!(theta >= 0.0f && theta <= 1.0f)) { snprintf(err, errlen, "%s: theta = %g outside [0, 1]", what, theta); return VC_ERR_ARG; }
  if (method == VC_RK_DOPRI5) {
    if (out_is_bf16) hipLaunchKernelGGL(dopri5_interp_kernel<true>, dim3(rk_blocks(n, 1)), dim3(RK_THREADS), 0, s, y0, y1, (const bf16_t*)k, dt_ptr,
                                        theta, out, (long)n);
    else hipLaunchKernelGGL(dopri5_interp_kernel<false>, dim3(rk_blocks(n, 1)), dim3(RK_THREADS), 0, s, y0, y1, (const bf16_t*)k, dt_ptr, theta,
                            out, (long)n);
    return rk_launch_status(what, err, errlen);
  }
  const int last = S - 1;
  const bool vec = rk_aligned16({y0, y1, k, out});
#define RK_HERMITE(W, BF)                                                                                                              \
  hipLaunchKernelGGL((rk_hermite_kernel<W, BF>), dim3(rk_blocks(n, W)), dim3(RK_THREADS), 0, s, last, y0, y1, (const bf16_t*)k, dt_ptr, \
                     theta, out, (long)n)
  if (vec && out_is_bf16) RK_HERMITE(8, true);
  else if (vec) RK_HERMITE(8, false);
  else if (out_is_bf16) RK_HERMITE(1, true);
  else RK_HERMITE(1, false);
#undef RK_HERMITE
  return rk_launch_status(what, err, errlen);
}

// vc_rk_interp: the Hermite pairs alone - the public route to Dormand-Prince's dense output is vc_dopri5_interp
int vc_rk_interp_launch(int method, const float* y0, const float* y1, const void* k, const float* dt_ptr, float theta, void* out,
                        int out_is_bf16, int64_t n, hipStream_t s, char* err, int errlen) {
  if (method != VC_RK_BOSH3 && method != VC_RK_ADAPTIVE_HEUN) {
    snprintf(err, errlen, "rk_interp: method %d has no Hermite dense output (VC_RK_BOSH3, VC_RK_ADAPTIVE_HEUN; Dormand-Prince: vc_dopri5_interp)",
             method);
    return VC_ERR_ARG;
  }
  return vc_rk_dense_launch(method, y0, y1, k, dt_ptr, theta, out, out_is_bf16, n, s, err, errlen);
}

int vc_dopri5_load_launch(const void* x, int x_is_bf16, float* y0, void* y_in, int64_t n, hipStream_t s, char* err, int errlen) {
  if (!x || !y0 || !y_in || !rk_n_ok(n)) { snprintf(err, errlen, "dopri5_load: bad args"); return VC_ERR_ARG; }
  if (x_is_bf16) hipLaunchKernelGGL(dopri5_load_kernel<true>, dim3(rk_blocks(n, 1)), dim3(RK_THREADS), 0, s, x, y0, (bf16_t*)y_in, (long)n);
  else hipLaunchKernelGGL(dopri5_load_kernel<false>, dim3(rk_blocks(n, 1)), dim3(RK_THREADS), 0, s, x, y0, (bf16_t*)y_in, (long)n);
  return vc_launch_status("dopri5_load launch", err, errlen);
}
