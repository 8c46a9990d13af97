// Embedded Runge-Kutta pairs, tableau-driven: the twin of dopri5.hip with the method as an argument ("the
// adaptive solve").  The contract is dopri5.hip's: f(t, y) = -model(bf16(y) || cond, 1 - f32(t)); every k is stored in bf16 (the
// model's output dtype), the state y is f32; every sum is taken left to right over the NON-ZERO coefficients, one f32 operation after
// the other with floating-point contraction off; every coefficient is a double rounded ONCE to f32.  A torch f32 expression of the
// same shape (transport.rk_step / rk_error_ratio / rk_hermite) gives the same bits.
//   rk_stage        k[stage] = -v and the next stage's input state (or y1 behind the last-but-one evaluation)
//   rk_error_ratio  the mixed-tolerance RMS norm of the embedded error estimate, and the three norms of the initial step size
//   rk_interp       the dense output of bosh3 / adaptive_heun: the Hermite cubic through (y0, f0, y1, f1)
// The methods (a method of S stages evaluates k1..kS per step; kS = f(t1, y1) is the next step's k1: first same as last):
//   VC_RK_DOPRI5 = 0         the rows of dopri5.hip, S = 7.  Stage and error kernels only: it holds the generic code to the pinned one
//   VC_RK_BOSH3 = 1          Bogacki-Shampine 3(2) (SciPy's RK23.C / .A / .B / .E), S = 4, order 3
//     c 0, 1/2, 3/4, 1;  a2 1/2;  a3 0, 3/4;  a4 = b 2/9, 1/3, 4/9;  e 5/72, -1/12, -1/9, 1/8
//   VC_RK_ADAPTIVE_HEUN = 2  Heun-Euler 2(1), S = 3, order 2
//     c 0, 1, 1;  a2 1;  a3 = b 1/2, 1/2;  e 1/2, -1/2, 0
// The Hermite cubic, as ONE sequence of f32 operations (x = theta, d = y1 - y0, f0 = k1, f1 = kS):
//   c0 = 1 - x; c1 = x - 1; c2 = 1 - 2 x; w = x c1; h0 = c1 dt; h1 = x dt
//   y(x) = (c0 y0 + x y1) + w ((c2 d + h0 f0) + h1 f1)                          theta = 0 / 1: the bits of y0 / y1
// For bosh3 this is SciPy's RK23 dense output (its P rows are this cubic expanded).  The controller around these kernels
// (flux_sample.hip, transport.rk_integrate) is torchdiffeq's as recalled, unpinned against real torchdiffeq.
// Memory: elementwise passes over n elements with 2..7 k planes.  The W = 8 kernels move 16 bytes per access - eight bf16 of a k
// plane, four f32 of the state - wherever the address allows it (plane j starts at element j n: 16-byte aligned for every j only
// where n % 8 == 0, which every [B, N, 64] state is); the last n % 8 elements, and every element where a base is not 16-byte
// aligned (the launcher picks W = 1), run one by one through the SAME per-element expression.  The norm keeps dopri5.hip's deal of
// single elements to threads: its summation order is what makes it bit-equal to vc_dopri5_error_ratio.
#include "common.h"
#include "vcloze_internal.h"

#pragma clang fp contract(off)

namespace {

constexpr int RK_THREADS = 256;                        // = VC_DOPRI5_MAX_BLOCKS: pass 2 reduces one partial per thread
static_assert(RK_THREADS == VC_DOPRI5_MAX_BLOCKS, "pass 2 holds one block partial per thread");
constexpr int RK_PROBE = 7;                            // the probe stage of every method (dopri5.hip's stage 7)
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

// sum over the non-zero coefficients of `row`, left to right: ((c_a k_a + c_b k_b) + c_c k_c) + ...  (dopri5.hip: dp_combine)
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

// the block's 256 partial sums -> thread 0, always the same tree (dopri5.hip: dp_block_sum)
VC_DEV float rk_block_sum(float (&l)[RK_THREADS], float s) {
  const int t = threadIdx.x;
  l[t] = s;
  __syncthreads();
#pragma unroll
  for (int o = RK_THREADS / 2; o >= 1; o >>= 1) {
    if (t < o) l[t] += l[t + o];
    __syncthreads();
  }
  const float r = l[0];
  __syncthreads();
  return r;
}

// pass 1, the deal and the modes of dopri5_norm_kernel: the n elements go to the nblk * 256 threads round-robin, a thread adds its q^2
// in ascending order.  mode 0 takes the method's e row; modes 1..3 read y0, k1 and k2 - k1 (k2 holds the probe evaluation)
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
  s = rk_block_sum(l, s);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// pass 2: ONE block; the nblk <= 256 partials -> out[0] = sqrt(sum / n)
__global__ __launch_bounds__(RK_THREADS) void rk_norm_finish_kernel(const float* __restrict__ partial, float* __restrict__ out, int nblk, long n) {
  __shared__ float l[RK_THREADS];
  const float s = rk_block_sum(l, (int)threadIdx.x < nblk ? partial[threadIdx.x] : 0.0f);
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

// a grid of ceil(n / 256) blocks must fit the x dimension
inline bool rk_n_ok(int64_t n) { return n > 0 && n <= (int64_t)0x7fffffff * RK_THREADS; }
inline unsigned rk_blocks(int64_t n, int W) { return (unsigned)(((n + W - 1) / W + RK_THREADS - 1) / RK_THREADS); }
// null counts as aligned: a buffer the call does not use
inline bool rk_aligned16(std::initializer_list<const void*> ps) {
  for (const void* p : ps) if ((uintptr_t)p & 15) return false;
  return true;
}

}  // namespace

#define VC_CHECK_LAUNCH(name)                                                                     \
  do {                                                                                            \
    hipError_t e_ = hipGetLastError();                                                            \
    if (e_ != hipSuccess) { snprintf(err, errlen, name " launch: %s", hipGetErrorString(e_)); return VC_ERR_HIP; } \
    return VC_OK;                                                                                 \
  } while (0)

int vc_rk_stage_launch(int method, int stage, const float* y0, void* k, const void* v, const float* dt_ptr, const int32_t* eval_ptr,
                       float* y_stage, void* y_in, int64_t n, hipStream_t s, char* err, int errlen) {
  const int S = vc_rk_stages_of(method);
  if (!S) { snprintf(err, errlen, "rk_stage: unknown method %d (VC_RK_DOPRI5, VC_RK_BOSH3, VC_RK_ADAPTIVE_HEUN)", method); return VC_ERR_ARG; }
  if (!y0 || !k || !dt_ptr || !rk_n_ok(n) || (stage >= S && stage != RK_PROBE) || (stage < 0 && !eval_ptr) || (stage == S - 1 && !v) ||
      (stage == RK_PROBE && v) || (stage != S - 1 && !y_stage && !y_in)) {
    snprintf(err, errlen, "rk_stage: bad args (method %d: stage 0..%d, or < 0 with the evaluation counter; stage 7, the probe state, takes no v)",
             method, S - 1);
    return VC_ERR_ARG;
  }
  if (rk_aligned16({y0, k, v, y_stage, y_in}))
    hipLaunchKernelGGL(rk_stage_kernel<8>, dim3(rk_blocks(n, 8)), dim3(RK_THREADS), 0, s, method, stage, y0, (bf16_t*)k, (const bf16_t*)v, dt_ptr,
                       (const int*)eval_ptr, y_stage, (bf16_t*)y_in, (long)n);
  else
    hipLaunchKernelGGL(rk_stage_kernel<1>, dim3(rk_blocks(n, 1)), dim3(RK_THREADS), 0, s, method, stage, y0, (bf16_t*)k, (const bf16_t*)v, dt_ptr,
                       (const int*)eval_ptr, y_stage, (bf16_t*)y_in, (long)n);
  VC_CHECK_LAUNCH("rk_stage");
}

int vc_rk_error_ratio_launch(int method, int mode, const float* y0, const float* y1, const void* k, const float* dt_ptr, float rtol, float atol,
                             float* out, float* scratch, int64_t n, hipStream_t s, char* err, int errlen) {
  if (!vc_rk_stages_of(method)) {
    snprintf(err, errlen, "rk_error_ratio: unknown method %d (VC_RK_DOPRI5, VC_RK_BOSH3, VC_RK_ADAPTIVE_HEUN)", method);
    return VC_ERR_ARG;
  }
  if (mode < 0 || mode > 3 || !y0 || !out || !scratch || !rk_n_ok(n) || (mode == 0 && (!y1 || !dt_ptr)) || (mode != 1 && !k)) {
    snprintf(err, errlen, "rk_error_ratio: bad args (mode 0..3; mode 0 needs y1, k and dt, modes 2 and 3 need k)");
    return VC_ERR_ARG;
  }
  if (!(rtol >= 0.0f) || !(atol >= 0.0f) || !(rtol + atol > 0.0f) || !(rtol + atol - (rtol + atol) == 0.0f)) {
    snprintf(err, errlen, "rk_error_ratio: rtol = %g and atol = %g must be finite, non-negative and not both zero", rtol, atol);
    return VC_ERR_ARG;
  }
  const int64_t want = (n + RK_THREADS - 1) / RK_THREADS;
  const int nblk = (int)(want < VC_DOPRI5_MAX_BLOCKS ? want : VC_DOPRI5_MAX_BLOCKS);
  hipLaunchKernelGGL(rk_norm_kernel, dim3(nblk), dim3(RK_THREADS), 0, s, method, mode, y0, y1, (const bf16_t*)k, dt_ptr, rtol, atol, scratch,
                     (long)n);
  hipLaunchKernelGGL(rk_norm_finish_kernel, dim3(1), dim3(RK_THREADS), 0, s, (const float*)scratch, out, nblk, (long)n);
  VC_CHECK_LAUNCH("rk_error_ratio");
}

int vc_rk_interp_launch(int method, const float* y0, const float* y1, const void* k, const float* dt_ptr, float theta, void* out,
                        int out_is_bf16, int64_t n, hipStream_t s, char* err, int errlen) {
  if (method != VC_RK_BOSH3 && method != VC_RK_ADAPTIVE_HEUN) {
    snprintf(err, errlen, "rk_interp: method %d has no Hermite dense output (VC_RK_BOSH3, VC_RK_ADAPTIVE_HEUN; Dormand-Prince: vc_dopri5_interp)",
             method);
    return VC_ERR_ARG;
  }
  if (!y0 || !y1 || !k || !dt_ptr || !out || !rk_n_ok(n)) { snprintf(err, errlen, "rk_interp: bad args"); return VC_ERR_ARG; }
  if (!(theta >= 0.0f && theta <= 1.0f)) { snprintf(err, errlen, "rk_interp: theta = %g outside [0, 1]", theta); return VC_ERR_ARG; }
  const int last = vc_rk_stages_of(method) - 1;
  const bool vec = rk_aligned16({y0, y1, k, out});
#define RK_HERMITE(W, BF)                                                                                                              \
  hipLaunchKernelGGL((rk_hermite_kernel<W, BF>), dim3(rk_blocks(n, W)), dim3(RK_THREADS), 0, s, last, y0, y1, (const bf16_t*)k, dt_ptr, \
                     theta, out, (long)n)
  if (vec && out_is_bf16) RK_HERMITE(8, true);
  else if (vec) RK_HERMITE(8, false);
  else if (out_is_bf16) RK_HERMITE(1, true);
  else RK_HERMITE(1, false);
#undef RK_HERMITE
  VC_CHECK_LAUNCH("rk_interp");
}
