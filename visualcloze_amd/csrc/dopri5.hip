// The adaptive Dormand-Prince 5(4) solve: every arithmetic line between two model evaluations ("the adaptive
// solve").  f(t, y) = -model(bf16(y) || cond, 1 - f32(t)); every k is stored in bf16 (the model's output dtype), the state y is f32.
//   dopri5_stage        k[stage] = -v and the next stage's input state (or y1 after the sixth evaluation)
//   dopri5_error_ratio  the mixed-tolerance RMS norm of the embedded error estimate, and the three norms of the initial step size
//   dopri5_interp       the dense output: the quartic through (y0, f0, y_mid, y1, f1)
// The controller around them (flux_engine.hip, transport.dopri5_integrate) is torchdiffeq's AS RECALLED - the package was not
// available to check against: "unpinned against real torchdiffeq" - and pinned to SciPy's RK45 in the tableau and in single steps
// (tests/test_dopri5_cpu.py).
//
// The tableau (Dormand & Prince 1980; SciPy's RK45.C / .A / .B / .E), as doubles rounded ONCE to f32:
//   c    0, 1/5, 3/10, 4/5, 8/9, 1, 1                  (the seventh evaluation, k7 = f(t1, y1), is the next step's k1: FSAL)
//   a2   1/5
//   a3   3/40, 9/40
//   a4   44/45, -56/15, 32/9
//   a5   19372/6561, -25360/2187, 64448/6561, -212/729
//   a6   9017/3168, -355/33, 46732/5247, 49/176, -5103/18656
//   b    35/384, 0, 500/1113, 125/192, -2187/6784, 11/84                       (5th order: y1; also the row a7)
//   e    -71/57600, 0, 71/16695, -71/1920, 17253/339200, -22/525, 1/40         (b - b^, the 4th-order companion)
//   DPS_C_MID  6025192743/30085553152/2, 0, 51252292925/65400821598/2, -2691868925/45128329728/2,
//              187940372067/1594534317056/2, -1776094331/19743644256/2, 11237099/235043384/2        (y at t0 + dt/2)
// Every sum below is taken left to right over the NON-ZERO coefficients, one f32 operation after the other with floating-point
// contraction off: a torch f32 expression of the same shape (transport._dopri5_combine) gives the same bits.
#include "common.h"
#include "vcloze_internal.h"

namespace {

constexpr int DP_THREADS = 256;                        // = VC_DOPRI5_MAX_BLOCKS: pass 2 reduces one partial per thread
static_assert(DP_THREADS == VC_DOPRI5_MAX_BLOCKS, "pass 2 holds one block partial per thread");

// rows 0..4: a2..a6 (row s feeds the evaluation behind stage s), row 5: b, row 6: e, row 7: DPS_C_MID
__constant__ float DP_ROWS[8][7] = {
    {(float)(1.0 / 5.0), 0, 0, 0, 0, 0, 0},
    {(float)(3.0 / 40.0), (float)(9.0 / 40.0), 0, 0, 0, 0, 0},
    {(float)(44.0 / 45.0), (float)(-56.0 / 15.0), (float)(32.0 / 9.0), 0, 0, 0, 0},
    {(float)(19372.0 / 6561.0), (float)(-25360.0 / 2187.0), (float)(64448.0 / 6561.0), (float)(-212.0 / 729.0), 0, 0, 0},
    {(float)(9017.0 / 3168.0), (float)(-355.0 / 33.0), (float)(46732.0 / 5247.0), (float)(49.0 / 176.0), (float)(-5103.0 / 18656.0), 0, 0},
    {(float)(35.0 / 384.0), 0, (float)(500.0 / 1113.0), (float)(125.0 / 192.0), (float)(-2187.0 / 6784.0), (float)(11.0 / 84.0), 0},
    {(float)(-71.0 / 57600.0), 0, (float)(71.0 / 16695.0), (float)(-71.0 / 1920.0), (float)(17253.0 / 339200.0), (float)(-22.0 / 525.0),
     (float)(1.0 / 40.0)},
    {(float)(6025192743.0 / 30085553152.0 / 2.0), 0, (float)(51252292925.0 / 65400821598.0 / 2.0),
     (float)(-2691868925.0 / 45128329728.0 / 2.0), (float)(187940372067.0 / 1594534317056.0 / 2.0),
     (float)(-1776094331.0 / 19743644256.0 / 2.0), (float)(11237099.0 / 235043384.0 / 2.0)},
};

// sum over the non-zero coefficients of row `row`, left to right: ((c_a k_a + c_b k_b) + c_c k_c) + ...
VC_DEV float dp_combine(int row, const bf16_t* __restrict__ k, long n, long i) {
#pragma clang fp contract(off)
  float acc = 0.0f;
  bool first = true;
  for (int j = 0; j < 7; ++j) {
    const float c = DP_ROWS[row][j];
    if (c == 0.0f) continue;
    const float term = c * bf2f(k[(long)j * n + i]);
    acc = first ? term : acc + term;
    first = false;
  }
  return acc;
}

// stage 0..4: y_s = y0 + dt * (a row), stage 5: y1 = y0 + dt * (b row), stage 6: k7 alone, stage 7 (no v): the probe state
// y0 + dt * k1 of the initial step size.  v null: k[stage] is in place already (k1 of a step is the last step's k7)
__global__ __launch_bounds__(DP_THREADS) void dopri5_stage_kernel(int stage_arg, const float* __restrict__ y0, bf16_t* __restrict__ k,
                                                                  const bf16_t* __restrict__ v, const float* __restrict__ dt_ptr,
                                                                  const int* __restrict__ eval_ptr, float* __restrict__ y_stage,
                                                                  bf16_t* __restrict__ y_in, long n) {
#pragma clang fp contract(off)
  const long i = (long)blockIdx.x * DP_THREADS + threadIdx.x;
  if (i >= n) return;
  const int stage = stage_arg >= 0 ? stage_arg : *eval_ptr;
  if (stage < 0 || stage > 7) return;                   // a counter outside the step: nothing is read or written
  if (v && stage < 7) k[(long)stage * n + i] = f2bf(-bf2f(v[i]));      // the drift is -model(...): exact
  if (stage == 6) return;
  const float dt = *dt_ptr;
  const float acc = stage == 7 ? bf2f(k[i]) : dp_combine(stage, k, n, i);
  const float ys = y0[i] + dt * acc;
  if (y_stage) y_stage[i] = ys;
  if (y_in) y_in[i] = f2bf(ys);
}

// the block's 256 partial sums -> thread 0, always the same tree
VC_DEV float dp_block_sum(float (&l)[DP_THREADS], float s) {
  const int t = threadIdx.x;
  l[t] = s;
  __syncthreads();
#pragma unroll
  for (int o = DP_THREADS / 2; o >= 1; o >>= 1) {
    if (t < o) l[t] += l[t + o];
    __syncthreads();
  }
  const float r = l[0];
  __syncthreads();
  return r;
}

// pass 1: the n elements are dealt to the nblk * 256 threads round-robin, a thread adds its q^2 in ascending order.
//   mode 0  q = dt * (e row) / (atol + rtol * max(|y0|, |y1|))        the error ratio of a step
//   mode 1  q = y0 / (atol + rtol * |y0|)                              d0 of the initial step size
//   mode 2  q = k1 / (atol + rtol * |y0|)                              d1
//   mode 3  q = (k2 - k1) / (atol + rtol * |y0|)                       d2 * h0 (k2 holds the probe evaluation)
__global__ __launch_bounds__(DP_THREADS) void dopri5_norm_kernel(int mode, const float* __restrict__ y0, const float* __restrict__ y1,
                                                                 const bf16_t* __restrict__ k, const float* __restrict__ dt_ptr, float rtol,
                                                                 float atol, float* __restrict__ partial, long n) {
#pragma clang fp contract(off)
  __shared__ float l[DP_THREADS];
  const float dt = mode == 0 ? *dt_ptr : 0.0f;
  float s = 0.0f;
  for (long i = (long)blockIdx.x * DP_THREADS + threadIdx.x; i < n; i += (long)gridDim.x * DP_THREADS) {
    const float a0 = fabsf(y0[i]);
    float num, mag = a0;
    if (mode == 0) { num = dt * dp_combine(6, k, n, i); mag = fmaxf(a0, fabsf(y1[i])); }
    else if (mode == 1) num = y0[i];
    else if (mode == 2) num = bf2f(k[i]);
    else num = bf2f(k[n + i]) - bf2f(k[i]);
    const float q = num / (atol + rtol * mag);
    s = s + q * q;
  }
  s = dp_block_sum(l, s);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// pass 2: ONE block; the nblk <= 256 partials -> out[0] = sqrt(sum / n)
__global__ __launch_bounds__(DP_THREADS) void dopri5_norm_finish_kernel(const float* __restrict__ partial, float* __restrict__ out, int nblk,
                                                                        long n) {
  __shared__ float l[DP_THREADS];
  const float s = dp_block_sum(l, (int)threadIdx.x < nblk ? partial[threadIdx.x] : 0.0f);
  if (threadIdx.x == 0) out[0] = sqrtf(s / (float)n);
}

// torchdiffeq's _interp_fit / _interp_evaluate, operation by operation; theta = 0 and theta = 1 hand back y0 and y1 themselves
template <bool BF16>
__global__ __launch_bounds__(DP_THREADS) void dopri5_interp_kernel(const float* __restrict__ y0, const float* __restrict__ y1,
                                                                   const bf16_t* __restrict__ k, const float* __restrict__ dt_ptr, float x,
                                                                   void* __restrict__ out, long n) {
#pragma clang fp contract(off)
  const long i = (long)blockIdx.x * DP_THREADS + threadIdx.x;
  if (i >= n) return;
  const float a0 = y0[i], a1 = y1[i];
  float r;
  if (x == 0.0f) r = a0;
  else if (x == 1.0f) r = a1;
  else {
    const float dt = *dt_ptr;
    const float f0 = bf2f(k[i]), f1 = bf2f(k[6 * n + i]);
    const float ym = a0 + dt * dp_combine(7, k, n, i);
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
__global__ __launch_bounds__(DP_THREADS) void dopri5_load_kernel(const void* __restrict__ x, float* __restrict__ y0, bf16_t* __restrict__ y_in,
                                                                 long n) {
  const long i = (long)blockIdx.x * DP_THREADS + threadIdx.x;
  if (i >= n) return;
  const float v = BF16 ? bf2f(((const bf16_t*)x)[i]) : ((const float*)x)[i];
  y0[i] = v;
  y_in[i] = f2bf(v);
}

inline unsigned dp_blocks(int64_t n) { return (unsigned)((n + DP_THREADS - 1) / DP_THREADS); }
// a grid of ceil(n / 256) blocks must fit the x dimension
inline bool dp_n_ok(int64_t n) { return n > 0 && n <= (int64_t)0x7fffffff * DP_THREADS; }

}  // namespace

#define VC_CHECK_LAUNCH(name)                                                                     \
  do {                                                                                            \
    hipError_t e_ = hipGetLastError();                                                            \
    if (e_ != hipSuccess) { snprintf(err, errlen, name " launch: %s", hipGetErrorString(e_)); return VC_ERR_HIP; } \
    return VC_OK;                                                                                 \
  } while (0)

int vc_dopri5_stage_launch(int stage, const float* y0, void* k, const void* v, const float* dt_ptr, const int32_t* eval_ptr, float* y_stage,
                           void* y_in, int64_t n, hipStream_t s, char* err, int errlen) {
  if (!y0 || !k || !dt_ptr || !dp_n_ok(n) || stage > 7 || (stage < 0 && !eval_ptr) || (stage == 6 && !v) || (stage == 7 && v) ||
      (stage != 6 && !y_stage && !y_in)) {
    snprintf(err, errlen, "dopri5_stage: bad args (stage 0..6, or < 0 with the evaluation counter; stage 7, the probe state, takes no v)");
    return VC_ERR_ARG;
  }
  hipLaunchKernelGGL(dopri5_stage_kernel, dim3(dp_blocks(n)), dim3(DP_THREADS), 0, s, stage, y0, (bf16_t*)k, (const bf16_t*)v, dt_ptr,
                     (const int*)eval_ptr, y_stage, (bf16_t*)y_in, (long)n);
  VC_CHECK_LAUNCH("dopri5_stage");
}

int vc_dopri5_error_ratio_launch(int mode, const float* y0, const float* y1, const void* k, const float* dt_ptr, float rtol, float atol,
                                 float* out, float* scratch, int64_t n, hipStream_t s, char* err, int errlen) {
  if (mode < 0 || mode > 3 || !y0 || !out || !scratch || !dp_n_ok(n) || (mode == 0 && (!y1 || !dt_ptr)) || (mode != 1 && !k)) {
    snprintf(err, errlen, "dopri5_error_ratio: bad args (mode 0..3; mode 0 needs y1, k and dt, modes 2 and 3 need k)");
    return VC_ERR_ARG;
  }
  if (!(rtol >= 0.0f) || !(atol >= 0.0f) || !(rtol + atol > 0.0f) || !(rtol + atol - (rtol + atol) == 0.0f)) {
    snprintf(err, errlen, "dopri5_error_ratio: rtol = %g and atol = %g must be finite, non-negative and not both zero", rtol, atol);
    return VC_ERR_ARG;
  }
  const int64_t want = (n + DP_THREADS - 1) / DP_THREADS;
  const int nblk = (int)(want < VC_DOPRI5_MAX_BLOCKS ? want : VC_DOPRI5_MAX_BLOCKS);
  hipLaunchKernelGGL(dopri5_norm_kernel, dim3(nblk), dim3(DP_THREADS), 0, s, mode, y0, y1, (const bf16_t*)k, dt_ptr, rtol, atol, scratch,
                     (long)n);
  hipLaunchKernelGGL(dopri5_norm_finish_kernel, dim3(1), dim3(DP_THREADS), 0, s, (const float*)scratch, out, nblk, (long)n);
  VC_CHECK_LAUNCH("dopri5_error_ratio");
}

int vc_dopri5_interp_launch(const float* y0, const float* y1, const void* k, const float* dt_ptr, float theta, void* out, int out_is_bf16,
                            int64_t n, hipStream_t s, char* err, int errlen) {
  if (!y0 || !y1 || !k || !dt_ptr || !out || !dp_n_ok(n)) { snprintf(err, errlen, "dopri5_interp: bad args"); return VC_ERR_ARG; }
  if (!(theta >= 0.0f && theta <= 1.0f)) { snprintf(err, errlen, "dopri5_interp: theta = %g outside [0, 1]", theta); return VC_ERR_ARG; }
  if (out_is_bf16) hipLaunchKernelGGL(dopri5_interp_kernel<true>, dim3(dp_blocks(n)), dim3(DP_THREADS), 0, s, y0, y1, (const bf16_t*)k, dt_ptr,
                                      theta, out, (long)n);
  else hipLaunchKernelGGL(dopri5_interp_kernel<false>, dim3(dp_blocks(n)), dim3(DP_THREADS), 0, s, y0, y1, (const bf16_t*)k, dt_ptr, theta, out,
                          (long)n);
  VC_CHECK_LAUNCH("dopri5_interp");
}

int vc_dopri5_load_launch(const void* x, int x_is_bf16, float* y0, void* y_in, int64_t n, hipStream_t s, char* err, int errlen) {
  if (!x || !y0 || !y_in || !dp_n_ok(n)) { snprintf(err, errlen, "dopri5_load: bad args"); return VC_ERR_ARG; }
  if (x_is_bf16) hipLaunchKernelGGL(dopri5_load_kernel<true>, dim3(dp_blocks(n)), dim3(DP_THREADS), 0, s, x, y0, (bf16_t*)y_in, (long)n);
  else hipLaunchKernelGGL(dopri5_load_kernel<false>, dim3(dp_blocks(n)), dim3(DP_THREADS), 0, s, x, y0, (bf16_t*)y_in, (long)n);
  VC_CHECK_LAUNCH("dopri5_load");
}
