// Small elementwise kernels of the denoising path (all HBM/launch-bound, bf16 storage, f32 math).
//   timestep_embedding  layers.py:28-49      silu / add3   MLPEmbedder + vec sum, model.py:102-107
//   concat_cols         transport.py:193-196 (x || cond)
//   ode_stage           the update of the fixed-grid Euler step and the stage combinations of midpoint / rk4 (integrators.py:119, method=...)
//   cfg_combine         true classifier-free guidance over the two halves of a batch (Flux.forward_with_cfg, model.py:126-145)
#include "common.h"
#include "vcloze_internal.h"

namespace {

__global__ void temb_kernel(const float* __restrict__ t, const float* __restrict__ freqs, bf16_t* __restrict__ out,
                            int n, int half, int round_t) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n * half) return;
  const int b = i / half, k = i % half;
  float tt = 1000.0f * t[b];
  if (round_t) tt = rbf(1000.0f * rbf(t[b]));  // reference multiplies a bf16 tensor: product rounds to bf16
  const float arg = tt * freqs[k];
  out[(long)b * 2 * half + k] = f2bf(cosf(arg));
  out[(long)b * 2 * half + half + k] = f2bf(sinf(arg));
}

__global__ void silu_kernel(const bf16_t* __restrict__ x, bf16_t* __restrict__ y, long n) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) y[i] = f2bf(silu_f(bf2f(x[i])));
}

// y[i] = bf16(bf16(a[i] + b[i % bn]) + c[i % cn]): b, c broadcast over rows (vec = time + guidance + vector)
__global__ void add3_kernel(const bf16_t* __restrict__ a, const bf16_t* __restrict__ b, const bf16_t* __restrict__ c,
                            bf16_t* __restrict__ y, long n, long bn, long cn) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float v = rbf(bf2f(a[i]) + bf2f(b[i % bn]));
  if (c) v = v + bf2f(c[i % cn]);
  y[i] = f2bf(v);
}

// 16-B chunks; cx, cc multiples of 8
__global__ void concat_cols_kernel(const u32x4* __restrict__ x, int cxc, const u32x4* __restrict__ cond, int ccc,
                                   u32x4* __restrict__ out, long rows) {
  const int w = cxc + ccc;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows * w) return;
  const long r = i / w;
  const int c = (int)(i % w);
  out[i] = (c < cxc) ? x[r * cxc + c] : cond[r * ccc + (c - cxc)];
}

// SDEdit start state (visualcloze.py:221): x0 = bf16(bf16(noise*(1-s)) + bf16(latent*s)), s a python float (a double): torch
// multiplies the bf16 tensors by c = f32(1.0 - s), the subtraction done in DOUBLE, and by f32(s).  The launcher forms both
// factors from the double; 1.0f - f32(s) is a different f32 for 41 of the 99 strengths 0.01 .. 0.99.
__global__ void sdedit_mix_kernel(const bf16_t* __restrict__ noise, const bf16_t* __restrict__ latent, float c, float s,
                                  bf16_t* __restrict__ out, long n) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  out[i] = f2bf(rbf(bf2f(noise[i]) * c) + rbf(bf2f(latent[i]) * s));
}

// y[m, n] = bf16(act(x[m, n])) on row views: act 0 = GELU(tanh), 1 = SiLU
__global__ void act2d_kernel(const bf16_t* __restrict__ x, long ldx, bf16_t* __restrict__ y, long ldy, int rows, int cols, int act) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)rows * cols) return;
  const int m = (int)(i / cols), n = (int)(i % cols);
  const float v = bf2f(x[m * ldx + n]);
  y[m * ldy + n] = f2bf(act == 0 ? gelu_tanh(v) : silu_f(v));
}

// out[m, n] = bf16(res[m, n] + bf16(gate[n] * y[m, n])): the gated residual of layers.py:190-195,245 as its own pass
// (un-merged LoRA mode, where y = base + lora is only complete after a second GEMM)
__global__ void gate_residual_kernel(const bf16_t* __restrict__ y, long ldy, const bf16_t* __restrict__ res, long ldres,
                                     const bf16_t* __restrict__ gate, bf16_t* __restrict__ out, long ldo, int rows, int cols,
                                     const int* __restrict__ step_ptr, long gate_step_stride) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)rows * cols) return;
  const int m = (int)(i / cols), n = (int)(i % cols);
  const bf16_t* g = gate + (step_ptr ? (long)(*step_ptr) * gate_step_stride : 0);
  out[m * ldo + n] = f2bf(bf2f(res[m * ldres + n]) + rbf(bf2f(g[n]) * bf2f(y[m * ldy + n])));
}

// p[i] = bf16(v): the lora scale as the gate vector of the un-merged mode (vc_flux_set_lora_scale)
__global__ void fill_bf16_kernel(bf16_t* __restrict__ p, float v, long n) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = f2bf(v);
}

__global__ void step_advance_kernel(int* step_ptr) { if (threadIdx.x == 0 && blockIdx.x == 0) *step_ptr += 1; }

// ---- the solver update: every arithmetic line of a fixed-grid Euler / midpoint / rk4 (3/8 rule) step that is not a model evaluation ----
// The step functions are torchdiffeq 0.2.x's fixed-grid solvers AS RECALLED (the package was not available to check against:
// "unpinned against real torchdiffeq"), with f = -v the drift of transport.py:361-410 and torch's own roundings,
// operation by operation, for the device-resident operands the sampler hands torch: a bf16 tensor times the 0-dim f32 DEVICE
// tensor dt (or 0.5 * dt) multiplies by bf16(dt) (verified against torch: 100 % bitwise agreement), a bf16 tensor times a Python
// float multiplies by the float UNROUNDED (f32(1/3)), and every bf16 intermediate is materialised.  THE expressions, one place:
// ode_update = the bf16 term U that is added to y0 (in bf16 for a bf16 state, in f32 for an f32 state - torch's promotion of
// f32 + bf16; integrators.py:119 keeps the state's dtype):
//   euler     stage 0: y1 = y0 + dt * f0                             (= the last midpoint stage)
//   midpoint  stage 0: y_mid = y0 + f0 * half_dt                     stage 1: y1 = y0 + dt * f1
//   rk4       stage 0: y0 + dt * k1 * (1/3)                          stage 1: y0 + dt * (k2 - k1 * (1/3))
//             stage 2: y0 + dt * (k1 - k2 + k3)                      stage 3: y1 = y0 + (k1 + 3 * (k2 + k3) + k4) * dt * 0.125
VC_DEV float ode_update(int method, int stage, float dtb, float hdb, float f, float k1, float k2, float k3) {
#pragma clang fp contract(off)
  const float c13 = (float)(1.0 / 3.0);
  if (method != VC_SOLVER_RK4) return method == VC_SOLVER_MIDPOINT && stage == 0 ? rbf(f * hdb) : rbf(dtb * f);
  switch (stage) {
    case 0: return rbf(rbf(dtb * f) * c13);
    case 1: return rbf(dtb * rbf(f - rbf(k1 * c13)));
    case 2: return rbf(dtb * rbf(rbf(k1 - k2) + f));
    default: return rbf(rbf(rbf(rbf(k1 + rbf(3.0f * rbf(k2 + k3))) + f) * dtb) * 0.125f);
  }
}

// One chunk of W elements per thread: W = 8 (16-byte accesses of the bf16 arrays, two of the f32 state) or 1.  Stage j keeps k_{j+1}
// where a later stage reads it (rk4, j < 3), writes the next evaluation's bf16 input y_in (the bf16 shadow of an f32 state: its
// Linear rounds the f32 input to bf16 under autocast, visualcloze.py:363; null where the bf16 state itself is read next), and the
// LAST stage updates the state.  v == nullptr: y_in = bf16(y) only, the state is untouched.
template <bool F32, int W>
__global__ void ode_stage_kernel(int method, int stage_arg, void* __restrict__ y, const bf16_t* __restrict__ v, bf16_t* __restrict__ k,
                                 bf16_t* __restrict__ y_in, const float* __restrict__ dts, const int* __restrict__ eval_ptr, long n) {
#pragma clang fp contract(off)
  const long c = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (c * W >= n) return;
  float f[W], k1[W], k2[W], k3[W], y0[W];
  auto load = [&](const bf16_t* p, float (&o)[W]) {
    if constexpr (W == 8) {
      const u32x4 w = ((const u32x4*)p)[c];
#pragma unroll
      for (int i = 0; i < 4; ++i) { o[2 * i] = lo_bf(w[i]); o[2 * i + 1] = hi_bf(w[i]); }
    } else {
      o[0] = bf2f(p[c]);
    }
  };
  auto store = [&](bf16_t* p, const float (&o)[W]) {
    if constexpr (W == 8) {
      u32x4 w;
#pragma unroll
      for (int i = 0; i < 4; ++i) w[i] = pack2bf(o[2 * i], o[2 * i + 1]);
      ((u32x4*)p)[c] = w;
    } else {
      p[c] = f2bf(o[0]);
    }
  };
  if constexpr (F32) {
    if constexpr (W == 8) {
      const f32x4 a = ((const f32x4*)y)[2 * c], b = ((const f32x4*)y)[2 * c + 1];
#pragma unroll
      for (int i = 0; i < 4; ++i) { y0[i] = a[i]; y0[4 + i] = b[i]; }
    } else {
      y0[0] = ((const float*)y)[c];
    }
  } else {
    load((const bf16_t*)y, y0);
  }
  if (!v) { store(y_in, y0); return; }
  const int evals = vc_evals_of(method);
  const int e = eval_ptr ? *eval_ptr : 0;
  const int stage = stage_arg >= 0 ? stage_arg : e % evals;
  const float dt = dts[e / evals];
  const float dtb = rbf(dt), hdb = rbf(0.5f * dt);
  const bool rk4 = method == VC_SOLVER_RK4, last = stage == evals - 1;
  load(v, f);
#pragma unroll
  for (int i = 0; i < W; ++i) { f[i] = -f[i]; k1[i] = k2[i] = k3[i] = 0.0f; }       // the drift is -model(...): exact
  if (rk4 && stage >= 1) load(k, k1);
  if (rk4 && stage >= 2) load(k + n, k2);
  if (rk4 && stage == 3) load(k + 2 * n, k3);
  if (rk4 && !last) store(k + (long)stage * n, f);
  float y1[W];
#pragma unroll
  for (int i = 0; i < W; ++i) {
    const float s = y0[i] + ode_update(method, stage, dtb, hdb, f[i], k1[i], k2[i], k3[i]);
    y1[i] = F32 ? s : rbf(s);
  }
  if (y_in) store(y_in, y1);
  if (!last) return;
  if constexpr (F32) {
    if constexpr (W == 8) {
      f32x4 a, b;
#pragma unroll
      for (int i = 0; i < 4; ++i) { a[i] = y1[i]; b[i] = y1[4 + i]; }
      ((f32x4*)y)[2 * c] = a; ((f32x4*)y)[2 * c + 1] = b;
    } else {
      ((float*)y)[c] = y1[0];
    }
  } else {
    store((bf16_t*)y, y1);
  }
}

// ---- true classifier-free guidance (Flux.forward_with_cfg, models/model.py:126-145): cond_v = uncond_v + cfg_scale * (cond_v - uncond_v) ----
// with torch's roundings for bf16 tensors and a Python float, operation by operation: out = bf16(u + bf16(f32(s) * bf16(c - u))), every
// op in f32, s NOT rounded to bf16, no fused multiply-add.  One chunk of W elements per thread (W = 8: 16-byte accesses, or 1); a
// thread reads its chunk of c and u before it writes the same chunk of out, so out may BE c or u (no __restrict__)
template <int W>
__global__ void cfg_combine_kernel(const bf16_t* c, const bf16_t* u, bf16_t* out, float s, long n) {
#pragma clang fp contract(off)
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t * W >= n) return;
  if constexpr (W == 8) {
    const u32x4 cw = ((const u32x4*)c)[t], uw = ((const u32x4*)u)[t];
    u32x4 o;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float ul = lo_bf(uw[i]), uh = hi_bf(uw[i]);
      o[i] = pack2bf(ul + rbf(s * rbf(lo_bf(cw[i]) - ul)), uh + rbf(s * rbf(hi_bf(cw[i]) - uh)));
    }
    ((u32x4*)out)[t] = o;
  } else {
    const float uf = bf2f(u[t]);
    out[t] = f2bf(uf + rbf(s * rbf(bf2f(c[t]) - uf)));
  }
}

}  // namespace

int vc_temb_launch(const float* t, const float* freqs, void* out, int n, int half, int round_t, hipStream_t s, char* err, int errlen) {
  if (!t || !freqs || !out || n <= 0 || half <= 0) { snprintf(err, errlen, "timestep_embedding: bad args"); return VC_ERR_ARG; }
  hipLaunchKernelGGL(temb_kernel, dim3((n * half + 255) / 256), dim3(256), 0, s, t, freqs, (bf16_t*)out, n, half, round_t);
  return vc_launch_status("timestep_embedding launch", err, errlen);
}
int vc_silu_launch(const void* x, void* y, int64_t n, hipStream_t s, char* err, int errlen) {
  if (!x || !y || n <= 0) { snprintf(err, errlen, "silu: bad args"); return VC_ERR_ARG; }
  hipLaunchKernelGGL(silu_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const bf16_t*)x, (bf16_t*)y, (long)n);
  return vc_launch_status("silu launch", err, errlen);
}
int vc_act2d_launch(const void* x, int64_t ldx, void* y, int64_t ldy, int32_t rows, int32_t cols, int32_t act, hipStream_t s,
                    char* err, int errlen) {
  if (!x || !y || rows <= 0 || cols <= 0 || act < 0 || act > 1) { snprintf(err, errlen, "act2d: bad args"); return VC_ERR_ARG; }
  const long n = (long)rows * cols;
  hipLaunchKernelGGL(act2d_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const bf16_t*)x, (long)ldx, (bf16_t*)y,
                     (long)ldy, rows, cols, act);
  return vc_launch_status("act2d launch", err, errlen);
}
int vc_gate_residual_launch(const void* y, int64_t ldy, const void* res, int64_t ldres, const void* gate, void* out, int64_t ldo,
                            int32_t rows, int32_t cols, const int32_t* step_ptr, int64_t gate_step_stride, hipStream_t s,
                            char* err, int errlen) {
  if (!y || !res || !gate || !out || rows <= 0 || cols <= 0) { snprintf(err, errlen, "gate_residual: bad args"); return VC_ERR_ARG; }
  const long n = (long)rows * cols;
  hipLaunchKernelGGL(gate_residual_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const bf16_t*)y, (long)ldy,
                     (const bf16_t*)res, (long)ldres, (const bf16_t*)gate, (bf16_t*)out, (long)ldo, rows, cols, step_ptr,
                     (long)gate_step_stride);
  return vc_launch_status("gate_residual launch", err, errlen);
}
int vc_add3_launch(const void* a, const void* b, const void* c, void* y, int64_t n, int64_t bn, int64_t cn, hipStream_t s, char* err, int errlen) {
  if (!a || !b || !y || n <= 0 || bn <= 0 || (c && cn <= 0)) { snprintf(err, errlen, "add3: bad args"); return VC_ERR_ARG; }
  hipLaunchKernelGGL(add3_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const bf16_t*)a, (const bf16_t*)b, (const bf16_t*)c, (bf16_t*)y, (long)n, (long)bn, (long)(c ? cn : 1));
  return vc_launch_status("add3 launch", err, errlen);
}
int vc_concat_cols_launch(const void* x, int cx, const void* cond, int cc, void* out, int64_t rows, hipStream_t s, char* err, int errlen) {
  if (!x || !cond || !out || rows <= 0 || cx <= 0 || cc <= 0 || cx % 8 || cc % 8) { snprintf(err, errlen, "concat_cols: need cx, cc positive multiples of 8"); return VC_ERR_ARG; }
  const long n = rows * ((cx + cc) / 8);
  hipLaunchKernelGGL(concat_cols_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const u32x4*)x, cx / 8, (const u32x4*)cond, cc / 8, (u32x4*)out, (long)rows);
  return vc_launch_status("concat_cols launch", err, errlen);
}
// the one launch behind vc_euler_step, vc_euler_step_f32 and vc_ode_stage, which check their own arguments (`what`: the caller's
// prefix of a launch error).  y_in may be null (the state alone is written), v may be null (y_in = bf16(y) alone, f32 state)
int vc_ode_update_launch(const char* what, int method, int stage, void* y, int state_is_bf16, const void* v, void* k, void* y_in,
                         const float* dts, const int32_t* eval_ptr, int64_t n, hipStream_t s, char* err, int errlen) {
  // 16-byte accesses: every base 16-byte aligned and n a multiple of 8 (k2, k3 start n and 2n elements into k); else element-wise
  const uintptr_t bases = (uintptr_t)y | (uintptr_t)v | (uintptr_t)k | (uintptr_t)y_in;
  const bool vec = n % 8 == 0 && (bases & 15) == 0;
  const long threads = vec ? n / 8 : n;
  const dim3 grid((unsigned)((threads + 255) / 256)), block(256);
#define VC_ODE_LAUNCH(F32, W)                                                                                               \
  hipLaunchKernelGGL((ode_stage_kernel<F32, W>), grid, block, 0, s, method, stage, y, (const bf16_t*)v, (bf16_t*)k, (bf16_t*)y_in, dts, \
                     (const int*)eval_ptr, (long)n)
  if (state_is_bf16) { if (vec) VC_ODE_LAUNCH(false, 8); else VC_ODE_LAUNCH(false, 1); }
  else { if (vec) VC_ODE_LAUNCH(true, 8); else VC_ODE_LAUNCH(true, 1); }
#undef VC_ODE_LAUNCH
  return vc_launch_status(what, err, errlen);
}
int vc_euler_launch(void* x, const void* v, const float* dts, const int32_t* step_ptr, int64_t n, hipStream_t s, char* err, int errlen) {
  if (!x || !v || !dts || n <= 0) { snprintf(err, errlen, "euler_step: bad args"); return VC_ERR_ARG; }
  return vc_ode_update_launch("euler_step launch", VC_SOLVER_EULER, 0, x, 1, v, nullptr, nullptr, dts, step_ptr, n, s, err, errlen);
}
int vc_euler_f32_launch(float* x32, void* shadow, const void* v, const float* dts, const int32_t* step_ptr, int64_t n, hipStream_t s,
                        char* err, int errlen) {
  if (!x32 || !shadow || (v && !dts) || n <= 0) { snprintf(err, errlen, "euler_step_f32: bad args"); return VC_ERR_ARG; }
  return vc_ode_update_launch("euler_step_f32 launch", VC_SOLVER_EULER, 0, x32, 0, v, nullptr, shadow, dts, step_ptr, n, s, err, errlen);
}
int vc_ode_stage_launch(int method, int stage, void* y, int state_is_bf16, const void* v, void* k, void* y_in, const float* dts,
                        const int32_t* eval_ptr, int64_t n, hipStream_t s, char* err, int errlen) {
  const int evals = vc_evals_of(method);
  if (evals < 2) { snprintf(err, errlen, "ode_stage: method %d is not VC_SOLVER_MIDPOINT or VC_SOLVER_RK4", method); return VC_ERR_ARG; }
  if (!y || !v || !y_in || !dts || n <= 0 || stage >= evals || (stage < 0 && !eval_ptr) || (method == VC_SOLVER_RK4 && !k)) {
    snprintf(err, errlen, "ode_stage: bad args");
    return VC_ERR_ARG;
  }
  return vc_ode_update_launch("ode_stage launch", method, stage, y, state_is_bf16, v, k, y_in, dts, eval_ptr, n, s, err, errlen);
}
int vc_cfg_combine_launch(const void* cond, const void* uncond, void* out, int64_t n, float cfg_scale, hipStream_t s, char* err, int errlen) {
  if (!cond || !uncond || !out) { snprintf(err, errlen, "cfg_combine: null pointer"); return VC_ERR_ARG; }
  if (n <= 0) { snprintf(err, errlen, "cfg_combine: n = %lld must be positive", (long long)n); return VC_ERR_ARG; }
  if (!(cfg_scale - cfg_scale == 0.0f)) { snprintf(err, errlen, "cfg_combine: cfg_scale is not finite"); return VC_ERR_ARG; }
  // out may BE cond or uncond (each element is read before it is written); any other overlap would read written elements
  const uintptr_t o = (uintptr_t)out, bytes = (uintptr_t)n * 2;
  const uintptr_t ins[2] = {(uintptr_t)cond, (uintptr_t)uncond};
  for (const uintptr_t a : ins) {
    if (a != o && a < o + bytes && o < a + bytes) { snprintf(err, errlen, "cfg_combine: out partially overlaps an input (it may only BE cond or uncond)"); return VC_ERR_ARG; }
  }
  // 16-byte accesses: every base 16-byte aligned and n a multiple of 8; else element-wise (the idiom of vc_ode_update_launch)
  const bool vec = n % 8 == 0 && (((uintptr_t)cond | (uintptr_t)uncond | o) & 15) == 0;
  const long threads = vec ? n / 8 : n;
  const dim3 grid((unsigned)((threads + 255) / 256)), block(256);
  if (vec) hipLaunchKernelGGL(cfg_combine_kernel<8>, grid, block, 0, s, (const bf16_t*)cond, (const bf16_t*)uncond, (bf16_t*)out, cfg_scale, (long)n);
  else hipLaunchKernelGGL(cfg_combine_kernel<1>, grid, block, 0, s, (const bf16_t*)cond, (const bf16_t*)uncond, (bf16_t*)out, cfg_scale, (long)n);
  return vc_launch_status("cfg_combine launch", err, errlen);
}
int vc_fill_bf16_launch(void* p, float value, int64_t n, hipStream_t s, char* err, int errlen) {
  if (!p || n <= 0) { snprintf(err, errlen, "fill_bf16: bad args"); return VC_ERR_ARG; }
  hipLaunchKernelGGL(fill_bf16_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (bf16_t*)p, value, (long)n);
  return vc_launch_status("fill_bf16 launch", err, errlen);
}
int vc_step_advance_launch(int32_t* step_ptr, hipStream_t s, char* err, int errlen) {
  if (!step_ptr) { snprintf(err, errlen, "step_advance: null"); return VC_ERR_ARG; }
  hipLaunchKernelGGL(step_advance_kernel, dim3(1), dim3(64), 0, s, step_ptr);
  return vc_launch_status("step_advance launch", err, errlen);
}
int vc_sdedit_mix_launch(const void* noise, const void* latent, double strength, void* out, int64_t n, hipStream_t s, char* err, int errlen) {
  if (!noise || !latent || !out || n <= 0) { snprintf(err, errlen, "sdedit_mix: bad args"); return VC_ERR_ARG; }
  hipLaunchKernelGGL(sdedit_mix_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const bf16_t*)noise, (const bf16_t*)latent,
                     (float)(1.0 - strength), (float)strength, (bf16_t*)out, (long)n);
  return vc_launch_status("sdedit_mix launch", err, errlen);
}
