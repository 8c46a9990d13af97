// Noise source: the counter-based Gaussian stream of include/vcloze_hip.h (Philox4x32-10 + Box-Muller in f32).
//   randn          out[i] = element offset + i of the stream of `seed`, as bf16 / f32 / the raw 32-bit word
//   randn_tokens   a [C, h, w] draw written as bf16 straight into pack_latent's token layout (pack.hip): the sampler's x(t0)
// Every element depends on (seed, position) only: a thread recomputes the Philox block(s) of whatever positions it stores, so
// the launch geometry, the split of a draw into calls and the layout written do not show in the values.  Store-rate kernels
// (about 100 integer and 20 float operations per block of 4 outputs): the draws of a grid are ~0.2 M values, nothing here is
// tuned beyond 16-byte stores and a capped grid.  seed / offset are kernel arguments by value: legal under stream capture, and
// a replayed graph repeats its noise.
//   sde_stage      the stochastic sampler's update: the same normals drawn in place, seed / offset read from DEVICE memory and the draw
//                  index taken from the device-side evaluation counter - a replayed graph draws fresh, reproducible noise
//
// Precision: ln, sqrt and sin/cos are the PRECISE device functions (logf, sqrtf, sincospif on the exact argument 2*u2, a few f32
// ulps each), not the bare v_log_f32 / v_sin_f32 approximations, whose error near u1 = 1 (ln u1 -> 0) and absolute error of the
// sine no guide states: the stream is a contract a host restates, and the budget of tests/test_noise_gpu.py (1/64 bf16 ulp of r
// against the fp64 value, i.e. >= 2^-14 r) is met with room by ~6 f32 roundings (2^-21 r), whatever u1 and u2.
#include "common.h"
#include "vcloze_internal.h"
#include "rng_device.h"

namespace {

constexpr int RNG_MAX_BLOCKS = 2048;      // 8 workgroups of 256 per CU of a 256-CU device; the grid-stride loop takes the rest

// Work items: `nvec` 16-byte chunks first (elements head + w*E ..: out + head is 16-byte aligned and offset + head a multiple
// of 4, so a chunk is one (f32 / u32) or two (bf16) whole blocks), then the n - nvec*E single elements of the head and the tail.
// Where the phase does not allow chunks (offset + head not a multiple of 4) the host passes head = n, nvec = 0.
template <int DT>
__global__ __launch_bounds__(256) void randn_kernel(void* __restrict__ out, long n, uint64_t seed, uint64_t offset, long head, long nvec) {
  constexpr int E = DT == VC_RNG_BF16 ? 8 : 4;
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  const long total = nvec + (n - nvec * E);
  for (long wi = blockIdx.x * 256L + threadIdx.x; wi < total; wi += gridDim.x * 256L) {
    if (wi < nvec) {
      const long i = head + wi * E;
      const uint64_t b = (offset + (uint64_t)i) >> 2;
      uint32_t v[4];
      block_words<DT>(b, k0, k1, v);
      u32x4 o;
      if (DT == VC_RNG_BF16) {
        uint32_t v2[4];
        block_words<DT>(b + 1, k0, k1, v2);
        o[0] = pack2(v[0], v[1]); o[1] = pack2(v[2], v[3]); o[2] = pack2(v2[0], v2[1]); o[3] = pack2(v2[2], v2[3]);
        *(u32x4*)((bf16_t*)out + i) = o;
      } else {
        o[0] = v[0]; o[1] = v[1]; o[2] = v[2]; o[3] = v[3];
        *(u32x4*)((uint32_t*)out + i) = o;
      }
    } else {
      const long s = wi - nvec, i = s < head ? s : s + nvec * E;     // the head, then the tail behind the chunks
      const uint64_t p = offset + (uint64_t)i;
      uint32_t v[4];
      block_words<DT>(p >> 2, k0, k1, v);
      const uint32_t word = pick(v, (uint32_t)p & 3u);
      if (DT == VC_RNG_BF16) ((bf16_t*)out)[i] = f2bf(__builtin_bit_cast(float, word));
      else ((uint32_t*)out)[i] = word;
    }
  }
}

// out[tok * ld + col0 + c*4 + ph*2 + pw] = bf16(z(offset + (c*h + 2*hh + ph)*w + 2*ww + pw)),  tok = hh*(w/2) + ww: a thread
// writes one 16-byte chunk (2 channels x 2 x 2) of a token row; each of its four words is the pair (pw 0, pw 1) at consecutive
// positions, one block unless the pair starts at the last element of one
__global__ __launch_bounds__(256) void randn_tokens_kernel(bf16_t* __restrict__ out, int C, int h, int w, long ld, int col0, uint64_t seed,
                                                          uint64_t offset) {
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  const int w2 = w >> 1, cpt = C >> 1;
  const long total = (long)(h >> 1) * w2 * cpt;
  for (long wi = blockIdx.x * 256L + threadIdx.x; wi < total; wi += gridDim.x * 256L) {
    const long tok = wi / cpt;
    const int ck = (int)(wi - tok * cpt), hh = (int)(tok / w2), ww = (int)(tok - (long)hh * w2);
    u32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int c = 2 * ck + (e >> 1), ph = e & 1;
      const uint64_t p = offset + ((uint64_t)c * h + 2 * hh + ph) * w + 2 * ww;
      const uint32_t j = (uint32_t)p & 3u;
      uint32_t v[4];
      block_words<VC_RNG_BF16>(p >> 2, k0, k1, v);
      uint32_t hi = pick(v, (j + 1) & 3u);
      if (j == 3) {
        uint32_t v2[4];
        block_words<VC_RNG_BF16>((p >> 2) + 1, k0, k1, v2);
        hi = v2[0];
      }
      o[e] = pack2(pick(v, j), hi);
    }
    *(u32x4*)(out + tok * ld + col0 + ck * 8) = o;
  }
}

int grid_for(long total) { return (int)((total + 255) / 256 < RNG_MAX_BLOCKS ? (total + 255) / 256 : RNG_MAX_BLOCKS); }

// ---- the stochastic sampler's update (vcloze_hip.h: vc_sde_stage): one row (mode, h, A, Bc, g) of the table per evaluation, the
// noise drawn in place from the stream above.  Here - and not beside the other solver updates - because the normals must be the
// VC_RNG_F32 values bit for bit: the same device functions, compiled once.
struct SdeRow { int mode; float h, A, Bc, g; };
struct SdeIo { float y, xhat, k1, y_in; };     // in: what the mode reads (else 0); out: what it stores
// one element of one row, f32, one operation after the other: the torch expression of transport.sde_integrate gives the same bits.
// vel = -v, the velocity; z is read only where g != 0 (g == 0: no noise is added, not even a signed zero)
VC_DEV SdeIo sde_element(const SdeRow& r, const SdeIo& in, float vel, float z) {
#pragma clang fp contract(off)
  SdeIo o = in;
  if (r.mode == VC_SDE_EM || r.mode == VC_SDE_LAST) {
    float yn = in.y + r.h * (r.A * vel - r.Bc * in.y);
    if (r.mode == VC_SDE_EM && r.g != 0.0f) yn = yn + r.g * z;
    o.y = yn; o.y_in = yn;
  } else if (r.mode == VC_SDE_HEUN1) {
    const float K1 = r.A * vel - r.Bc * in.xhat;
    const float xp = in.xhat + r.h * K1;
    o.k1 = K1; o.y = xp; o.y_in = xp;
  } else if (r.mode == VC_SDE_HEUN2) {
    const float K2 = r.A * vel - r.Bc * in.y;
    const float xn = in.xhat + r.h * (in.k1 + K2);
    const float xh = r.g != 0.0f ? xn + r.g * z : xn;
    o.y = xn; o.xhat = xh; o.y_in = xh;
  } else {                                          // VC_SDE_INJECT
    const float xh = r.g != 0.0f ? in.y + r.g * z : in.y;
    o.xhat = xh; o.y_in = xh;
  }
  return o;
}

// work items: `nvec` chunks of 8 elements (16-byte accesses: the host found every base 16-byte aligned), then the n - 8 nvec single
// elements of the tail.  Everything the row decides (what is read, what is stored, whether noise is drawn) is uniform over the grid.
__global__ __launch_bounds__(256) void sde_stage_kernel(int eval_arg, const float* __restrict__ table, int n_rows, float* __restrict__ y,
                                                        const bf16_t* __restrict__ v, bf16_t* __restrict__ y_in, float* __restrict__ xhat,
                                                        float* __restrict__ k1, const uint64_t* __restrict__ rng,
                                                        const int* __restrict__ eval_ptr, long n, long nvec) {
  const int ev = eval_arg >= 0 ? eval_arg : *eval_ptr;
  if (ev < 0 || ev >= n_rows) return;                // a counter outside the table: nothing is read or written
  const float* row = table + (long)ev * VC_SDE_ROW;
  const SdeRow r{(int)row[0], row[1], row[2], row[3], row[4]};
  if (r.mode < VC_SDE_EM || r.mode > VC_SDE_INJECT) return;
  const bool heun = r.mode == VC_SDE_HEUN1 || r.mode == VC_SDE_HEUN2;
  if ((r.mode != VC_SDE_INJECT && !v) || ((heun || r.mode == VC_SDE_INJECT) && !xhat) || (heun && !k1)) return;   // a row the call has no buffers for
  const bool rd_y = r.mode != VC_SDE_HEUN1, rd_xh = heun, rd_k1 = r.mode == VC_SDE_HEUN2, rd_v = r.mode != VC_SDE_INJECT;
  const bool wr_y = r.mode != VC_SDE_INJECT, wr_xh = r.mode == VC_SDE_HEUN2 || r.mode == VC_SDE_INJECT, wr_k1 = r.mode == VC_SDE_HEUN1;
  const bool noisy = r.g != 0.0f && (r.mode == VC_SDE_EM || r.mode == VC_SDE_HEUN2 || r.mode == VC_SDE_INJECT);
  // draw d of the trajectory: the step an Euler-Maruyama row belongs to, the NEXT step behind a Heun row (its noise is injected ahead
  // of that step's first evaluation), draw 0 for the injection in front of the first step
  const uint64_t d = r.mode == VC_SDE_EM ? (uint64_t)ev : r.mode == VC_SDE_HEUN2 ? (uint64_t)(ev + 1) >> 1 : 0;
  const uint32_t k0 = (uint32_t)rng[0], kk1 = (uint32_t)(rng[0] >> 32);
  const uint64_t p0 = rng[1] + d * (uint64_t)n;
  const long total = nvec + (n - nvec * 8);
  for (long wi = blockIdx.x * 256L + threadIdx.x; wi < total; wi += gridDim.x * 256L) {
    if (wi < nvec) {
      const long i = wi * 8;
      float z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      if (noisy) {
        const uint64_t p = p0 + (uint64_t)i;
        switch ((uint32_t)p & 3u) {
          case 0: normals8<0>(p, k0, kk1, z); break;
          case 1: normals8<1>(p, k0, kk1, z); break;
          case 2: normals8<2>(p, k0, kk1, z); break;
          default: normals8<3>(p, k0, kk1, z); break;
        }
      }
      f32x4 yv[2] = {}, xv[2] = {}, kv[2] = {};
      u32x4 vv = {0, 0, 0, 0};
      if (rd_y) { yv[0] = *(const f32x4*)(y + i); yv[1] = *(const f32x4*)(y + i + 4); }
      if (rd_xh) { xv[0] = *(const f32x4*)(xhat + i); xv[1] = *(const f32x4*)(xhat + i + 4); }
      if (rd_k1) { kv[0] = *(const f32x4*)(k1 + i); kv[1] = *(const f32x4*)(k1 + i + 4); }
      if (rd_v) vv = *(const u32x4*)(v + i);
      f32x4 yo[2], xo[2], ko[2];
      float in8[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float vel = -((e & 1) ? hi_bf(vv[e >> 1]) : lo_bf(vv[e >> 1]));       // the drift's sign: exact
        const SdeIo o = sde_element(r, SdeIo{yv[e >> 2][e & 3], xv[e >> 2][e & 3], kv[e >> 2][e & 3], 0.0f}, vel, z[e]);
        yo[e >> 2][e & 3] = o.y; xo[e >> 2][e & 3] = o.xhat; ko[e >> 2][e & 3] = o.k1; in8[e] = o.y_in;
      }
      if (wr_y) { *(f32x4*)(y + i) = yo[0]; *(f32x4*)(y + i + 4) = yo[1]; }
      if (wr_xh) { *(f32x4*)(xhat + i) = xo[0]; *(f32x4*)(xhat + i + 4) = xo[1]; }
      if (wr_k1) { *(f32x4*)(k1 + i) = ko[0]; *(f32x4*)(k1 + i + 4) = ko[1]; }
      u32x4 w;
#pragma unroll
      for (int e = 0; e < 4; ++e) w[e] = pack2bf(in8[2 * e], in8[2 * e + 1]);
      *(u32x4*)(y_in + i) = w;
    } else {
      const long i = nvec * 8 + (wi - nvec);
      const float z = noisy ? normal_at(p0 + (uint64_t)i, k0, kk1) : 0.0f;
      const float vel = rd_v ? -bf2f(v[i]) : 0.0f;
      const SdeIo o = sde_element(r, SdeIo{rd_y ? y[i] : 0.0f, rd_xh ? xhat[i] : 0.0f, rd_k1 ? k1[i] : 0.0f, 0.0f}, vel, z);
      if (wr_y) y[i] = o.y;
      if (wr_xh) xhat[i] = o.xhat;
      if (wr_k1) k1[i] = o.k1;
      y_in[i] = f2bf(o.y_in);
    }
  }
}

// the F32 state -> the caller's buffer (a trajectory row, the result): bf16 rounded once, or F32 as it is
template <bool BF16>
__global__ __launch_bounds__(256) void sde_store_kernel(const float* __restrict__ y, void* __restrict__ out, long n) {
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += gridDim.x * 256L) {
    if (BF16) ((bf16_t*)out)[i] = f2bf(y[i]);
    else ((float*)out)[i] = y[i];
  }
}

}  // namespace

int vc_randn_launch(void* out, int dtype, int64_t n, uint64_t seed, uint64_t offset, hipStream_t s, char* err, int errlen) {
  if (!out) { snprintf(err, errlen, "randn: null output pointer"); return VC_ERR_ARG; }
  if (n <= 0) { snprintf(err, errlen, "randn: n = %lld, need n >= 1", (long long)n); return VC_ERR_ARG; }
  if (dtype != VC_RNG_BF16 && dtype != VC_RNG_F32 && dtype != VC_RNG_U32) {
    snprintf(err, errlen, "randn: unknown dtype %d (VC_RNG_BF16, VC_RNG_F32, VC_RNG_U32)", dtype); return VC_ERR_ARG; }
  if ((uint64_t)n - 1 > UINT64_MAX - offset) {          // the last position is offset + n - 1
    snprintf(err, errlen, "randn: offset + n wraps the 64-bit stream position (offset=%llu n=%lld)", (unsigned long long)offset, (long long)n);
    return VC_ERR_ARG; }
  const int es = dtype == VC_RNG_BF16 ? 2 : 4, E = 16 / es;
  if ((uintptr_t)out % es) { snprintf(err, errlen, "randn: the output must be aligned to its %d-byte elements", es); return VC_ERR_ARG; }
  long head = (long)((E - (int)((uintptr_t)out / es % E)) % E);      // elements before the first 16-byte boundary
  if (head > n) head = n;
  long nvec = (n - head) / E;
  if ((offset + (uint64_t)head) & 3) { head = n; nvec = 0; }          // the 16-byte chunks would straddle blocks: element-wise
  const int grid = grid_for(nvec + (n - nvec * E));
  if (dtype == VC_RNG_BF16) hipLaunchKernelGGL(randn_kernel<VC_RNG_BF16>, dim3(grid), dim3(256), 0, s, out, (long)n, seed, offset, head, nvec);
  else if (dtype == VC_RNG_F32) hipLaunchKernelGGL(randn_kernel<VC_RNG_F32>, dim3(grid), dim3(256), 0, s, out, (long)n, seed, offset, head, nvec);
  else hipLaunchKernelGGL(randn_kernel<VC_RNG_U32>, dim3(grid), dim3(256), 0, s, out, (long)n, seed, offset, head, nvec);
  return vc_launch_status("randn launch", err, errlen);
}

int vc_randn_tokens_launch(void* tokens, int C, int h, int w, int64_t ld, int col0, uint64_t seed, uint64_t offset, hipStream_t s, char* err,
                           int errlen) {
  if (!tokens) { snprintf(err, errlen, "randn_tokens: null token pointer"); return VC_ERR_ARG; }
  if (C <= 0 || h <= 0 || w <= 0 || (C & 1) || (h & 1) || (w & 1)) {
    snprintf(err, errlen, "randn_tokens: need positive even C, h, w (C=%d h=%d w=%d)", C, h, w); return VC_ERR_ARG; }
  if (ld <= 0 || col0 < 0 || ld % 8 || col0 % 8 || (int64_t)col0 + 4 * (int64_t)C > ld) {
    snprintf(err, errlen, "randn_tokens: ld and col0 must be multiples of 8 with col0 + 4C <= ld (ld=%lld col0=%d C=%d)", (long long)ld, col0, C);
    return VC_ERR_ARG; }
  if ((uintptr_t)tokens & 15) { snprintf(err, errlen, "randn_tokens: the token rows must be 16-byte aligned"); return VC_ERR_ARG; }
  const unsigned __int128 n = (unsigned __int128)C * (unsigned)h * (unsigned)w;
  if (n - 1 > (unsigned __int128)(UINT64_MAX - offset)) {
    snprintf(err, errlen, "randn_tokens: offset + C*h*w wraps the 64-bit stream position (offset=%llu)", (unsigned long long)offset);
    return VC_ERR_ARG; }
  hipLaunchKernelGGL(randn_tokens_kernel, dim3(grid_for((long)(h / 2) * (w / 2) * (C / 2))), dim3(256), 0, s, (bf16_t*)tokens, C, h, w, (long)ld,
                     col0, seed, offset);
  return vc_launch_status("randn_tokens launch", err, errlen);
}

int vc_sde_stage_launch(int eval, const float* table, int n_rows, float* y, const void* v, void* y_in, float* xhat, float* k1,
                        const uint64_t* rng, const int32_t* eval_ptr, int64_t n, hipStream_t s, char* err, int errlen) {
  if (!table || !y || !y_in || !rng || n <= 0 || n_rows <= 0 || eval >= n_rows || (eval < 0 && !eval_ptr)) {
    snprintf(err, errlen, "sde_stage: bad args (table, y, y_in, rng required; n, n_rows >= 1; eval in [0, n_rows), or < 0 with the evaluation "
                          "counter; eval=%d n_rows=%d n=%lld)", eval, n_rows, (long long)n);
    return VC_ERR_ARG;
  }
  if (((uintptr_t)table | (uintptr_t)y | (uintptr_t)xhat | (uintptr_t)k1) & 3 || ((uintptr_t)v | (uintptr_t)y_in) & 1 || (uintptr_t)rng & 7) {
    snprintf(err, errlen, "sde_stage: every buffer must be aligned to its elements (F32: 4 bytes, bf16: 2, rng: 8)");
    return VC_ERR_ARG;
  }
  const bool vec = !(((uintptr_t)y | (uintptr_t)v | (uintptr_t)y_in | (uintptr_t)xhat | (uintptr_t)k1) & 15);   // (NULL counts as aligned)
  const long nvec = vec ? (long)(n / 8) : 0;
  hipLaunchKernelGGL(sde_stage_kernel, dim3(grid_for(nvec + (n - nvec * 8))), dim3(256), 0, s, eval, table, n_rows, y, (const bf16_t*)v,
                     (bf16_t*)y_in, xhat, k1, rng, (const int*)eval_ptr, (long)n, nvec);
  return vc_launch_status("sde_stage launch", err, errlen);
}

int vc_sde_store_launch(const float* y, void* out, int out_is_bf16, int64_t n, hipStream_t s, char* err, int errlen) {
  if (!y || !out || n <= 0) { snprintf(err, errlen, "sde_store: bad args"); return VC_ERR_ARG; }
  if (out_is_bf16) hipLaunchKernelGGL(sde_store_kernel<true>, dim3(grid_for((long)n)), dim3(256), 0, s, y, out, (long)n);
  else hipLaunchKernelGGL(sde_store_kernel<false>, dim3(grid_for((long)n)), dim3(256), 0, s, y, out, (long)n);
  return vc_launch_status("sde_store launch", err, errlen);
}
