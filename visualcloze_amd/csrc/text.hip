// Text-encoder glue kernels (T5-XXL encoder and CLIP-L text model, reference call site
// models/modules/conditioner.py:5-37 -> transformers T5EncoderModel / CLIPTextModel).  The projections and the per-head
// attention products run on the bf16 MFMA GEMM; these are the HBM-bound pieces between them.  Rounding points follow the
// transformers modules run in bfloat16.
//   embedding     out[i, :] = table[ids[i], :]                                   (nn.Embedding)
//   rmsnorm       y = bf16(w * bf16(x * rsqrt(mean(x^2) + eps)))                 (T5LayerNorm: no mean, no bias, f32 stats)
//   layernorm     y = bf16(LN(x) * w + b), f32 statistics                         (nn.LayerNorm, CLIP)
//   mul / add     elementwise bf16                                                (T5 gated FF product; CLIP token + position)
//   quick_gelu    y = bf16(x * bf16(sigmoid(bf16(1.702 * x))))                    (CLIP hidden_act)
//   t5_position_bias  out[h*L + i, j] = table[bucket(j - i), h]                   (T5Attention.compute_bias: a pure gather)
//   clip_embed    out[i, :] = bf16(tok[ids[i]] + pos[i]) for i < L, bf16(tok[0] + 0) for the pad rows   (CLIPTextEmbeddings)
//   clip_pool     pooled = hidden[first i with ids[i] == eos, or 0]               (CLIPTextTransformer.forward's pooler_output)
#include "common.h"
#include "vcloze_internal.h"
#include <math.h>

namespace {

__global__ void embedding_kernel(const int32_t* __restrict__ ids, const bf16_t* __restrict__ table, long ldt, int V,
                                 bf16_t* __restrict__ out, int L, int D) {
  const int cpr = D >> 3;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)L * cpr) return;
  const int row = (int)(i / cpr), c8 = (int)(i % cpr);
  int id = ids[row];
  id = id < 0 ? 0 : (id >= V ? V - 1 : id);
  *(u32x4*)(out + (long)row * D + c8 * 8) = *(const u32x4*)(table + (long)id * ldt + c8 * 8);
}

// one wave per row; D <= 64 * 8 * NV elements, 16-B chunks strided across the wave
template <int AFFINE_LN>
__global__ __launch_bounds__(256) void rownorm_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ w,
                                                      const bf16_t* __restrict__ b, bf16_t* __restrict__ y, int rows, int D, float eps) {
  constexpr int NV = 8;                        // up to 8 chunks of 8 elements per lane -> D <= 4096
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int cpr = D >> 3;
  float v[NV][8];
  float s = 0.f, q = 0.f;
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const int c8 = k * 64 + lane;
    if (c8 < cpr) {
      const u32x4 u = *(const u32x4*)(x + (long)row * D + c8 * 8);
#pragma unroll
      for (int e = 0; e < 4; ++e) { v[k][2 * e] = lo_bf(u[e]); v[k][2 * e + 1] = hi_bf(u[e]); }
#pragma unroll
      for (int e = 0; e < 8; ++e) { s += v[k][e]; q += v[k][e] * v[k][e]; }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { s += __shfl_xor(s, o, 64); q += __shfl_xor(q, o, 64); }
  const float inv_d = 1.0f / (float)D;
  float mean = 0.f, rstd;
  if (AFFINE_LN) {
    mean = s * inv_d;
    float var = 0.f;                            // second pass over the registers: sum (x - mean)^2
#pragma unroll
    for (int k = 0; k < NV; ++k)
      if (k * 64 + lane < cpr)
#pragma unroll
        for (int e = 0; e < 8; ++e) { const float d = v[k][e] - mean; var += d * d; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) var += __shfl_xor(var, o, 64);
    rstd = 1.0f / sqrtf(var * inv_d + eps);
  } else {
    rstd = 1.0f / sqrtf(q * inv_d + eps);
  }
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const int c8 = k * 64 + lane;
    if (c8 < cpr) {
      const u32x4 wu = *(const u32x4*)(w + c8 * 8);
      u32x4 bu = {0u, 0u, 0u, 0u};
      if (AFFINE_LN) bu = *(const u32x4*)(b + c8 * 8);
      u32x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float r[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const float xv = v[k][2 * e + h];
          const float wv = h ? hi_bf(wu[e]) : lo_bf(wu[e]);
          if (AFFINE_LN) r[h] = (xv - mean) * rstd * wv + (h ? hi_bf(bu[e]) : lo_bf(bu[e]));
          else r[h] = wv * rbf(xv * rstd);
        }
        o[e] = pack2bf(r[0], r[1]);
      }
      *(u32x4*)(y + (long)row * D + c8 * 8) = o;
    }
  }
}

// op 0: a*b, op 1: a+b, op 2: quick_gelu(a)
__global__ void ewise_kernel(const bf16_t* __restrict__ a, const bf16_t* __restrict__ b, bf16_t* __restrict__ y, long n8, int op) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n8) return;
  const u32x4 ua = *(const u32x4*)(a + i * 8);
  u32x4 ub = {0u, 0u, 0u, 0u};
  if (op != 2) ub = *(const u32x4*)(b + i * 8);
  u32x4 o;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    float r[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const float av = h ? hi_bf(ua[e]) : lo_bf(ua[e]);
      const float bv = h ? hi_bf(ub[e]) : lo_bf(ub[e]);
      if (op == 0) r[h] = av * bv;
      else if (op == 1) r[h] = av + bv;
      else {
        const float t = rbf(1.702f * av);
        r[h] = av * rbf(1.0f / (1.0f + expf(-t)));
      }
    }
    o[e] = pack2bf(r[0], r[1]);
  }
  *(u32x4*)(y + i * 8) = o;
}

// The bucket of a relative position depends on |j - i| and its sign only, and grows with |j - i|: the host hands over the
// distances at which it steps (VcT5Steps, kernel arguments), the kernel counts the steps passed and gathers.  One thread writes 8
// consecutive j of one (head, query) row: eight 2-byte reads of the (cache-resident, <= 16 KB) table, one 16-byte store.
__global__ void t5_position_bias_kernel(const bf16_t* __restrict__ table, long ld, int H, int L, int half, int max_exact, VcT5Steps st,
                                        bf16_t* __restrict__ out) {
  const int cpr = L >> 3;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)H * L * cpr) return;
  const int c8 = (int)(i % cpr);
  const long row = i / cpr;
  const int h = (int)(row / L), qi = (int)(row % L);
  bf16_t v[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int r = c8 * 8 + e - qi, d = r < 0 ? -r : r;
    int b = d;
    if (d >= max_exact) {
      b = max_exact;
      for (int k = 0; k < st.n; ++k) b += st.at[k] <= d;
    }
    if (r > 0) b += half;
    v[e] = table[(long)b * ld + h];
  }
  u32x4 o;
#pragma unroll
  for (int e = 0; e < 4; ++e) o[e] = (uint32_t)v[2 * e] | ((uint32_t)v[2 * e + 1] << 16);
  *(u32x4*)(out + row * L + c8 * 8) = o;
}

__global__ void clip_embed_kernel(const int32_t* __restrict__ ids, const bf16_t* __restrict__ tok, long ldt, int V,
                                  const bf16_t* __restrict__ pos, long ldp, bf16_t* __restrict__ out, int L, int Lp, int D) {
  const int cpr = D >> 3;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)Lp * cpr) return;
  const int row = (int)(i / cpr), c8 = (int)(i % cpr);
  int id = 0;
  u32x4 up = {0u, 0u, 0u, 0u};             // pad rows: token 0 plus a position row of zeros (-0 becomes +0, as in the sum it replaces)
  if (row < L) {
    id = ids[row];
    id = id < 0 ? 0 : (id >= V ? V - 1 : id);
    up = *(const u32x4*)(pos + (long)row * ldp + c8 * 8);
  }
  const u32x4 ut = *(const u32x4*)(tok + (long)id * ldt + c8 * 8);
  u32x4 o;
#pragma unroll
  for (int e = 0; e < 4; ++e) o[e] = pack2bf(lo_bf(ut[e]) + lo_bf(up[e]), hi_bf(ut[e]) + hi_bf(up[e]));
  *(u32x4*)(out + (long)row * D + c8 * 8) = o;
}

// every wave finds the first EOS position itself (L is a prompt: 77 ids), then the block's threads copy that row
__global__ __launch_bounds__(256) void clip_pool_kernel(const int32_t* __restrict__ ids, const bf16_t* __restrict__ hidden, long ld, int L,
                                                        int D, int eos, bf16_t* __restrict__ pooled) {
  const int lane = threadIdx.x & 63;
  int first = L;
  for (int i = lane; i < L; i += 64)
    if (ids[i] == eos) { first = i; break; }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { const int other = __shfl_xor(first, o, 64); first = other < first ? other : first; }
  if (first >= L) first = 0;               // no EOS: argmax over all-zero is index 0
  const int c8 = blockIdx.x * blockDim.x + threadIdx.x;
  if (c8 < (D >> 3)) *(u32x4*)(pooled + c8 * 8) = *(const u32x4*)(hidden + (long)first * ld + c8 * 8);
}

}  // namespace

int vc_embedding_launch(const int32_t* ids, const void* table, int64_t ldt, int V, void* out, int L, int D, hipStream_t s, char* err, int errlen) {
  if (!ids || !table || !out) { snprintf(err, errlen, "embedding: null pointer"); return VC_ERR_ARG; }
  if (L <= 0 || D <= 0 || D % 8 || V <= 0 || ldt < D || ldt % 8) { snprintf(err, errlen, "embedding: bad shape L=%d D=%d V=%d", L, D, V); return VC_ERR_ARG; }
  const long total = (long)L * (D >> 3);
  hipLaunchKernelGGL(embedding_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, ids, (const bf16_t*)table, (long)ldt, V, (bf16_t*)out, L, D);
  return vc_launch_status("embedding launch", err, errlen);
}

int vc_rownorm_launch(const void* x, const void* w, const void* b, void* y, int rows, int D, float eps, int affine_ln, hipStream_t s, char* err, int errlen) {
  if (!x || !w || !y || (affine_ln && !b)) { snprintf(err, errlen, "rmsnorm/layernorm: null pointer"); return VC_ERR_ARG; }
  if (rows <= 0 || D <= 0 || D % 8 || D > 4096) { snprintf(err, errlen, "rmsnorm/layernorm: rows=%d D=%d (D %% 8 == 0, D <= 4096)", rows, D); return VC_ERR_ARG; }
  if (affine_ln) hipLaunchKernelGGL(rownorm_kernel<1>, dim3((rows + 3) / 4), dim3(256), 0, s, (const bf16_t*)x, (const bf16_t*)w, (const bf16_t*)b, (bf16_t*)y, rows, D, eps);
  else hipLaunchKernelGGL(rownorm_kernel<0>, dim3((rows + 3) / 4), dim3(256), 0, s, (const bf16_t*)x, (const bf16_t*)w, (const bf16_t*)b, (bf16_t*)y, rows, D, eps);
  return vc_launch_status("rmsnorm/layernorm launch", err, errlen);
}

int vc_ewise_launch(const void* a, const void* b, void* y, int64_t n, int op, hipStream_t s, char* err, int errlen) {
  if (!a || !y || (op != 2 && !b)) { snprintf(err, errlen, "elementwise: null pointer"); return VC_ERR_ARG; }
  if (n <= 0 || n % 8) { snprintf(err, errlen, "elementwise: n=%ld must be a positive multiple of 8", (long)n); return VC_ERR_ARG; }
  const long n8 = n >> 3;
  hipLaunchKernelGGL(ewise_kernel, dim3((unsigned)((n8 + 255) / 256)), dim3(256), 0, s, (const bf16_t*)a, (const bf16_t*)b, (bf16_t*)y, n8, op);
  return vc_launch_status("elementwise launch", err, errlen);
}

// T5Attention._relative_position_bucket (bidirectional) of relative position r = key - query, in the arithmetic of
// visualcloze_amd/text.py::t5_relative_buckets: every step of the "large" branch is an f32 operation (the ratio, its log, the division
// by f32(log(max_distance / max_exact)), the product), then a truncation.  `volatile` keeps the compiler from contracting or
// re-associating them.
static int t5_bucket(int r, int num_buckets, int max_distance) {
  const int half = num_buckets / 2, max_exact = half / 2;
  const int side = r > 0 ? half : 0, d = r < 0 ? -r : r;
  if (d < max_exact) return side + d;
  volatile float ratio = (float)d / (float)max_exact;
  volatile float lg = logf(ratio);
  volatile float den = (float)log((double)max_distance / (double)max_exact);
  volatile float q = lg / den;
  volatile float v = q * (float)(half - max_exact);
  const long large = (long)max_exact + (long)v;
  return side + (int)(large < half - 1 ? large : half - 1);
}
static int t5_bucket_args(const char* what, int L, int num_buckets, int max_distance, char* err, int errlen) {
  const int max_exact = num_buckets / 4;
  if (L <= 0 || num_buckets < 4 || num_buckets % 2 || num_buckets > 4 * (VC_T5_MAX_STEPS + 1) || max_distance <= max_exact) {
    snprintf(err, errlen, "%s: L=%d num_buckets=%d max_distance=%d (L > 0, num_buckets even in 4..%d, max_distance > num_buckets / 4)", what, L,
             num_buckets, max_distance, 4 * (VC_T5_MAX_STEPS + 1));
    return VC_ERR_ARG;
  }
  return VC_OK;
}

int vc_t5_relative_buckets_impl(int L, int num_buckets, int max_distance, int32_t* out, char* err, int errlen) {
  if (!out) { snprintf(err, errlen, "t5_relative_buckets: null result pointer"); return VC_ERR_ARG; }
  int rc = t5_bucket_args("t5_relative_buckets", L, num_buckets, max_distance, err, errlen);
  if (rc != VC_OK) return rc;
  for (int r = -(L - 1); r < L; ++r) out[r + L - 1] = t5_bucket(r, num_buckets, max_distance);
  return VC_OK;
}

int vc_t5_position_bias_launch(const void* table, int64_t ld, int H, int L, int num_buckets, int max_distance, void* out, hipStream_t s,
                               char* err, int errlen) {
  if (!table || !out) { snprintf(err, errlen, "t5_position_bias: null pointer"); return VC_ERR_ARG; }
  int rc = t5_bucket_args("t5_position_bias", L, num_buckets, max_distance, err, errlen);
  if (rc != VC_OK) return rc;
  if (H <= 0 || ld < H || L % 8 || ((uintptr_t)out & 15) || (int64_t)H * L >= (1ll << 31)) {
    snprintf(err, errlen, "t5_position_bias: H=%d L=%d ld=%ld (ld >= H, L %% 8 == 0, H * L < 2^31, out 16-byte aligned)", H, L, (long)ld);
    return VC_ERR_ARG;
  }
  const int half = num_buckets / 2, max_exact = half / 2;
  VcT5Steps st;
  st.n = 0;
  for (int d = max_exact, b = max_exact; d < L && b < half - 1; ++d)       // at[k] = the first distance whose bucket exceeds max_exact + k
    for (const int bd = t5_bucket(d, num_buckets, max_distance) - half; b < bd; ++b) st.at[st.n++] = d;
  const long total = (long)H * L * (L >> 3);
  hipLaunchKernelGGL(t5_position_bias_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, (const bf16_t*)table, (long)ld, H, L, half,
                     max_exact, st, (bf16_t*)out);
  return vc_launch_status("t5_position_bias launch", err, errlen);
}

int vc_clip_embed_launch(const int32_t* ids, const void* tok, int64_t ldt, int V, const void* pos, int64_t ldp, void* out, int L, int Lp, int D,
                         hipStream_t s, char* err, int errlen) {
  if (!ids || !tok || !pos || !out) { snprintf(err, errlen, "clip_embed: null pointer"); return VC_ERR_ARG; }
  if (L <= 0 || Lp < L || D <= 0 || D % 8 || V <= 0 || ldt < D || ldt % 8 || ldp < D || ldp % 8 || (((uintptr_t)tok | (uintptr_t)pos | (uintptr_t)out) & 15)) {
    snprintf(err, errlen, "clip_embed: bad shape L=%d Lp=%d D=%d V=%d (D, row strides %% 8 == 0, 16-byte aligned bases)", L, Lp, D, V);
    return VC_ERR_ARG;
  }
  const long total = (long)Lp * (D >> 3);
  hipLaunchKernelGGL(clip_embed_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, ids, (const bf16_t*)tok, (long)ldt, V, (const bf16_t*)pos,
                     (long)ldp, (bf16_t*)out, L, Lp, D);
  return vc_launch_status("clip_embed launch", err, errlen);
}

int vc_clip_pool_launch(const int32_t* ids, const void* hidden, int64_t ld, int L, int D, int eos, void* pooled, hipStream_t s, char* err, int errlen) {
  if (!ids || !hidden || !pooled) { snprintf(err, errlen, "clip_pool: null pointer"); return VC_ERR_ARG; }
  if (L <= 0 || D <= 0 || D % 8 || ld < D || ld % 8 || (((uintptr_t)hidden | (uintptr_t)pooled) & 15)) {
    snprintf(err, errlen, "clip_pool: bad shape L=%d D=%d ld=%ld (D, ld %% 8 == 0, 16-byte aligned bases)", L, D, (long)ld);
    return VC_ERR_ARG;
  }
  hipLaunchKernelGGL(clip_pool_kernel, dim3(((D >> 3) + 255) / 256), dim3(256), 0, s, ids, (const bf16_t*)hidden, (long)ld, L, D, eos, (bf16_t*)pooled);
  return vc_launch_status("clip_pool launch", err, errlen);
}
