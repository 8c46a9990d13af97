// Noise source, second stream: torch's device generator stream (include/vcloze_hip.h, "THE TORCH STREAM"), opt-in beside the
// library's own stream of rng.hip, which this file leaves alone (its Philox rounds are restated here with a four-word counter
// rather than shared, so that rng.hip compiles to what it did).
//   randn_torch          out[i] = element i of the draw of n elements that torch.randn(n, device, generator) makes at (seed, offset)
//   randn_torch_tokens   a [C, h, w] draw written as bf16 straight into pack_latent's token layout (pack.hip)
//   torch_randn_policy   the host rule: torch's grid for n elements on a device of (sm_count, threads_per_sm), the offset's advance
// torch (ATen/native/hip/DistributionTemplates.h) launches G blocks of 256 threads; thread t takes Philox subsequence t and, in
// round r of its grid-stride loop, turns block o/4 + r into four normals that go to elements r*4T + lane*T + t, T = 256 G.  So an
// element is a function of (seed, offset, n, cap) - through T - and of nothing else: the kernels below recompute the block of
// whatever (thread, round) they store, their own launch geometry does not show.  The transform is rocrand's Box-Muller
// (rocrand_normal.h, box_muller) followed by torch's `z * std + mean` at std 1, mean 0, which only turns -0 into +0 - restated
// here operation by operation instead of included, because bit-equality hangs on which multiply-adds are fused: in the kernel
// torch ships, u and v are one fma each and NOTHING else is contracted (in particular not the last sum of logf's expansion,
// which a compiler is free to fuse when the call site allows contraction).  normal_pair pins exactly that.
// Store-rate kernels beside a 49 ms evaluation: 16-byte stores, a capped grid, nothing else is tuned.
#include "common.h"
#include "vcloze_internal.h"

namespace {

constexpr uint32_t PH_M0 = 0xD2511F53u, PH_M1 = 0xCD9E8D57u, PH_W0 = 0x9E3779B9u, PH_W1 = 0xBB67AE85u;
constexpr int RNGT_MAX_BLOCKS = 2048;      // as rng.hip: the grid-stride loop takes the rest
constexpr int64_t RNGT_MAX_N = 1ll << 48;  // keeps every element index below 2^52; no device holds such a draw

struct TorchDraw {
  uint32_t k0, k1;    // key = (lo32(seed), hi32(seed))
  uint64_t c0;        // offset / 4: the Philox block of round 0
  long T;             // threads of torch's grid
};

// counter (lo32(c), hi32(c), lo32(thread), hi32(thread)): where rocrand_init(seed, subsequence, offset) puts offset / 4 and subsequence
VC_DEV void philox4x32_10(uint64_t c, uint64_t thread, uint32_t k0, uint32_t k1, uint32_t (&x)[4]) {
  uint32_t c0 = (uint32_t)c, c1 = (uint32_t)(c >> 32), c2 = (uint32_t)thread, c3 = (uint32_t)(thread >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t h0 = __umulhi(PH_M0, c0), l0 = PH_M0 * c0, h1 = __umulhi(PH_M1, c2), l1 = PH_M1 * c2;
    c0 = h1 ^ c1 ^ k0; c1 = l1; c2 = h0 ^ c3 ^ k1; c3 = l0;
    k0 += PH_W0; k1 += PH_W1;
  }
  x[0] = c0; x[1] = c1; x[2] = c2; x[3] = c3;
}

// rocrand's pair (r sin, r cos) of two words, then torch's z * 1 + 0.  u = 2^-32 + x 2^-32 and v = k + y k, k = 2^-32 f32(2 pi),
// are single fmas; sin / cos are the device's fast ones (__sincosf: v_sin_f32 / v_cos_f32 of v / 2 pi), as rocrand calls them
VC_DEV void normal_pair(uint32_t xa, uint32_t xb, float& za, float& zb) {
#pragma clang fp contract(off)
  const float u = __builtin_fmaf((float)xa, 0x1p-32f, 0x1p-32f), v = __builtin_fmaf((float)xb, 0x1.921fb6p-30f, 0x1.921fb6p-30f);
  // logf as that kernel expands it: m = log2 u from the hardware, times ln 2 held in two words, the product's error recovered by fma
  // and the two parts ADDED (not fused).  u >= 2^-32 is never subnormal, so the expansion's input scaling is left out: it is exact
  const float m = __builtin_amdgcn_logf(u), t = m * 0x1.62e42ep-1f;
  const float ln_u = t + __builtin_fmaf(m, 0x1.efa39ep-25f, __builtin_fmaf(m, 0x1.62e42ep-1f, -t));
  const float r = sqrtf(-2.0f * ln_u);
  float sn, cs;
  __sincosf(v, &sn, &cs);
  za = sn * r + 0.0f; zb = cs * r + 0.0f;
}

// the four 32-bit words (thread, round) stores in lanes 0..3: the raw words (VC_RNG_U32) or the f32 bit patterns of the normals
template <int DT>
VC_DEV void block_words(const TorchDraw& d, uint64_t thread, uint64_t round, uint32_t (&v)[4]) {
  philox4x32_10(d.c0 + round, thread, d.k0, d.k1, v);
  if (DT != VC_RNG_U32) {
    float z[4];
    normal_pair(v[0], v[1], z[0], z[1]);
    normal_pair(v[2], v[3], z[2], z[3]);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = __builtin_bit_cast(uint32_t, z[e]);
  }
}

// element i of the draw as f32: one block, the one pair the lane is in
VC_DEV float element(const TorchDraw& d, uint64_t i) {
  const uint64_t q = i / (uint64_t)d.T, thread = i - q * (uint64_t)d.T;
  const uint32_t lane = (uint32_t)q & 3u;
  uint32_t x[4];
  philox4x32_10(d.c0 + (q >> 2), thread, d.k0, d.k1, x);
  float za, zb;
  normal_pair(lane < 2 ? x[0] : x[2], lane < 2 ? x[1] : x[3], za, zb);
  return (lane & 1) ? zb : za;
}

// A work item is E consecutive threads of one round (E elements = 16 bytes): E blocks, then per lane the E elements
// r*4T + lane*T + t0 .. + E - 1 in one 16-byte store where `vec` (a 16-byte aligned base; T is a multiple of 256, so the index is
// one of E) and the draw's end allow, else one by one.
template <int DT>
__global__ __launch_bounds__(256) void randn_torch_kernel(void* __restrict__ out, long n, TorchDraw d, long rounds, int vec) {
  constexpr int E = DT == VC_RNG_BF16 ? 8 : 4;
  const long groups = d.T / E, total = rounds * groups;
  for (long wi = blockIdx.x * 256L + threadIdx.x; wi < total; wi += gridDim.x * 256L) {
    const long r = wi / groups, t0 = (wi - r * groups) * E, base = r * 4 * d.T + t0;
    if (base >= n) continue;                       // the lanes only come later
    uint32_t v[E][4];
#pragma unroll
    for (int e = 0; e < E; ++e) block_words<DT>(d, (uint64_t)(t0 + e), (uint64_t)r, v[e]);
#pragma unroll
    for (int lane = 0; lane < 4; ++lane) {
      const long i = base + lane * d.T;
      if (vec && i + E <= n) {
        u32x4 o;
        if (DT == VC_RNG_BF16) {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            o[e] = pack2bf(__builtin_bit_cast(float, v[2 * e][lane]), __builtin_bit_cast(float, v[2 * e + 1][lane]));
          *(u32x4*)((bf16_t*)out + i) = o;
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) o[e] = v[e][lane];
          *(u32x4*)((uint32_t*)out + i) = o;
        }
      } else {
#pragma unroll
        for (int e = 0; e < E; ++e) {
          if (i + e >= n) break;
          if (DT == VC_RNG_BF16) ((bf16_t*)out)[i + e] = f2bf(__builtin_bit_cast(float, v[e][lane]));
          else ((uint32_t*)out)[i + e] = v[e][lane];
        }
      }
    }
  }
}

// out[tok * ld + col0 + c*4 + ph*2 + pw] = bf16(element (c*h + 2*hh + ph)*w + 2*ww + pw),  tok = hh*(w/2) + ww: a thread writes one
// 16-byte chunk (2 channels x 2 x 2) of a token row.  Neighbouring elements belong to different threads of torch's grid, so each
// of the eight takes a block of its own.
__global__ __launch_bounds__(256) void randn_torch_tokens_kernel(bf16_t* __restrict__ out, int C, int h, int w, long ld, int col0, TorchDraw d) {
  const int w2 = w >> 1, cpt = C >> 1;
  const long total = (long)(h >> 1) * w2 * cpt;
  for (long wi = blockIdx.x * 256L + threadIdx.x; wi < total; wi += gridDim.x * 256L) {
    const long tok = wi / cpt;
    const int ck = (int)(wi - tok * cpt), hh = (int)(tok / w2), ww = (int)(tok - (long)hh * w2);
    u32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int c = 2 * ck + (e >> 1), ph = e & 1;
      const uint64_t i = ((uint64_t)c * h + 2 * hh + ph) * w + 2 * ww;
      o[e] = pack2bf(element(d, i), element(d, i + 1));
    }
    *(u32x4*)(out + tok * ld + col0 + ck * 8) = o;
  }
}

int grid_for(long total) { return (int)((total + 255) / 256 < RNGT_MAX_BLOCKS ? (total + 255) / 256 : RNGT_MAX_BLOCKS); }

// everything the draw's geometry decides; (sm_count, threads_per_sm) already the device's where they were given as 0
struct Policy { int64_t G, T, rounds; uint64_t advance; };

int policy_of(const char* who, int64_t n, int sm_count, int threads_per_sm, Policy& p, char* err, int errlen) {
  const int64_t cap = (int64_t)sm_count * (threads_per_sm / 256);
  if (cap < 1 || cap > 0x7fffffff) {
    snprintf(err, errlen, "%s: sm_count * (threads_per_sm / 256) = %lld, a grid cap in 1 .. 2^31 - 1 expected", who, (long long)cap); return VC_ERR_ARG; }
  const int64_t blocks = (n + 255) / 256;
  p.G = blocks < cap ? blocks : cap;
  p.T = 256 * p.G;
  p.rounds = (n - 1) / (4 * p.T) + 1;
  p.advance = (uint64_t)p.rounds * 4;
  return VC_OK;
}

int check_n(const char* who, int64_t n, char* err, int errlen) {
  if (n <= 0) { snprintf(err, errlen, "%s: n = %lld, need n >= 1", who, (long long)n); return VC_ERR_ARG; }
  if (n > RNGT_MAX_N) { snprintf(err, errlen, "%s: n = %lld, at most 2^48 elements per draw", who, (long long)n); return VC_ERR_ARG; }
  return VC_OK;
}

int check_caps(const char* who, int sm_count, int threads_per_sm, char* err, int errlen) {
  if (sm_count < 0) { snprintf(err, errlen, "%s: sm_count = %d, 0 (the current device's) or a positive count expected", who, sm_count); return VC_ERR_ARG; }
  if (threads_per_sm != 0 && threads_per_sm < 256) {
    snprintf(err, errlen, "%s: threads_per_sm = %d, 0 (the current device's) or at least 256 expected", who, threads_per_sm); return VC_ERR_ARG; }
  return VC_OK;
}

int check_offset(const char* who, uint64_t offset, char* err, int errlen) {
  if (offset & 3) {
    snprintf(err, errlen, "%s: philox_offset = %llu is not a multiple of 4 (torch.Generator.get_offset())", who, (unsigned long long)offset);
    return VC_ERR_ARG; }
  return VC_OK;
}

int check_wrap(const char* who, uint64_t offset, const Policy& p, char* err, int errlen) {
  if (p.advance > UINT64_MAX - offset) {
    snprintf(err, errlen, "%s: philox_offset + advance wraps the 64-bit offset (philox_offset=%llu advance=%llu)", who, (unsigned long long)offset,
             (unsigned long long)p.advance);
    return VC_ERR_ARG; }
  return VC_OK;
}

}  // namespace

#define RNGT_TRY(x) { int rc_ = (x); if (rc_ != VC_OK) return rc_; }
int vc_torch_caps_resolve(const char* who, int* sm_count, int* threads_per_sm, char* err, int errlen) {
  RNGT_TRY(check_caps(who, *sm_count, *threads_per_sm, err, errlen));
  if (*sm_count && *threads_per_sm) return VC_OK;
  int dev = 0, sm = 0, tpsm = 0;
  hipError_t he = hipGetDevice(&dev);
  if (he == hipSuccess) he = hipDeviceGetAttribute(&sm, hipDeviceAttributeMultiprocessorCount, dev);
  if (he == hipSuccess) he = hipDeviceGetAttribute(&tpsm, hipDeviceAttributeMaxThreadsPerMultiProcessor, dev);
  if (he != hipSuccess) {
    (void)hipGetLastError();
    snprintf(err, errlen, "%s: the current device's properties: %s", who, hipGetErrorString(he)); return VC_ERR_HIP; }
  if (!*sm_count) *sm_count = sm;
  if (!*threads_per_sm) *threads_per_sm = tpsm;
  return VC_OK;
}

int vc_torch_randn_policy_impl(int64_t n, int sm_count, int threads_per_sm, int32_t* grid, uint64_t* offset_advance, char* err, int errlen) {
  const char* who = "torch_randn_policy";
  if (!grid || !offset_advance) { snprintf(err, errlen, "%s: null result pointer", who); return VC_ERR_ARG; }
  RNGT_TRY(check_n(who, n, err, errlen));
  RNGT_TRY(vc_torch_caps_resolve(who, &sm_count, &threads_per_sm, err, errlen));
  Policy p;
  RNGT_TRY(policy_of(who, n, sm_count, threads_per_sm, p, err, errlen));
  *grid = (int32_t)p.G;
  *offset_advance = p.advance;
  return VC_OK;
}

int vc_randn_torch_launch(void* out, int dtype, int64_t n, uint64_t seed, uint64_t offset, int sm_count, int threads_per_sm, hipStream_t s,
                          char* err, int errlen) {
  const char* who = "randn_torch";
  if (!out) { snprintf(err, errlen, "%s: null output pointer", who); return VC_ERR_ARG; }
  RNGT_TRY(check_n(who, n, err, errlen));
  if (dtype != VC_RNG_BF16 && dtype != VC_RNG_F32 && dtype != VC_RNG_U32) {
    snprintf(err, errlen, "%s: unknown dtype %d (VC_RNG_BF16, VC_RNG_F32, VC_RNG_U32)", who, dtype); return VC_ERR_ARG; }
  RNGT_TRY(check_offset(who, offset, err, errlen));
  const int es = dtype == VC_RNG_BF16 ? 2 : 4, E = 16 / es;
  if ((uintptr_t)out % es) { snprintf(err, errlen, "%s: the output must be aligned to its %d-byte elements", who, es); return VC_ERR_ARG; }
  RNGT_TRY(vc_torch_caps_resolve(who, &sm_count, &threads_per_sm, err, errlen));
  Policy p;
  RNGT_TRY(policy_of(who, n, sm_count, threads_per_sm, p, err, errlen));
  RNGT_TRY(check_wrap(who, offset, p, err, errlen));
  const TorchDraw d{(uint32_t)seed, (uint32_t)(seed >> 32), offset >> 2, (long)p.T};
  const int vec = ((uintptr_t)out & 15) == 0, grid = grid_for(p.rounds * (p.T / E));
  if (dtype == VC_RNG_BF16) hipLaunchKernelGGL(randn_torch_kernel<VC_RNG_BF16>, dim3(grid), dim3(256), 0, s, out, (long)n, d, (long)p.rounds, vec);
  else if (dtype == VC_RNG_F32) hipLaunchKernelGGL(randn_torch_kernel<VC_RNG_F32>, dim3(grid), dim3(256), 0, s, out, (long)n, d, (long)p.rounds, vec);
  else hipLaunchKernelGGL(randn_torch_kernel<VC_RNG_U32>, dim3(grid), dim3(256), 0, s, out, (long)n, d, (long)p.rounds, vec);
  return vc_launch_status("randn_torch launch", err, errlen);
}

int vc_randn_torch_tokens_launch(void* tokens, int C, int h, int w, int64_t ld, int col0, uint64_t seed, uint64_t offset, int sm_count,
                                 int threads_per_sm, hipStream_t s, char* err, int errlen) {
  const char* who = "randn_torch_tokens";
  if (!tokens) { snprintf(err, errlen, "%s: null token pointer", who); return VC_ERR_ARG; }
  if (C <= 0 || h <= 0 || w <= 0 || (C & 1) || (h & 1) || (w & 1)) {
    snprintf(err, errlen, "%s: need positive even C, h, w (C=%d h=%d w=%d)", who, C, h, w); return VC_ERR_ARG; }
  if (ld <= 0 || col0 < 0 || ld % 8 || col0 % 8 || (int64_t)col0 + 4 * (int64_t)C > ld) {
    snprintf(err, errlen, "%s: ld and col0 must be multiples of 8 with col0 + 4C <= ld (ld=%lld col0=%d C=%d)", who, (long long)ld, col0, C);
    return VC_ERR_ARG; }
  if ((uintptr_t)tokens & 15) { snprintf(err, errlen, "%s: the token rows must be 16-byte aligned", who); return VC_ERR_ARG; }
  const unsigned __int128 n128 = (unsigned __int128)C * (unsigned)h * (unsigned)w;
  if (n128 > (unsigned __int128)RNGT_MAX_N) { snprintf(err, errlen, "%s: C*h*w exceeds 2^48 elements per draw", who); return VC_ERR_ARG; }
  RNGT_TRY(check_offset(who, offset, err, errlen));
  RNGT_TRY(vc_torch_caps_resolve(who, &sm_count, &threads_per_sm, err, errlen));
  Policy p;
  RNGT_TRY(policy_of(who, (int64_t)n128, sm_count, threads_per_sm, p, err, errlen));
  RNGT_TRY(check_wrap(who, offset, p, err, errlen));
  const TorchDraw d{(uint32_t)seed, (uint32_t)(seed >> 32), offset >> 2, (long)p.T};
  hipLaunchKernelGGL(randn_torch_tokens_kernel, dim3(grid_for((long)(h / 2) * (w / 2) * (C / 2))), dim3(256), 0, s, (bf16_t*)tokens, C, h, w,
                     (long)ld, col0, d);
  return vc_launch_status("randn_torch_tokens launch", err, errlen);
}
