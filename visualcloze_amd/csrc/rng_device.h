// The device side of the noise stream of include/vcloze_hip.h (THE STREAM: Philox4x32-10 + Box-Muller in f32), for the kernels that draw
// in place: rng.hip (vc_randn, vc_randn_tokens, vc_sde_stage) and fm_loss.hip (vc_fm_plan).  ONE definition, so that a normal drawn
// inside a kernel is the VC_RNG_F32 value of vc_randn bit for bit: the same operations, compiled with the same flags.
#pragma once
#include "common.h"
#include "../../include/vcloze_hip.h"

namespace {

constexpr uint32_t PH_M0 = 0xD2511F53u, PH_M1 = 0xCD9E8D57u, PH_W0 = 0x9E3779B9u, PH_W1 = 0xBB67AE85u;

// x0..x3 of block b: counter (lo32(b), hi32(b), 0, 0), key (k0, k1) = (lo32(seed), hi32(seed))
VC_DEV void philox4x32_10(uint64_t b, uint32_t k0, uint32_t k1, uint32_t (&x)[4]) {
  uint32_t c0 = (uint32_t)b, c1 = (uint32_t)(b >> 32), c2 = 0, c3 = 0;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t h0 = __umulhi(PH_M0, c0), l0 = PH_M0 * c0, h1 = __umulhi(PH_M1, c2), l1 = PH_M1 * c2;
    c0 = h1 ^ c1 ^ k0; c1 = l1; c2 = h0 ^ c3 ^ k1; c3 = l0;
    k0 += PH_W0; k1 += PH_W1;
  }
  x[0] = c0; x[1] = c1; x[2] = c2; x[3] = c3;
}

// one Box-Muller pair: u1 in (0, 1] and u2 in [0, 1) are exact in f32 (24-bit integers times 2^-24)
VC_DEV void normal_pair(uint32_t xa, uint32_t xb, float& za, float& zb) {
  const float u1 = (float)((xa >> 8) + 1u) * 0x1p-24f, u2 = (float)(xb >> 8) * 0x1p-24f;
  const float r = sqrtf(0.0f - 2.0f * logf(u1));        // u1 = 1: r = +0
  float s, c;
  sincospif(2.0f * u2, &s, &c);
  za = r * c; zb = r * s;
}

// the four 32-bit words block b stores: the raw words (VC_RNG_U32) or the f32 bit patterns of z0..z3
template <int DT>
VC_DEV void block_words(uint64_t b, uint32_t k0, uint32_t k1, uint32_t (&v)[4]) {
  philox4x32_10(b, k0, k1, v);
  if (DT != VC_RNG_U32) {
    float z[4];
    normal_pair(v[0], v[1], z[0], z[1]);
    normal_pair(v[2], v[3], z[2], z[3]);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = __builtin_bit_cast(uint32_t, z[e]);
  }
}
VC_DEV uint32_t pick(const uint32_t (&v)[4], uint32_t j) { return j == 0 ? v[0] : j == 1 ? v[1] : j == 2 ? v[2] : v[3]; }
VC_DEV uint32_t pack2(uint32_t flo, uint32_t fhi) { return pack2bf(__builtin_bit_cast(float, flo), __builtin_bit_cast(float, fhi)); }

// the 8 normals at stream positions p .. p + 7, p & 3 == J: two whole blocks, or the tails and heads of three
template <int J>
VC_DEV void normals8(uint64_t p, uint32_t k0, uint32_t k1, float (&z)[8]) {
  uint32_t a[4], b[4], c[4] = {0, 0, 0, 0};
  block_words<VC_RNG_F32>(p >> 2, k0, k1, a);
  block_words<VC_RNG_F32>((p >> 2) + 1, k0, k1, b);
  if (J != 0) block_words<VC_RNG_F32>((p >> 2) + 2, k0, k1, c);
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int q = J + e;
    z[e] = __builtin_bit_cast(float, q < 4 ? a[q & 3] : q < 8 ? b[q & 3] : c[q & 3]);
  }
}
VC_DEV float normal_at(uint64_t p, uint32_t k0, uint32_t k1) {
  uint32_t v[4];
  block_words<VC_RNG_F32>(p >> 2, k0, k1, v);
  return __builtin_bit_cast(float, pick(v, (uint32_t)p & 3u));
}

}  // namespace
