// vc_pixels_out: the end of both pipeline stages in one launch - the decoded image [3, H, W] in [-1, 1] (bf16 or f32), a column
// window [x0, x0 + w) of it (the crop of a grid cell, visualcloze.py:452,461), to [0, 1] as ((img.float() + 1.0) / 2.0).clamp_(0.0, 1.0)
// (:238-240,430-432) and either stored as f32 [3, H, w] or quantised as torchvision's to_pil_image does, pic.mul(255).byte(): a
// TRUNCATING cast, [H, w, 3] bytes (:437-439).  HBM/launch-bound; every operation is rounded on its own (contraction off: the
// compiler would otherwise turn (x + 1) * 0.5 into fma(x, 0.5, 0.5), which rounds once instead of twice).
#include "common.h"
#include "vcloze_internal.h"

namespace {

VC_DEV float unit_range(float x) {
#pragma clang fp contract(off)
  const float s = x + 1.0f;
  const float v = s * 0.5f;                   // / 2.0: exact either way
  return v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v);   // a NaN stays, as clamp_ keeps it
}
VC_DEV uint32_t to_byte(float v) {
#pragma clang fp contract(off)
  const float p = v * 255.0f;
  return (uint32_t)(int)p & 0xffu;            // v in [0, 1]: p in [0, 255], truncated
}

// element-wise: one thread per pixel (y, x) of the window, its three channels
template <bool IN_F32, bool U8>
__global__ void pixels_out_kernel(const void* __restrict__ img, int H, int W, int x0, int w, void* __restrict__ out) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)H * w) return;
  const int y = (int)(i / w), x = (int)(i % w);
  float v[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const long src = ((long)c * H + y) * W + x0 + x;
    v[c] = unit_range(IN_F32 ? ((const float*)img)[src] : bf2f(((const bf16_t*)img)[src]));
  }
  if (U8) {
    unsigned char* o = (unsigned char*)out + i * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = (unsigned char)to_byte(v[c]);
  } else {
#pragma unroll
    for (int c = 0; c < 3; ++c) ((float*)out)[((long)c * H + y) * w + x] = v[c];
  }
}

// 16-byte accesses: one thread per run of 16 pixels of one row.  x0, w, W multiples of 16 and 16-byte aligned bases make every
// load ((c H + y) W + x0 + 16 k elements of 2 or 4 bytes) and every store (f32: ((c H + y) w + 16 k) * 4 bytes; bytes: (y w + 16 k) * 3
// = a multiple of 48) 16-byte aligned.
template <bool IN_F32, bool U8>
__global__ void pixels_out_vec_kernel(const void* __restrict__ img, int H, int W, int x0, int w, void* __restrict__ out) {
  const int runs = w >> 4;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)H * runs) return;
  const int y = (int)(i / runs), x = (int)(i % runs) << 4;
  float v[3][16];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const long src = ((long)c * H + y) * W + x0 + x;
    if (IN_F32) {
      const f32x4* p = (const f32x4*)((const float*)img + src);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const f32x4 t = p[q];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[c][4 * q + e] = unit_range(t[e]);
      }
    } else {
      const u32x4* p = (const u32x4*)((const bf16_t*)img + src);
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const u32x4 t = p[q];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          v[c][8 * q + 2 * e] = unit_range(lo_bf(t[e]));
          v[c][8 * q + 2 * e + 1] = unit_range(hi_bf(t[e]));
        }
      }
    }
  }
  if (U8) {
    uint32_t words[12] = {};                  // 16 pixels x 3 interleaved bytes
#pragma unroll
    for (int px = 0; px < 16; ++px)
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int b = px * 3 + c;
        words[b >> 2] |= to_byte(v[c][px]) << (8 * (b & 3));
      }
    u32x4* o = (u32x4*)((unsigned char*)out + ((long)y * w + x) * 3);
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      u32x4 t;
#pragma unroll
      for (int e = 0; e < 4; ++e) t[e] = words[4 * q + e];
      o[q] = t;
    }
  } else {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      f32x4* o = (f32x4*)((float*)out + ((long)c * H + y) * w + x);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        f32x4 t;
#pragma unroll
        for (int e = 0; e < 4; ++e) t[e] = v[c][4 * q + e];
        o[q] = t;
      }
    }
  }
}

}  // namespace

int vc_pixels_out_launch(const void* img, int img_is_f32, int H, int W, int x0, int w, void* out, int out_form, hipStream_t s, char* err,
                         int errlen) {
  if (!img || !out) { snprintf(err, errlen, "pixels_out: null pointer"); return VC_ERR_ARG; }
  if (H <= 0 || W <= 0 || H >= 65536 || W >= 65536) { snprintf(err, errlen, "pixels_out: image size %dx%d must lie in 1..65535", H, W); return VC_ERR_ARG; }
  if (x0 < 0 || w < 1 || (int64_t)x0 + w > W) {
    snprintf(err, errlen, "pixels_out: the window [%d, %d + %d) leaves the %d columns of the image", x0, x0, w, W);
    return VC_ERR_ARG;
  }
  if (out_form != VC_PIXELS_F32 && out_form != VC_PIXELS_U8) { snprintf(err, errlen, "pixels_out: unknown out_form %d (VC_PIXELS_F32, VC_PIXELS_U8)", out_form); return VC_ERR_ARG; }
  img_is_f32 = img_is_f32 != 0;
  const bool u8 = out_form == VC_PIXELS_U8;
  const uintptr_t a = (uintptr_t)img, abytes = (uintptr_t)3 * H * W * (img_is_f32 ? 4 : 2);
  const uintptr_t o = (uintptr_t)out, obytes = (uintptr_t)3 * H * w * (u8 ? 1 : 4);
  if (a < o + obytes && o < a + abytes) { snprintf(err, errlen, "pixels_out: out overlaps img"); return VC_ERR_ARG; }
  if ((a & (img_is_f32 ? 3 : 1)) || (!u8 && (o & 3))) { snprintf(err, errlen, "pixels_out: a base is not aligned to its element size"); return VC_ERR_ARG; }
  const bool vec = !((x0 | w | W) & 15) && !((a | o) & 15);
  const long threads = vec ? (long)H * (w >> 4) : (long)H * w;
  const dim3 grid((unsigned)((threads + 255) / 256)), block(256);
#define VC_PX_LAUNCH(K, F, U) hipLaunchKernelGGL((K<F, U>), grid, block, 0, s, img, H, W, x0, w, out)
  if (vec) {
    if (img_is_f32) { if (u8) VC_PX_LAUNCH(pixels_out_vec_kernel, true, true); else VC_PX_LAUNCH(pixels_out_vec_kernel, true, false); }
    else { if (u8) VC_PX_LAUNCH(pixels_out_vec_kernel, false, true); else VC_PX_LAUNCH(pixels_out_vec_kernel, false, false); }
  } else {
    if (img_is_f32) { if (u8) VC_PX_LAUNCH(pixels_out_kernel, true, true); else VC_PX_LAUNCH(pixels_out_kernel, true, false); }
    else { if (u8) VC_PX_LAUNCH(pixels_out_kernel, false, true); else VC_PX_LAUNCH(pixels_out_kernel, false, false); }
  }
#undef VC_PX_LAUNCH
  return vc_launch_status("pixels_out launch", err, errlen);
}
