// vc_pixels_in: the inverse of vc_pixels_out (pixels_out.hip) - an 8-bit [H, W, 3] photograph, a crop window of it that may reach
// outside the image (Image.crop: outside pixels are 0), into the column window [x0, x0 + w) of a row tensor [3, h, Wrow] in [-1, 1]:
// ToTensor then Normalize(0.5, 0.5) (visualcloze.py:133-137), v = (f32(u8) / 255 - 0.5) / 0.5 with a TRUE division by 255, every
// operation rounded on its own, then rounded to bf16 for the bf16 form (:377).  vc_mask_fill: the same window of the row's bf16 pixel
// mask set to 0 or 1 (:369-374).  Element-wise, launch-bound.
#include "common.h"
#include "vcloze_internal.h"

namespace {

VC_DEV float normalised(unsigned char b) {
#pragma clang fp contract(off)
  const float u = (float)b / 255.0f;            // correctly rounded IEEE division: no reciprocal
  const float c = u - 0.5f;
  return c / 0.5f;                              // exact
}

// one thread per pixel (y, x) of the window, its three channels
template <bool OUT_F32>
__global__ void pixels_in_kernel(const unsigned char* __restrict__ src, int H, int W, int left, int top, void* __restrict__ out, int h,
                                 int Wrow, int x0, int w) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)h * w) return;
  const int y = (int)(i / w), x = (int)(i % w);
  const long sy = (long)top + y, sx = (long)left + x;
  const bool inside = src && sy >= 0 && sy < H && sx >= 0 && sx < W;
  const unsigned char* p = inside ? src + (sy * W + sx) * 3 : nullptr;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float v = normalised(inside ? p[c] : (unsigned char)0);
    const long o = ((long)c * h + y) * Wrow + x0 + x;
    if (OUT_F32) ((float*)out)[o] = v;
    else ((bf16_t*)out)[o] = f2bf(v);
  }
}

__global__ void mask_fill_kernel(bf16_t* __restrict__ mask, int h, int Wrow, int x0, int w, bf16_t bits) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)h * w) return;
  mask[(i / w) * Wrow + x0 + (i % w)] = bits;
}

bool window_ok(int h, int Wrow, int x0, int w) {
  return h >= 1 && h <= 65535 && Wrow >= 1 && Wrow <= 65535 && x0 >= 0 && w >= 1 && (int64_t)x0 + w <= Wrow;
}

}  // namespace

int vc_pixels_in_launch(const void* src, int H, int W, int left, int top, void* out, int out_is_f32, int h, int Wrow, int x0, int w,
                        hipStream_t s, char* err, int errlen) {
  if (!out) { snprintf(err, errlen, "pixels_in: null out"); return VC_ERR_ARG; }
  if (!window_ok(h, Wrow, x0, w)) {
    snprintf(err, errlen, "pixels_in: the window [%d, %d + %d) of a %dx%d row: sizes in 1..65535 and a window inside the row expected", x0, x0, w, h, Wrow);
    return VC_ERR_ARG;
  }
  if (src && (H < 1 || W < 1 || H > 65535 || W > 65535)) { snprintf(err, errlen, "pixels_in: image size %dx%d must lie in 1..65535", H, W); return VC_ERR_ARG; }
  if (left < -65535 || left > 65535 || top < -65535 || top > 65535) { snprintf(err, errlen, "pixels_in: crop offset (%d, %d) outside +-65535", left, top); return VC_ERR_ARG; }
  out_is_f32 = out_is_f32 != 0;
  if ((uintptr_t)out & (out_is_f32 ? 3 : 1)) { snprintf(err, errlen, "pixels_in: out is not aligned to its element size"); return VC_ERR_ARG; }
  if (src) {
    const uintptr_t a = (uintptr_t)src, ab = (uintptr_t)3 * H * W, o = (uintptr_t)out, ob = (uintptr_t)3 * h * Wrow * (out_is_f32 ? 4 : 2);
    if (a < o + ob && o < a + ab) { snprintf(err, errlen, "pixels_in: out overlaps src"); return VC_ERR_ARG; }
  }
  const long threads = (long)h * w;
  const dim3 grid((unsigned)((threads + 255) / 256)), block(256);
  if (out_is_f32) hipLaunchKernelGGL((pixels_in_kernel<true>), grid, block, 0, s, (const unsigned char*)src, H, W, left, top, out, h, Wrow, x0, w);
  else hipLaunchKernelGGL((pixels_in_kernel<false>), grid, block, 0, s, (const unsigned char*)src, H, W, left, top, out, h, Wrow, x0, w);
  return vc_launch_status("pixels_in launch", err, errlen);
}

int vc_mask_fill_launch(void* mask, int h, int Wrow, int x0, int w, int value, hipStream_t s, char* err, int errlen) {
  if (!mask) { snprintf(err, errlen, "mask_fill: null mask"); return VC_ERR_ARG; }
  if (!window_ok(h, Wrow, x0, w)) {
    snprintf(err, errlen, "mask_fill: the window [%d, %d + %d) of a %dx%d mask: sizes in 1..65535 and a window inside the row expected", x0, x0, w, h, Wrow);
    return VC_ERR_ARG;
  }
  if (value != 0 && value != 1) { snprintf(err, errlen, "mask_fill: value = %d, 0 or 1 expected", value); return VC_ERR_ARG; }
  if ((uintptr_t)mask & 1) { snprintf(err, errlen, "mask_fill: mask is not aligned to its element size"); return VC_ERR_ARG; }
  const long threads = (long)h * w;
  hipLaunchKernelGGL(mask_fill_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, (bf16_t*)mask, h, Wrow, x0, w,
                     (bf16_t)(value ? 0x3F80 : 0));
  return vc_launch_status("mask_fill launch", err, errlen);
}
