// The host arithmetic of vc_image_compare (include/vcloze_hip.h: IMAGE COMPARE), host only - no HIP type - so that a plain host
// program can check it (tests/c_abi/image_tiling_check.cpp): the tile grid, the partition of a channel's pixels among the tiles
// for the error sums, and the eleven window weights.  image_metrics.hip uses the same functions in its kernels.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define VC_IMG_FN __host__ __device__ inline
#else
#define VC_IMG_FN inline
#endif

namespace vcimg {

constexpr int TILE = 32;                     // VC_IMG_TILE: windows per tile side
constexpr int TAPS = 11;                     // the window's side
constexpr int HALO = TILE + TAPS - 1;        // 42: the pixels a tile's windows cover, per side

// tiles along an axis of `extent` pixels (extent >= TAPS)
VC_IMG_FN int tiles(int extent) { return (extent - (TAPS - 1) + TILE - 1) / TILE; }
// of tile `t` along that axis: the halo pixels that lie inside the image, 11 .. 42
VC_IMG_FN int halo_extent(int extent, int t) {
  const int left = extent - t * TILE;
  return left < HALO ? left : HALO;
}
// ... its valid windows, 1 .. 32
VC_IMG_FN int windows(int extent, int t) { return halo_extent(extent, t) - (TAPS - 1); }
// ... and the halo pixels it OWNS for the error sums: the first 32, the last tile all of its halo - the owned ranges
// [t * 32, t * 32 + owned) tile [0, extent) without gap or overlap
VC_IMG_FN int owned(int extent, int t) { return t == tiles(extent) - 1 ? halo_extent(extent, t) : TILE; }

// exp(-(k - 5)^2 / 4.5) normalised in double to sum 1, rounded to f32 once: what VC_SSIM_WEIGHTS lists
inline void weights(float out[TAPS]) {
  double g[TAPS], sum = 0.0;
  for (int k = 0; k < TAPS; ++k) { g[k] = exp(-(double)((k - 5) * (k - 5)) / 4.5); sum += g[k]; }
  for (int k = 0; k < TAPS; ++k) out[k] = (float)(g[k] / sum);
}

}  // namespace vcimg
