// vc_image_compare (include/vcloze_hip.h: IMAGE COMPARE): the distance between two renderings of equal geometry - error sums and
// the mean SSIM over the valid 11 x 11 Gaussian windows - in two launches, without atomics: repeated runs give the same bits.
//   image_tile_kernel    one workgroup of 256 threads per tile of 32 x 32 windows of one channel.  The 42 x 42 halo of both images
//                        goes to LDS once as f32 (16-byte loads where the host found them legal, element loads otherwise: the LDS
//                        image is the same); the horizontal pass writes the five moment planes (a, b, a^2, b^2, ab) to LDS, the
//                        vertical pass and the SSIM formula stay in registers; the error sums run over the pixels the tile OWNS
//                        (image_tiling.h: every pixel in exactly one tile), read back from LDS so that their order does not depend
//                        on the load path.  LDS trees, one 32-byte record per tile.
//   image_finish_kernel  one workgroup folds the records in a fixed order (doubles and 64-bit integers) and writes VcImageMetrics.
// The order of every operation is the header's; nothing may be contracted.  LDS rows: a half-wave reads or writes 32 consecutive
// words of one row in every pass (ds_read_b32 / ds_write_b32 bank by word % 32 per 32-lane half): no bank conflict at any stride.
// Memory-bound and small beside a model evaluation: NOT tuned beyond that (one channel per workgroup re-reads the interleaved
// 8-bit rows three times, from L2).
#include <type_traits>
#include "common.h"
#include "vcloze_internal.h"
#include "block_reduce.h"
#include "image_tiling.h"

namespace {

using vcimg::HALO;
using vcimg::TAPS;
using vcimg::TILE;
constexpr int IMG_THREADS = 256;
constexpr int HS = 44;                       // halo row stride: 11 chunks of 4 f32 land without a guard
constexpr int ROWS_PER_THREAD = TILE * TILE / IMG_THREADS;                    // 4 windows per thread
constexpr int ERR_VISITS = (HALO * HALO + IMG_THREADS - 1) / IMG_THREADS;     // 7 halo positions per thread
static_assert(VC_IMG_TILE == TILE && (IMG_THREADS % TILE) == 0, "thread t owns column t % 32");
__constant__ const float IMG_W[TAPS] = VC_SSIM_WEIGHTS;

struct ImgRecord { uint64_t sse_u; float ssim; float sse_f; float max_abs; uint32_t n_diff; uint32_t pad[2]; };
static_assert(sizeof(ImgRecord) == VC_IMG_RECORD_BYTES, "the scratch record of the header");

template <bool U8, bool WIDE>
VC_DEV void load_halo(const void* __restrict__ img, float (&h)[HALO][HS], int c, int C, int H, int W, int y0, int x0) {
  const int t = threadIdx.x;
  if constexpr (!WIDE) {
    for (int q = t; q < HALO * HALO; q += IMG_THREADS) {
      const int r = q / HALO, col = q - r * HALO, y = y0 + r, x = x0 + col;
      float v = 0.0f;
      if (y < H && x < W) {
        if constexpr (U8) v = (float)((const unsigned char*)img)[((long)y * W + x) * C + c];
        else v = ((const float*)img)[((long)c * H + y) * W + x];
      }
      h[r][col] = v;
    }
  } else if constexpr (U8) {
    // C == 3, W % 16 == 0, base 16-byte aligned: a row is 3 W bytes, the tile's segment starts 96 tx bytes into it - both multiples of
    // 16 - and its 126 bytes lie in 8 chunks, each wholly inside the row or wholly outside
    const long rowb = 3L * W;
    for (int q = t; q < HALO * 8; q += IMG_THREADS) {
      const int r = q >> 3, k = q & 7, y = y0 + r;
      const long xb = 3L * x0 + 16 * k;
      u32x4 w = {0u, 0u, 0u, 0u};
      if (y < H && xb < rowb) w = *(const u32x4*)((const unsigned char*)img + y * rowb + xb);
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const int bo = 16 * k + j, px = bo / 3;
        const uint32_t word = w[j >> 2];
        if (bo - 3 * px == c && px < HALO) h[r][px] = (float)((word >> (8 * (j & 3))) & 0xffu);
      }
    }
  } else {
    // W % 16 == 0, base 16-byte aligned: 11 chunks of 4 f32 from column 32 tx, each wholly inside the row or wholly outside
    for (int q = t; q < HALO * 11; q += IMG_THREADS) {
      const int r = q / 11, k = q - 11 * r, y = y0 + r, x = x0 + 4 * k;
      f32x4 w = {0.0f, 0.0f, 0.0f, 0.0f};
      if (y < H && x < W) w = *(const f32x4*)((const float*)img + ((long)c * H + y) * W + x);
#pragma unroll
      for (int e = 0; e < 4; ++e) h[r][4 * k + e] = w[e];
    }
  }
}

// s = w[0] * p[0];  s = s + w[k] * p[k], k ascending, every product and every sum rounded on its own
VC_DEV float taps11(const float (&p)[TAPS]) {
#pragma clang fp contract(off)
  float s = IMG_W[0] * p[0];
#pragma unroll
  for (int k = 1; k < TAPS; ++k) {
    const float m = IMG_W[k] * p[k];
    s = s + m;
  }
  return s;
}

VC_DEV float ssim_of(float mu_a, float mu_b, float e_aa, float e_bb, float e_ab, float c1, float c2) {
#pragma clang fp contract(off)
  const float ma2 = mu_a * mu_a, mb2 = mu_b * mu_b, mab = mu_a * mu_b;
  const float va = e_aa - ma2, vb = e_bb - mb2, cab = e_ab - mab;
  const float t1 = mab + mab, t2 = cab + cab, s1 = ma2 + mb2, s2 = va + vb;
  const float n1 = t1 + c1, n2 = t2 + c2, d1 = s1 + c1, d2 = s2 + c2;
  const float num = n1 * n2, den = d1 * d2;
  return num / den;
}

struct MaxOp { VC_DEV float operator()(float x, float y) const { return y > x ? y : x; } };
// a tile's sums go down ONE tree (block_reduce.h), field by field; `sse` is the integer sum for 8-bit images, the float one otherwise
template <bool U8> struct TileAcc { float ssim, mx; uint32_t nd; std::conditional_t<U8, uint32_t, float> sse; };
struct TileOp {
  template <typename A> VC_DEV A operator()(A x, A y) const { return A{x.ssim + y.ssim, MaxOp()(x.mx, y.mx), x.nd + y.nd, x.sse + y.sse}; }
};
// the finish kernel's 8-byte fields; max_abs keeps a tree of its own
struct ImgTotals { double ssim, sse_f; uint64_t sse_u, nd; };
struct TotalsOp {
  VC_DEV ImgTotals operator()(ImgTotals x, ImgTotals y) const { return ImgTotals{x.ssim + y.ssim, x.sse_f + y.sse_f, x.sse_u + y.sse_u, x.nd + y.nd}; }
};

// grid (TX, TY, C)
template <bool U8, bool WIDE>
__global__ __launch_bounds__(IMG_THREADS) void image_tile_kernel(const void* __restrict__ a, const void* __restrict__ b, int C, int H, int W,
                                                                  float c1, float c2, ImgRecord* __restrict__ rec) {
#pragma clang fp contract(off)
  __shared__ float ha[HALO][HS], hb[HALO][HS];
  __shared__ float pl[5][HALO][TILE];
  __shared__ TileAcc<U8> lt[IMG_THREADS];
  const int t = threadIdx.x, tx = blockIdx.x, ty = blockIdx.y, c = blockIdx.z;
  const int y0 = ty * TILE, x0 = tx * TILE;
  load_halo<U8, WIDE>(a, ha, c, C, H, W, y0, x0);
  load_halo<U8, WIDE>(b, hb, c, C, H, W, y0, x0);
  __syncthreads();

  // the error sums of the pixels this tile owns
  const int own_y = vcimg::owned(H, ty), own_x = vcimg::owned(W, tx);
  float sse_f = 0.0f, mx = 0.0f;
  uint32_t sse_u = 0u, nd = 0u;
#pragma unroll
  for (int i = 0; i < ERR_VISITS; ++i) {
    const int q = t + IMG_THREADS * i, r = q / HALO, col = q - r * HALO;
    if (q < HALO * HALO && r < own_y && col < own_x) {
      const float va = ha[r][col], vb = hb[r][col];
      const float d = va - vb, ad = __builtin_fabsf(d);
      nd += va != vb ? 1u : 0u;
      mx = ad > mx ? ad : mx;
      if constexpr (U8) {
        const uint32_t di = (uint32_t)ad;
        sse_u += di * di;
      } else {
        const float sq = d * d;
        sse_f = sse_f + sq;
      }
    }
  }

  // horizontal pass: 42 halo rows x 32 columns, five planes
  for (int q = t; q < HALO * TILE; q += IMG_THREADS) {
    const int r = q / TILE, x = q - r * TILE;
    float pa[TAPS], pb[TAPS], paa[TAPS], pbb[TAPS], pab[TAPS];
#pragma unroll
    for (int k = 0; k < TAPS; ++k) {
      pa[k] = ha[r][x + k];
      pb[k] = hb[r][x + k];
      paa[k] = pa[k] * pa[k];
      pbb[k] = pb[k] * pb[k];
      pab[k] = pa[k] * pb[k];
    }
    pl[0][r][x] = taps11(pa);
    pl[1][r][x] = taps11(pb);
    pl[2][r][x] = taps11(paa);
    pl[3][r][x] = taps11(pbb);
    pl[4][r][x] = taps11(pab);
  }
  __syncthreads();

  // vertical pass and the formula: thread t owns column t % 32, rows t / 32 + 8 i
  const int win_y = vcimg::windows(H, ty), win_x = vcimg::windows(W, tx);
  const int x = t % TILE;
  float ssim = 0.0f;
#pragma unroll
  for (int i = 0; i < ROWS_PER_THREAD; ++i) {
    const int y = t / TILE + (IMG_THREADS / TILE) * i;
    if (y < win_y && x < win_x) {
      float m[5];
#pragma unroll
      for (int p = 0; p < 5; ++p) {
        float col[TAPS];
#pragma unroll
        for (int j = 0; j < TAPS; ++j) col[j] = pl[p][y + j][x];
        m[p] = taps11(col);
      }
      const float v = ssim_of(m[0], m[1], m[2], m[3], m[4], c1, c2);
      ssim = ssim + v;
    }
  }

  TileAcc<U8> acc;
  acc.ssim = ssim; acc.mx = mx; acc.nd = nd;
  if constexpr (U8) acc.sse = sse_u;
  else acc.sse = sse_f;
  acc = block_tree(lt, acc, TileOp());
  if (t == 0) {
    ImgRecord o;
    o.sse_u = 0; o.sse_f = 0.0f;
    if constexpr (U8) o.sse_u = acc.sse;
    else o.sse_f = acc.sse;
    o.ssim = acc.ssim; o.max_abs = acc.mx; o.n_diff = acc.nd; o.pad[0] = 0u; o.pad[1] = 0u;
    rec[((long)c * gridDim.y + ty) * gridDim.x + tx] = o;
  }
}

// one workgroup: thread t folds records t, t + 256, .. in ascending order, then the tree
__global__ __launch_bounds__(IMG_THREADS) void image_finish_kernel(const ImgRecord* __restrict__ rec, long P, uint64_t n, uint64_t n_windows, int form,
                                                                    VcImageMetrics* __restrict__ out) {
  __shared__ ImgTotals lt[IMG_THREADS];
  __shared__ float lm[IMG_THREADS];
  double ssim = 0.0, sse_f = 0.0;
  uint64_t sse_u = 0, nd = 0;
  float mx = 0.0f;
  for (long p = threadIdx.x; p < P; p += IMG_THREADS) {
    const ImgRecord r = rec[p];
    ssim = ssim + (double)r.ssim;
    sse_f = sse_f + (double)r.sse_f;
    sse_u += r.sse_u;
    nd += r.n_diff;
    mx = r.max_abs > mx ? r.max_abs : mx;
  }
  const ImgTotals tot = block_tree(lt, ImgTotals{ssim, sse_f, sse_u, nd}, TotalsOp());
  mx = block_tree(lm, mx, MaxOp());
  if (threadIdx.x == 0) {
    VcImageMetrics m;
    m.n = n; m.n_windows = n_windows; m.sse_u64 = tot.sse_u; m.n_diff = tot.nd;
    m.sse_f32 = form == VC_IMG_U8_HWC ? (float)tot.sse_u : (float)tot.sse_f;
    m.max_abs = mx;
    m.ssim_mean = (float)(tot.ssim / (double)n_windows);
    m.form = form;
    *out = m;
  }
}

int image_geometry(int C, int H, int W, long* P, char* err, int errlen) {
  if (C < 1 || C > 65535) { snprintf(err, errlen, "image_compare: C = %d must lie in 1..65535", C); return VC_ERR_ARG; }
  if (H < TAPS || W < TAPS || H > 65535 || W > 65535) {
    snprintf(err, errlen, "image_compare: image size %dx%d must lie in 11..65535 (one 11 x 11 window needs 11 rows and 11 columns)", H, W);
    return VC_ERR_ARG;
  }
  *P = (long)C * vcimg::tiles(H) * vcimg::tiles(W);
  return VC_OK;
}

}  // namespace

int vc_image_compare_scratch_bytes_impl(int C, int H, int W, int64_t* bytes, char* err, int errlen) {
  if (!bytes) { snprintf(err, errlen, "image_compare_scratch_bytes: null bytes"); return VC_ERR_ARG; }
  long P;
  const int rc = image_geometry(C, H, W, &P, err, errlen);
  if (rc != VC_OK) return rc;
  *bytes = (int64_t)P * VC_IMG_RECORD_BYTES;
  return VC_OK;
}

int vc_image_compare_launch(const void* a, const void* b, int form, int C, int H, int W, VcImageMetrics* out_dev, void* scratch, int64_t scratch_bytes,
                            hipStream_t s, char* err, int errlen) {
  if (!a || !b || !out_dev || !scratch) { snprintf(err, errlen, "image_compare: null a / b / out_dev / scratch"); return VC_ERR_ARG; }
  if (form != VC_IMG_U8_HWC && form != VC_IMG_F32_CHW) {
    snprintf(err, errlen, "image_compare: unknown form %d (VC_IMG_U8_HWC, VC_IMG_F32_CHW)", form);
    return VC_ERR_ARG;
  }
  long P;
  const int rc = image_geometry(C, H, W, &P, err, errlen);
  if (rc != VC_OK) return rc;
  const bool u8 = form == VC_IMG_U8_HWC;
  if (!u8 && (((uintptr_t)a | (uintptr_t)b) & 3)) { snprintf(err, errlen, "image_compare: an F32 image is not aligned to 4 bytes"); return VC_ERR_ARG; }
  if (((uintptr_t)out_dev | (uintptr_t)scratch) & 15) { snprintf(err, errlen, "image_compare: out_dev / scratch must be aligned to 16 bytes"); return VC_ERR_ARG; }
  if (scratch_bytes < (int64_t)P * VC_IMG_RECORD_BYTES) {
    snprintf(err, errlen, "image_compare: scratch_bytes = %lld is smaller than the %lld bytes of %ld tile records", (long long)scratch_bytes,
             (long long)((int64_t)P * VC_IMG_RECORD_BYTES), P);
    return VC_ERR_ARG;
  }
  const double L = u8 ? 255.0 : 1.0;
  const float c1 = (float)((0.01 * L) * (0.01 * L)), c2 = (float)((0.03 * L) * (0.03 * L));
  const bool wide = W % 16 == 0 && !(((uintptr_t)a | (uintptr_t)b) & 15) && (!u8 || C == 3);
  const dim3 grid((unsigned)vcimg::tiles(W), (unsigned)vcimg::tiles(H), (unsigned)C), block(IMG_THREADS);
  ImgRecord* rec = (ImgRecord*)scratch;
#define VC_IMG_LAUNCH(U, V) hipLaunchKernelGGL((image_tile_kernel<U, V>), grid, block, 0, s, a, b, C, H, W, c1, c2, rec)
  if (u8) { if (wide) VC_IMG_LAUNCH(true, true); else VC_IMG_LAUNCH(true, false); }
  else { if (wide) VC_IMG_LAUNCH(false, true); else VC_IMG_LAUNCH(false, false); }
#undef VC_IMG_LAUNCH
  const uint64_t n = (uint64_t)C * (uint64_t)H * (uint64_t)W, nw = (uint64_t)C * (uint64_t)(H - TAPS + 1) * (uint64_t)(W - TAPS + 1);
  hipLaunchKernelGGL(image_finish_kernel, dim3(1), block, 0, s, (const ImgRecord*)rec, P, n, nw, form, out_dev);
  return vc_launch_status("image_compare launch", err, errlen);
}

int vc_image_psnr_impl(const VcImageMetrics* m, double* psnr_db, char* err, int errlen) {
  if (!m || !psnr_db) { snprintf(err, errlen, "image_psnr: null m / psnr_db"); return VC_ERR_ARG; }
  const bool u8 = m->form == VC_IMG_U8_HWC;
  const double sse = u8 ? (double)m->sse_u64 : (double)m->sse_f32, L = u8 ? 255.0 : 1.0;
  *psnr_db = sse == 0.0 ? (double)INFINITY : 10.0 * log10(L * L * (double)m->n / sse);
  return VC_OK;
}
