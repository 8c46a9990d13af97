// LoRA merge: out = bf16(W + s * (B @ A)), bias_out = bf16(b + s * b_B) - LinearLora (models/modules/lora.py:66-67, 92-98) folded
// into ONE weight, what vc_flux_bind_weight wants bound.  One launch per Linear (+ a tiny one for the bias).
//
//   W [O, I] bf16 or f32, A = lora_A.weight [R, I] bf16, B = lora_B.weight [O, R] bf16, all in nn.Linear's own layout.
//   acc[o, i] = sum_k B[o, k] * A[k, i] on v_mfma_f32_16x16x32_bf16 (bf16 x bf16 is exact in f32, f32 accumulation), then
//   out[o, i] = bf16_rne(W[o, i] + s * acc[o, i]) with the multiply and the add rounded SEPARATELY, as torch's
//   `W32 += scale * (B32 @ A32)` does; only the order of the f32 sums inside acc differs from an f32 matmul.
//
// The launch is bound by HBM (W is read once and written once; A and B are a few MB and live in L2), so the structure is the
// plainest one that keeps W's traffic in 16-byte pieces:
//   * a workgroup owns a strip of 128 columns of `in` and a run of rows of `out`.  It first writes its strip of A TRANSPOSED into
//     LDS - At[i][k], the whole K (R <= 512) resident, zero beyond R (up to the next multiple of 128) and beyond `in` - which
//     is the only place where A's layout matters: nothing transposed ever exists in HBM;
//   * each of the 8 waves then walks 16 rows of `out` at a time: the MFMA's A operand (its 16 rows = 16 columns i) comes from
//     the LDS image by ds_read_b128, its B operand (its 16 columns = 16 rows o) straight from lora_B's rows in global memory,
//     K-contiguous as they are;  8 accumulator tiles cover the 128 columns;
//   * the i <-> MFMA-row assignment is permuted so that a lane ends with 8 CONSECUTIVE columns of one row o (tile 2p holds
//     columns 32p + 8g + 0..3 in lane group g, tile 2p+1 columns 32p + 8g + 4..7): W is loaded and out is stored 16 bytes per lane.
// IN PLACE (out == W, bf16): a wave loads its 16 x 128 piece of W into registers before it stores the same piece, and no piece
// is read or written by any other wave or workgroup, so no element is overwritten before it was read.
// LDS image: row i = 2 * ks bytes (ks = R rounded up to 128 elements: 16-byte chunk c of a row lives at chunk c ^ key, key = the
// MFMA row that reads it, 0..15) - the 16 lanes ds_read_b128 serves together then touch 16 different chunks.
// Shapes: any O, I, 1 <= R <= 512; VEC = every base 16-byte aligned, I and every row stride multiples of 8 elements - otherwise
// the same kernel runs with element-wise global accesses (the tiny test model, in = 12).  R == 0: a conversion / copy of W.
// PERM (vc_lora_merge_qkv, qkv_heads = H > 0): the same arithmetic, and row r of the result is STORED at row dest_row(r) - the
// head-permuted order of VcGemmProblem.kn_heads (the inverse of hip.qkv_head_permutation), rows >= 3 * 128 H (linear1's MLP rows)
// where they were.  A wave's 16 rows start at a multiple of 16, which divides 64 and 128: they stay 16 consecutive rows, and every
// access keeps its width.  No in-place form: the piece a wave writes is not the piece it read.
#include "common.h"
#include "vcloze_internal.h"

namespace {

constexpr int LM_TI = 128;        // columns of `in` per workgroup
constexpr int LM_THREADS = 512;   // 8 waves share one LDS image of A
constexpr int LM_WROWS = 16;      // rows of `out` per wave and pass
constexpr int LM_MAX_RANK = 512;

struct LoraMergeArgs {
  const void* w;
  const bf16_t* a;
  const bf16_t* b;
  bf16_t* out;
  int64_t ldw, lda, ldb, ldo;
  float s;
  int O, I, R;
  int ks;            // LDS row length in elements: R rounded up to 128 (0 with R == 0)
  int rows_per_wg;   // multiple of 128
  int qd;            // PERM only: 128 * qkv_heads
};
// where row r of a qkv weight [3 * D + ..., K] goes: 2H blocks of 192 rows = [query / key head t | V rows 64 t .. 64 t + 63]
VC_DEV int dest_row(int r, int D) {
  if (r < 2 * D) return 192 * (r >> 7) + (r & 127);
  if (r < 3 * D) return 192 * ((r - 2 * D) >> 6) + 128 + ((r - 2 * D) & 63);
  return r;
}

// 8 consecutive bf16 of a row of n elements starting at col, zero beyond n
template <bool VEC>
VC_DEV u32x4 ld8(const bf16_t* row, int col, int n) {
  if (VEC && col + 8 <= n) return *(const u32x4*)(row + col);
  u32x4 v = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int e = 0; e < 8; ++e)
    if (col + e < n) v[e >> 1] |= (uint32_t)row[col + e] << (16 * (e & 1));
  return v;
}
VC_DEV uint32_t elem16(const u32x4 v, int e) { return (v[e >> 1] >> (16 * (e & 1))) & 0xffffu; }
// w + s * d as torch's `W32 += scale * delta` rounds it: the product to f32, then the sum to f32.  Contraction is switched OFF
// for this function (hipcc's default would fuse the two into one v_fma_f32; __fmul_rn / __fadd_rn are plain * and + in this
// toolchain's headers and do not prevent it) - the flags travel with the instructions through inlining, as in qknorm_rope8.
VC_DEV float scale_add(float w, float s, float d) {
#pragma clang fp contract(off)
  const float sd = s * d;
  return w + sd;
}

template <bool VEC, bool WF32, bool PERM>
__global__ __launch_bounds__(LM_THREADS) void lora_merge_kernel(const LoraMergeArgs p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lm_lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m = lane & 15, g = lane >> 4;
  const int i0 = blockIdx.x * LM_TI;
  const int row_bytes = p.ks * 2;

  // ---- A[0:R, i0:i0+128] -> LDS, transposed: a thread takes 8 columns of two consecutive rows k, k + 1 and writes 8 dwords
  // (the whole padded K, ks: the main loop runs in groups of four MFMA steps and multiplies the padding by B's zero fill)
#pragma unroll 8
  for (int it = tid; it < (p.ks >> 5) * 16 * 16; it += LM_THREADS) {
    const int cc = it & 15, k0 = (it >> 4) * 2;
    const int col = i0 + 8 * cc;
    u32x4 r0 = {0u, 0u, 0u, 0u}, r1 = {0u, 0u, 0u, 0u};
    if (k0 < p.R) r0 = ld8<VEC>(p.a + (int64_t)k0 * p.lda, col, p.I);
    if (k0 + 1 < p.R) r1 = ld8<VEC>(p.a + (int64_t)(k0 + 1) * p.lda, col, p.I);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int il = 8 * cc + e;
      const int key = ((cc & 3) << 2) | (e & 3);          // = the MFMA row that reads column il
      const int off = il * row_bytes + (((k0 >> 3) ^ key) << 4) + (k0 & 7) * 2;
      *(uint32_t*)(lm_lds + off) = elem16(r0, e) | (elem16(r1, e) << 16);
    }
  }
  __syncthreads();

  // byte offset of the LDS row this lane reads for accumulator tile t: column 32 (t >> 1) + 4 (t & 1) + 8 (m >> 2) + (m & 3)
  const int arow = (8 * (m >> 2) + (m & 3)) * row_bytes;
  const int row_end = min(p.O, (int)(blockIdx.y + 1) * p.rows_per_wg);
  for (int row0 = blockIdx.y * p.rows_per_wg + wave * LM_WROWS; row0 < row_end; row0 += (LM_THREADS / 64) * LM_WROWS) {
    const int o = row0 + m;
    const bool ok = o < p.O;
    // this lane's 4 x 8 values of W: row o, columns i0 + 32 q + 8 g + 0..7 - in flight while the MFMAs run
    float wv[4][8];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int col = i0 + 32 * q + 8 * g;
#pragma unroll
      for (int e = 0; e < 8; ++e) wv[q][e] = 0.0f;
      if (!ok) continue;
      if (WF32) {
        const float* wr = (const float*)p.w + (int64_t)o * p.ldw;
        if (VEC && col + 8 <= p.I) {
          const f32x4 lo = *(const f32x4*)(wr + col), hi = *(const f32x4*)(wr + col + 4);
#pragma unroll
          for (int e = 0; e < 4; ++e) { wv[q][e] = lo[e]; wv[q][4 + e] = hi[e]; }
        } else {
#pragma unroll
          for (int e = 0; e < 8; ++e)
            if (col + e < p.I) wv[q][e] = wr[col + e];
        }
      } else {
        const u32x4 v = ld8<VEC>((const bf16_t*)p.w + (int64_t)o * p.ldw, col, p.I);
#pragma unroll
        for (int e = 0; e < 4; ++e) { wv[q][2 * e] = lo_bf(v[e]); wv[q][2 * e + 1] = hi_bf(v[e]); }
      }
    }
    f32x4 acc[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) acc[t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    const bf16_t* brow = p.b + (int64_t)(ok ? o : 0) * p.ldb;
    // four MFMA steps (128 of K) at a time; the four pieces of B[o, :] of the NEXT group are requested before the 32 MFMAs of
    // this one run, so that one trip to L2 is exposed per pass, not one per group
    u32x4 bf[4], nx[4];                                  // B[o, 128 kg + 32 j + 8 g + 0..7]: the MFMA's B operand, column o
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      nx[j] = u32x4{0u, 0u, 0u, 0u};
      if (ok) nx[j] = ld8<VEC>(brow, 32 * j + 8 * g, p.R);      // (zero beyond R, and everywhere with R == 0)
    }
    for (int kg = 0; kg < (p.ks >> 7); ++kg) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        bf[j] = nx[j];
        nx[j] = u32x4{0u, 0u, 0u, 0u};
        if (ok) nx[j] = ld8<VEC>(brow, 128 * (kg + 1) + 32 * j + 8 * g, p.R);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int chunk = ((16 * kg + 4 * j + g) ^ m) << 4;
#pragma unroll
        for (int t = 0; t < 8; ++t) {
          const u32x4 af = *(const u32x4*)(lm_lds + arow + (32 * (t >> 1) + 4 * (t & 1)) * row_bytes + chunk);
          acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, af), __builtin_bit_cast(bf16x8, bf[j]), acc[t], 0, 0, 0);
        }
      }
    }
    if (!ok) continue;
    bf16_t* orow = p.out + (int64_t)(PERM ? dest_row(o, p.qd) : o) * p.ldo;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int col = i0 + 32 * q + 8 * g;
      if (col >= p.I) continue;
      float y[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float d = acc[2 * q + (e >> 2)][e & 3];
        // two roundings (scale_add), never one fused multiply-add; R == 0 is a pure conversion (keeps the sign of a zero)
        y[e] = p.R ? scale_add(wv[q][e], p.s, d) : wv[q][e];
      }
      if (VEC && col + 8 <= p.I) {
        u32x4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = pack2bf(y[2 * e], y[2 * e + 1]);
        *(u32x4*)(orow + col) = v;
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e)
          if (col + e < p.I) orow[col + e] = f2bf(y[e]);
      }
    }
  }
}

// bias_out[o] = bf16(b[o] + s * bB[o]);  b NULL = 0;  bB NULL: a conversion / copy of b;  qd > 0: stored at dest_row(o)
__global__ __launch_bounds__(256) void lora_bias_kernel(const void* b, int b_f32, const bf16_t* bB, float s, bf16_t* out, int n, int qd) {
  const int o = blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= n) return;
  const float v = !b ? 0.0f : b_f32 ? ((const float*)b)[o] : bf2f(((const bf16_t*)b)[o]);
  out[qd ? dest_row(o, qd) : o] = f2bf(bB ? scale_add(v, s, bf2f(bB[o])) : v);
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
// [first, last) byte range of a matrix of `rows` rows of `cols` elements of `esz` bytes with row stride ld
inline void span(const void* p, int64_t rows, int64_t cols, int64_t ld, int esz, uintptr_t* lo, uintptr_t* hi) {
  *lo = (uintptr_t)p;
  *hi = *lo + (uintptr_t)(((rows - 1) * ld + cols) * esz);
}
inline bool overlap(uintptr_t alo, uintptr_t ahi, uintptr_t blo, uintptr_t bhi) { return alo < bhi && blo < ahi; }

}  // namespace

#define LM_FAIL(...) do { snprintf(err, errlen, __VA_ARGS__); return VC_ERR_ARG; } while (0)

int vc_lora_merge_qkv_launch(const void* w, int32_t w_is_f32, int64_t ldw, const void* lora_a, int64_t lda, const void* lora_b, int64_t ldb,
                             float scale, void* out, int64_t ldo, const void* bias, int32_t bias_is_f32, const void* lora_b_bias,
                             void* bias_out, int32_t O, int32_t I, int32_t R, int32_t qkv_heads, hipStream_t s, char* err, int errlen) {
  // ---- every check before the first HIP call
  if (O <= 0 || I <= 0) LM_FAIL("lora_merge: out_features and in_features must be positive (got %d, %d)", O, I);
  if (R < 0 || R > LM_MAX_RANK) LM_FAIL("lora_merge: rank %d outside 0 .. %d", R, LM_MAX_RANK);
  if (!w || !out) LM_FAIL("lora_merge: null weight or out");
  if (qkv_heads < 0 || (int64_t)qkv_heads * 384 > O)
    LM_FAIL("lora_merge: qkv_heads = %d needs out_features >= 3 * 128 * qkv_heads, got %d", qkv_heads, O);
  if (R > 0 && (!lora_a || !lora_b)) LM_FAIL("lora_merge: null LoRA factor with rank %d", R);
  if (ldw < I || ldo < I) LM_FAIL("lora_merge: row stride of weight (%lld) or out (%lld) shorter than a row of %d", (long long)ldw, (long long)ldo, I);
  if (R > 0 && (lda < I || ldb < R)) LM_FAIL("lora_merge: row stride of lora_a (%lld, row %d) or lora_b (%lld, row %d) shorter than a row", (long long)lda, I, (long long)ldb, R);
  uintptr_t wlo, whi, olo, ohi;
  span(w, O, I, ldw, w_is_f32 ? 4 : 2, &wlo, &whi);
  span(out, O, I, ldo, 2, &olo, &ohi);
  if (qkv_heads > 0 && overlap(wlo, whi, olo, ohi)) LM_FAIL("lora_merge: out overlaps weight (with qkv_heads > 0 there is no in-place form)");
  if (out == w) {
    if (w_is_f32) LM_FAIL("lora_merge: an f32 weight cannot be merged in place (out is bf16)");
    if (ldo != ldw) LM_FAIL("lora_merge: in place (out == weight) needs equal row strides, got %lld and %lld", (long long)ldw, (long long)ldo);
  } else if (overlap(wlo, whi, olo, ohi)) {
    LM_FAIL("lora_merge: out overlaps weight without being equal to it");
  }
  if (R > 0) {
    uintptr_t lo, hi;
    span(lora_a, R, I, lda, 2, &lo, &hi);
    if (overlap(lo, hi, olo, ohi)) LM_FAIL("lora_merge: out overlaps lora_a");
    span(lora_b, O, R, ldb, 2, &lo, &hi);
    if (overlap(lo, hi, olo, ohi)) LM_FAIL("lora_merge: out overlaps lora_b");
  }
  if (!bias_out && (bias || lora_b_bias)) LM_FAIL("lora_merge: a bias was passed but bias_out is null");
  if (bias_out && !bias && !lora_b_bias) LM_FAIL("lora_merge: bias_out without bias or lora_b_bias");
  if (bias_out && bias_out == bias && bias_is_f32) LM_FAIL("lora_merge: an f32 bias cannot be merged in place (bias_out is bf16)");
  if (bias_out && bias_out == bias && qkv_heads > 0) LM_FAIL("lora_merge: bias_out overlaps bias (with qkv_heads > 0 there is no in-place form)");
  if (bias_out) {
    uintptr_t blo = (uintptr_t)bias_out, bhi = blo + (uintptr_t)O * 2;
    if (overlap(blo, bhi, olo, ohi)) LM_FAIL("lora_merge: bias_out overlaps out");
    if (bias && bias_out != bias && overlap(blo, bhi, (uintptr_t)bias, (uintptr_t)bias + (uintptr_t)O * (bias_is_f32 ? 4 : 2)))
      LM_FAIL("lora_merge: bias_out overlaps bias without being equal to it");
    if (lora_b_bias && overlap(blo, bhi, (uintptr_t)lora_b_bias, (uintptr_t)lora_b_bias + (uintptr_t)O * 2))
      LM_FAIL("lora_merge: bias_out overlaps lora_b_bias");
  }

  LoraMergeArgs p;
  p.w = w; p.a = (const bf16_t*)lora_a; p.b = (const bf16_t*)lora_b; p.out = (bf16_t*)out;
  p.ldw = ldw; p.lda = lda; p.ldb = ldb; p.ldo = ldo;
  p.s = scale; p.O = O; p.I = I; p.R = R;
  p.ks = (R + 127) / 128 * 128;
  p.qd = 128 * qkv_heads;
  // rows per workgroup: 256, halved to 128 (one pass of the 8 waves) while the launch has fewer than 1024 workgroups.  Measured
  // on MI355X the choice moves the time by a few per cent either way (thresholds 256 / 512 / 1024 at 3072 x 3072 .. 9216 x 3072).
  const int strips = (I + LM_TI - 1) / LM_TI;
  int rows = 256;
  while (rows > 128 && (int64_t)strips * ((O + rows - 1) / rows) < 1024) rows >>= 1;
  while ((O + rows - 1) / rows > 65535) rows <<= 1;
  p.rows_per_wg = rows;
  const bool vec = aligned16(w) && aligned16(out) && I % 8 == 0 && ldw % 8 == 0 && ldo % 8 == 0 &&
                   (R == 0 || (aligned16(lora_a) && aligned16(lora_b) && lda % 8 == 0 && ldb % 8 == 0));
  void (*const fns[8])(const LoraMergeArgs) = {
      lora_merge_kernel<false, false, false>, lora_merge_kernel<false, true, false>, lora_merge_kernel<true, false, false>,
      lora_merge_kernel<true, true, false>,   lora_merge_kernel<false, false, true>, lora_merge_kernel<false, true, true>,
      lora_merge_kernel<true, false, true>,   lora_merge_kernel<true, true, true>};
  const int lds = LM_TI * p.ks * 2;     // 32 KiB per 128 of rank: 128 KiB at rank 512
  static VcOncePerDevice attr_done[8];
  const int slot = (qkv_heads > 0 ? 4 : 0) + (vec ? 2 : 0) + (w_is_f32 ? 1 : 0);
  void (*fn)(const LoraMergeArgs) = fns[slot];
  if (attr_done[slot].need()) {
    hipError_t e = hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, LM_TI * LM_MAX_RANK * 2);
    if (e != hipSuccess) { snprintf(err, errlen, "lora_merge: hipFuncSetAttribute: %s", hipGetErrorString(e)); return VC_ERR_HIP; }
    attr_done[slot].mark();
  }
  hipLaunchKernelGGL(fn, dim3(strips, (O + rows - 1) / rows), dim3(LM_THREADS), lds, s, p);
  int rc = vc_launch_status("lora_merge", err, errlen);
  if (rc == VC_OK && bias_out) {
    hipLaunchKernelGGL(lora_bias_kernel, dim3((O + 255) / 256), dim3(256), 0, s, bias, bias_is_f32, (const bf16_t*)lora_b_bias, scale,
                       (bf16_t*)bias_out, O, p.qd);
    rc = vc_launch_status("lora_merge", err, errlen);
  }
  return rc;
}

int vc_lora_merge_launch(const void* w, int32_t w_is_f32, int64_t ldw, const void* lora_a, int64_t lda, const void* lora_b, int64_t ldb,
                         float scale, void* out, int64_t ldo, const void* bias, int32_t bias_is_f32, const void* lora_b_bias,
                         void* bias_out, int32_t O, int32_t I, int32_t R, hipStream_t s, char* err, int errlen) {
  return vc_lora_merge_qkv_launch(w, w_is_f32, ldw, lora_a, lda, lora_b, ldb, scale, out, ldo, bias, bias_is_f32, lora_b_bias, bias_out, O, I,
                                  R, 0, s, err, errlen);
}
