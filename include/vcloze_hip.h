/* vcloze_hip.h — C ABI of the MI355X (gfx950) denoising-path kernels for VisualCloze.
 *
 * The reference (lzyhha/VisualCloze) has no FFI layer: its hot path is Python calling torch /
 * flash-attn.  This header is the boundary a maintainer would bind instead (ctypes stub in
 * INTEGRATION.md).  Every entry point names the reference interface it replaces.
 *
 * Conventions: plain pointers are DEVICE pointers (HBM) unless marked host; bf16 = raw uint16;
 * `stream` is a hipStream_t passed as void* (NULL = default stream).  Return 0 on success,
 * negative VC_ERR_* otherwise; vc_last_error() returns the message for the calling thread.
 * Not thread-safe per stream/graph handle.  No ownership is ever transferred.
 */
#ifndef VCLOZE_HIP_H
#define VCLOZE_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define VC_OK 0
#define VC_ERR_ARG (-1)
#define VC_ERR_HIP (-2)
#define VC_ERR_STATE (-3)

#define VC_ABI_VERSION 11
int vc_abi_version(void);
const char* vc_last_error(void);
/* sizeof(VcGemmProblem), sizeof(VcGemmArgs), sizeof(VcLnStream), sizeof(VcAttention), sizeof(VcFluxConfig),
 * sizeof(VcFluxInputs), sizeof(VcFluxLaunchClass) (ABI 10: SEVEN entries) as this library was compiled: a binding checks them
 * against its own mirrors at load time, so a stale .so cannot silently disagree with the caller. */
void vc_struct_sizes(int32_t out[7]);
/* number of visible devices / name of device 0 ("" when none) — fails loudly, never falls back */
int vc_device_count(void);
int vc_device_info(int dev, char* name, int namelen, int* cu_count, int64_t* hbm_bytes);

/* ---- GEMM epilogues ---- */
#define VC_EPI_BIAS 0      /* y = bf16(acc + b)                         nn.Linear              */
#define VC_EPI_GELU 1      /* y = bf16(gelu_tanh(bf16(acc + b)))        layers.py:141-145,229  */
#define VC_EPI_GATE_RES 2  /* y = bf16(res + bf16(gate*bf16(acc + b)))  layers.py:190-195,245  */
#define VC_EPI_SILU 3      /* y = bf16(silu(bf16(acc + b)))             layers.py:55-60        */
#define VC_EPI_QKV 4       /* BIAS, and columns >= vt_col0 go TRANSPOSED to vt instead of C:        */
                           /* the "K H D" split of layers.py:166,236 with V laid out key-contiguous */
                           /* for the attention kernel (what vc_qknorm_rope_vt's VC_QKN_VT part does)*/

typedef struct VcGemmProblem {
  const void* A;    /* [M,K] bf16, row stride lda (elements) */
  const void* W;    /* [N,K] bf16, row stride ldw (nn.Linear.weight layout; rows may be padded) */
  const void* bias; /* [N] bf16 or NULL */
  void* C;          /* [M,N] bf16, row stride ldc */
  const void* res;  /* GATE_RES: residual [M,N] bf16 (may alias C), row stride ldres */
  const void* gate; /* GATE_RES: gate vector(s) bf16; row b of batch uses gate + b*gate_bstride */
  int64_t lda, ldw, ldc, ldres, gate_bstride;
  /* batch-strided rows (samples of a per-GPU batch interleave text and image rows): with a_rpb > 0 row m of A lives at
   * (m / a_rpb) * a_bstride + (m % a_rpb) * lda; likewise C and res with c_rpb / c_bstride (res must share C's layout).
   * 0 = plain rows at m * ld. */
  int64_t a_bstride, c_bstride;
  int32_t M, N, K;
  int32_t rows_per_batch; /* GATE_RES: batch index of row m is m / rows_per_batch */
  int32_t a_rpb, c_rpb;
  int32_t tiles_m, tiles_n, tile_start; /* filled by the launcher */
  int32_t m_begin;                      /* filled by the launcher (first row of a split launch, see vc_gemm); pass 0 */
  /* VC_EPI_QKV (vt may be NULL = plain BIAS): element (m, n >= vt_col0) is written to
   * vt[(m / vt_rpb) * vt_bstride + (n - vt_col0) * vt_lpad + vt_row0 + m % vt_rpb], i.e. vt is [batch][N - vt_col0][vt_lpad]
   * (= [B][H][128][Lpad] of vc_attention), vt_rpb the rows of this problem per batch element and vt_row0 where they start
   * in the joint sequence (text rows 0, image rows T).  Fast when vt_col0 is a multiple of the tile width the launcher
   * picks (2 * 3072 is, for every tile) and vt_rpb, vt_row0, vt_lpad are multiples of 8; correct otherwise. */
  void* vt;
  int64_t vt_bstride;
  int32_t vt_col0, vt_rpb, vt_row0, vt_lpad;
  /* VC_EPI_QKV, kn_heads = H > 0 (N = 3 * 128 * H): W's rows / bias arrive HEAD-PERMUTED so that every 192-column tile holds one
   * whole query or key head and half a value head - permuted column p is logical column (t = p / 192, j = p % 192)
   *     j < 128:   128 t + j             (t < H: query head t; t >= H: key head t - H)
   *     else:      256 H + 64 t + j - 128 (V columns 64 t .. 64 t + 63; vt_col0 = 256 H)
   * and C is written at the logical columns ("B L (K H D)", layers.py:166,236) by any tile shape (only the 256x192 tile writes V^T
   * in whole 16-B runs).  With kn_scale and / or qn_scale != NULL (forces the 256x192 tile) the epilogue ALSO applies QKNorm with
   * kn_scale / qn_scale [128] bf16 and RoPE from kn_rope ([B?][L][64][2] f32, row vt_row0 + m % vt_rpb of batch element
   * m / vt_rpb) to every key / query head before the row leaves (layers.py:63-84, math.py:112-117): bit-identical to
   * vc_qknorm_rope_vt(parts = VC_QKN_K / VC_QKN_Q) over the plain output, which is then not needed - the "QKV + RoPE fused
   * projection".  qn_prescale != 0: the query heads leave multiplied by 128^-0.5 * log2(e) before their one rounding
   * (= parts | VC_QKN_QPRE), the form VcAttention.q_prescaled reads. */
  const void* kn_scale;
  const float* kn_rope;
  int64_t kn_rope_bstride;
  int32_t kn_heads, qn_prescale;
  const void* qn_scale;
  /* VcGemmArgs.batch = Z > 1: Z independent GEMMs of this shape in ONE launch (blockIdx.y) - instance z reads A + z * a_zstride,
   * W + z * w_zstride and writes C + z * c_zstride (elements, multiples of 8): the per-head S = Q K^T and O = P V products of an
   * attention whose head_dim the fused kernel does not cover (T5: 64 heads x d_kv 64; CLIP) as two launches per layer. */
  int64_t a_zstride, w_zstride, c_zstride;
} VcGemmProblem;

#define VC_GEMM_MAX_PROBLEMS 4
typedef struct VcGemmArgs {
  VcGemmProblem p[VC_GEMM_MAX_PROBLEMS];
  int32_t nprob; /* 1..4 problems in one grid (img+txt streams of up to two samples) */
  int32_t epi;
  const int32_t* step_ptr;  /* optional device step counter: gate += *step_ptr * gate_step_stride */
  int64_t gate_step_stride;
  uint64_t* debug_ts;       /* NULL in production; profiling: per-segment s_memtime stamps of block 0 (tools/) */
  /* Split-K remainder (ABI 7).  splitk_ws: optional f32 scratch of splitk_ws_bytes >= VC_GEMM_SPLITK_WS_BYTES in device
   * memory, NULL = never split.  With it, an auto-tiled call (tile_cfg 0) whose 256x192 tiles are R whole rounds of the CUs
   * plus a remainder of r tiles may run the remainder as r * S work items of K / S each (S <= 8, r * S <= CUs), which leave
   * f32 partial tiles in the scratch; a second, HBM-bound launch sums the S partials of each tile in a fixed order and applies
   * the epilogue (bias, GELU / SiLU / gate + residual) - bit-reproducible (static assignment), equal to the one-pass kernel up
   * to f32 summation order.  Not for VC_EPI_QKV.  The scratch belongs to ONE stream at a time: launches that share it must be
   * ordered (one stream, one linear graph) - a reduce launch of one call and the slices of the next would race otherwise.
   * sk_*: filled by the launcher. */
  void* splitk_ws;
  int64_t splitk_ws_bytes;
  int32_t sk_full, sk_rem, sk_S;
  int32_t batch;            /* 0 / 1: one GEMM per problem; Z > 1: see VcGemmProblem.a_zstride (VC_EPI_BIAS, the 128x128 tile) */
  /* ABI 8, filled by the launcher: > 0 = the STREAM form of the remainder - where it is more than half a round of tiles (no
   * S >= 2 fits), sk_stream work items (one per CU) share the remainder's K-iterations evenly, tile-major: item p owns
   * iterations [p I / n, (p + 1) I / n) of I = sk_rem * K / 64, i.e. at most two segments (end of one tile, start of the next)
   * with one f32 partial tile each (slot 2 p + segment); the reduce launch sums a tile's pieces in K order.  Static: bit-reproducible. */
  int32_t sk_stream, sk_pad_;
} VcGemmArgs;
#define VC_GEMM_SPLITK_WS_BYTES (2LL * 256 * 256 * 192 * 4)   /* two 256x192 f32 partial tiles per work item of one round of 256 CUs */

/* Replaces torch.nn.functional.linear (+ fused neighbours) on the hot path.
 * tile_cfg: 0 = chosen by the launcher's cost model (what the product path passes); a fixed tile for tests and A/B runs:
 * 1 = 128x128, 2 = 256x128, 3 = 256x256, 4 = 256x192, 5 = 256x288, +16 = ping-pong main loop (3, 4, 5),
 * +32 = ping-pong with loader waves (2, 4).
 * With tile_cfg 0 the call may become TWO launches on `stream`: when the 256x192 tiles of the problems are far from a whole
 * number of rounds of the 256 CUs, the rows of problem 0 are cut at a multiple of 256 so that the first launch is exact
 * rounds and the remainder runs on the tile shape that suits it (block-round quantisation: e.g. M = 6656, N = 3072 is
 * 416 tiles = 2 rounds at 81 % fill, or 256 tiles + 240 narrower ones).  Results do not depend on the cut.
 * VC_GEMM_NO_SPLIT (64) as tile_cfg keeps it one launch; (k << 8), k <= 255, forces the cut at row k * 256 (tests).
 * VC_GEMM_SPLITK(S) (S << 16, 2 <= S <= 8; tests and A/B runs) forces the 256x192 loader-wave tile with the tiles beyond the
 * last whole round of the CUs (all tiles when there is no whole round) cut S ways along K (needs splitk_ws);
 * VC_GEMM_NO_SPLITK keeps an auto-tiled call from doing so. */
#define VC_GEMM_NO_SPLIT 64
#define VC_GEMM_SPLITK(S) ((S) << 16)
#define VC_GEMM_NO_SPLITK (1 << 20)
#define VC_GEMM_STREAMK (1 << 21)   /* tests / A-B: force the 256x192 loader-wave tile with the remainder tiles in the STREAM form */
#define VC_GEMM_PREFER_STREAMK (1 << 22)  /* A-B: an auto-tiled call takes the stream form wherever it is eligible, whatever the cost model says */
#define VC_GEMM_STREAMK_ANY_K (1 << 23)   /* A-B: ... also below the K the launcher offers it from */
/* VC_GEMM_PERSIST (128) added to tile_cfg: a launch with more tiles than CUs on a loader-wave tile runs as ONE persistent
 * workgroup per CU that walks the tiles of its XCD's strip and fetches the next tile's first operands during the current
 * tile's epilogue (same results bit for bit; not for VC_EPI_GATE_RES).  Opt-in: measured neutral on MI355X (+0.05 % steps/s;
 * the time it removes is idle time the power-limited clock already gives back), kept for boards where it is not. */
#define VC_GEMM_PERSIST 128
int vc_gemm(const VcGemmArgs* args, int tile_cfg, void* stream);
/* The plan vc_gemm would execute for these arguments, without launching anything (works without a GPU): out[0] = first row
 * of the second launch (0 = a single launch), out[1], out[2] = tile number (1..5 as above) and main-loop form (0 plain,
 * 1 ping-pong, 2 loader waves) of the first or only launch, out[3], out[4] = of the second, out[5] = tiles of both,
 * out[6] = split-K factor S of the remainder tiles (0 = none; -n = the stream form with n work items), out[7] = how many tiles
 * are split. */
int vc_gemm_plan(const VcGemmArgs* args, int tile_cfg, int32_t out[8]);

/* LayerNorm(eps=1e-6, no affine) + AdaLN modulate: y = bf16((1+scale)*LN(x) + shift).
 * Replaces layers.py:163-164,191,195,234 / 257.  x,y: [rows, D] bf16 (row strides ldx/ldy);
 * shift/scale: bf16 vectors of D, batch b at +b*mod_bstride, step s at +s*mod_step_stride. */
int vc_ln_modulate(const void* x, int64_t ldx, void* y, int64_t ldy, const void* shift, const void* scale,
                   int64_t mod_bstride, int32_t rows, int32_t D, int32_t rows_per_batch,
                   const int32_t* step_ptr, int64_t mod_step_stride, void* stream);

/* The same op over two row sets in ONE launch - the img and txt streams of a DoubleStreamBlock, which normalise
 * different tensors with different modulation rows (layers.py:163-164 / 175-176 and 191 / 195).  b may be NULL. */
typedef struct VcLnStream {
  const void* x; int64_t ldx;        /* [rows, D] bf16, row stride ldx */
  void* y; int64_t ldy;
  const void* shift; const void* scale;
  int32_t rows; int32_t rows_per_batch;
} VcLnStream;
int vc_ln_modulate2(const VcLnStream* a, const VcLnStream* b, int64_t mod_bstride, int32_t D, const int32_t* step_ptr,
                    int64_t mod_step_stride, void* stream);

/* QK-RMSNorm (layers.py:63-84) + RoPE (math.py:112-117) in place on q,k, and V transposed to
 * vt[b][h][d][Lpad] for the attention kernel.  qkv: token rows of stride ld (elements) holding
 * q | k | v at column offsets 0, H*128, 2*H*128 ("B L (K H D)", layers.py:166).
 * rope: [B?][L][64][2] f32 (cos, sin) per pair; rope_bstride 0 = shared by the batch.
 * Token rows < split use (q_scale, k_scale), rows >= split use (q_scale2, k_scale2): the text and image
 * streams of a DoubleStreamBlock own separate QKNorm scales (layers.py:167,174); NULL scale2 = one set.
 * parts: bit 0 = the q rows, bit 1 = the k rows, bit 2 = V -> vt; 7 = everything.  6 when the attention call
 * normalises the queries itself (VcAttention.q_scale).  Bit 3 (VC_QKN_QPRE, with bit 0): the softmax scale is folded into q. */
#define VC_QKN_Q 1
#define VC_QKN_K 2
#define VC_QKN_VT 4
#define VC_QKN_QPRE 8   /* with VC_QKN_Q: the query rows leave multiplied by 128^-0.5 * log2(e) (VcAttention.q_prescaled) */
int vc_qknorm_rope_vt(void* qkv, int64_t ld, int64_t bstride, const void* q_scale, const void* k_scale,
                      const void* q_scale2, const void* k_scale2, int32_t split, const float* rope,
                      int64_t rope_bstride, void* vt, int32_t B, int32_t L, int32_t Lpad, int32_t H, int32_t parts,
                      void* stream);

/* Joint text+image attention, non-causal, D=128, softmax scale 128^-0.5 (math.py:63-99 /
 * flash_attn_varlen_func).  q,k from the qkv rows above; vt from vc_qknorm_rope_vt.
 * kv_len[b] (host-visible semantics: keys >= kv_len masked, query rows >= kv_len written as 0,
 * = pad_input of math.py:96); NULL = all L.  kv_gap (optional, with kv_len): int32 [B][2] = (lo, hi): keys and query rows
 * lo <= i < hi are masked as well - the padded tail of the TEXT stream in the joint (txt, img) order; with a valid-first
 * permutation of each stream on the host this covers arbitrary masks (math.py:9-60).  out: [B, L, H*128] bf16, row stride ldo.
 * variant: 0 = 8 waves x 32 queries per workgroup, 1 = 4 waves x 32 queries (two workgroups per CU); +2 = the same
 * kernel on a persistent grid (one workgroup per resident slot, work items assigned statically); variants 0-3 produce
 * bit-identical results.  8 = ONE WAVE PER SIMD, 4 waves x 64 queries, software-pipelined inside the wave
 * (attention64.hip), persistent; q * 128^-0.5 log2(e) is rounded to bf16 when the queries are loaded.
 * +4 (7, 12) = TAIL SPLIT: the items beyond the last full round of resident workgroups are cut along the keys into one
 * equal chunk per workgroup; partial (O, m, l) go to `scratch` (>= vc_attention_scratch_bytes(), device memory,
 * contents undefined afterwards) and a second kernel on the same stream merges them.  One scratch serves one stream at a time.  Same softmax, different f32
 * summation order for those rows.  The launcher drops the split when scratch is NULL / too small, kv_len is given, or
 * it would not shorten the critical path.
 * +16 (28; ABI 9): NO second kernel - where the kernel's stream form runs (q_prescaled and logit_bound <= 100: the product's
 * launches) each workgroup does its share of the tail FIRST, publishes its pieces (agent-scope stores + one flag word per
 * piece and query block, at the end of `scratch`) and combines the pieces assigned to it at the very end of its own work -
 * same arithmetic and order as the merge kernel (bit-identical).  CONTRACT of bit 16: `scratch` is a whole
 * vc_attention_scratch_bytes() buffer whose LAST 16 * CUs bytes (rounded up to 256: the flag words, behind the partials of
 * every variant) were ZERO before the first launch; launches that use a scratch are ordered on one stream (every launch leaves
 * the flag words zero); all workgroups of the grid (one per CU) must be able to run concurrently.  A smaller scratch, or any
 * other kernel form, ignores the bit.  28 is the default of the host engines.
 * q_scale != NULL (variants 8, 12 only): the q columns of qkv hold the RAW projection output and QKNorm + RoPE
 * (layers.py:75-84, math.py:112-117) are applied to the 64 query rows a wave loads, with q_scale / q_scale2 / split /
 * rope / rope_bstride as in vc_qknorm_rope_vt (which is then called with parts = VC_QKN_K | VC_QKN_VT).
 * q_prescaled != 0 (variants 8, 12 only; excludes q_scale): the q columns already hold QK-normed, rotated queries TIMES
 * 128^-0.5 * log2(e), rounded once (VcGemmProblem.qn_prescale / VC_QKN_QPRE): the kernel loads them straight into its MFMA
 * operand registers - no per-item prologue arithmetic. */
typedef struct VcAttention {
  const void* qkv; int64_t ld, bstride;
  const void* vt; void* out; int64_t ldo, out_bstride;
  const int32_t* kv_len;
  int32_t B, L, Lpad, H, variant, split;
  void* scratch; int64_t scratch_bytes;
  const void* q_scale; const void* q_scale2; const float* rope; int64_t rope_bstride;
  const int32_t* kv_gap;
  /* > 0 (variants 8 / 12): the caller guarantees |q.k| * 128^-0.5 * log2(e) <= logit_bound for every query / key pair - with
   * QK-normed operands (layers.py:75-84) |q|, |k| <= sqrt(128) * max|scale|, i.e. logit_bound = 16.33 * max|query_norm.scale|
   * * max|key_norm.scale| is a property of the model's weights.  For logit_bound <= 100 the kernel then runs its softmax
   * with a fixed reference point 0 (no running max: same function, 4 of 68 MFMAs and the row-max VALU work per tile
   * saved); 0 = unknown: online softmax with running max. */
  float logit_bound; int32_t q_prescaled;
} VcAttention;
int vc_attention(const VcAttention* a, void* stream);
int64_t vc_attention_scratch_bytes(void);
/* The plan vc_attention would execute for these arguments on a device of n_cu compute units (n_cu <= 0: the current device's;
 * 256 without a device), without launching anything and without touching a pointer (works without a GPU; detect by SYMBOL,
 * VC_ABI_VERSION did not change).  The argument errors of vc_attention are returned the same way.
 * out[0] = the variant the host engines choose by size for (B, L, H, n_cu), whatever a->variant says (28, 8 or 3);
 * out[1] = kernel family: 0 = 8 waves x 32 queries, 1 = 4 waves x 32 queries, 2 = 64 queries per wave with one launch slot per
 * item, 3 = its stream form; out[2] = 1: the template without a running max (logit_bound); out[3], out[4], out[5] = grid,
 * threads and dynamic LDS bytes of the attention kernel; out[6] = query blocks per (sample, head); out[7] = work items;
 * out[8] = full rounds in front of the tail split (-1 = no split), out[9] = tail items, out[10] = their (item, KV tile) units;
 * out[11] = 1: pieces combined inside the launch (bit 16 honoured); out[12] = grid of the merge kernel (0 = none runs);
 * out[13] = byte offset of the flag words in a vc_attention_scratch_bytes() buffer at n_cu; out[14] = the scratch bytes the
 * split was granted on (0 = the call touches no scratch); out[15] = 0. */
int vc_attention_plan(const VcAttention* a, int32_t n_cu, int32_t out[16]);

/* timestep_embedding (layers.py:28-49): out[b, 0:half]=cos(1000*t*f), [half:]=sin, f host table. */
int vc_timestep_embedding(const float* t, const float* freqs, void* out_bf16, int32_t n, int32_t half,
                          int32_t round_t_bf16, void* stream);
/* elementwise helpers on bf16 vectors */
int vc_silu(const void* x, void* y, int64_t n, void* stream);
/* the two epilogues of vc_gemm as stand-alone passes, for the un-merged LoRA execution mode (LinearLora.forward,
 * models/modules/lora.py:92-98: base_out + lora_B(lora_A(x)) * scale is only complete after a second GEMM):
 * act2d: y[m,n] = bf16(act(x[m,n])) on row views, act 0 = GELU(tanh) (layers.py:141-145,229), 1 = SiLU (layers.py:55-60);
 * gate_residual: out[m,n] = bf16(res[m,n] + bf16(gate[n] * y[m,n])), gate advanced by *step_ptr * gate_step_stride
 * like VcGemmArgs (layers.py:190-195,245). */
int vc_act2d(const void* x, int64_t ldx, void* y, int64_t ldy, int32_t rows, int32_t cols, int32_t act, void* stream);
int vc_gate_residual(const void* y, int64_t ldy, const void* res, int64_t ldres, const void* gate, void* out, int64_t ldo,
                     int32_t rows, int32_t cols, const int32_t* step_ptr, int64_t gate_step_stride, void* stream);
/* y[i] = bf16(bf16(a[i] + b[i % bn]) + c[i % cn]); c may be NULL (model.py:102-107: vec = time + guidance + vector) */
int vc_add3(const void* a, const void* b, const void* c, void* y, int64_t n, int64_t bn, int64_t cn, void* stream);
/* device-to-device copy on `stream` (captured as a memcpy node): restores the step-invariant txt rows */
int vc_copy(void* dst, const void* src, int64_t bytes, void* stream);
/* x||cond -> [rows, cx+cc] (transport.py:195) */
int vc_concat_cols(const void* x, int32_t cx, const void* cond, int32_t cc, void* out, int64_t rows, void* stream);
/* Euler update of the fixed-grid solver: x = bf16(x + bf16(bf16(dt) * (-v))), dt = dts[*step_ptr] (f32 table;
 * torch casts the 0-dim f32 dt to the bf16 common dtype before the multiply, transport/integrators.py:119). */
int vc_euler_step(void* x, const void* v, const float* dts, const int32_t* step_ptr, int64_t n, void* stream);
/* The same update for an f32 ODE state (the solver keeps the caller's state dtype, integrators.py:119): x32 = x32 +
 * f32(bf16(bf16(dt) * (-v))) - torch's promotion of f32 + (0-dim f32 * bf16) - and shadow = bf16(x32), what img_in's Linear
 * reads under autocast.  v == NULL: refresh the shadow only. */
int vc_euler_step_f32(float* x32, void* shadow, const void* v, const float* dts, const int32_t* step_ptr, int64_t n, void* stream);
int vc_step_advance(int32_t* step_ptr, void* stream);
/* ---- higher-order fixed-grid solvers: what odeint(method="midpoint" | "rk4") runs between model evaluations
 * (transport/integrators.py:119).  Added WITHOUT a change of VC_ABI_VERSION: a binding detects these entry points (vc_solver_evals,
 * vc_ode_stage, vc_flux_sample_ode, vc_flux_sample_begin_ode) by SYMBOL - look up vc_solver_evals - not by version.
 * The step functions are torchdiffeq 0.2.x's fixed-grid solvers as recalled, unpinned against real torchdiffeq (the package was not
 * available to check against; the same holds for the Euler rule).  With f(t, y) = -model(y || cond, 1 - t), dt = t1 - t0:
 *   midpoint (2 evaluations)   y_mid = y0 + f0 * half_dt,  half_dt = 0.5 * dt;   y1 = y0 + dt * f(t0 + half_dt, y_mid)
 *   rk4      (4, 3/8 rule)     k1 = f(t0, y0);  k2 = f(t0 + dt * (1/3), y0 + dt * k1 * (1/3));
 *                              k3 = f(t0 + dt * (2/3), y0 + dt * (k2 - k1 * (1/3)));  k4 = f(t1, y0 + dt * (k1 - k2 + k3));
 *                              y1 = y0 + (k1 + 3 * (k2 + k3) + k4) * dt * 0.125
 * evaluated left to right with torch's roundings: every intermediate of the bf16 velocities is a bf16 tensor, a bf16 tensor times
 * the 0-dim f32 device tensor dt multiplies by bf16(dt), times a Python float by that float in f32, and the sum with y0 is bf16 for
 * a bf16 state, f32 for an f32 state. */
#define VC_SOLVER_EULER 0
#define VC_SOLVER_MIDPOINT 1
#define VC_SOLVER_RK4 2
/* model evaluations per solver step: 1, 2, 4; VC_ERR_ARG for anything else.  Works without a GPU. */
int vc_solver_evals(int method);
/* One stage combination on n elements, method VC_SOLVER_MIDPOINT or VC_SOLVER_RK4.  v: the model's bf16 output of this stage's
 * evaluation (the drift is -v).  stage >= 0: that stage; stage < 0: (*eval_ptr) % evals - the device-side evaluation counter, so
 * one captured launch serves every stage.  dt = dts[(*eval_ptr) / evals] (eval_ptr NULL: dts[0]).  y: the state y0, bf16
 * (state_is_bf16) or F32, read by every stage and replaced by y1 by the LAST one only.  k: bf16 [3][n], receives k1..k3 from rk4's
 * stages 0..2 and is read by its later stages (midpoint: unused, may be NULL).  y_in: bf16 [n], the NEXT evaluation's input state
 * - the stage state, or after the last stage bf16(y1), what img_in reads under autocast.  y, v, k, y_in must not overlap.
 * 16-byte accesses need n % 8 == 0 and 16-byte aligned bases; anything else runs element-wise with the same results. */
int vc_ode_stage(int32_t method, int32_t stage, void* y, int32_t state_is_bf16, const void* v, void* k, void* y_in,
                 const float* dts, const int32_t* eval_ptr, int64_t n, void* stream);
/* ---- the adaptive Dormand-Prince 5(4) solve: what an error-controlled odeint runs between model evaluations.  Added WITHOUT a
 * change of VC_ABI_VERSION: detect these entry points (vc_dopri5_stage, vc_dopri5_error_ratio, vc_dopri5_interp,
 * vc_flux_sample_dopri5, vc_flux_dopri5_log) by SYMBOL - look up vc_dopri5_stage.  VC_SOLVER_* has no code for it and
 * vc_solver_evals / vc_flux_sample_ode keep refusing anything but the fixed-grid methods.
 * With f(t, y) = -model(bf16(y) || cond, 1 - f32(t)): every k is stored in bf16 (the model's output dtype), the state y is F32.  The
 * tableau is SciPy's RK45.C / .A / .B / .E and torchdiffeq's DPS_C_MID (written out in csrc/rk_embedded.hip), each coefficient a double
 * rounded once to f32; every sum runs left to right over the non-zero coefficients, one f32 operation after the other, no fused
 * multiply-add, so a torch f32 expression of the same shape gives the same bits (transport.dopri5_integrate is that expression).
 * The controller is torchdiffeq's as recalled, unpinned against real torchdiffeq (the package was not available to check against); it is
 * pinned to SciPy in the tableau and in single steps only.
 * stage: k [7][n] bf16; stage s = 0..6 stores k[s] = -v (v NULL: k[s] is in place already - k1 of a step is the last step's k7,
 *        first same as last) and forms, for s <= 4, y_s = y0 + dt * (a_{s+2,1} k1 + .. + a_{s+2,s+1} k_{s+1}), the state of the NEXT
 *        evaluation; s = 5 forms y1 = y0 + dt * (b1 k1 + .. + b6 k6); s = 6 only stores k7 = f(t1, y1).  stage 7 (v NULL) forms the
 *        probe state y0 + dt * k1 of the initial step size.  stage < 0: *eval_ptr, the device-side evaluation counter, so one
 *        captured launch serves every stage (a counter outside 0..7 writes nothing).  dt = *dt_ptr (device).  The formed state goes
 *        to y_stage (F32) and, rounded, to y_in (bf16, what img_in reads); either may be NULL.  Buffers must not overlap.
 * error_ratio: out[0] = sqrt(mean(q^2)) over ALL n elements, summed in f32 in a fixed order (two-pass block reduction, no atomics:
 *        repeated runs give the same bits).  scratch: VC_DOPRI5_MAX_BLOCKS F32 of device memory.
 *        mode 0: q = dt * (e1 k1 + .. + e7 k7) / (atol + rtol * max(|y0|, |y1|)), the error ratio of a step;
 *        mode 1, 2, 3: q = a / (atol + rtol * |y0|) with a = y0, k1, k2 - k1 - the norms d0, d1 and h0 * d2 of the initial step size.
 * interp: the dense output at theta in [0, 1] of the step t0 -> t0 + dt, the quartic through (y0, f0 = k1, y_mid, y1, f1 = k7) with
 *        y_mid = y0 + dt * (DPS_C_MID . k), evaluated as torchdiffeq's _interp_fit / _interp_evaluate; theta = 0 and theta = 1 return
 *        y0 and y1 themselves.  out: n values, bf16 (out_is_bf16, rounded once) or F32. */
#define VC_DOPRI5_MAX_BLOCKS 256
int vc_dopri5_stage(int32_t stage, const float* y0, void* k, const void* v, const float* dt_ptr, const int32_t* eval_ptr, float* y_stage,
                    void* y_in, int64_t n, void* stream);
int vc_dopri5_error_ratio(int32_t mode, const float* y0, const float* y1, const void* k, const float* dt_ptr, float rtol, float atol,
                          float* out, float* scratch, int64_t n, void* stream);
int vc_dopri5_interp(const float* y0, const float* y1, const void* k, const float* dt_ptr, float theta, void* out, int32_t out_is_bf16,
                     int64_t n, void* stream);
/* ---- embedded Runge-Kutta pairs, tableau-driven: the three kernels above with the method as an argument, and the cheaper pairs an
 * error-controlled odeint offers beside Dormand-Prince.  Added WITHOUT a change of VC_ABI_VERSION: detect these entry points
 * (vc_rk_evals, vc_rk_stage, vc_rk_error_ratio, vc_rk_interp, vc_flux_sample_rk, vc_flux_rk_log) by SYMBOL - look up vc_rk_stage.
 * VC_SOLVER_* has no code for them and vc_solver_evals / vc_flux_sample_ode keep refusing anything but the fixed-grid methods.
 * The contract is the Dormand-Prince group's: f(t, y) = -model(bf16(y) || cond, 1 - f32(t)), every k bf16, the state F32, every
 * coefficient a double rounded once to f32, every sum left to right over the non-zero coefficients, one f32 operation after the
 * other, no fused multiply-add (transport.rk_step / rk_error_ratio / rk_hermite are the same expressions in torch: the same bits).
 * A method of S stages evaluates k1..kS per step; kS = f(t1, y1) is the next step's k1 (first same as last), so an attempt costs
 * S - 1 model evaluations:
 *   VC_RK_DOPRI5         S = 7, order 5: exactly the tableau of vc_dopri5_stage.  Taken by vc_rk_stage and vc_rk_error_ratio ONLY,
 *                        where it returns the bits of vc_dopri5_stage / vc_dopri5_error_ratio: it holds the generic code to the
 *                        pinned one.  vc_rk_interp and vc_flux_sample_rk refuse it (VC_ERR_ARG): use the vc_dopri5 entry points.
 *   VC_RK_BOSH3          Bogacki-Shampine 3(2), S = 4, order 3 (SciPy's RK23.C / .A / .B / .E):
 *                        c 0, 1/2, 3/4, 1;  a2 1/2;  a3 0, 3/4;  a4 = b 2/9, 1/3, 4/9;  e 5/72, -1/12, -1/9, 1/8
 *   VC_RK_ADAPTIVE_HEUN  Heun-Euler 2(1), S = 3, order 2:
 *                        c 0, 1, 1;  a2 1;  a3 = b 1/2, 1/2;  e 1/2, -1/2, 0
 * The tableaus are pinned to SciPy (bosh3) and to the closed form (adaptive_heun) in single steps; the controller around them is
 * torchdiffeq's as recalled, unpinned against real torchdiffeq.
 * evals: *start = 2 (k1 and the probe of the first step size), *per_attempt = S - 1, *order; any may be NULL.  Works without a GPU.
 * stage: as vc_dopri5_stage with k [S][n] (a [7][n] buffer serves every method): stage s <= S - 3 forms y0 + dt * (a row s + 2),
 *        s = S - 2 forms y1 = y0 + dt * (b . k), s = S - 1 only stores kS; stage 7 (v NULL) forms the probe state y0 + dt * k1;
 *        stage < 0: *eval_ptr (a counter outside 0..S-1 and 7 reads and writes nothing).
 * error_ratio: as vc_dopri5_error_ratio - the same four modes, the same fixed summation order - with the method's e row in mode 0.
 * interp: VC_RK_BOSH3 / VC_RK_ADAPTIVE_HEUN: the Hermite cubic through (y0, f0 = k1, y1, f1 = kS),
 *          y(x) = (1-x) y0 + x y1 + x (x-1) ((1-2x)(y1-y0) + (x-1) dt f0 + x dt f1),  evaluated in f32 as
 *          c0 = 1 - x; c1 = x - 1; c2 = 1 - 2 x; w = x c1; h0 = c1 dt; h1 = x dt;  y = (c0 y0 + x y1) + w ((c2 (y1 - y0) + h0 f0) + h1 f1)
 *        theta = 0 and theta = 1 return y0 and y1 themselves.  For bosh3 this IS SciPy's RK23 dense output (its P rows are this cubic
 *        expanded).
 * stage and interp move 16 bytes per access where n % 8 == 0 and the bases are 16-byte aligned; anything else runs element-wise
 * with the same results. */
#define VC_RK_DOPRI5 0
#define VC_RK_BOSH3 1
#define VC_RK_ADAPTIVE_HEUN 2
int vc_rk_evals(int32_t method, int32_t* start, int32_t* per_attempt, int32_t* order);
int vc_rk_stage(int32_t method, int32_t stage, const float* y0, void* k, const void* v, const float* dt_ptr, const int32_t* eval_ptr,
                float* y_stage, void* y_in, int64_t n, void* stream);
int vc_rk_error_ratio(int32_t method, int32_t mode, const float* y0, const float* y1, const void* k, const float* dt_ptr, float rtol,
                      float atol, float* out, float* scratch, int64_t n, void* stream);
int vc_rk_interp(int32_t method, const float* y0, const float* y1, const void* k, const float* dt_ptr, float theta, void* out,
                 int32_t out_is_bf16, int64_t n, void* stream);
/* ---- the stochastic (SDE) sampler: what the reference's Sampler.sample_sde runs between model evaluations (transport.py:300-359,
 * the step rules of the class sde, integrators.py:27-49, and the score / diffusion forms of ICPlan in transport/path.py).  Added
 * WITHOUT a change of VC_ABI_VERSION: detect these entry points (vc_sde_plan, vc_sde_stage, vc_flux_sample_sde) by SYMBOL - look up
 * vc_sde_stage.  VC_SOLVER_* has no code for it and vc_solver_evals / vc_flux_sample_ode keep refusing anything but the
 * fixed-grid methods.
 * The reference adapted only sample_ode to Flux's reversed time (transport.py:384); its sample_sde cannot drive Flux.forward as
 * written.  What is taken from it is the mathematics, applied to the velocity v(x, t) = -model(x || cond, timesteps = 1 - t).
 * Time runs as in sample_ode (t = 0 noise, t = 1 data; Linear path: alpha = t, sigma = 1 - t).  With w(t) the diffusion coefficient:
 *   score       s = (t v - x) / (1 - t)
 *   sde drift   D(x, t) = v + w s = A(t) v - Bc(t) x,   A = 1 + w t / (1 - t),  Bc = w / (1 - t)
 *   w(t)        "constant" norm | "SBDM" norm (1 - t) / t | "sigma" norm (1 - t) | "linear" norm (1 - t)
 *               "decreasing" 0.25 (norm cos(pi t) + 1)^2 | "inccreasing-decreasing" norm sin^2(pi t)   (the reference's spelling;
 *               "increasing-decreasing" is accepted as an alias)
 *   "Euler"     Euler-Maruyama: x' = x + dt D(x, t) + g z,  g = sqrt(2 w(t) dt),  z ~ N(0, 1)
 *   "Heun"      xh = x + g z;  K1 = D(xh, t);  xp = xh + dt K1;  K2 = D(xp, t + dt);  x' = xh + (0.5 dt) (K1 + K2)
 *   last step   at t1 = the last grid point: "Mean" x + lss D(x, t1) | "Euler" x + lss v | "Tweedie" x + (1 - t1) v | none: x
 * Every update is y + h (A v - Bc y) + g z with scalar coefficients.  The HOST RULE (plan) computes them in double from the F32
 * grid - t = t_grid[i], dt = f32(t_grid[i + 1] - t_grid[i]), t + dt the double sum - and rounds each ONCE to F32.
 * plan: host only, needs no device.  method "Euler" | "Heun"; form as above; last_step "Mean" | "Euler" | "Tweedie", or NULL / "" for
 *        none.  Evaluations: Euler (n_points - 1) + (last step ? 1 : 0), Heun 2 (n_points - 1) + (last step ? 1 : 0); draws:
 *        n_points - 1.  rows receives *n_evals rows of VC_SDE_ROW F32 (mode, h, A, Bc, g), one per evaluation, and for Heun ONE more
 *        row behind them, the injection of draw 0 in front of the first evaluation; times receives the model's time 1 - f32(t) of
 *        every evaluation.  rows / times may be NULL (the counts alone); capacity: the rows `rows` holds, the values `times` holds.
 *        VC_ERR_ARG with a message: an unknown method / form / last step, n_points < 2, a grid that does not increase strictly, a
 *        capacity that is too small, and ANY NON-FINITE COEFFICIENT - the message names the time and the form.  That covers "SBDM"
 *        at t = 0 and any row at t = 1, hence "Heun" without a last step on a grid that ends at 1: a refusal, never a NaN latent.
 *        "constant" is implemented (in the reference it raises a TypeError, a bug).
 * stage: one elementwise pass over n elements.  Row e = eval (>= 0), or *eval_ptr - the device-side evaluation counter, so one
 *        captured launch serves every evaluation; a row outside [0, n_rows), an unknown mode, or a mode whose buffers are NULL
 *        writes nothing.  y, xhat, k1: F32 [n]; v: the model's bf16 output (the velocity is -v); y_in: bf16 [n], the NEXT evaluation's
 *        input.  With D = A (-v) - Bc (.):
 *          VC_SDE_EM      y <- (y + h D(y)) + g z_d,  d = e;                       y_in <- bf16(y)
 *          VC_SDE_HEUN1   k1 <- D(xhat);  y <- xhat + h k1  (= xp);                y_in <- bf16(y)
 *          VC_SDE_HEUN2   y <- xhat + h (k1 + D(y))  (= x');  xhat <- y + g z_d,  d = (e + 1) / 2  (the NEXT step's noise);
 *                         y_in <- bf16(xhat)
 *          VC_SDE_LAST    y <- y + h D(y);                                         y_in <- bf16(y)
 *          VC_SDE_INJECT  xhat <- y + g z_0;  (v unused, may be NULL)              y_in <- bf16(xhat)
 *        g == 0 adds NO noise term (not even a signed zero).  F32 arithmetic, left to right, one operation after the other, no fused
 *        multiply-add: a torch F32 expression of the same shape gives the same bits (transport.sde_integrate is that expression).
 *        NOISE: z_d[i] is the VC_RNG_F32 value of the stream of `seed` at position offset + d * n + i, bit for bit what a
 *        vc_randn call gives there - generated in the kernel, no noise tensor exists.  seed = rng[0], offset = rng[1]: TWO UINT64
 *        IN DEVICE MEMORY, read when the kernel runs, so a captured launch serves every seed and every replay draws fresh,
 *        reproducible noise.  The caller keeps offset + (draws) * n inside the 64-bit stream.  Buffers must not overlap.  16-byte
 *        accesses where every base is 16-byte aligned (8 elements per work item, the n % 8 tail element-wise); anything else
 *        runs element-wise with the same results.  Grid capped, grid-stride loop. */
#define VC_SDE_EM 0
#define VC_SDE_HEUN1 1
#define VC_SDE_HEUN2 2
#define VC_SDE_LAST 3
#define VC_SDE_INJECT 4
#define VC_SDE_ROW 5   /* F32 values per table row: mode, h, A, Bc, g */
int vc_sde_plan(const char* method, const char* form, double norm, const char* last_step, double last_step_size, const float* t_grid,
                int32_t n_points, float* rows, float* times, int32_t capacity, int32_t* n_evals, int32_t* n_draws);
int vc_sde_stage(int32_t eval, const float* table, int32_t n_rows, float* y, const void* v, void* y_in, float* xhat, float* k1,
                 const uint64_t* rng, const int32_t* eval_ptr, int64_t n, void* stream);
/* ---- the Adams-Bashforth multistep solver: a fixed-grid, VARIABLE-STEP rule of order 1..4 that costs exactly ONE model evaluation
 * per step - it reuses the velocities of the steps before.  The reference's sample_ode advertises torchdiffeq's Adams methods and
 * ships none that run; the rule below is the textbook one, stated in full.  Added WITHOUT a change of VC_ABI_VERSION: detect these
 * entry points (vc_ms_plan, vc_ms_stage, vc_flux_sample_multistep, vc_flux_plan_count) by SYMBOL - look up vc_ms_plan.  VC_SOLVER_*
 * has no code for it and vc_solver_evals / vc_flux_sample_ode keep refusing anything but the fixed-grid methods.
 * Time runs as in sample_ode (t = 0 noise, t = 1 data); the drift is f(t, y) = -model(bf16(y) || cond, 1 - f32(t)).
 * For step i (0-based) from t_i to t_{i+1} the order used is k_i = min(order, i + 1) - the usual low-order start, no extra
 * evaluations -, the nodes are tau_j = t_{i-j}, j = 0 .. k_i - 1, and
 *   c_{i,j} = INT_{t_i}^{t_{i+1}} PROD_{m != j} (tau - tau_m) / (tau_j - tau_m) dtau
 * computed on the HOST in double from the F32 grid values, widened, and rounded ONCE to F32; unused coefficients are exactly 0.0f.
 * Each coefficient contains the step length: SUM_j c_{i,j} = t_{i+1} - t_i.  The update is
 *   y <- y + (((c_{i,0} f_i) + c_{i,1} f_{i-1}) + c_{i,2} f_{i-2}) + c_{i,3} f_{i-3}
 * in F32, left to right, one operation after the other, no fused multiply-add - that is, as a compiler reads the line:
 * z = c0 f_i;  z = z + c1 f_{i-1};  z = z + c2 f_{i-2};  y = y + z;  y = y + c3 f_{i-3}.  A torch F32 expression of the same shape
 * gives the same bits (transport.multistep_integrate is that expression).  A coefficient c_{i,j}, j >= 1, that is exactly zero adds
 * NO term and its velocity is NOT READ (the c_{i,0} term is always there: f_i is what the model has just written).
 * Order 1 is Euler's rule with F32 roundings - not bit-equal to vc_euler_step_f32, which multiplies by bf16(dt).  Orders 3 and 4
 * have small stability regions; nothing here recommends an order.
 * plan:  host only, needs no device.  rows receives n_points - 1 rows of VC_MS_ROW F32 (c_{i,0..3}), times the model's time
 *        1 - f32(t_i) of every evaluation; both may be NULL (the count alone); capacity: the rows `rows` holds, the values `times`
 *        holds; *n_evals = n_points - 1.  VC_ERR_ARG with a message: an order outside 1..4, n_points < 2, a grid that does not increase
 *        strictly, a capacity that is too small, ANY NON-FINITE COEFFICIENT.
 * stage: one elementwise pass over n elements.  Row e = eval (>= 0), or *eval_ptr - the device-side evaluation counter, so one
 *        captured launch serves every step and every order; a row outside [0, n_rows) writes nothing.  y: F32 [n]; v: the model's
 *        bf16 output v_e (f_e = -v_e); hist: bf16 [VC_MS_HIST][n], a RING of past outputs as the model wrote them - v_{e-j} lives in
 *        slot (e - j) mod VC_MS_HIST; y_in: bf16 [n] <- bf16(y), the NEXT evaluation's input.  After the sum, v_e is stored into slot
 *        e mod VC_MS_HIST: the element it overwrites, v_{e-3}, is the one the same work item has just read.  During the start the
 *        slots hold whatever the buffer held: they are not read, and 0 * NaN never reaches the state.  Buffers must not overlap.
 *        16-byte accesses where n % 8 == 0 (the ring's planes start n elements apart) and every base is 16-byte aligned, 8
 *        elements per work item; anything else runs element-wise with the same results.  Grid capped, grid-stride loop; no LDS,
 *        no atomics. */
#define VC_MS_ROW 4    /* F32 values per table row: c_{i,0} .. c_{i,3}; also the highest order */
#define VC_MS_HIST 3   /* planes of the ring of past model outputs */
int vc_ms_plan(int32_t order, const float* t_grid, int32_t n_points, float* rows, float* times, int32_t capacity, int32_t* n_evals);
int vc_ms_stage(int32_t eval, const float* table, int32_t n_rows, float* y, const void* v, void* hist, void* y_in, const int32_t* eval_ptr,
                int64_t n, void* stream);
/* ---- the three elementwise passes of the first-block step cache (vc_flux_set_step_cache below; the rule is this library's own,
 * DESIGN.md section 4).  Added without a change of VC_ABI_VERSION, like the solver entry points: detect by SYMBOL (look up
 * vc_flux_set_step_cache).  bf16 storage, f32 math, 16-byte accesses: n, every sample stride a multiple of 8, bases 16-byte aligned
 * (VC_ERR_ARG otherwise).
 * residual_change: h0, h1, p [B][n] bf16 -> r [B][n] = bf16(f32(h1) - f32(h0)); sums [B][2] F32 = per sample
 *                  (sum |f32(r) - f32(p)|, sum |f32(p)|), summed in f32 in a fixed order (two-pass block reduction, no atomics:
 *                  repeated runs give the same bits); metric [1] F32 = max over the samples of sums[b][0] / sums[b][1], NaN as soon as
 *                  one ratio is.  sums or metric may be NULL.  scratch: B * 2 * VC_RESIDUAL_CHANGE_MAX_BLOCKS F32 of device memory.
 *                  r must not overlap h0, h1, p.
 * residual_sub / residual_add: out[b][i] = bf16(f32(a[b][i]) -/+ f32(b[b][i])), i < n, sample b of each operand starting
 *                  b * its stride (elements) after the base: rows of a strided stream (the image rows of the joint stream). */
#define VC_RESIDUAL_CHANGE_MAX_BLOCKS 256
int vc_residual_change(const void* h0, const void* h1, const void* p, void* r, float* sums, float* metric, float* scratch, int32_t B,
                       int64_t n, void* stream);
int vc_residual_sub(const void* a, int64_t a_bstride, const void* b, int64_t b_bstride, void* out, int64_t out_bstride, int32_t B,
                    int64_t n, void* stream);
int vc_residual_add(const void* a, int64_t a_bstride, const void* b, int64_t b_bstride, void* out, int64_t out_bstride, int32_t B,
                    int64_t n, void* stream);
/* ---- the numerics monitor's reduction: per sample of a strided tensor, how many elements are NaN / +-inf and how large the rest
 * is.  The reference has nothing like it.  Added WITHOUT a change of VC_ABI_VERSION (tests pin 11): detect by SYMBOL (look up
 * vc_tensor_stats); vc_monitor_struct_sizes reports sizeof(VcStat).
 * x: B samples of rows x cols elements, bf16 or F32 (x_is_f32); element (b, r, c) lies b * bstride + r * ld + c elements behind x - the
 * image rows, the text rows or all rows of a strided joint stream.  Per sample b:
 *   nonfinite  the number of NaN / +-inf elements (exact)           count    the number of elements examined, rows * cols (exact)
 *   max_abs    max |x| over the FINITE elements (exact; 0 without)  sum_sq   sum x^2 over the finite elements, in f32, in a fixed order
 * The order of sum_sq: a row is cut into UNITS of E consecutive elements (E = 8 for bf16, 4 for F32; the last unit of a row is shorter
 * where cols % E != 0); the sample's units, numbered row by row, are dealt round-robin to the nblk * 256 threads of its
 * nblk = min(ceil(units / 256), VC_MONITOR_MAX_BLOCKS) blocks (thread t of block k: units k * 256 + t, + nblk * 256, ...).  A thread
 * adds its elements in ascending order, s = s + x * x, the product rounded to f32 on its own (no fused multiply-add); the block's 256
 * sums go through a tree (l[t] += l[t + o], o = 128, 64, .., 1) and the sample's nblk block sums through the same tree (thread t holds
 * block t's, 0 for t >= nblk).  A two-pass block reduction without atomics, as vc_dopri5_error_ratio and vc_residual_change: repeated
 * runs give the same bits.  A unit is ONE 16-byte load where cols, ld, bstride are multiples of E and x is 16-byte aligned, E
 * element loads otherwise: the choice is made on the host and gives the same bits.
 * out: the VcStat of sample b goes to out[row * out_stride + b], row = *row_ptr - a device-side counter, read when the kernel runs,
 * so ONE captured launch serves every evaluation of a trajectory - or 0 with row_ptr NULL; a row outside [0, capacity) writes
 * NOTHING.  scratch: B * 4 * VC_MONITOR_MAX_BLOCKS F32 of device memory.  VC_ERR_ARG before the device is touched: a null x / out /
 * scratch; B, rows, cols or capacity <= 0; B > 65535; bstride < 0; ld < cols; out_stride < B; an out that is not 16-byte aligned; an x
 * or a scratch that is not aligned to its elements (2 bytes for bf16, 4 for F32); rows * cols >= 2^32 or more than 2^31 - 1 units. */
typedef struct VcStat { float max_abs; float sum_sq; uint32_t nonfinite; uint32_t count; } VcStat;   /* 16 bytes */
#define VC_MONITOR_MAX_BLOCKS 256
void vc_monitor_struct_sizes(int32_t out[1]);
int vc_tensor_stats(const void* x, int32_t x_is_f32, int64_t bstride, int64_t ld, int32_t B, int64_t rows, int32_t cols, VcStat* out,
                    int64_t out_stride, const int32_t* row_ptr, int32_t capacity, float* scratch, void* stream);
/* ---- the flow-matching loss of ONE model evaluation, forward only: Transport.training_losses (transport.py:132-176) on
 * Transport.sample (transport.py:98-130) for the Linear path (alpha = t, sigma = 1 - t) and velocity prediction - the objective a
 * VisualCloze LoRA is trained on, as a validation loss.  No backward pass exists.  Added WITHOUT a change of VC_ABI_VERSION (tests
 * pin 11): detect by SYMBOL (look up vc_fm_plan).  Every argument is checked before the device is touched.
 * vc_fm_plan: the path sample.  x1: B samples of rows x cols elements, bf16 or F32 (x1_is_f32); element (b, r, c) lies
 *   b * x1_bstride + r * x1_ld + c elements behind x1.  t: DEVICE F32 [B].  x0: a dense [B, rows, cols] tensor of x1's dtype, or
 *   NULL: element i (the flat index (b * rows + r) * cols + c) is then drawn IN the kernel - the VC_RNG_F32 value of THE STREAM of
 *   `seed` at position offset + i, rounded to bf16 for a bf16 x1 (the VC_RNG_BF16 value): what a vc_randn call of x1's dtype gives
 *   there, with no draw launch and no stored x0 (seed and offset are unused with a tensor).  In F32, one operation after the other,
 *   no fused multiply-add, with x1 and x0 converted to F32:
 *       xt[(b * rows + r) * xt_ld + c] = bf16( t[b] * x1 + (1 - t[b]) * x0 )      rounded ONCE; columns >= cols of xt are not touched
 *       ut[(b * rows + r) * cols + c]  = x1 - x0                                   F32, dense
 *   - the torch F32 expression of the same shape gives the same bits.  xt is the model-input row (xt_ld = in_channels): the cond
 *   columns beside x_t are the caller's, the concat costs no pass.  16-byte accesses where cols, x1_ld, x1_bstride, xt_ld are
 *   multiples of 8 (4 for the strides of an F32 x1) and x1, x0, xt, ut are 16-byte aligned; anything else runs element-wise: the
 *   choice is made on the host and gives the same bits.  Grid capped, grid-stride loop.  Buffers must not overlap.
 *   VC_ERR_ARG: a null x1 / t / xt / ut; B, rows or cols <= 0; x1_bstride < 0; x1_ld or xt_ld < cols; a buffer that is not aligned to
 *   its elements; B * rows * cols beyond a 64-bit byte offset; with x0 NULL, offset + B * rows * cols - 1 past 2^64 - 1.
 * vc_fm_loss: the masked squared error.  out: the model's bf16 output, element (b, r, c) at (b * rows + r) * out_ld + c; ut: as
 *   vc_fm_plan left it.  valid_rows: per sample the number of VALID rows, a prefix of its rows (the handle's valid-first row
 *   order) - int32 [B] in device memory (valid_on_host 0; clamped to [0, rows] by the kernel; 0 gives NaN), or on the host
 *   (valid_on_host != 0; at most VC_FM_MAX_HOST_COUNTS samples, the counts travel as kernel arguments), or NULL = every row.
 *       loss[b] = ( sum over r < valid_rows[b], c < cols of ((-out) - ut)^2 ) / F32(valid_rows[b] * cols)            F32 [B], device
 *   The order of the sum is vc_tensor_stats' above, with units of 8 elements: a row is cut into units of 8 consecutive elements
 *   (the last one shorter where cols % 8 != 0); the units of the sample's valid rows, numbered row by row, are dealt round-robin to
 *   the nblk * 256 threads of nblk = min(ceil(rows * ceil(cols / 8) / 256), VC_FM_LOSS_MAX_BLOCKS) blocks - nblk from ALL rows, the
 *   same for every sample - thread t of block k taking units k * 256 + t, + nblk * 256, ...  A thread adds its elements in ascending
 *   order, d = (-out) - ut, s = s + d * d, the product rounded on its own; the block's 256 sums go through a tree (l[t] += l[t + o],
 *   o = 128, 64, .., 1), the nblk block sums through the same tree (thread t holds block t's, 0 for t >= nblk); one F32 division.
 *   No atomics: repeated runs give the same bits.  An inf in `out` gives inf.  A unit is one 16-byte load of out and two of ut where
 *   cols and out_ld are multiples of 8 and out, ut are 16-byte aligned, element loads otherwise, with the same bits.
 *   scratch: B * VC_FM_LOSS_MAX_BLOCKS F32 of device memory.  VC_ERR_ARG: a null out / ut / loss / scratch; B, rows or cols <= 0;
 *   B > 65535; out_ld < cols; a buffer that is not aligned to its elements; more than 2^31 - 1 units per sample; with host counts
 *   B > VC_FM_MAX_HOST_COUNTS or a count outside [1, rows] - a sample without a valid row has no loss.
 * vc_fm_times: HOST only.  The training times Transport.sample draws (transport.py:107-129), from the caller's n base draws: F32
 *   uniforms in [0, 1) for snr_type "uniform" and "uniform_<t0>_<t1>", F32 standard normals for "lognorm"; anything else - and a
 *   "uniform_..." that is not two finite plain decimal numbers - is VC_ERR_ARG, as the reference raises.  check_interval
 *   (transport.py:70-96) gives (0, 1) for Linear + velocity.  In torch's F32 operations, nothing contracted:
 *       uniform   t = u * F32(t1 - t0) + F32(t0)                  (t1 - t0 in double)
 *       lognorm   t = (1 / (1 + e)) * 1 + 0,  e = F32(exp(-u)) with the exponential taken in double: the correctly rounded F32
 *                 exponential (torch's own vectorised F32 exp is within an ulp of it)
 *   then, with do_shift, step 3 of vc_time_grid below with n_tokens = x1.shape[1] (time_shift of transport.py:123-127).  out: HOST
 *   F32 [n], bit for bit transport.fm_times.  VC_ERR_ARG also: a null pointer, n <= 0, n_tokens < 1. */
#define VC_FM_LOSS_MAX_BLOCKS 256
#define VC_FM_MAX_HOST_COUNTS 64
int vc_fm_plan(const void* x1, int32_t x1_is_f32, int64_t x1_bstride, int64_t x1_ld, const float* t, const void* x0, uint64_t seed,
               uint64_t offset, void* xt, int64_t xt_ld, float* ut, int32_t B, int64_t rows, int32_t cols, void* stream);
int vc_fm_loss(const void* out, int64_t out_ld, const float* ut, const int32_t* valid_rows, int32_t valid_on_host, float* loss,
               float* scratch, int32_t B, int64_t rows, int32_t cols, void* stream);
int vc_fm_times(const char* snr_type, const float* base, int32_t n, int32_t n_tokens, int32_t do_shift, float* out);
/* ---- true classifier-free guidance: the combine of Flux.forward_with_cfg (models/model.py:126-145), which runs forward on a batch
 * whose first half is the conditional and whose second half the unconditional samples and returns
 * cat([uncond_v + cfg_scale * (cond_v - uncond_v), uncond_v]).  Added without a change of VC_ABI_VERSION: detect by SYMBOL (look up
 * vc_flux_set_cfg).  cond, uncond, out: n bf16 values each; with torch's roundings for bf16 tensors and a Python float, operation by
 * operation,
 *     out[i] = bf16( uncond[i] + bf16( f32(cfg_scale) * bf16( cond[i] - uncond[i] ) ) )
 * every operation evaluated in f32 and rounded to bf16 (nearest even); cfg_scale is taken as f32 and NOT rounded to bf16; no fused
 * multiply-add.  cfg_scale = 1 is therefore not the identity (cond - uncond is rounded).  out may BE cond or uncond exactly (each
 * element is read before it is written); any other overlap of out with an input is VC_ERR_ARG, as are a null pointer, n <= 0 and a
 * non-finite cfg_scale - all checked before the device is touched.  16-byte accesses need n % 8 == 0 and 16-byte aligned bases;
 * anything else runs element-wise with the same results.  Flux.forward_with_cfg for a C caller = vc_flux_forward, then
 * vc_cfg_combine(out, out + n, out, n, cfg_scale) with n = (B / 2) * N * out_channels. */
int vc_cfg_combine(const void* cond, const void* uncond, void* out, int64_t n, float cfg_scale, void* stream);
/* SDEdit start state x0 = noise*(1-s) + latent*s with the reference's bf16 roundings (visualcloze.py:221).  strength is the
 * reference's Python float, a double: the noise factor is f32(1.0 - s) with the subtraction in double, the latent factor
 * f32(s) - the two f32 scalars torch multiplies the bf16 tensors by. */
int vc_sdedit_mix(const void* noise, const void* latent, double strength, void* out, int64_t n, void* stream);

/* ---- latent-grid packer / unpacker (the steps either side of the loop) ----
 * pack:   latent [C,h,w] bf16 -> tokens[(h/2)(w/2)][col0 .. col0+4C) of rows with stride ld
 *         ("c (h ph) (w pw) -> (h w) (c ph pw)", models/sampling.py:61, visualcloze.py:208-209,385-386)
 * mask:   pixel mask [H,W] bf16 -> [(H/16)(W/16)][col0 .. col0+256)  (8x8 unshuffle + 2x2 pack, visualcloze.py:381-382)
 * unpack: the inverse of pack (visualcloze.py:237,428)
 * ld and col0 are multiples of 8 and the token base is 16-byte aligned (16-byte accesses on the token side; the latent is read
 * and written in 4-byte words, the mask in 16-byte vectors); anything else is VC_ERR_ARG. */
int vc_pack_latent(const void* latent, void* tokens, int32_t C, int32_t h, int32_t w, int64_t ld, int32_t col0, void* stream);
int vc_pack_mask(const void* mask, void* tokens, int32_t H, int32_t W, int64_t ld, int32_t col0, void* stream);
int vc_unpack_latent(const void* tokens, int64_t ld, int32_t col0, void* latent, int32_t C, int32_t h, int32_t w, void* stream);

/* ---- noise source: a counter-based Gaussian stream of this library's own (csrc/rng.hip) ----
 * The reference draws its noise with torch.randn(generator=...) (visualcloze.py:217,394-399) and torch.randn_like (autoencoder.py:272);
 * torch's device stream depends on the grid torch picks from the device's properties and on how a run is split into draws.
 * This stream does not: every element depends on (seed, position) ONLY - not on the launch geometry, not on how a draw is
 * split into calls, not on the memory layout it is written in.  It is the DEFAULT stream of the C entry points and differs from
 * torch's: a seed here does not reproduce the images torch's generator gives for the same seed.  torch's stream is the opt-in
 * second source below (vc_randn_torch, THE TORCH STREAM; vc_grid_set_noise).  Added WITHOUT a change of VC_ABI_VERSION (tests pin
 * 11): detect these entry points by SYMBOL - look up vc_randn.
 *
 * THE STREAM (the contract).  Element at stream position p = offset + i, offset a uint64, offset + n does not wrap:
 *   block    b = p >> 2
 *   counter  (lo32(b), hi32(b), 0, 0)
 *   key      (lo32(seed), hi32(seed))
 * Philox4x32-10: multipliers M0 = 0xD2511F53, M1 = 0xCD9E8D57, Weyl increments W = (0x9E3779B9, 0xBB67AE85), ten rounds, giving
 * x0..x3.  One round is
 *   c <- (hi(M1*c2)^c1^k0, lo(M1*c2), hi(M0*c0)^c3^k1, lo(M0*c0))
 * followed by k += W.  Known answers (counter | key | output):
 *   00000000 00000000 00000000 00000000 | 00000000 00000000 | 6627e8d5 e169c58d bc57ac4c 9b00dbd8
 *   ffffffff ffffffff ffffffff ffffffff | ffffffff ffffffff | 408f276d 41c83b0e a20bc7c6 6d5451fd
 *   243f6a88 85a308d3 13198a2e 03707344 | a4093822 299f31d0 | d16cfe09 94fdcceb 5001e420 24126ea1
 * Normals: two Box-Muller pairs per block, in f32:
 *   u1 = ((x0 >> 8) + 1) * 2^-24 in (0, 1],  u2 = (x1 >> 8) * 2^-24 in [0, 1)      (both exact in f32)
 *   r = sqrt(-2 ln u1),  z0 = r cos(2 pi u2),  z1 = r sin(2 pi u2);  z2, z3 the same from x2, x3
 * Element p is z[p & 3].  u1 = 1 gives r = 0; the largest possible r is sqrt(48 ln 2) ~ 5.77: no inf or NaN can occur.
 * VC_RNG_U32 words are exact; the normals of a restatement agree with the device's to f32 arithmetic (tests/noise_ref.py,
 * tests/test_noise_gpu.py: within 1/64 bf16 ulp of r of the fp64 value, plus the bf16 store's half ulp). */
#define VC_RNG_BF16 0  /* the f32 normal rounded to nearest-even, as torch.randn(...).to(bf16) rounds */
#define VC_RNG_F32 1
#define VC_RNG_U32 2   /* the raw word x[p & 3] (exact tests) */
/* out[i] = element offset + i of the stream of `seed`, i < n.  Any n >= 1, any offset, any base aligned to the element size (2 / 4
 * / 4 bytes); stores are 16 bytes wide wherever the base and the phase offset & 3 allow, the element-wise head and tail give the
 * same values.  seed and offset are by-value kernel arguments: the call is legal under stream capture, and A REPLAYED GRAPH
 * REPEATS ITS NOISE - a caller who wants fresh noise per replay draws outside the graph (vc_sde_stage, which reads seed and offset
 * from device memory, is the exception built for the sampling loop).  Arguments are checked before the device
 * is touched (VC_ERR_ARG: null pointer, n <= 0, unknown dtype, offset + n wrapping, misaligned base). */
int vc_randn(void* out, int32_t dtype, int64_t n, uint64_t seed, uint64_t offset, void* stream);
/* The sampler's start state x(t0) in one launch, no intermediate tensor: latent element (c, y, x) of a [C, h, w] draw takes stream
 * position offset + (c*h + y)*w + x and is written as bf16 straight into the packed-token layout of vc_pack_latent, under its
 * ld / col0 / alignment rules (even C, h, w; ld and col0 multiples of 8; 16-byte aligned token base).  Bit-identical to a
 * VC_RNG_BF16 draw of C*h*w elements into [C, h, w] followed by vc_pack_latent. */
int vc_randn_tokens(void* tokens, int32_t C, int32_t h, int32_t w, int64_t ld, int32_t col0, uint64_t seed, uint64_t offset, void* stream);

/* ---- noise source, opt-in: torch's device generator stream (csrc/rng_torch.hip) ----
 * What G = torch.Generator(device).manual_seed(seed); torch.randn(n, device=device, generator=G) stores, restated: a seed then gives
 * the images the reference (visualcloze.py:217,394-399) and this package's default path give for it.  The stream is a pure
 * function of six quantities: the seed, the generator's Philox offset, the element count and three integers of the device - torch's
 * block size 256, the multiprocessor count and the threads per multiprocessor.  The library reads the last two from the current
 * device (pass 0) or takes them from the caller, who then needs no GPU to know the geometry (vc_torch_randn_policy) and gets one
 * machine's noise on another.  Added WITHOUT a change of VC_ABI_VERSION (tests pin 11): detect by symbol: look up vc_randn_torch.
 * Parity is with the torch build this library is tested against (2.10 / ROCm 7; ATen/native/hip/DistributionTemplates.h,
 * rocrand_philox4x32_10.h, rocrand_normal.h): another torch may lay its stream out differently, THE CONTRACT BELOW is what this
 * library guarantees.  torch splits a tensor it cannot index in 32 bits into several draws: parity holds for n < 2^31.
 *
 * THE TORCH STREAM (the contract).  A draw of n elements, 1 <= n <= 2^48, at seed s and offset o; o is a multiple of 4 and counts
 * Philox outputs per thread, as torch.Generator.get_offset() reports it.  The grid:
 *   cap = sm_count * (threads_per_sm / 256)   (integer division; 1 <= cap < 2^31)
 *   G   = min(ceil(n / 256), cap)             T = 256 G
 * Element i belongs to thread i mod T, lane (i div T) mod 4, round i div (4 T).  Its Philox4x32-10 block (the rounds, multipliers
 * and known answers of THE STREAM above) has
 *   counter  (lo32(c), hi32(c), lo32(thread), hi32(thread)),  c = o / 4 + round
 *   key      (lo32(s), hi32(s))
 * which is where rocrand_init(seed, subsequence = thread, offset = o) and one rocrand_normal4 per round put them.  With x0..x3 the
 * block's words, in f32:
 *   u = 2^-32 + f32(x0) * 2^-32 in (0, 1],   v = k + f32(x1) * k in (0, 2 pi],  k = f32(2^-32) * f32(2 pi)
 *   r = sqrt(-2 ln u),  z0 = r sin(v),  z1 = r cos(v);  z2, z3 the same from x2, x3       (SINE FIRST; cuRAND's order differs)
 * Element i is z[lane], stored as z + 0 (torch's z * std + mean: a negative zero becomes +0).  The operations, as the kernel torch
 * ships performs them: u and v are ONE fma each; ln u = t + fma(m, L2, fma(m, L1, -t)) with m = log2 u from the hardware (v_log_f32),
 * t = m * L1, L1 = 0x1.62e42ep-1, L2 = 0x1.efa39ep-25 (ln 2 in two words; the two parts ADDED, not fused); -2 * ln u; a correctly
 * rounded sqrt; sin / cos the hardware's fast ones on v / (2 pi) (rocrand's __sincosf: v_sin_f32 / v_cos_f32); one product each.
 * Nothing else is contracted.  VC_RNG_U32 words are exact for any restatement; the normals are bit-equal to torch's on the device
 * (tests/test_torch_noise_gpu.py: 0 differing elements, f32 and bf16, at every tested size and seed), a host restatement agrees
 * to the hardware approximations' error only.
 * After the draw the offset stands at o + ((n - 1) div (4 T) + 1) * 4.  Draws of more than 256 * cap elements depend on the
 * device's two integers (MI355X: 256 and 2048, cap 2048, 524288 elements); the start state of a 1024 x 3456 grid, 221184
 * elements, does not.  VC_RNG_BF16 is the f32 normal rounded to nearest-even, torch.randn(f32).to(bf16) - the only bf16 form promised
 * (torch.randn(dtype=bfloat16) is not restated). */
/* Host only: torch's grid G and the advance of the offset for a draw of n elements.  sm_count / threads_per_sm: the two device
 * integers, each 0 = the current device's - only then is a device needed, VC_ERR_HIP without one.  VC_ERR_ARG: null result
 * pointer, n outside 1 .. 2^48, sm_count < 0, threads_per_sm in 1 .. 255, a cap outside 1 .. 2^31 - 1. */
int vc_torch_randn_policy(int64_t n, int32_t sm_count, int32_t threads_per_sm, int32_t* grid, uint64_t* offset_advance);
/* out[i] = element i of the draw (seed, philox_offset, n) of THE TORCH STREAM, dtype VC_RNG_BF16 / VC_RNG_F32 / VC_RNG_U32 (the raw
 * word x[lane], before the transform).  A function of the contract only: the launch geometry does not show.  Any base aligned to
 * the element size; 16-byte stores where the base is 16-byte aligned.  seed and philox_offset are by-value kernel arguments, as in
 * vc_randn: legal under stream capture, and a replayed graph repeats its noise.  The CALLER advances its offset (vc_torch_randn_policy).
 * Arguments are checked before the device is touched (VC_ERR_ARG: null pointer, n <= 0 or > 2^48, unknown dtype, philox_offset not a
 * multiple of 4, philox_offset + advance wrapping, misaligned base, sm_count < 0, an explicit threads_per_sm < 256). */
int vc_randn_torch(void* out, int32_t dtype, int64_t n, uint64_t seed, uint64_t philox_offset, int32_t sm_count, int32_t threads_per_sm,
                   void* stream);
/* The start state in one launch: element (c, y, x) of a [C, h, w] draw is element i = (c*h + y)*w + x of the draw of n = C*h*w,
 * written as bf16 into the packed-token layout under vc_randn_tokens' rules.  Bit-identical to a VC_RNG_BF16 vc_randn_torch of
 * C*h*w elements into [C, h, w] followed by vc_pack_latent. */
int vc_randn_torch_tokens(void* tokens, int32_t C, int32_t h, int32_t w, int64_t ld, int32_t col0, uint64_t seed, uint64_t philox_offset,
                          int32_t sm_count, int32_t threads_per_sm, void* stream);

/* ---- VAE decoder glue (reference twin models/modules/autoencoder.py): activations are NHWC bf16
 * [H*W, C], C % 8 == 0; the 3x3 convolutions and 1x1 projections themselves are vc_gemm over these buffers. ----
 * im2col3x3:   src [Hs*Ws, C] -> dst [H*W, 9*C], column (dy*3+dx)*C + c of row (y,x) = src(y+dy-1, x+dx-1), zero outside
 *              (nn.Conv2d(k=3, padding=1), autoencoder.py:64,66,101,126,157,209,235); mode 1 reads src at (y>>1, x>>1),
 *              i.e. F.interpolate(scale_factor=2, mode="nearest") folded into the gather (Upsample.forward, :103-106);
 *              mode 2 reads src [2H*2W, C] at (2y+dy, 2x+dx), zero beyond the edge = pad (0,1,0,1) + stride-2 conv
 *              (Downsample.forward, :91-95).
 * groupnorm:   nn.GroupNorm(G, C, eps, affine) over the whole [HW, C] map, f32 statistics (two-level, deterministic),
 *              y = bf16(.), then bf16(y*sigmoid(y)) if swish (autoencoder.py:21-22,30,63,65,234; :70-77,257-258).
 *              scratch: >= (ceil(HW/128) + 1) * 2 * G floats of device memory.
 * softmax_rows: x[r, 0:cols] <- bf16(softmax(v)) in place, v = bf16(scale * x[r, :]) (+ bias[r, :], rounded to bf16 again),
 *              f32 internal, cols <= 16384; bias NULL or bf16 [rows, cols] (T5 relative position bias); causal_period
 *              P > 0 masks columns j > r % P (CLIP text)   (scaled_dot_product_attention of AttnBlock.attention, :47;
 *              T5Attention / CLIPAttention of transformers).
 * transpose:   dst[c, r] = src[r, c] (V^T operand of the P.V GEMM).
 * nchw_to_nhwc: dst[p, c] = bf16(src[c, p] / div + add), zero for C <= c < Cp  (decode: z / scale_factor + shift_factor,
 *              :306-307); src f32 or bf16.   nhwc_to_nchw: dst[c, p] = src[p, c] for c < C; dst f32 or bf16.
 * gaussian_sample: moments [HW, Cp] NHWC (mean channels [0,Z), logvar [Z,2Z)) -> out [Z, HW] bf16 =
 *              scale * ((mean + exp(0.5*logvar) * noise) - shift); noise [Z, HW] bf16 or NULL for the mean
 *              (DiagonalGaussian.forward :268-275, AutoEncoder.encode :301-304). */
int vc_im2col3x3(const void* src, void* dst, int32_t H, int32_t W, int32_t C, int32_t mode, void* stream);
/* conv3x3: the same convolution as vc_im2col3x3 + vc_gemm in ONE launch, no [H*W, 9C] matrix in HBM: the GEMM's loader
 * waves gather the taps from the NHWC map x, which must carry ONE EXTRA ZERO ROW after its Hs*Ws pixel rows (the source
 * of every out-of-image tap).  w [O, 9*C] with K ordered (dy, dx, c), C % 64 == 0, O % 8 == 0; out [H*W, O] row stride
 * ldc; res/gate NULL -> y = bf16(acc + bias), else y = bf16(res + bf16(gate * bf16(acc + bias))) (gate [O]). */
int vc_conv3x3(const void* x, const void* w, const void* bias, void* out, int64_t ldc, const void* res, int64_t ldres,
               const void* gate, int32_t H, int32_t W, int32_t C, int32_t O, int32_t mode, void* stream);
int vc_groupnorm(const void* x, const void* gamma, const void* beta, void* y, void* scratch, int64_t scratch_bytes,
                 int64_t HW, int32_t C, int32_t G, float eps, int32_t swish, void* stream);
int vc_softmax_rows(void* x, int64_t ld, int32_t rows, int32_t cols, float scale, const void* bias, int64_t ld_bias,
                    int32_t causal_period, void* stream);
int vc_transpose(const void* src, int64_t ld_src, void* dst, int64_t ld_dst, int32_t rows, int32_t cols, void* stream);
int vc_nchw_to_nhwc(const void* src, int32_t src_is_f32, void* dst, int32_t C, int32_t Cp, int64_t HW, float div, float add, void* stream);
int vc_nhwc_to_nchw(const void* src, void* dst, int32_t dst_is_f32, int32_t C, int32_t Cp, int64_t HW, void* stream);
int vc_gaussian_sample(const void* moments, int32_t Cp, const void* noise, void* out, int32_t Z, int64_t HW, float scale, float shift, void* stream);

/* ---- text-encoder glue (reference call site models/modules/conditioner.py:5-37, arithmetic of
 * transformers' T5EncoderModel / CLIPTextModel run in bf16).  Projections and per-head attention products are vc_gemm. ----
 * embedding:  out[i, :] = table[clamp(ids[i]), :]                                       (nn.Embedding)
 * rmsnorm:    y = bf16(w * bf16(x * rsqrt(mean(x^2) + eps))), f32 statistics, D <= 4096   (T5LayerNorm)
 * layernorm:  y = bf16((x - mean) * rstd * w + b), f32 statistics, D <= 4096              (nn.LayerNorm, CLIP)
 * mul / add:  y = bf16(a * b) / bf16(a + b), n % 8 == 0          (T5DenseGatedActDense product; CLIP token + position)
 * quick_gelu: y = bf16(x * bf16(sigmoid(bf16(1.702 * x))))                                (CLIP hidden_act)
 * t5_relative_buckets: HOST-ONLY, no device: out HOST [2 L - 1], out[(j - i) + L - 1] = the bucket of relative position key j - query i
 *             (T5Attention._relative_position_bucket, bidirectional) in the f32 arithmetic transformers runs it in - the table that
 *             visualcloze_amd/text.py::t5_relative_buckets holds as [L, L].  num_buckets even in 4..128, max_distance > num_buckets / 4.
 * t5_position_bias: out[h * L + i, j] = table[bucket(j - i), h]: the [H * L, L] bias operand of vc_softmax_rows from
 *             relative_attention_bias.weight [num_buckets, H] (row stride ld) - a pure gather, bit-exact; the buckets are computed on
 *             the host as above and travel as kernel arguments (no upload, no allocation).  L % 8 == 0.
 *             Replaces: buckets -> fancy index -> permute -> contiguous in torch (T5Attention.compute_bias).
 * clip_embed: out [Lp, D]: rows i < L = bf16(f32(tok[clamp(ids[i])]) + f32(pos[i])) (CLIPTextEmbeddings), rows L..Lp-1 = tok[0] plus a
 *             position row of zeros (the padding of the 64-row GEMM tiles; causal masking keeps it out of rows < L).  One launch for
 *             vc_embedding over zero-padded ids + a zeroed position buffer + its first L rows copied in + vc_add: the same bits.
 * clip_pool:  pooled [D] = hidden[e, :], e = the first i < L with ids[i] == eos_token_id, 0 if there is none (pooler_output of
 *             CLIPTextTransformer.forward: argmax over (ids == eos)) - on the device, no host read-back. */
int vc_embedding(const int32_t* ids, const void* table, int64_t ld_table, int32_t vocab, void* out, int32_t L, int32_t D, void* stream);
int vc_rmsnorm(const void* x, const void* weight, void* y, int32_t rows, int32_t D, float eps, void* stream);
int vc_layernorm(const void* x, const void* weight, const void* bias, void* y, int32_t rows, int32_t D, float eps, void* stream);
int vc_mul(const void* a, const void* b, void* y, int64_t n, void* stream);
int vc_add(const void* a, const void* b, void* y, int64_t n, void* stream);
int vc_quick_gelu(const void* x, void* y, int64_t n, void* stream);
int vc_t5_relative_buckets(int32_t L, int32_t num_buckets, int32_t max_distance, int32_t* out);
int vc_t5_position_bias(const void* table, int64_t ld, int32_t H, int32_t L, int32_t num_buckets, int32_t max_distance, void* out, void* stream);
int vc_clip_embed(const int32_t* ids, const void* tok, int64_t ld_tok, int32_t vocab, const void* pos, int64_t ld_pos, void* out, int32_t L,
                  int32_t Lp, int32_t D, void* stream);
int vc_clip_pool(const int32_t* ids, const void* hidden, int64_t ld, int32_t L, int32_t D, int32_t eos_token_id, void* pooled, void* stream);

/* ---- LoRA merge (ABI 11): LinearLora (models/modules/lora.py:66-67 the factor pair, :92-98 its forward) folded into ONE weight ----
 *   out[o, i]   = bf16( f32(W[o, i]) + scale * acc[o, i] ),   acc[o, i] = sum_k f32(B[o, k]) * f32(A[k, i])
 *   bias_out[o] = bf16( f32(b[o])    + scale * f32(bB[o]) )
 * W = the Linear's weight [out_features, in_features], bf16 or F32 (w_is_f32), row stride ldw; A = lora_A.weight [rank, in_features]
 * and B = lora_B.weight [out_features, rank], bf16, each in nn.Linear's OWN layout (row strides lda, ldb: no transposed copy is
 * asked for); out [out_features, in_features] bf16, row stride ldo.  The products are bf16 x bf16 on the matrix cores, exact in
 * f32, and accumulate in f32 - only the order of those sums differs from an f32 matmul.  TWO more roundings follow, as in
 * `W32 += scale * (B32 @ A32)`: scale * acc is rounded to f32, then the sum with W is, then the result goes to bf16 (nearest even);
 * no fused multiply-add.  0 <= rank <= 512; any out_features, in_features.  16-byte accesses need 16-byte aligned bases and
 * in_features and every row stride a multiple of 8; anything else runs element-wise, slower, with the same results.
 * out may BE w (bf16 weight, ldo == ldw: merged in place, no second matrix exists); it must not overlap w in any other way, nor
 * the factors.  bias: b [out_features] bf16 or F32 (bias_is_f32) or NULL (= 0), bB = lora_B.bias bf16 or NULL (bias_out = bf16(b));
 * bias_out NULL with both NULL, and may be b itself when b is bf16.  rank == 0 with NULL factors: a conversion / copy of W
 * (and b), so that every Linear of a checkpoint can go through this one entry point.  Arguments are checked before the device
 * is touched (VC_ERR_ARG + message).  Replaces: the torch f32 matmul a host would otherwise need to fold a LoRA checkpoint. */
int vc_lora_merge(const void* w, int32_t w_is_f32, int64_t ldw, const void* lora_a, int64_t lda, const void* lora_b, int64_t ldb,
                  float scale, void* out, int64_t ldo, const void* bias, int32_t bias_is_f32, const void* lora_b_bias, void* bias_out,
                  int32_t out_features, int32_t in_features, int32_t rank, void* stream);

/* vc_lora_merge_qkv: vc_lora_merge with the result's rows stored HEAD-PERMUTED, the order VcGemmProblem.kn_heads describes and
 * option "qkv_heads" announces.  Added WITHOUT a change of VC_ABI_VERSION: detect by SYMBOL (look up vc_flux_load_tensor).  With
 * H = qkv_heads and D = 128 * H, row r of the merged weight (and element r of bias_out) is stored at row
 *     r < 2D:        192 * (r / 128) + r % 128
 *     2D <= r < 3D:  192 * (u / 64) + 128 + u % 64,   u = r - 2D
 *     r >= 3D:       r                                  (the MLP rows of a SingleStream block's linear1)
 * The arithmetic, the roundings and the order of the sums are vc_lora_merge's; only the store address differs.  out (and bias_out)
 * must not overlap w (bias) AT ALL - there is no in-place form, the piece a wave writes is not the piece it read - and
 * out_features >= 3 * 128 * qkv_heads; both are VC_ERR_ARG.  qkv_heads == 0 is vc_lora_merge, in-place form included. */
int vc_lora_merge_qkv(const void* w, int32_t w_is_f32, int64_t ldw, const void* lora_a, int64_t lda, const void* lora_b, int64_t ldb,
                      float scale, void* out, int64_t ldo, const void* bias, int32_t bias_is_f32, const void* lora_b_bias, void* bias_out,
                      int32_t out_features, int32_t in_features, int32_t rank, int32_t qkv_heads, void* stream);

/* ---- handle API: the whole of Flux.forward, and the whole fixed-grid Euler loop, behind one call each ----
 * vc_flux_forward       replaces Flux.forward                      (models/model.py:85-124)
 * vc_flux_sample_euler  replaces odeint(method="euler") over it    (transport/integrators.py:106-120, transport.py:361-410:
 *                       drift = -model(x || cond, 1 - t); x += dt * drift with the reference's bf16 roundings)
 * The handle holds no tensor: weights are zero-copy views bound by name, every activation lives in a caller-provided
 * workspace.  It does own small host-side state (a pinned staging buffer, the captured hipGraph of one solver step, events).
 * One handle per device per process; not thread-safe per handle.  bf16 everywhere, LoRA pairs already folded into the
 * bound weights (W + s*B@A, lora.py:92-98) - or, with option "lora_mode" 1, bound next to the un-merged base weights and executed
 * as the reference's LinearLora does (vc_flux_bind_lora below).  A C caller gets to the merged form from a
 * LoRA checkpoint with one vc_lora_merge call per Linear - in place on its own copy of the base weight, or with `out` pointing at
 * the Linear's rows of the stacked "modulation" matrix - and binds the results. */
typedef struct VcFluxConfig {   /* FluxParams, models/model.py:18-32 */
  int32_t in_channels, out_channels, vec_in_dim, context_in_dim, hidden_size, num_heads, depth, depth_single_blocks;
  int32_t mlp_hidden;           /* hidden_size * mlp_ratio */
  int32_t guidance_embed;
  int32_t axes_dim[3];          /* sum = 128 */
  int32_t theta;
} VcFluxConfig;
int vc_flux_create(const VcFluxConfig* cfg, void** handle);
int vc_flux_destroy(void* handle);
/* name = reference module path of an nn.Linear ("img_in", "time_in.in_layer", "double_blocks.3.img_attn.qkv",
 * "single_blocks.7.linear1", "final_layer.linear", ...): w [rows, cols] bf16 with row stride ldw, bias [rows] or NULL;
 * or of a QKNorm scale ("double_blocks.3.img_attn.norm.query_norm.scale": w [128], rows = 1);
 * or "modulation": EVERY Modulation / adaLN Linear (layers.py:120-126, 253) stacked along the rows in the order
 * double_blocks.i.img_mod.lin, double_blocks.i.txt_mod.lin (i ascending), single_blocks.i.modulation.lin,
 * final_layer.adaLN_modulation.1 - vc_flux_mod_offset(name) is each module's first row, vc_flux_mod_offset(NULL) the total -
 * so that one GEMM yields every shift / scale / gate of every solver step;
 * or, optionally, "timestep_freqs": the 128 F32 frequencies exp(-ln(10000) * k / 128) of timestep_embedding
 * (layers.py:41-43) as the caller's framework computes them (rows = 1, cols = 128; default: exp in f64, rounded to f32,
 * which is within 1 ulp of torch's f32 exp);
 * or, optionally, "splitk_ws": ONE device scratch of rows * cols F32 values >= VC_GEMM_SPLITK_WS_BYTES for the split-K / stream
 * remainders of every geometry this handle runs (rows = 1, cols = the float count) - bound BEFORE vc_flux_workspace_bytes is
 * asked, it keeps those 100 MB out of each workspace (default: carved into every workspace); a FIRST bind after
 * vc_flux_workspace_bytes or vc_flux_prepare has answered is refused (VC_ERR_STATE: it would change the layout of workspaces the
 * caller already holds); re-binding another buffer is allowed at any time.  Pointers must stay valid while bound. */
int vc_flux_bind_weight(void* handle, const char* name, const void* w, const void* bias, int32_t rows, int32_t cols, int64_t ldw);
int64_t vc_flux_mod_offset(void* handle, const char* module_name);
/* knobs for tests and A/B runs: "attn_variant" (-1 = by size, the default), "tile_cfg" (0; flag bits such as
 * VC_GEMM_PREFER_STREAMK ride along), "fuse_qnorm" (2, the default: query QKNorm + RoPE + the softmax scale in the qkv GEMM's
 * epilogue wherever the key heads are normalised there, VcGemmProblem.qn_scale / VcAttention.q_prescaled; 1: inside the attention
 * kernel, VcAttention.q_scale; 0: by the pre-pass), "fuse_vt" (1: V^T from the qkv GEMM's epilogue, VC_EPI_QKV);
 * "qkv_heads" (0; = num_heads when the caller bound HEAD-PERMUTED qkv weights - every `*_attn.qkv` and the first
 * 3 * hidden rows of every `linear1`, with their biases, in the row order VcGemmProblem.kn_heads describes) and, with it,
 * "fuse_knorm" (0; 1: QKNorm + RoPE of the key heads inside the qkv GEMM's epilogue - with fuse_qnorm and fuse_vt the
 * projection, the norms, RoPE and the V transpose are then ONE GEMM launch + the attention kernel: no pre-pass, no prologue);
 * "logit_bound_milli" (0 = every attention launch keeps a running max; > 0: the softmax without one where the logits are bounded -
 * the value, 16330 * max|query_norm.scale| * max|key_norm.scale| over all blocks rounded up, is a CAP: each attention launch gets
 * the smaller of it and its OWN block's bound, which the library computes from the bound QK-norm scales when it resolves the
 * weights (one 256-byte read-back per scale vector), so a checkpoint with outlier scales in a few blocks runs the running-max
 * template in those blocks only); "mlp_first", "splitk" (1: split-K / stream remainders where the launcher takes them);
 * "lora_mode" (0; 1: un-merged LoRA execution, see vc_flux_bind_lora). */
int vc_flux_set_option(void* handle, const char* name, int32_t value);

/* ---- un-merged LoRA execution: LinearLora.forward (models/modules/lora.py:92-98) with the reference's three roundings, the parity
 * mode of the handle.  Added WITHOUT a change of VC_ABI_VERSION (tests pin 11): detect these entry points by SYMBOL - look up
 * vc_flux_bind_lora.  Off by default; while off nothing changes (the same launches, the same workspace size, the same bits).
 * vc_flux_set_option(handle, "lora_mode", 1): the weights bound by vc_flux_bind_weight are the UN-MERGED base weights (the stacked
 * "modulation" matrix included, qkv rows in their natural order: "qkv_heads" 0), and every Linear runs as
 *     y = bf16(x W^T + b);  h = bf16(x A^T);  y = bf16(y + bf16(bf16(h B^T + b_B) * scale));  out = epilogue(y)
 * - three vc_gemm launches (the last one with VC_EPI_GATE_RES: y as the residual, the scale as a bf16 gate vector) and the Linear's
 * own epilogue (GELU, SiLU, gated residual: vc_act2d / vc_gate_residual; QK-norm + RoPE + V^T: vc_qknorm_rope_vt) as a pass of its
 * own; no split-K.  A Linear without a bound pair runs the first launch and its pass.  In mode 0 bound pairs are ignored.
 * The mode changes the workspace (three scratch matrices and the scale vector behind everything else): set it, THEN ask
 * vc_flux_workspace_bytes and prepare; a switch un-prepares the handle, and between vc_flux_sample_begin* and vc_flux_sample_end
 * it is refused (VC_ERR_STATE).  The sampling loop (batches, F32 states, midpoint / rk4, true CFG, the step cache) runs either mode.
 * vc_flux_bind_lora: name as for vc_flux_bind_weight - a Linear whose weight is bound already (VC_ERR_STATE otherwise), or a module of
 * the stacked modulation matrix ("double_blocks.0.img_mod.lin", ...: the names of vc_flux_mod_offset); "single_blocks.i.linear1" takes
 * ONE pair for its 3 * hidden + mlp rows.  lora_a [rank, in_features] (row stride lda), lora_b [out_features, rank] (ldb),
 * lora_b_bias [out_features] or NULL: bf16 device memory the caller keeps alive.  rank: a multiple of 64, the GEMM's K granularity
 * (zero-pad the factors); out_features / in_features must be those of the bound weight; anything else is VC_ERR_ARG naming the
 * argument, nothing is launched.  lora_a == lora_b == NULL removes the pair.  Binding un-prepares the handle (the widest rank sizes
 * the scratch).
 * vc_flux_set_lora_scale: the scale of EVERY pair (default 1.0).  It must be a bf16 value (1, 0.5, 0.75, ...: the reference rounds
 * bf16(lora_out * scale) once, and so does a bf16 gate only then), else VC_ERR_ARG.  Host only: no re-bind, no re-merge, no
 * re-capture.  vc_flux_prepare writes the value into the scale vector (one fill launch), which keeps its place in that workspace, so
 * a step captured there replays with the new scale.  vc_flux_prepare also runs txt_in, vector_in and guidance_in and parks their
 * results in the workspace, and vc_flux_sample_begin* every modulation row of the trajectory - all un-merged Linears that read the
 * scale.  Hence: in mode 1 a CHANGED scale on a prepared handle makes vc_flux_forward / vc_flux_sample_begin* return VC_ERR_STATE
 * until vc_flux_prepare has been called again (never old-scale projections under a new-scale body), and between
 * vc_flux_sample_begin* and vc_flux_sample_end the call itself is VC_ERR_STATE. */
int vc_flux_bind_lora(void* handle, const char* name, const void* lora_a, int64_t lda, const void* lora_b, int64_t ldb,
                      const void* lora_b_bias, int32_t out_features, int32_t in_features, int32_t rank);
int vc_flux_set_lora_scale(void* handle, float scale);

/* ---- a checkpoint AS STORED: from the tensors of FluxLoraWrapper.state_dict() (models/model.py:154-175; the checkpoints
 * models/util.py:409-411 and visualcloze.py:111-112 load) in device memory to the bound, merged set - what Flux.prepare does with
 * torch, behind the handle.  Added WITHOUT a change of VC_ABI_VERSION (tests pin 11): detect these entry points by SYMBOL - look up
 * vc_flux_load_tensor.  No new struct.  Reading the file (.safetensors, .pth) stays with the caller, as image decoding does.
 *   vc_flux_load_key     host only: key `index` (0, 1, ... until VC_ERR_ARG) of the state_dict the handle's VcFluxConfig implies, in
 *                        state_dict order, with its shape: for every Linear `<path>.weight` [out, in], `<path>.bias` [out],
 *                        `<path>.lora_A.weight` [rank, in], `<path>.lora_B.weight` [out, rank], `<path>.lora_B.bias` [out], and the
 *                        QK-norm scales `...norm.query_norm.scale` / `...norm.key_norm.scale` [128].  The rank dimension is reported
 *                        as -1: it is free per Linear.  name receives at most namelen - 1 characters and a terminator.
 *   vc_flux_load_tensor  host only, launches nothing: records the device tensor `ptr` under `key` - dense, row-major, as stored.
 *                        Weights, biases and scales are bf16 or F32 (is_f32); LoRA factors and lora_B.bias are bf16 (vc_lora_merge's
 *                        rule).  An unknown key, a shape other than the key's (rank 0 .. 512, equal between a Linear's two factors)
 *                        or an F32 factor is VC_ERR_ARG naming the key, and nothing is recorded.  ptr == NULL forgets the key.
 *                        The pointers must stay valid until vc_flux_load_finish has returned and its stream work is done.
 *   vc_flux_load_bytes   host only: the size of the arena the prepared set takes, every tensor 256-byte aligned (c = round up to 256):
 *                          sum over the Linears outside the modulation stack of  c(2 out in) + c(2 out)          merged weight, bias
 *                          + c(2 n_mod hidden) + c(2 n_mod)                      the stacked modulation matrix and its bias
 *                          + 256 n_scales + c(4 n_scales)                        the bf16 scales, their F32 maxima
 *                        n_mod = vc_flux_mod_offset(handle, NULL), n_scales = 4 depth + 2 depth_single_blocks.
 *   vc_flux_load_finish  one vc_lora_merge_qkv launch per Linear with `lora_scale` (any F32 value) - qkv_heads = num_heads for every
 *                        `*_attn.qkv` and `linear1`, out = the Linear's rows of the stacked matrix for the modulation Linears, rank 0
 *                        for a Linear without a recorded pair (a lora_B.bias counts only with its pair; a Linear without any bias is
 *                        bound without one, zeros in the stacked bias) - then ONE launch that casts every scale vector to bf16 and
 *                        takes its max|.|, then one read of those maxima.  The results are bound under the names of
 *                        vc_flux_bind_weight, and the options that describe them are set: "qkv_heads" = num_heads, "fuse_knorm" 1,
 *                        "logit_bound_milli" = the largest block's 1.02 sqrt(128) log2(e) max|q scale| max|k scale| (held as F32)
 *                        times 1000, rounded up - or 0 where a scale is NaN or that value is not below 2e9.  The handle is
 *                        un-prepared (vc_flux_prepare again); "timestep_freqs" and "splitk_ws" stay separate binds.  A weight or
 *                        scale that was never recorded, or one factor without the other, is VC_ERR_STATE naming the first missing
 *                        key; option "lora_mode" 1, a NULL or misaligned arena or one smaller than vc_flux_load_bytes is VC_ERR_ARG;
 *                        between vc_flux_sample_begin* and vc_flux_sample_end the call is VC_ERR_STATE - all found before the device
 *                        is touched.  Synchronises `stream` once, at its end.  A second call - another lora_scale, re-recorded
 *                        tensors - merges again into the arena given: the way to change a merged LoRA without a framework.
 *   vc_flux_bound        host only: what is bound under a vc_flux_bind_weight name (any of the outputs may be NULL), or VC_ERR_STATE. */
int vc_flux_load_key(void* handle, int32_t index, char* name, int32_t namelen, int64_t* shape, int32_t* ndim);
int vc_flux_load_tensor(void* handle, const char* key, const void* ptr, int32_t is_f32, const int64_t* shape, int32_t ndim);
int64_t vc_flux_load_bytes(void* handle);
int vc_flux_load_finish(void* handle, float lora_scale, void* arena, int64_t arena_bytes, void* stream);
int vc_flux_bound(void* handle, const char* name, const void** w, const void** bias, int32_t* rows, int32_t* cols, int64_t* ldw);
/* ---- per-block taps: the residual streams after img_in / txt_in ("img_in", "txt_in"), after DoubleStream block i ("double.{i}.img",
 * "double.{i}.txt") and after SingleStream block i ("single.{i}": the joint stream, per sample the text rows, then the image rows).
 * Detect by SYMBOL (vc_flux_set_tap).  dst: the caller's bf16 device buffer of vc_flux_tap_shape's rows x cols (rows in the engine's
 * order, samples stacked; the shape is that of the prepared geometry: VC_ERR_STATE before vc_flux_prepare), NULL removes the tap.
 * A tap is ONE device-to-device copy on the evaluation's own stream directly behind the block - no second stream, no branch in the
 * captured step, of which it is a node: the tap set is part of the key a captured step is kept under, and takes effect at the next
 * vc_flux_forward / vc_flux_sample_begin*; between vc_flux_sample_begin* and vc_flux_sample_end a change is VC_ERR_STATE (the
 * captured step of the trajectory keeps its copy node: dst must stay valid until vc_flux_sample_end).  With no tap set the plan is
 * launch for launch what it was.  During a trajectory a tap
 * holds the value of the last evaluation issued (a stage of midpoint / rk4 included; an evaluation the step cache reuses runs block
 * 0 only and leaves the later taps as they were).  An unknown name or a block index beyond the model's depth is VC_ERR_ARG. */
int vc_flux_set_tap(void* handle, const char* name, void* dst);
int vc_flux_tap_shape(void* handle, const char* name, int64_t* rows, int32_t* cols);
int64_t vc_flux_workspace_bytes(void* handle, int32_t B, int32_t T, int32_t N, int32_t max_steps);

typedef struct VcFluxInputs {   /* everything of model_kwargs that does not change along the trajectory */
  int32_t B, T, N, max_steps;   /* samples stacked in one launch sequence; text / image tokens; model EVALUATIONS the workspace holds
                                   (= solver steps for Euler; steps * vc_solver_evals(method) otherwise) */
  const void* txt;              /* [B, T, context_in_dim] bf16, device */
  const void* y;                /* [B, vec_in_dim] bf16, device */
  const float* guidance;        /* HOST [B], NULL without guidance_embed */
  const float* img_ids;         /* HOST [B, N, 3] */
  const float* txt_ids;         /* HOST [B, T, 3] */
  const int32_t* kv_len;        /* HOST [B] or NULL: rows >= kv_len[b] of the joint (txt, img) sequence are masked */
  const int32_t* kv_gap;        /* HOST [B][2] or NULL: a second masked range (see VcAttention.kv_gap) */
  int32_t guidance_is_bf16;     /* the caller's guidance tensor is bf16: 1000 * g rounds to bf16 (layers.py:38) */
  int32_t _pad;
} VcFluxInputs;
/* txt_in, the guidance / vector embedders, the RoPE table (f64 on the host as math.py:102-109), masks; zeroes the V^T
 * padding.  workspace: device memory, >= vc_flux_workspace_bytes(B, T, N, max_steps), 256-B aligned, the caller's for as
 * long as forward / sample calls follow. */
int vc_flux_prepare(void* handle, const VcFluxInputs* in, void* workspace, int64_t workspace_bytes, void* stream);
/* ONE evaluation: out [B, N, out_channels] = Flux(img [B, N, in_channels]; timesteps HOST [B]) */
int vc_flux_forward(void* handle, const void* img, const float* timesteps, int32_t timesteps_is_bf16, void* out, void* stream);
/* ONE evaluation as the flow-matching loss: Transport.training_losses (transport.py:132-176) on the prepared samples, forward only.
 * Detect by SYMBOL (look up vc_flux_eval_loss).  OPT-IN: vc_flux_set_option(handle, "eval_loss", 1) BEFORE vc_flux_workspace_bytes /
 * vc_flux_prepare (max_steps >= 1) - it adds u_t (B * N * out_channels F32), the B times and the B * VC_FM_LOSS_MAX_BLOCKS partial
 * sums behind everything else; with it off the workspace, the captured steps and every output bit are what they were.  A switch
 * un-prepares the handle; VC_ERR_STATE without the option, before vc_flux_prepare, between vc_flux_sample_begin* and
 * vc_flux_sample_end, and with true CFG on (vc_flux_set_cfg: the reference never trains through forward_with_cfg).
 * x1 [B, N, out_channels] dense, bf16 or F32 (x1_is_f32), rows in the handle's order (image rows valid-first per sample, as img of
 * vc_flux_forward); cond [B, N, in_channels - out_channels] bf16, required (vc_flux_create takes in_channels > out_channels only: a model whose img_in
 * reads x_t alone runs vc_fm_plan / vc_fm_loss around its own evaluation); t HOST F32 [B],
 * finite; x0 a tensor of x1's dtype, or NULL for the draw of vc_fm_plan at (seed, offset); loss DEVICE F32 [B].  One call issues
 *   vc_fm_plan(x1, t', x0 | seed, offset) -> the model-input rows and u_t;   the cond columns beside x_t (one strided copy);
 *   vc_flux_forward's evaluation of those rows at timesteps = 1 - t' -> the velocity buffer;   vc_fm_loss over each sample's
 *   valid image rows, kv_len[b] - T (all N without kv_len) -> loss
 * with t' = t rounded to bf16 for a bf16 x1 (transport.py:129: t.to(x1[0])) and 1 - t' rounded likewise (a bf16 timesteps tensor,
 * timesteps_is_bf16 of vc_flux_forward); for an F32 x1 both stay F32.  It reuses the forward's buffers for the model input and
 * output.  The numerics monitor, if on, logs this evaluation into row 0 like vc_flux_forward.  Not captured: the launches are
 * issued on `stream`.  VC_ERR_ARG: a null x1 / cond / t / loss, a non-finite t, a sample without
 * a valid image row, B > VC_FM_MAX_HOST_COUNTS, a stream position past 2^64 - 1. */
int vc_flux_eval_loss(void* handle, const void* x1, int32_t x1_is_f32, const void* cond, const float* t, const void* x0, uint64_t seed,
                      uint64_t offset, float* loss, void* stream);
/* The loop.  x [B, N, out_channels]: in = x(t_grid[0]), out = x(t_grid[n_points-1]); cond [B, N, in - out channels] bf16;
 * t_grid HOST f32 [n_points] (n_points - 1 <= max_steps evaluations); state_is_bf16 != 0: x, x_out and trajectory are bf16 -
 * the pipeline's state dtype, visualcloze.py:399 - and the model sees 1 - bf16(t_i) (torchdiffeq hands the drift
 * t.to(y.dtype)); state_is_bf16 == 0: x, x_out and trajectory are F32, the state is stepped in f32 (integrators.py:119 keeps
 * the caller's dtype; the velocity and dt * velocity stay bf16 as under autocast) and the model sees 1 - t_i; dt is
 * t[i+1] - t[i] in f32 either way; trajectory: NULL or [n_points - 1][B][N][out_channels] receiving the state after every step.  One captured hipGraph per step (re-captured only
 * when geometry, masks' kind, workspace or options change); with stream == NULL the steps are launched uncaptured.
 * begin / steps / end expose the same loop piecewise (bench.py times single steps): sample_euler = begin; steps(n-1); end. */
int vc_flux_sample_euler(void* handle, void* x, const void* cond, const float* t_grid, int32_t n_points, int32_t state_is_bf16,
                         void* trajectory, void* stream);
int vc_flux_sample_begin(void* handle, const void* x, const void* cond, const float* t_grid, int32_t n_points,
                         int32_t state_is_bf16, void* stream);
int vc_flux_sample_steps(void* handle, int32_t n_steps, void* trajectory, void* stream);
int vc_flux_sample_end(void* handle, void* x_out, void* stream);
/* The same loop for any VC_SOLVER_* method (sample_euler / sample_begin are the VC_SOLVER_EULER case; steps / end serve every
 * method and count whole solver STEPS: trajectory receives the state after every step, never a stage state).  A step is
 * vc_solver_evals(method) replays of ONE captured evaluation whose last node is vc_ode_stage switching on the device-side
 * evaluation counter; the time embeddings and modulation rows of all (n_points - 1) * evals evaluations are built up front, in
 * evaluation order: t0 | t0 + half_dt (midpoint), t0 | t0 + dt * (1/3) | t0 + dt * (2/3) | t1 (rk4), formed in f32 and then
 * rounded to the state's dtype - rk4's last evaluation is at t_grid[n_points - 1], i.e. timesteps = 1 - t1.  An unknown method or
 * (n_points - 1) * evals > max_steps is VC_ERR_ARG, checked before the device is touched.  The captured step is kept per
 * (geometry, method). */
int vc_flux_sample_ode(void* handle, int32_t method, void* x, const void* cond, const float* t_grid, int32_t n_points,
                       int32_t state_is_bf16, void* trajectory, void* stream);
int vc_flux_sample_begin_ode(void* handle, int32_t method, const void* x, const void* cond, const float* t_grid, int32_t n_points,
                             int32_t state_is_bf16, void* stream);
/* ---- the adaptive solve: Dormand-Prince 5(4) with step-size control around the same captured evaluation.  OPT-IN: set
 * vc_flux_set_option(handle, "adaptive", 1) BEFORE vc_flux_workspace_bytes / vc_flux_prepare - it adds k [7], y0 and y1 (F32) and a
 * few words to the workspace - and prepare with max_steps >= 7 (the modulation rows of one attempt: k1's row and six evaluations).
 * With the option off nothing changes: the same graphs, workspace bytes and bits.  Detect by SYMBOL (look up vc_dopri5_stage).
 * x [B, N, out_channels]: in = x(t_grid[0]), out = x(t_grid[n_points - 1]); trajectory: NULL or [n_points - 1][B][N][out_channels]
 * receiving x(t_grid[1..]); both bf16 (state_is_bf16) or F32.  The controller is torchdiffeq's as recalled, unpinned against real
 * torchdiffeq (see vc_dopri5_stage above for what is pinned to SciPy):
 *   state   F32 inside whatever the caller's dtype: a bf16 state is widened on entry and rounded ONCE per output.  A departure:
 *           torchdiffeq would carry a bf16 state in bf16, where rtol = 1e-3 lies below the format's resolution.
 *   time    t and dt live on the host in double; the model sees 1 - f32(t).
 *   first step (Hairer, order 4; two evaluations)  scale = atol + rtol |y0|, d0 = rms(y0 / scale), d1 = rms(f0 / scale),
 *           h0 = 1e-6 if d0 < 1e-5 or d1 < 1e-5 else 0.01 d0 / d1;  f1 = f(t0 + h0, y0 + h0 f0);  d2 = rms((f1 - f0) / scale) / h0;
 *           h1 = max(1e-6, 1e-3 h0) if max(d1, d2) <= 1e-15 else (0.01 / max(d1, d2))^(1/5);  dt = min(100 h0, h1)
 *   attempt the six stage times and dt go up, the modulation rows are refilled, the captured evaluation is replayed six times
 *           (its last node is vc_dopri5_stage on the device-side counter), the error ratio is reduced and ONE stream
 *           synchronisation reads its 4 bytes from pinned memory
 *   decision  accept iff ratio <= 1;  dt_next = 10 dt if ratio == 0, else dt * min(10, max(0.9 / ratio^(1/5), ratio < 1 ? 1 : 0.2))
 *   errors  a NaN ratio, t + dt == t, or more than max_attempts attempts: VC_ERR_STATE with a message; the handle stays usable
 *   outputs steps are NOT clamped to the output times: a step runs past them and t_grid[1..] come from vc_dopri5_interp inside the
 *           accepted step that covers them.  The last step may overshoot t_grid[n_points - 1], so the model may be evaluated at
 *           timesteps = 1 - t < 0.
 *   ONE step size is shared by all samples of the call (the norm runs over the whole [B, N, out_channels] state, as torchdiffeq's
 *           does over its tensor): a sample's result depends on which samples share its call.
 * True CFG (vc_flux_set_cfg: the solver steps both halves), the un-merged LoRA mode and taps work unchanged; the step cache on is
 * VC_ERR_ARG.  Synchronises `stream` once per attempt (three more times for the first step).
 * log: of the last vc_flux_sample_dopri5 - for attempt i < min(capacity, *attempts): t[i], dt[i] (double), ratio[i], accepted[i];
 * *evaluations = every model evaluation it ran (2 + 6 per attempt).  Any array may be NULL. */
int vc_flux_sample_dopri5(void* handle, void* x, const void* cond, const float* t_grid, int32_t n_points, int32_t state_is_bf16,
                          float rtol, float atol, int32_t max_attempts, void* trajectory, void* stream);
int vc_flux_dopri5_log(void* handle, double* t, double* dt, float* ratio, int32_t* accepted, int32_t capacity, int32_t* attempts,
                       int32_t* evaluations);
/* ---- the same adaptive solve with a cheaper embedded pair: method VC_RK_BOSH3 (3 evaluations per attempt) or VC_RK_ADAPTIVE_HEUN
 * (2), against Dormand-Prince's 6.  OPT-IN through the SAME option "adaptive": it reuses that option's buffers (the first S planes of
 * k [7]), so the workspace bytes are those of vc_flux_sample_dopri5; prepare with max_steps >= S (4 / 3).  Everything said for
 * vc_flux_sample_dopri5 holds - the F32 state, host-side double time, ONE step size per call, one stream synchronisation per attempt
 * (three more for the first step), unclamped steps, its refusals and errors - with these differences:
 *   first step / decision   the same rules with the exponent 1 / order (order 3 / 2) where Dormand-Prince has 1/5; safety 0.9, growth
 *           capped at 10, shrink at 0.2, an accepted step never shrinks.  torchdiffeq's as recalled, unpinned against real torchdiffeq.
 *   probe   the evaluation at t0 + h0 runs as the last stage (c_S = 1), whose node stores k alone.
 *   outputs from vc_rk_interp, the Hermite cubic of the accepted step that covers them.
 *   VC_RK_DOPRI5 is VC_ERR_ARG: there is one route to Dormand-Prince, vc_flux_sample_dopri5.
 * The captured step is kept per (geometry, method).  log: of the last adaptive solve on the handle, of either entry point;
 * *evaluations = 2 + (S - 1) per attempt. */
int vc_flux_sample_rk(void* handle, int32_t method, void* x, const void* cond, const float* t_grid, int32_t n_points, int32_t state_is_bf16,
                      float rtol, float atol, int32_t max_attempts, void* trajectory, void* stream);
int vc_flux_rk_log(void* handle, double* t, double* dt, float* ratio, int32_t* accepted, int32_t capacity, int32_t* attempts,
                   int32_t* evaluations);
/* ---- the stochastic sampler around the same captured evaluation (vc_sde_plan / vc_sde_stage above have the mathematics).  OPT-IN:
 * set vc_flux_set_option(handle, "sde", 1) BEFORE vc_flux_workspace_bytes / vc_flux_prepare - it adds the F32 state, xhat, K1, the
 * coefficient table and the seed / offset words to the workspace - and prepare with max_steps >= the plan's evaluations.  With the
 * option off nothing changes: the same workspace bytes, graphs, nodes and bits.  Detect by SYMBOL (look up vc_sde_stage).
 * method, form, norm, last_step, last_step_size, t_grid, n_points: as for vc_sde_plan, which is run first - its refusals are this
 * call's, before anything touches the device.  x [B, N, out_channels]: in = x(t_grid[0]), out = the sample; bf16 (state_is_bf16) or
 * F32.  The state is stepped in F32 whatever the caller's dtype: a bf16 state is widened on entry and rounded ONCE per output.
 *   step    the captured step is the existing evaluation with vc_sde_stage on the device-side counter as its last node, kept per
 *           (geometry, method); for "Euler" it has exactly the nodes of the VC_SOLVER_EULER step (vc_flux_step_nodes).  The
 *           time embeddings, modulation rows and coefficient rows of all evaluations are built up front.
 *   noise   draw d (= solver step) of the call takes stream positions offset + d * n + i of the stream of `seed`, n = B * N *
 *           out_channels, i the flat index in THIS call's [B, N, out_channels] state; n_points - 1 draws.  seed and offset go to the
 *           device words the stage reads: one captured step serves every seed and every replay.  offset + (n_points - 1) * n
 *           leaving the 64-bit stream is VC_ERR_ARG.
 *   trajectory  NULL, or [n_points][B][N][out_channels] in the state's dtype: row i < n_points - 1 receives x' after loop step i,
 *           the last row the last step's result (the sample; without a last step it repeats row n_points - 2) - n_points rows, as
 *           the reference's list has num_steps entries.
 * True CFG (vc_flux_set_cfg: the combine comes before the update; both halves are stepped, each with its own noise positions),
 * taps and the un-merged LoRA mode work unchanged.  Refused: the option off (VC_ERR_STATE); the step cache on, the monitor on
 * (its log is indexed by the evaluations of a fixed-grid trajectory; turn it off with level 0), more evaluations than max_steps,
 * an odd B with true CFG (all VC_ERR_ARG) - each found before the device is touched; the handle stays usable.
 * Image quality under any diffusion form is UNMEASURED (only random-init weights exist here), and no throughput claim is made:
 * the update costs one elementwise pass like Euler's, and this was not timed on a GPU. */
int vc_flux_sample_sde(void* handle, const char* method, void* x, const void* cond, const float* t_grid, int32_t n_points, const char* form,
                       double norm, const char* last_step, double last_step_size, uint64_t seed, uint64_t offset, int32_t state_is_bf16,
                       void* trajectory, void* stream);
/* ---- the Adams-Bashforth multistep solve around the same captured evaluation (vc_ms_plan / vc_ms_stage above have the rule).
 * OPT-IN: set vc_flux_set_option(handle, "multistep", 1) BEFORE vc_flux_workspace_bytes / vc_flux_prepare - it adds the F32 state,
 * the ring of VC_MS_HIST past outputs and the coefficient table to the workspace - and prepare with max_steps >= n_points - 1.  With
 * the option off nothing changes: the same workspace bytes, graphs, nodes and bits.  Detect by SYMBOL (look up vc_ms_plan).
 * order, t_grid, n_points: as for vc_ms_plan, which is run first - its refusals are this call's, before anything touches the device.
 * x [B, N, out_channels]: in = x(t_grid[0]), out = x(t_grid[n_points - 1]); bf16 (state_is_bf16) or F32.  The state is stepped in F32
 * whatever the caller's dtype: a bf16 state is widened on entry and rounded ONCE per output.  One evaluation per step.
 *   step    the captured step is the existing evaluation with vc_ms_stage on the device-side counter as its last node, kept per
 *           geometry; it has exactly the nodes of the VC_SOLVER_EULER step (vc_flux_step_nodes).  ONE captured step serves every
 *           order: the order lives in the uploaded table, not in the graph (vc_flux_plan_count tells the captured steps the handle
 *           holds).  The time embeddings, modulation rows and coefficient rows of all evaluations are built up front.
 *   ring    the first evaluation of a call writes slot 0, the second slot 1, the third slot 2, each BEFORE any row reads it (row i
 *           reads i, at most 3, slots back); nothing of an earlier call or of the workspace's earlier contents is read.
 *   trajectory  NULL, or [n_points][B][N][out_channels] in the state's dtype: row 0 receives x(t_grid[0]) as the solver holds it
 *           (the caller's values), row i the state after step i - 1 - n_points rows.
 * True CFG (vc_flux_set_cfg: the combine comes before the update, the ring holds the combined velocity; both halves are stepped),
 * taps and the un-merged LoRA mode work unchanged.  Refused: the option off (VC_ERR_STATE); the step cache on, the monitor on
 * (turn it off with level 0), more evaluations than max_steps, an odd B with true CFG (all VC_ERR_ARG) - each found before the
 * device is touched; the handle stays usable.
 * Image quality at any order is UNMEASURED (only random-init weights exist here), and no throughput claim is made beyond "one
 * evaluation per step": the update is one elementwise pass like Euler's. */
int vc_flux_sample_multistep(void* handle, int32_t order, void* x, const void* cond, const float* t_grid, int32_t n_points,
                             int32_t state_is_bf16, void* trajectory, void* stream);
/* the captured steps the handle holds (most recently used first), or -1 for a null handle.  Host only.  The list holds at most 4: at
 * 4 a new capture evicts the least recently used step and the count STAYS 4 - a caller who reads it to tell whether a call
 * captured must start below 4. */
int vc_flux_plan_count(void* handle);

/* ---- first-block step cache of the Euler loop: OPT-IN, off by default.  IT CHANGES RESULTS: a reused evaluation is an
 * approximation, not the model.  Its effect on image quality is unmeasured (only random-init weights were available) and no default
 * threshold is recommended.  The rule is this library's own (the reference evaluates all blocks at every step), DESIGN.md section 4:
 * with h0 = the image stream after img_in, h1 = after double block 0, hE = the image rows after the last single block,
 * r = bf16(h1 - h0), P = the r of the last COMPUTED evaluation and R = bf16(hE - h1) of that evaluation, an evaluation is REUSED
 * - the image rows become bf16(h1 + R), then the last layer and the Euler update run as usual, blocks 1..end are not launched -
 * iff a P exists, m = max over the chunk's samples of sum|r - P| / sum|P| < threshold, and fewer than max_consecutive evaluations
 * were reused in a row.  The first evaluation after vc_flux_sample_begin* always computes.
 * threshold <= 0 or max_consecutive == 0: off (the default); max_consecutive < 0: no limit on consecutive reuses.  A changed setting
 * takes effect at the next vc_flux_sample_begin* (which is where a non-Euler method with the cache on is refused: VC_ERR_ARG).
 * While on: 3 * B * N * hidden_size bf16 (+ a few KB) more workspace - ask vc_flux_workspace_bytes AFTER setting it and prepare
 * again; the step is three captured graphs (head / tail-compute / tail-reuse) and vc_flux_sample_steps synchronises `stream` once
 * per step to read the 4-byte metric.  While off nothing changes: one graph, no host read, the same workspace size, the same bits.
 * vc_flux_forward and vc_flux_profile ignore the cache.
 * stats: of the trajectory in flight or just finished - *computed / *reused evaluation counts and, for the first `capacity`
 * evaluations, metrics[i] = the m of evaluation i (NaN where none existed: the first evaluation, or the cache off). */
int vc_flux_set_step_cache(void* handle, float threshold, int32_t max_consecutive);
/* ---- true CFG in the sampling loop: the drift is Flux.forward_with_cfg (models/model.py:126-145) instead of Flux.forward.  Off by
 * default.  While on, EVERY evaluation of the loop (each stage of midpoint and rk4, bf16 and F32 states alike) combines its velocity
 * V [B * N, out_channels] in place before the solver's update: with h = B / 2 the first h samples are the conditional half, the
 * rest the unconditional half, V[:h] <- vc_cfg_combine(V[:h], V[h:], cfg_scale), V[h:] stays.  The solver then steps the whole
 * B-sample state, both halves, as the reference's does; nothing of the conditional half reaches the unconditional one.
 * A changed setting takes effect at the next vc_flux_sample_begin*, where - while on - an odd B, the step cache on and a non-finite
 * cfg_scale are VC_ERR_ARG, checked before the device is touched.  The combine is one more node of the captured step, which is kept
 * per (geometry, method, on, cfg_scale).  While off nothing changes: the same graph, the same workspace size, the same bits.
 * vc_flux_forward and vc_flux_profile ignore the setting (forward_with_cfg = vc_flux_forward + vc_cfg_combine).  No new workspace. */
int vc_flux_set_cfg(void* handle, int32_t on, float cfg_scale);
int vc_flux_step_cache_stats(void* handle, int32_t* computed, int32_t* reused, float* metrics, int32_t capacity);
/* ---- the numerics monitor of the captured step: OPT-IN, off by default.  A sample call returns VC_OK for a latent full of NaN; with
 * the monitor on, every evaluation leaves vc_tensor_stats of chosen tensors in a log, and vc_flux_monitor_report names the first
 * (evaluation, site, sample) that held a NaN / +-inf.  Added WITHOUT a change of VC_ABI_VERSION: detect by SYMBOL
 * (look up vc_flux_set_monitor).  The return codes of the sample calls do NOT change: a caller who wants an error asks the report.
 * The log is sized for the B prepared when the monitor takes effect: after a prepare with another B, forward / sample_begin* are
 * VC_ERR_STATE until vc_flux_set_monitor is called again (a call outside a trajectory, with new or the same arguments, also forgets
 * what was logged).  vc_flux_monitor_report is NOT refused then: it reads the rows with the B they were logged with, so the report of a
 * finished trajectory can still be asked after the next batch has been prepared.
 * level 0  off.  The plan is launch for launch, node for node, what it is without these entry points.
 * level 1  two sites per evaluation: "v", the model's output [B, N, out_channels] before the solver's update (with true CFG on: before
 *          the combine, every sample's own velocity), and "x", the ODE state behind the solver's update - read as F32 where the state
 *          is F32.  (vc_flux_forward has no state: its "x" stays zeroed.)
 * level 2  those, then every tap site under its tap name, in tap order: "img_in", "txt_in", "double.{i}.img", "double.{i}.txt" for
 *          every i, "single.{i}" for every i.  Each is read in place in the workspace directly behind the block: no copy, and no tap
 *          needs to be set.  vc_flux_monitor_sites lists the names of the level set, index 0, 1, .. until VC_ERR_ARG (host only).
 * log, scratch: the caller's device buffers, as tap destinations are (the workspace's size and carve-up do not change); log is
 * [capacity_evals][n_sites][B] VcStat, sites in the order of vc_flux_monitor_sites, 16-byte aligned.  vc_flux_monitor_bytes gives both
 * sizes for the PREPARED B (host only; VC_ERR_STATE before vc_flux_prepare or with the monitor off); prepare with another B and they
 * are to be asked again.  A null log / scratch, a misaligned log, capacity_evals <= 0 or a level outside 0..2 is VC_ERR_ARG.
 * Every site is one vc_tensor_stats launch (two kernels) of the captured step, indexed by the device-side evaluation counter: the
 * setting is part of the key a captured step is kept under, exactly as the tap set is, takes effect at the next vc_flux_forward /
 * vc_flux_sample_begin*, and a change between vc_flux_sample_begin* and vc_flux_sample_end is VC_ERR_STATE.  vc_flux_sample_begin*
 * zeroes the whole log (one kernel launch outside the captured step) and refuses a trajectory of more EVALUATIONS (steps *
 * vc_solver_evals) than capacity_evals with VC_ERR_ARG; evaluation e of the trajectory - a stage of midpoint / rk4 included - logs
 * into row e.  vc_flux_forward zeroes the log and logs into row 0.  An evaluation that the step cache reuses runs block 0 only and
 * leaves the rows of the blocks it skipped zeroed (count == 0); its "img_in", "txt_in", "double.0.*", "v" and "x" are logged.
 * vc_flux_sample_dopri5 with the monitor on is VC_ERR_ARG: its device-side counter is the STAGE of an attempt, not an evaluation
 * index.  vc_flux_profile issues its evaluations without the monitor's launches.
 * report: a reduction over the rows logged so far on the device plus ONE small read-back (synchronises `stream`): the entry with
 * nonfinite != 0 that was WRITTEN first - in evaluation order, within an evaluation in the order its sites are written (the tap sites
 * in tap order, then "v", then "x": what lies upstream comes first, so the site named is where the trajectory went bad), then in
 * sample order - as the evaluation, the site's index in vc_flux_monitor_sites and the sample, or -1, -1, -1 when there is none;
 * *evals_logged = the evaluations issued since the log was zeroed (0, and -1s, before anything was logged).  Any output may be NULL.
 * VC_ERR_STATE with the monitor off.
 * vc_flux_step_nodes: host only - the number of graph nodes of the captured step of the trajectory begun last, nodes[0] the step (with
 * the step cache on: head, tail-compute, tail-reuse in nodes[0..2]; else nodes[1] = nodes[2] = 0).  What "node for node" is held to:
 * every monitor site adds two kernel nodes, level 0 adds none.  VC_ERR_STATE without a captured step (stream NULL captures none). */
int vc_flux_step_nodes(void* handle, int32_t nodes[3]);
int vc_flux_set_monitor(void* handle, int32_t level, VcStat* log, int32_t capacity_evals, float* scratch);
int vc_flux_monitor_sites(void* handle, int32_t index, char* name, int32_t namelen);
int vc_flux_monitor_bytes(void* handle, int32_t capacity_evals, int64_t* log_bytes, int64_t* scratch_bytes);
int vc_flux_monitor_report(void* handle, int32_t* first_bad_eval, int32_t* first_bad_site, int32_t* first_bad_sample, int32_t* evals_logged,
                           void* stream);

/* ---- the plan's own stopwatch (ABI 10): HIP-event times of the launches of whole evaluations, class by class ----
 * What bench.py's `roofline` leg reports.  With a sample in flight (vc_flux_sample_begin), `evaluations` more evaluations of
 * Flux.forward at the trajectory's CURRENT step are issued on `stream` by the same code the step graph was captured from - not
 * captured, no Euler update: the state, the step counter and the graph stay as they are - with an event in front of and behind
 * every GEMM, attention and LayerNorm-modulate launch (one warm evaluation first).  Every launch therefore finds the caches as
 * its predecessor in the step leaves them.  Synchronises `stream`; entries come in order of first appearance.
 * Reference: there is none (the reference times whole pipelines, visualcloze.py); replaces the Python-ordered twin of the plan
 * (visualcloze_amd/engine.py) as the thing bench.py times. */
enum { VC_LAUNCH_GEMM = 1, VC_LAUNCH_ATTENTION = 2, VC_LAUNCH_LN_MODULATE = 3,
       VC_LAUNCH_PASS = 4,   /* lora_mode 1: the epilogue of a Linear as its own pass (epi = its VC_EPI_*, n = the columns) */
       VC_LAUNCH_TAP = 5 };  /* the copies of all taps, one class */
typedef struct VcFluxLaunchClass {
  int32_t kind;        /* VC_LAUNCH_* */
  int32_t epi;         /* GEMM: the VC_EPI_* of the launch; attention: the VcAttention.variant that ran; else 0 */
  int32_t n, k;        /* GEMM: N and K of the launch's first problem (a grouped launch: its img stream); else 0 */
  int32_t launches;    /* launches of this class in the timed evaluations */
  int32_t reserved;
  double flops;        /* their arithmetic: 2 M N K over all problems (GEMM), 4 L^2 D B (attention: masked keys included), else 0 */
  double bytes;        /* LayerNorm-modulate, pass, tap: rows read + rows written; else 0 */
  float total_us;      /* sum of the launches' event times (an attention launch: the kernel and, where one runs, its merge kernel) */
  float min_us, max_us;
  float reserved2;
} VcFluxLaunchClass;
int vc_flux_profile(void* handle, int32_t evaluations, VcFluxLaunchClass* out, int32_t capacity, int32_t* count, void* stream);

/* ---- autoencoder handle: AutoEncoder.decode / AutoEncoder.encode (models/modules/autoencoder.py:277-311) behind one call each ----
 * Added WITHOUT a change of VC_ABI_VERSION (tests pin 11): detect these entry points by SYMBOL - look up vc_vae_create.
 * vc_vae_decode replaces AutoEncoder.decode (autoencoder.py:306-308: z / scale_factor + shift_factor, then Decoder.forward :237-259)
 * vc_vae_encode replaces AutoEncoder.encode (autoencoder.py:301-304: Encoder.forward :159-180, DiagonalGaussian :268-275, then
 *               scale_factor * (z - shift_factor))
 * The launch plan is the one visualcloze_amd/vae.py spells in Python over the op-level entry points above (vc_conv3x3, vc_groupnorm,
 * vc_gemm, vc_softmax_rows, vc_transpose, vc_nchw_to_nhwc, vc_nhwc_to_nchw, vc_gaussian_sample, vc_pack_latent, vc_unpack_latent): the
 * same kernels in the same order, so the two give the same bits.  ONE image per call, activations NHWC bf16.  Every activation lives
 * in a caller-provided workspace.  The handle OWNS the prepared weights: device copies in the GEMM's operand layout, made by
 * vc_vae_bind_weight and freed by vc_vae_destroy (this is the one place where the library allocates device memory), and the captured
 * hipGraphs.  One handle per device; not thread-safe per handle; the encoder and the decoder halves have separate workspace
 * regions, each half serves one stream at a time. */
typedef struct VcVaeConfig {    /* AutoEncoderParams, autoencoder.py:8-18, without `resolution` (the plan is built per image size) */
  int32_t in_channels, ch, out_ch;
  int32_t ch_mult[8];           /* the first n_ch_mult entries; every ch * ch_mult[i] a multiple of 64 */
  int32_t n_ch_mult;            /* 1..8: the image is 2^(n_ch_mult - 1) times the latent */
  int32_t num_res_blocks, z_channels;
  float scale_factor, shift_factor;
} VcVaeConfig;
/* sizeof(VcVaeConfig) as this library was compiled (vc_struct_sizes keeps its seven entries) */
void vc_vae_struct_sizes(int32_t out[1]);
/* host-only: needs no device */
int vc_vae_create(const VcVaeConfig* cfg, void** handle);
int vc_vae_destroy(void* handle);
/* the weights the handle expects, in the order of AutoEncoder.state_dict(): index 0, 1, ... until VC_ERR_ARG.  name receives the
 * module path - the state_dict key of the module's weight without the trailing ".weight" ("decoder.up.3.block.0.conv1",
 * "encoder.mid.attn_1.norm", ...); its ".bias" key is the same path.  Host-only. */
int vc_vae_weight_name(void* handle, int32_t index, char* name, int32_t namelen);
/* name: a module path as above (a trailing ".weight" is accepted).  w / bias: the tensors of the module's ".weight" / ".bias" keys
 * AS A CHECKPOINT STORES THEM, contiguous, both bf16 or both F32 (is_f32); shape HOST [ndim] = the weight's shape: [O, I, k, k] of an
 * nn.Conv2d (k = 3, or 1 for nin_shortcut and the attention projections), [C] of an nn.GroupNorm.  The call rounds to bf16 and
 * writes the handle's own copy - a convolution as [O_pad8, k * k * I_pad64] with K ordered (dy, dx, c), the operand layout of
 * vc_conv3x3 - with two small kernels on `stream`, which it synchronises: w and bias may be released when it returns.  An unknown
 * name, a shape other than the module's, or a null pointer is VC_ERR_ARG with the name in the message (nothing is launched).
 * Binding again replaces the copy and drops the captured plans. */
int vc_vae_bind_weight(void* handle, const char* name, const void* w, const void* bias, int32_t is_f32, const int64_t* shape,
                       int32_t ndim, void* stream);
/* H, W: the IMAGE size in pixels, multiples of 2^(n_ch_mult - 1) (the latent is [z_channels, H / f, W / f]).  which: */
#define VC_VAE_ENCODER 1
#define VC_VAE_DECODER 2   /* VC_VAE_ENCODER | VC_VAE_DECODER = both */
/* Host-only; a bad size or `which` is VC_ERR_ARG. */
int vc_vae_workspace_bytes(void* handle, int32_t H, int32_t W, int32_t which, int64_t* bytes);
/* Carves the activation maps (each with the zero row vc_conv3x3 reads), the GroupNorm scratch and the attention buffers of the
 * chosen halves out of `workspace` (device memory, >= vc_vae_workspace_bytes, 256-B aligned, the caller's while decode / encode
 * calls follow) and fills the residual gate of ones - the only thing a plan reads that it does not write.  The handle serves ONE
 * prepared (H, W, which, workspace) at a time; preparing another and coming back keeps the captured plans of both.  A workspace
 * that is too small is VC_ERR_ARG and nothing is launched.  The fill is asynchronous on `stream`: a decode / encode call on ANOTHER
 * stream must be ordered behind it by the caller (an event, or a synchronise).  The carve-up depends on `which` (the decoder's
 * buffers start the workspace when it is prepared alone, and follow the encoder's otherwise), and so do the captured plans: a
 * workspace prepared again with another `which` gets plans of its own, the earlier ones serve again once the earlier `which` is
 * prepared again (which also refills the gate). */
int vc_vae_prepare(void* handle, int32_t H, int32_t W, int32_t which, void* workspace, int64_t workspace_bytes, void* stream);
/* latent_form: what the sampler leaves / what the sampler reads */
#define VC_VAE_LATENT_BF16 0   /* [z_channels, H / f, W / f] bf16, contiguous */
#define VC_VAE_LATENT_F32 1    /* the same in F32 (decode only) */
#define VC_VAE_TOKENS 2        /* packed tokens [(h / 2) (w / 2)][col0 .. col0 + 4 z_channels) of bf16 rows with stride ld, as
                                  vc_unpack_latent reads and vc_pack_latent writes them (ld, col0 multiples of 8; even h, w) */
/* pixels [out_ch, H, W] (bf16, or F32 with pixels_is_f32) = decoder(latent / scale_factor + shift_factor).  ld, col0: VC_VAE_TOKENS only.
 * An unbound decoder weight is VC_ERR_STATE naming the first missing key; so is a call before vc_vae_prepare with VC_VAE_DECODER.
 * With a stream, the call is ONE hipGraph launch: the plan for (workspace, H, W, which, direction, forms, the caller's pointers, stream) is
 * captured on first use - after one un-captured run that sets the kernels' attributes - and kept in a list of 8, most recently used
 * first; the pointers are kernel arguments of the graph, so a caller that keeps its buffers hits the list, and one that rotates
 * them pays a capture (no second un-captured run: that happens once per size, direction and forms) per new set of pointers.  stream == NULL runs
 * the same plan un-captured on the default stream. */
int vc_vae_decode(void* handle, const void* latent, int32_t latent_form, int64_t ld, int32_t col0, void* pixels, int32_t pixels_is_f32,
                  void* stream);
/* latent = scale_factor * ((mean + exp(0.5 * logvar) * noise) - shift_factor) of pixels [in_channels, H, W] (bf16 or F32); noise
 * [z_channels, H / f, W / f] bf16 is an INPUT as in vc_gaussian_sample, NULL = the mean (the mode of latent_dist).  latent_form
 * VC_VAE_LATENT_BF16 or VC_VAE_TOKENS (the packing then happens inside).  Errors and graph capture as vc_vae_decode. */
int vc_vae_encode(void* handle, const void* pixels, int32_t pixels_is_f32, const void* noise, void* latent, int32_t latent_form,
                  int64_t ld, int32_t col0, void* stream);
/* captured plans the handle holds (0..8); -1 for a null handle */
int vc_vae_plan_count(void* handle);

/* ---- text-encoder handle: T5EncoderModel / CLIPTextModel behind one call (HFEmbedder.forward, models/modules/conditioner.py:5-37;
 * loaded by load_t5 / load_clip of models/util.py, called from prepare_modified of models/sampling.py) ----
 * Added WITHOUT a change of VC_ABI_VERSION (tests pin 11): detect these entry points by SYMBOL - look up vc_text_create.
 * One handle is ONE encoder: VC_TEXT_T5 yields last_hidden_state (VcFluxInputs.txt), VC_TEXT_CLIP yields last_hidden_state and
 * pooler_output (VcFluxInputs.y).  Tokenisation stays host work: the handle takes token ids.  The launch plan is the one
 * visualcloze_amd/text.py spells in Python over the op-level entry points above (vc_embedding / vc_clip_embed, vc_rmsnorm / vc_layernorm,
 * vc_gemm - all heads of a layer in one batched launch -, vc_softmax_rows, vc_transpose, vc_mul, vc_quick_gelu, vc_clip_pool): the same
 * kernels, the same problem structs, the same order, so the two give the same bits.  bf16 everywhere.  The handle holds NO device
 * memory: tensors are bound by pointer, every activation lives in a caller-provided workspace; it owns the captured hipGraphs.  One
 * handle per device; not thread-safe per handle; it serves one stream at a time. */
#define VC_TEXT_T5 1
#define VC_TEXT_CLIP 2
typedef struct VcTextConfig {   /* T5Config / CLIPTextConfig of transformers, the fields the encoders read */
  int32_t kind;                 /* VC_TEXT_T5 or VC_TEXT_CLIP */
  int32_t vocab_size;
  int32_t d_model;              /* CLIP: hidden_size.  A multiple of 64, <= 4096 */
  int32_t d_kv;                 /* the head width, a multiple of 64.  CLIP: 0 or d_model / num_heads */
  int32_t d_ff;                 /* CLIP: intermediate_size.  A multiple of 64 */
  int32_t num_layers, num_heads;
  int32_t num_buckets, max_distance;     /* T5: relative_attention_num_buckets / relative_attention_max_distance */
  int32_t max_positions, eos_token_id;   /* CLIP: max_position_embeddings; the id whose hidden row is the pooled output */
  float eps;                    /* layer_norm_epsilon / layer_norm_eps */
} VcTextConfig;
/* sizeof(VcTextConfig) as this library was compiled */
void vc_text_struct_sizes(int32_t out[1]);
/* host-only: need no device.  A null config, an unknown kind or a width the GEMM does not take is VC_ERR_ARG. */
int vc_text_create(const VcTextConfig* cfg, void** handle);
int vc_text_destroy(void* handle);
/* the tensors the handle expects: the FULL state_dict() keys of the encoder, in order: index 0, 1, ... until VC_ERR_ARG
 * ("shared.weight", "encoder.block.0.layer.0.SelfAttention.q.weight", ... / "text_model.embeddings.token_embedding.weight", ...,
 * "text_model.encoder.layers.0.self_attn.k_proj.bias", ...).  T5 lists both tied keys: the plan reads "shared.weight";
 * "encoder.embed_tokens.weight" is accepted, shape-checked and never read (it need not be bound).  Host-only. */
int vc_text_weight_name(void* handle, int32_t index, char* name, int32_t namelen);
/* ptr: the tensor of state_dict key `key`, bf16, contiguous, 16-byte aligned, device memory; shape HOST [ndim] = its shape ([out, in]
 * of a Linear / Embedding weight, [n] of a bias or norm weight).  Bound BY POINTER as in vc_flux_bind_weight: no copy, no launch, the
 * caller keeps it alive while bound.  An unknown key, a shape other than the module's or a null pointer is VC_ERR_ARG with the key in
 * the message.  Binding again drops the captured plans (and T5's bias table is rebuilt by the next encode).  Host-only. */
int vc_text_bind_tensor(void* handle, const char* key, const void* ptr, const int64_t* shape, int32_t ndim);
/* L: ids per prompt.  T5: a multiple of 64 (the pipeline pads to 512; padding is attended, as with attention_mask=None).
 * CLIP: 1..max_positions; the rows are padded to ceil64(L) inside.  Host-only; a bad L is VC_ERR_ARG. */
int vc_text_workspace_bytes(void* handle, int32_t L, int64_t* bytes);
/* Carves the activations (x, n, q, k, v, S, V^T, O, the FF pair), the resident ids / output staging buffers and T5's [H L, L] bias
 * table out of `workspace` (device memory, >= vc_text_workspace_bytes, 256-B aligned, the caller's while encode calls follow), fills
 * the residual gate of ones and - T5, with relative_attention_bias bound - builds the bias table with vc_t5_position_bias: once per
 * prepare, not per prompt.  The handle serves ONE prepared (L, workspace) at a time; preparing another and coming back keeps the
 * captured plans of both.  A workspace that is too small is VC_ERR_ARG and nothing is launched.  The fills are asynchronous on
 * `stream`: an encode on ANOTHER stream must be ordered behind them by the caller. */
int vc_text_prepare(void* handle, int32_t L, void* workspace, int64_t workspace_bytes, void* stream);
/* ids: DEVICE int32 [n_prompts][L].  hidden: [n_prompts][L][d_model] bf16 or NULL.  pooled: CLIP [n_prompts][d_model] bf16 or NULL; T5:
 * must be NULL (VC_ERR_ARG); hidden and pooled both NULL is VC_ERR_ARG.  An unbound tensor is VC_ERR_STATE naming the first missing key,
 * a call before vc_text_prepare is VC_ERR_STATE; all of that is checked before anything is launched.  Per prompt: the ids are copied
 * into the resident buffer, the plan runs, the results are copied out.  With a stream the plan is ONE hipGraph launch - a chain of
 * kernel nodes over workspace-resident buffers, the copies stay outside it - captured on first use per (workspace, L, stream) after one
 * un-captured run that sets the kernels' attributes, and kept in a list of 8, most recently used first: rotating ids / hidden / pooled
 * pointers never re-captures.  stream == NULL runs the same launches un-captured on the default stream. */
int vc_text_encode(void* handle, const int32_t* ids, int32_t n_prompts, void* hidden, void* pooled, void* stream);
/* captured plans the handle holds (0..8); -1 for a null handle */
int vc_text_plan_count(void* handle);

/* ---- the grid: the host rules, the pixel epilogue and the handle that turn the pieces above into images ----
 * Added WITHOUT a change of VC_ABI_VERSION (tests pin 11): detect these entry points by SYMBOL - look up vc_grid_create.
 *
 * HOST RULES (no device, like vc_solver_evals).
 * vc_time_grid: the solver's n_points time points, F32, bit for bit what the pipeline's sampler builds (ode.__init__ + ode.sample,
 *   transport/integrators.py:99-101,113-116; time_shift of transport/utils.py:33-39), every step rounded as torch rounds it:
 *     1. torch.linspace(t0, t1, n_points) in f32: step = (f32(t1) - f32(t0)) / (n_points - 1); point i < n_points / 2 is
 *        fma(step, i, f32(t0)), every other point fma(-step, n_points - 1 - i, f32(t1)) - the two-sided formula, each point ONE
 *        fused multiply-add, as torch's kernel evaluates it;
 *     2. time_shifting_factor f != 0:  t <- t / ((t + f32(f)) - f32(f) * t), four f32 operations;
 *     3. do_shift != 0:  mu = m * n_tokens + b in double with m = (1.15 - 0.5) / (4096 - 256), b = 0.5 - m * 256 (get_lin_function),
 *        E = f32(exp(mu)), and per point u = 1 - t; r = (1 / u) - 1; t <- 1 - (1 / (E + r)) * E, all f32 - torch divides a number by
 *        a tensor as reciprocal times number.  The endpoints pass through inf arithmetic to exactly 0 and 1.
 *   Apart from the fused multiply-adds of step 1 nothing is contracted.  n_points < 2, n_tokens < 1, t0 >= t1, a non-finite
 *   t0 / t1 / time_shifting_factor or a null `out` is VC_ERR_ARG.
 * vc_grid_tokens: the image tokens of a sample of `rows` grid rows with LATENT sizes lat_h[i] x lat_w[i] (even, positive):
 *   sum (lat_h[i] / 2) * (lat_w[i] / 2); VC_ERR_ARG (negative) for rows < 1, a null pointer or an odd / non-positive size.
 * vc_grid_img_ids: out HOST [vc_grid_tokens][3] F32 = the img_ids of prepare_modified (models/sampling.py:56-59) for that sample:
 *   per row j, in token order (y outer, x inner): (j + 1, y, x).  What VcFluxInputs.img_ids takes for B = 1. */
int vc_time_grid(int32_t n_points, int32_t n_tokens, double t0, double t1, int32_t do_shift, double time_shifting_factor, float* out);
int64_t vc_grid_tokens(int32_t rows, const int32_t* lat_h, const int32_t* lat_w);
int vc_grid_img_ids(int32_t rows, const int32_t* lat_h, const int32_t* lat_w, float* out);

/* PIXELS OUT: the last step of both stages (visualcloze.py:238-240,430-432 and to_pil_image of :437-439) in one launch.
 * img [3, H, W] bf16 (or F32 with img_is_f32) is the VAE's decoded image in [-1, 1]; the column window [x0, x0 + w) of it - the crop
 * of cell i of a row of grid_w cells is x0 = i * W / grid_w (:452,461) - leaves as
 *   VC_PIXELS_F32: out F32 [3, H, w],  v = clamp((f32(img) + 1) / 2, 0, 1)         ((img.float() + 1.0) / 2.0).clamp_(0.0, 1.0)
 *   VC_PIXELS_U8:  out 8-bit [H, w, 3], (uint8)(v * 255), TRUNCATING               (pic.mul(255).byte() of torchvision's to_pil_image)
 * bit for bit the torch expressions (the sum and the product are rounded separately, nothing is contracted; a NaN stays a NaN in the
 * F32 form).  16-byte accesses when x0, w and W are multiples of 16 and both bases are 16-byte aligned; anything else runs
 * element-wise with the same results.  0 < H, W < 65536, 0 <= x0, 1 <= w, x0 + w <= W; out must not overlap img; violations and null
 * pointers are VC_ERR_ARG, checked before the device is touched. */
#define VC_PIXELS_F32 0
#define VC_PIXELS_U8 1
int vc_pixels_out(const void* img, int32_t img_is_f32, int32_t H, int32_t W, int32_t x0, int32_t w, void* out, int32_t out_form,
                  void* stream);

/* IMAGE COMPARE: how far two renderings of equal geometry C x H x W lie apart - error sums, PSNR and the mean SSIM of Wang, Bovik,
 * Sheikh, Simoncelli 2004 - computed on the device, deterministically, on what vc_pixels_out writes.  The reference has nothing like
 * it; the rule below is this library's own.  Added WITHOUT a change of VC_ABI_VERSION (tests pin 11): detect by SYMBOL (look up
 * vc_image_compare); vc_image_struct_sizes reports sizeof(VcImageMetrics).
 * form names the storage of BOTH images and the data range L:
 *   VC_IMG_U8_HWC   8-bit [H, W, C], element (c, y, x) at (y * W + x) * C + c, value v = F32(byte) (exact), L = 255
 *   VC_IMG_F32_CHW  F32 [C, H, W], element (c, y, x) at (c * H + y) * W + x, value as stored, meant to lie in [0, 1], L = 1
 * ERROR SUMS over all n = C * H * W elements: d = a - b (F32, exact for bytes), sse = sum d * d, max_abs = max |d|, n_diff = the
 *   number of elements with a != b.  8-bit form: sse_u64, max_abs, n_diff are exact integers (255^2 * n passes 2^32 at 66052
 *   elements, so the sum is carried in 64 bits) and sse_f32 = F32(sse_u64).  F32 form: sse_u64 = 0 and sse_f32 is a fixed-order F32
 *   sum (below); a NaN difference counts in n_diff, makes sse_f32 NaN and is skipped by max_abs.
 * PSNR: vc_image_psnr - a HOST function on a copied-back VcImageMetrics - stores, in double, 10 * log10(L^2 * n / sse) with sse =
 *   sse_u64 (8-bit form) or sse_f32 (F32 form); sse == 0 gives +inf; a NULL argument is VC_ERR_ARG.  The device never computes it.
 * MEAN SSIM: the window is the 11 x 11 Gaussian with sigma = 1.5, applied separably; the eleven one-dimensional weights are
 *   exp(-(k - 5)^2 / 4.5), k = 0 .. 10, normalised in double to sum 1 and rounded to F32 ONCE - VC_SSIM_WEIGHTS below.  Only VALID
 *   positions count: window (c, y, x), 0 <= y < H - 10, 0 <= x < W - 10, covers rows y .. y + 10 and columns x .. x + 10 of channel c;
 *   no padding; n_windows = C * (H - 10) * (W - 10).  All arithmetic is F32, one operation after the other, every operation rounded
 *   on its own (no fused multiply-add), in this order:
 *     five planes  p in { a, b, F32(a * a), F32(b * b), F32(a * b) }
 *     horizontal   h_p(r, x) = sum over k = 0 .. 10, ascending, of w[k] * p(r, x + k):  s = w[0] * p(r, x);  s = s + w[k] * p(r, x + k)
 *     vertical     m_p(y, x) = sum over j = 0 .. 10, ascending, of w[j] * h_p(y + j, x), the same way
 *                  -> mu_a, mu_b, e_aa, e_bb, e_ab
 *     ma2 = mu_a * mu_a;  mb2 = mu_b * mu_b;  mab = mu_a * mu_b;   va = e_aa - ma2;  vb = e_bb - mb2;  cab = e_ab - mab
 *     n1 = (mab + mab) + C1;  n2 = (cab + cab) + C2;  d1 = (ma2 + mb2) + C1;  d2 = (va + vb) + C2
 *     ssim = (n1 * n2) / (d1 * d2)                      the division correctly rounded
 *   C1 = F32((0.01 * L)^2), C2 = F32((0.03 * L)^2), the squares taken in double.  Every step is symmetric in (a, b) - products and
 *   sums of two values commute - so swapping the operands gives the same bits; and with a == b numerator and denominator are formed
 *   by the same operations on equal values (mab == ma2 == mb2, cab == va == vb bit for bit), so every window gives exactly 1.0f.
 *   ssim_mean = F32(S / n_windows) with S the sum below, the division in double.
 * TILES AND THE ORDER OF THE SUMS (VC_IMG_TILE = 32; nothing else about the launch enters the result): channel c is cut into tiles of
 *   32 x 32 WINDOWS, tile (c, ty, tx) holding windows y in [32 ty, 32 ty + 32), x in [32 tx, 32 tx + 32) inside the valid range;
 *   TY = ceil((H - 10) / 32), TX = ceil((W - 10) / 32); its index is p = (c * TY + ty) * TX + tx.  One workgroup of 256 threads per
 *   tile.  Thread t owns column x = t % 32 and rows y = t / 32 + 8 i, i = 0 .. 3, of the tile: it adds the ssim of its valid windows
 *   in ascending i, starting from 0.  The ERROR SUMS of a tile run over its share of PIXELS: the tile's halo is the 42 x 42 pixels
 *   its windows cover; the tile owns halo rows r < 32, or ALL its halo rows inside the image if ty = TY - 1, and likewise columns -
 *   every pixel of the channel belongs to exactly one tile.  Thread t visits halo positions q = t + 256 i, i = 0 .. 6 (row q / 42,
 *   column q % 42) in ascending i and takes the owned ones: s = s + d * d (F32 form), exact integers (8-bit form).  The 256 thread
 *   values of a tile go through a tree, l[t] = l[t] (op) l[t + o], o = 128, 64, .., 1 (op: F32 add, integer add, max), and make the
 *   tile's record.  A second launch of ONE workgroup folds the P = C * TY * TX records: thread t adds records t, t + 256, .. in
 *   ascending order, then the same tree - the ssim sums and the F32 sse in DOUBLE (rounded to F32 once, at the end), the integers in
 *   64 bits.  No atomics: repeated runs give the same bits.  Rows are fetched with 16-byte loads where W % 16 == 0 and both bases
 *   are 16-byte aligned (and C == 3 for the 8-bit form), element-wise otherwise; the choice is made on the host and the values that
 *   reach the arithmetic are the same, so are the bits.
 * vc_image_compare_scratch_bytes: HOST only; bytes = P * VC_IMG_RECORD_BYTES.  vc_image_compare: a, b, out_dev, scratch are DEVICE
 *   pointers, nothing is allocated, nothing is read back: two launches on `stream`, legal under stream capture.  a and b may be the
 *   same buffer.  VC_ERR_ARG with a message, before the device is touched: a null pointer; an unknown form; C outside 1 .. 65535;
 *   H or W outside 11 .. 65535 (a window needs 11 rows and 11 columns); an F32 image not aligned to 4 bytes; out_dev or scratch not
 *   aligned to 16 bytes; scratch_bytes smaller than vc_image_compare_scratch_bytes answers. */
#define VC_IMG_U8_HWC 0
#define VC_IMG_F32_CHW 1
#define VC_IMG_TILE 32
#define VC_IMG_RECORD_BYTES 32
#define VC_SSIM_WEIGHTS { 0.00102838012f, 0.00759875821f, 0.0360007733f, 0.109360687f, 0.213005543f, 0.266011715f, \
                          0.213005543f, 0.109360687f, 0.0360007733f, 0.00759875821f, 0.00102838012f }
typedef struct VcImageMetrics {
  uint64_t n;                                /* C * H * W */
  uint64_t n_windows;                        /* C * (H - 10) * (W - 10) */
  uint64_t sse_u64;                          /* 8-bit form: exact; F32 form: 0 */
  uint64_t n_diff;
  float sse_f32;                             /* F32 form: the fixed-order sum; 8-bit form: F32(sse_u64) */
  float max_abs;
  float ssim_mean;
  int32_t form;
} VcImageMetrics;                            /* 48 bytes */
/* sizeof(VcImageMetrics) as this library was compiled */
void vc_image_struct_sizes(int32_t out[1]);
int vc_image_compare_scratch_bytes(int32_t C, int32_t H, int32_t W, int64_t* bytes);
int vc_image_compare(const void* a, const void* b, int32_t form, int32_t C, int32_t H, int32_t W, VcImageMetrics* out_dev, void* scratch,
                     int64_t scratch_bytes, void* stream);
int vc_image_psnr(const VcImageMetrics* m, double* psnr_db);

/* THE HANDLE: VisualClozeModel.process_images' tensor path (visualcloze.py:363-434) and `upsampling`'s (:184-240) as ONE call each,
 * composed of the entry points above in the order visualcloze_amd/pipeline.py composes them (generate_grid with
 * rng = NoiseStream(seed); upsample_images): the same kernels on the same operands, so the same bits.  The handle BORROWS its four
 * sub-handles (it never destroys them; they must outlive it, with their weights bound): whatever is set on the Flux handle - LoRA
 * mode and scale, taps, the step cache, true CFG (leave it off: the grid runs B = 1) - acts as it does in vc_flux_sample_ode.  It
 * prepares the sub-handles inside ITS workspace on every call: a caller who also drives a sub-handle directly prepares that one again
 * afterwards.  Image decoding, prefix stripping and tokenisation stay host work; resizing does not (the photo front end below takes
 * 8-bit images).  Needs an autoencoder of 8x reduction (n_ch_mult 4) with 4 * z_channels == the Flux out_channels and
 * in_channels - out_channels == 4 * z_channels + 256, a T5 of d_model == context_in_dim and a CLIP of d_model == vec_in_dim
 * (VC_ERR_ARG from vc_grid_create otherwise).  One handle per device; not thread-safe; one stream at a time. */
#define VC_GRID_MAX_ROWS 16
#define VC_GRID_SDEDIT_CHUNK 4   /* samples per solve of vc_grid_sdedit: the per-GPU batch limit the pipeline runs the Flux handle with */
typedef struct VcGridConfig {
  void* flux;   /* vc_flux_create */
  void* vae;    /* vc_vae_create */
  void* t5;     /* vc_text_create, VC_TEXT_T5 */
  void* clip;   /* vc_text_create, VC_TEXT_CLIP */
} VcGridConfig;
typedef struct VcGridJob {
  int32_t rows;                              /* 1..VC_GRID_MAX_ROWS grid rows */
  int32_t pixels_is_f32;                     /* the row pixels are F32 instead of bf16 */
  int32_t height[VC_GRID_MAX_ROWS];          /* per row, pixels: multiples of 16 */
  int32_t width[VC_GRID_MAX_ROWS];
  const void* pixels[VC_GRID_MAX_ROWS];      /* per row, device [3, H, W] in [-1, 1]: the images of the row side by side */
  const void* masks[VC_GRID_MAX_ROWS];       /* per row, device bf16 [H, W]: the pixel fill mask, 1 = generate */
  int32_t decode[VC_GRID_MAX_ROWS];          /* != 0: this row is decoded into out_rows[row] */
  const int32_t* t5_ids;                     /* HOST [t5_len]; t5_len a multiple of 64 (the pipeline pads to 512) */
  const int32_t* clip_ids;                   /* HOST [clip_len] */
  int32_t t5_len, clip_len;
  uint64_t seed, noise_offset;               /* the library's noise stream (vc_randn): every draw of the job, in the reference's order -
                                                per row the DiagonalGaussian draw of its encode (z_channels * H/8 * W/8 elements,
                                                autoencoder.py:272), then per row the start noise (:394-399), each a contiguous stretch */
  uint64_t* noise_offset_out;                /* HOST or NULL: receives the stream position behind the last draw */
  float guidance;                            /* rounded to bf16 as visualcloze.py:413 holds it */
  int32_t n_points;                          /* the pipeline's "steps": time POINTS of the solver, >= 2 */
  int32_t method;                            /* VC_SOLVER_* */
  int32_t out_form;                          /* VC_PIXELS_F32 or VC_PIXELS_U8 */
  int32_t max_evals;                         /* model evaluations the workspace is sized for; 0 = what this job needs,
                                                (n_points - 1) * vc_solver_evals(method) */
  int32_t _pad;
  double time_shifting_factor;               /* 0 = none; the pipeline's default is 1 */
} VcGridJob;
typedef struct VcGridSdedit {                /* `upsampling` for `count` targets of ONE size and prompt, refined together */
  int32_t count;                             /* 1..VC_GRID_MAX_ROWS targets */
  int32_t pixels_is_f32;
  int32_t height, width;                     /* multiples of 16: the FINAL size - the images arrive resized */
  const void* pixels[VC_GRID_MAX_ROWS];      /* per target, device [3, H, W] in [-1, 1] */
  const int32_t* t5_ids;                     /* HOST: the content prompt */
  const int32_t* clip_ids;
  int32_t t5_len, clip_len;
  uint64_t seed, noise_offset;               /* per target: the draw of encode(image), of encode(blank), the start noise (:200-217) */
  uint64_t* noise_offset_out;
  float guidance;
  int32_t n_points, method, out_form, max_evals;
  int32_t _pad;
  double strength;                           /* (0, 1): the un-shifted grid runs from t0 = strength; >= 1 returns the input converted */
} VcGridSdedit;
/* sizeof(VcGridConfig), sizeof(VcGridJob), sizeof(VcGridSdedit) as this library was compiled */
void vc_grid_struct_sizes(int32_t out[3]);
/* host-only */
int vc_grid_create(const VcGridConfig* cfg, void** handle);
int vc_grid_destroy(void* handle);
/* The noise source of the handle's jobs.  VC_NOISE_OWN (the default): seed / noise_offset / noise_offset_out of VcGridJob,
 * VcGridSdedit, VcGridPhotos and VcGridSdeditU8 are the library's own stream, as their comments say.  VC_NOISE_TORCH: they are the
 * torch generator's seed and Philox offset (a multiple of 4), and every draw of vc_grid_generate, vc_grid_sdedit,
 * vc_grid_generate_photos and vc_grid_sdedit_u8 is the draw of THE TORCH STREAM (vc_randn_torch VC_RNG_BF16, vc_randn_torch_tokens)
 * in the same order, the offset advancing per draw as torch's does: the parity twin is pipeline.generate_grid / upsample_images with
 * rng = TorchNoiseStream(seed).  sm_count / threads_per_sm as in vc_randn_torch (0 = the device's, read when a job runs).  No struct
 * changes; added WITHOUT a change of VC_ABI_VERSION: look up vc_randn_torch.  Host-only.  VC_ERR_ARG: null handle, unknown source,
 * sm_count < 0, threads_per_sm in 1 .. 255. */
#define VC_NOISE_OWN 0
#define VC_NOISE_TORCH 1
int vc_grid_set_noise(void* handle, int32_t source, int32_t sm_count, int32_t threads_per_sm);
/* The bytes vc_grid_generate (vc_grid_sdedit) needs for this job: the sub-handles' own *_workspace_bytes (the autoencoder at the
 * job's largest row, both halves; T5 and CLIP at the ids' lengths; Flux at B = 1 - the sdedit job: min(count, VC_GRID_SDEDIT_CHUNK) -
 * and max_evals) plus the intermediates (cond, the state, the prompt embeddings, staged pixels).  Host-only; the job is checked as
 * the run checks it. */
int vc_grid_workspace_bytes(void* handle, const VcGridJob* job, int64_t* bytes);
int vc_grid_sdedit_workspace_bytes(void* handle, const VcGridSdedit* job, int64_t* bytes);
/* out_rows HOST [rows] of device pointers: out_rows[i] receives row i ([3, H, W] F32 or [H, W, 3] 8-bit) where decode[i] != 0; the
 * other entries are not read.  workspace: device memory, 256-B aligned, >= vc_grid_workspace_bytes, the caller's during the call -
 * and, kept between calls, what lets the sub-handles' captured plans serve again: a second job of the same geometry in the same
 * workspace captures nothing (each row's encode and each decoded row's decode is one plan of the autoencoder's list of 8).
 * Every argument error - a null handle or pointer, rows or count outside 1..VC_GRID_MAX_ROWS, a size that is no multiple of 16,
 * n_points < 2, an unknown method or out_form, (n_points - 1) * vc_solver_evals(method) > max_evals, a workspace that is too small
 * or misaligned, ids' lengths the encoders refuse, a draw that leaves the 64-bit stream - is VC_ERR_ARG with a message, found
 * before the device is touched. */
int vc_grid_generate(void* handle, const VcGridJob* job, void* workspace, int64_t workspace_bytes, void* const* out_rows, void* stream);
/* out_images HOST [count] of device pointers, each [3, H, W] F32 or [H, W, 3] 8-bit.  Per target, in the reference's order:
 * encode(image), encode(blank) - a zero image - and the start noise; vc_sdedit_mix; cond = the blank latent and an all-ones mask;
 * the grid vc_time_grid(n_points, tokens, strength, 1, 0, 1.0); one batched solve per VC_GRID_SDEDIT_CHUNK targets; decode;
 * vc_pixels_out.  strength >= 1: the input pixels converted, nothing drawn (visualcloze.py:180-181). */
int vc_grid_sdedit(void* handle, const VcGridSdedit* job, void* workspace, int64_t workspace_bytes, void* const* out_images, void* stream);

/* ---- the photo front end: 8-bit photographs in.  Resampling, pixels in, the size rules and two more calls of the grid handle ----
 * Added WITHOUT a change of VC_ABI_VERSION (tests pin 11): detect these entry points by SYMBOL - look up vc_resample_u8.
 *
 * RESAMPLING.  vc_resample_u8 resizes an 8-bit image src [H, W, 3] to dst [h, w, 3] with a separable filter in fixed point.  The
 * rule is the library's own and is stated here in full; it is the rule Pillow's Image.resize applies to 8-bit images, so the bytes
 * are Pillow's (the tests hold the tables to PIL.Image.resize byte for byte).  Per axis - horizontal first, then vertical, with an
 * 8-BIT intermediate [H, w, 3]; an axis whose size does not change is skipped, and if neither changes dst is a copy of src - with
 * `in` and `out` the sizes along the axis, everything in double:
 *     scale = in / out;   fs = max(scale, 1);   support = S * fs,  S = 2 (VC_FILTER_BICUBIC) or 3 (VC_FILTER_LANCZOS)
 *     for the output index xx:   c = (xx + 0.5) * scale
 *         xmin = max((int)(c - support + 0.5), 0);    len = min((int)(c + support + 0.5), in) - xmin
 *         k[x] = f((x + xmin - c + 0.5) * (1 / fs))   for x < len, then divided by their sum (summed in index order; a sum of 0
 *                                                     leaves them as they are)
 *         ki[x] = (int)(0.5 + k[x] * 2^22) for k[x] >= 0, (int)(-0.5 + k[x] * 2^22) otherwise
 *     bicubic, a = -0.5:  f(x) = ((a + 2)|x| - (a + 3)) x^2 + 1 for |x| < 1,  (((|x| - 5)|x| + 8)|x| - 4) a for |x| < 2,  else 0
 *     Lanczos:            f(x) = sinc(x) sinc(x / 3) for -3 <= x < 3, else 0;  sinc(0) = 1, sinc(x) = sin(pi x) / (pi x)
 *     output byte = clip to 0..255 of (2^21 + sum over x < len of pixel[xmin + x] * ki[x]) >> 22   (int32, arithmetic shift)
 * The tables hold kmax = (int)ceil(support) * 2 + 1 weights per output index (vc_resample_kmax); entries from len on are 0.
 *
 * vc_resample_kmax, vc_resample_coeffs, vc_resample_tmp_bytes are HOST-ONLY (no device, like vc_solver_evals).  vc_resample_coeffs
 * fills xmin[out], len[out], ki[out][kmax] for one axis; kmax must be vc_resample_kmax's value.  vc_resample_tmp_bytes is the size
 * of the device scratch `tmp` of vc_resample_u8 (the two axes' tables and the intermediate; 256-B aligned, never 0); it returns a
 * negative VC_ERR_ARG on bad arguments.  vc_resample_u8 builds the tables on the host, stages them through pinned memory and
 * uploads them on `stream` ahead of its (at most two) kernels; because of that upload it cannot be captured into a graph.  Sizes
 * outside 1..65535, an unknown filter, a null pointer, overlap of src, dst and tmp or a tmp that is too small or misaligned are
 * VC_ERR_ARG, found before the device is touched. */
#define VC_FILTER_BICUBIC 0
#define VC_FILTER_LANCZOS 1
int vc_resample_kmax(int32_t in, int32_t out, int32_t filter);
int vc_resample_coeffs(int32_t in, int32_t out, int32_t filter, int32_t* xmin, int32_t* len, int32_t* ki, int32_t kmax);
int64_t vc_resample_tmp_bytes(int32_t H, int32_t W, int32_t h, int32_t w, int32_t filter);
int vc_resample_u8(const void* src, int32_t H, int32_t W, void* dst, int32_t h, int32_t w, int32_t filter, void* tmp, int64_t tmp_bytes,
                   void* stream);

/* PIXELS IN: the inverse of vc_pixels_out.  src 8-bit [H, W, 3]; the crop window of h x w pixels whose corner is (left, top) may
 * reach OUTSIDE the image, where it reads 0 (Image.crop); it is written to the columns [x0, x0 + w) of the row tensor out
 * [3, h, Wrow], bf16 (or F32 with out_is_f32), as ToTensor and Normalize(0.5, 0.5) give it (visualcloze.py:133-137):
 *     v = (f32(byte) / 255 - 0.5) / 0.5      a true division, each operation rounded in f32, nothing contracted; then, for the
 *                                            bf16 form, rounded to nearest even (:377)
 * src == NULL (H, W, left, top ignored) writes the blank cell: byte 0, v = -1.  vc_mask_fill sets the same window of the row's
 * bf16 pixel mask [h, Wrow] to value = 0 or 1 (:369-374).  1 <= h, Wrow <= 65535, 0 <= x0, 1 <= w, x0 + w <= Wrow, image sizes in
 * 1..65535, |left|, |top| <= 65535; violations, a null out / mask, a misaligned base, out overlapping src are VC_ERR_ARG, found
 * before the device is touched. */
int vc_pixels_in(const void* src, int32_t H, int32_t W, int32_t left, int32_t top, void* out, int32_t out_is_f32, int32_t h,
                 int32_t Wrow, int32_t x0, int32_t w, void* stream);
int vc_mask_fill(void* mask, int32_t h, int32_t Wrow, int32_t x0, int32_t w, int32_t value, void* stream);

/* SIZE RULES (HOST-ONLY): what visualcloze.py:28-75,298-360,166-180 compute with Python floats and ints, restated in double with
 * truncation by (int) and floor division where Python floors.
 * vc_fit_size: the size an image of w x h is fitted to at `resolution` R:  ar = w / h;  nh = (int)pow(R * R / ar, 0.5);
 *   nw = (int)(nh * ar);  both then max(n / 16, 1) * 16.
 * vc_grid_layout: the plan of every cell of a grid of grid_h x grid_w cells, row-major; cell_w[i] = cell_h[i] = 0 marks an absent
 *   image.  A row's reference size is the fitted size of its first present image.  A present cell is resized with
 *   VC_FILTER_LANCZOS to its fitted size (fit_w x fit_h), then with VC_FILTER_BICUBIC to cover_w x cover_h - fit_w <= fit_h:
 *   (ref_w, (int)(ref_w / fit_w * fit_h)), else ((int)(ref_h / fit_h * fit_w), ref_h) - and centre-cropped to the reference size
 *   at (crop_left, crop_top) = floor((cover - ref) / 2), NEGATIVE when the image is smaller than the reference size (the window
 *   then reaches outside, which reads 0).  An absent cell is black at the reference size - resolution x resolution in a row
 *   without any image - and carries mask = 1; above the last row it is VC_ERR_ARG.  cell_w x cell_h is the size after the crop.
 *   If the grid has more than one column and more than one cell is masked, every cell is resized once more (bicubic) to
 *   final_w x final_h, in cell order with a running width:  new_w starts at the last row's reference width (384 if it has none);
 *   per cell new_h = (int)(cell_h * (new_w / cell_w)), new_w = (int)(new_w / 16) * 16, new_h = (int)(new_h / 16) * 16.  Otherwise
 *   final = cell.  A size that leaves 1..65535 is VC_ERR_ARG; so is a row whose cells differ in final height (they would not
 *   make one row tensor) or width (the reference sizes every cell's mask by the row's first cell).
 * vc_upsampling_size: the size the cells are refined at, from the size of the last row's first image (0, 0 = none: 1024 x 1024):
 *   above 1024^2 pixels  ar = w / h;  h = (int)pow(1024 * 1024 / ar, 0.5);  w = (int)(h * ar);  then both / 16 * 16. */
typedef struct VcCellPlan {
  int32_t present;                 /* 0: an absent image (black, masked) */
  int32_t fit_w, fit_h;            /* VC_FILTER_LANCZOS target */
  int32_t cover_w, cover_h;        /* VC_FILTER_BICUBIC target */
  int32_t crop_left, crop_top;     /* corner of the centre crop inside cover_w x cover_h; may be negative */
  int32_t cell_w, cell_h;          /* the cropped cell = the row's reference size */
  int32_t final_w, final_h;        /* after the second bicubic pass; = cell_w x cell_h where there is none */
  int32_t mask;                    /* 1: this cell is generated */
} VcCellPlan;
int vc_fit_size(int32_t w, int32_t h, int32_t resolution, int32_t* nw, int32_t* nh);
int vc_grid_layout(int32_t grid_h, int32_t grid_w, const int32_t* cell_w, const int32_t* cell_h, int32_t resolution, VcCellPlan* out);
int vc_upsampling_size(int32_t orig_w, int32_t orig_h, int32_t* w, int32_t* h);

/* THE GRID HANDLE FROM PHOTOGRAPHS.  Two calls over vc_grid_generate and vc_grid_sdedit; they add no model work of their own.
 * vc_grid_generate_photos: per cell a device 8-bit [H, W, 3] image or NULL; it runs vc_grid_layout, the resamples, vc_pixels_in and
 *   vc_mask_fill into row tensors and masks in the FRONT part of its workspace, then exactly vc_grid_generate on the rest (same
 *   noise stream, same outputs, same errors).  Rows must come to multiples of 16 pixels.
 * vc_grid_sdedit_u8: `count` 8-bit cells [cell_h, cell_w, 3] of one size - what vc_pixels_out with VC_PIXELS_U8 and a cell's column
 *   window writes - resized (bicubic) to height x width (vc_upsampling_size) and passed through vc_pixels_in, then exactly
 *   vc_grid_sdedit.  strength >= 1: out_images receive the RESIZED 8-bit images (visualcloze.py:180-182), out_form must be
 *   VC_PIXELS_U8, nothing is drawn.
 * The workspace is kept between calls as for vc_grid_generate: a second job of the same geometry captures nothing.  Argument errors
 * are VC_ERR_ARG with a message, found before the device is touched. */
typedef struct VcGridPhotos {
  int32_t grid_h, grid_w;                    /* 1..VC_GRID_MAX_ROWS each */
  int32_t resolution;                        /* the reference's default is 384 */
  int32_t out_form;                          /* VC_PIXELS_F32 or VC_PIXELS_U8 */
  const void* const* images;                 /* HOST [grid_h * grid_w], row-major: device 8-bit [H, W, 3], or NULL = absent */
  const int32_t* width;                      /* HOST [grid_h * grid_w]; not read where the image is NULL */
  const int32_t* height;
  int32_t decode[VC_GRID_MAX_ROWS];          /* as VcGridJob */
  const int32_t* t5_ids;
  const int32_t* clip_ids;
  int32_t t5_len, clip_len;
  uint64_t seed, noise_offset;
  uint64_t* noise_offset_out;
  float guidance;
  int32_t n_points, method, max_evals;
  double time_shifting_factor;
} VcGridPhotos;
typedef struct VcGridSdeditU8 {
  int32_t count;                             /* 1..VC_GRID_MAX_ROWS cells */
  int32_t cell_h, cell_w;                    /* the size of every cell */
  int32_t height, width;                     /* the target: multiples of 16 */
  int32_t out_form;
  const void* pixels[VC_GRID_MAX_ROWS];      /* per cell, device 8-bit [cell_h, cell_w, 3] */
  const int32_t* t5_ids;                     /* as VcGridSdedit from here on */
  const int32_t* clip_ids;
  int32_t t5_len, clip_len;
  uint64_t seed, noise_offset;
  uint64_t* noise_offset_out;
  float guidance;
  int32_t n_points, method, max_evals;
  double strength;
} VcGridSdeditU8;
/* sizeof(VcCellPlan), sizeof(VcGridPhotos), sizeof(VcGridSdeditU8) as this library was compiled */
void vc_photo_struct_sizes(int32_t out[3]);
int vc_grid_photos_workspace_bytes(void* handle, const VcGridPhotos* job, int64_t* bytes);
int vc_grid_sdedit_u8_workspace_bytes(void* handle, const VcGridSdeditU8* job, int64_t* bytes);
int vc_grid_generate_photos(void* handle, const VcGridPhotos* job, void* workspace, int64_t workspace_bytes, void* const* out_rows,
                            void* stream);
int vc_grid_sdedit_u8(void* handle, const VcGridSdeditU8* job, void* workspace, int64_t workspace_bytes, void* const* out_images,
                      void* stream);

/* ---- hipGraph helpers: capture the launches issued on `stream` between begin/end ---- */
int vc_stream_create(void** stream);
int vc_stream_destroy(void* stream);
int vc_stream_sync(void* stream);
int vc_graph_begin(void* stream);
int vc_graph_end(void* stream, void** graph_exec);
int vc_graph_launch(void* graph_exec, void* stream);
int vc_graph_destroy(void* graph_exec);

/* ---- timing on the launch stream (HIP events), for bench.py's roofline leg ---- */
int vc_event_create(void** ev);
int vc_event_record(void* ev, void* stream);
int vc_event_elapsed_ms(void* ev_start, void* ev_stop, float* ms); /* synchronises on ev_stop */
int vc_event_destroy(void* ev);

#ifdef __cplusplus
}
#endif
#endif
