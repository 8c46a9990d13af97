// The launch planner of vc_attention: everything that DECIDES (argument checks, the variant word, kernel family and template,
// grids, the tail-split rules, the scratch layout, the by-size variant rule) and nothing that launches.  Host code only, a pure
// function of sizes, strides, the variant word, logit_bound, q_prescaled, split, scratch_bytes, which pointers are null, and the
// CU count: attn_plan.hip makes no HIP call and dereferences no pointer, and vc_attention_plan answers without a GPU.
// attention.hip / attention64.hip hold the kernels and turn a plan into launches.
#pragma once
#include "../../include/vcloze_hip.h"

namespace vcplan {

// ---- byte constants of the kernels' LDS images and partial results (the kernel files use them from here) ----
constexpr int KVB = 64;                               // keys per tile
constexpr int K_TILE = KVB * 256, V_TILE = 128 * KVB * 2;      // bytes
constexpr int LDS32 = 2 * (K_TILE + V_TILE);          // 32 queries per wave: a double-buffered ring
constexpr int RING = 3;
constexpr int LDS64 = RING * (K_TILE + V_TILE);       // 64 queries per wave: 48 KB of K ring, then 48 KB of V^T ring
constexpr int QW = 64;                                // attention64: queries per wave
constexpr int QB = 4 * QW;                            //              queries per work item
// attention.hip, one partial result: [wave 4][16 groups][lane 64][4] f32 accumulator fragments in register order, then
// [wave 4][lane 64] (m, l) pairs; every store / load is 16 B (8 B) per lane, lane-contiguous
constexpr int PART_O = 4 * 16 * 64 * 4;               // floats
constexpr int PART_FLOATS = PART_O + 4 * 64 * 2;
// attention64.hip, one partial result of the tail split: O^T fragments NORMALISED by the piece's own row sums, as f16 (11-bit
// mantissa: 8x finer than the bf16 output; values are convex combinations of V) [wave 4][qb 2][16 groups][lane 64][4 x f16],
// then [wave 4][qb 2][lane 64] (m, l) in f32.  Half the bytes of f32 accumulators: the pieces are written once and read
// once through the Infinity Cache, 17 MB each way at cfg 2.
constexpr int PART64_O_BYTES = 4 * 2 * 16 * 64 * 8;
constexpr int PART64_BYTES = PART64_O_BYTES + 4 * 2 * 64 * 8;

// Work schedule of attention64's persistent grid, PER XCD (grid % 8 == 0; block b runs on XCD b % 8 - observed placement, used
// for speed only).  XCD x owns the contiguous logical items [start, start + n) that xcd_remap gives it: all query blocks of a
// head are neighbours there, so the K / V^T tiles of a head stream through ONE L2.  Its W = grid / 8 workgroups take
// `rounds` whole items each (item start + r * W + slot); the remaining `tail` items are cut along the keys into W equal
// chunks of (item, KV tile) units - inside the SAME XCD, so that the tail round re-reads K / V^T from the L2 that already
// holds them (round 2 cut the tail across the whole grid: every XCD streamed every tail head, 204 MB fetched per launch
// for 73 MB of operands).  ONE definition for the kernels and for the planner's tail-split rule.
struct Sched64 {
  int W, start, n, rounds, tail, units;
};
__host__ __device__ inline __attribute__((always_inline)) Sched64 sched64(int x, int G, int items, int nkt) {
  Sched64 s;
  s.W = G >> 3;
  const int q = items >> 3, r = items & 7;
  s.n = q + (x < r ? 1 : 0);
  s.start = x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q;
  s.rounds = s.n / s.W;
  s.tail = s.n - s.rounds * s.W;
  s.units = s.tail * nkt;
  return s;
}

// the variant word of VcAttention, decoded once (its values: include/vcloze_hip.h)
struct AttnRequest {
  bool wave64;        // bit 8: one wave per SIMD, 64 queries per wave (attention64.hip)
  bool tail_split;    // bit 4: tail items cut along the keys (with 1 and 2 = variant 7; with 8 = 12)
  bool persist;       // bit 2: persistent grid with static item assignment (variants 2, 3)
  bool four_waves;    // bit 1 of the 32-query family: 4 waves x 32 queries instead of 8 x 32
  bool inmerge;       // bit 16: the tail pieces combined inside the launch (stream form only)
};
AttnRequest decode_variant(int variant);

enum AttnFamily { ATTN_32Q_8W = 0, ATTN_32Q_4W = 1, ATTN_64Q_ITEM = 2, ATTN_64Q_STREAM = 3 };
// The plan of one vc_attention call.  full_rounds < 0 = no tail split; merge_grid 0 = no merge launch.
struct AttnPlan {
  int family;                 // AttnFamily: which kernel
  bool bounded;               // attention64: the template without a running max (0 < logit_bound <= 100)
  int grid, threads, lds;     // of the attention kernel; lds = dynamic LDS bytes
  int qblocks, items, full_rounds, tail_items, tail_units;
  bool inmerge;               // 64q stream form: pieces combined in the launch (flag words at flags_offset)
  int merge_grid;             // workgroups of the merge kernel behind the launch
  int64_t flags_offset;       // byte offset of the flag words in the scratch (the layout at this CU count, whatever the call does)
  int64_t scratch_need;       // scratch bytes the call's tail split was granted on (0 = it touches no scratch)
};

int validate_attention(const VcAttention& a, char* err, int errlen);
AttnPlan plan_attention(const VcAttention& a, int n_cu);      // (of validated arguments)
// what vc_attention_plan answers (out layout: include/vcloze_hip.h)
int attention_plan_words(const VcAttention& a, int n_cu, int32_t out[16], char* err, int errlen);

// Scratch layout: [partials of whichever variant runs: the larger of the two layouts][flag words of attention64's in-launch
// combine, zero between launches (VcAttention.variant bit 16): behind everything any other variant writes]
int64_t attention64_scratch_bytes(int n_cu);      // attention64's pieces: two per workgroup
int64_t attention64_flags_bytes(int n_cu);        // [2 pieces per workgroup][2 query blocks] words
int64_t attention_flags_offset(int n_cu);
int64_t attention_scratch_bytes(int n_cu);        // the whole buffer (vc_attention_scratch_bytes)

int attention_variant_by_size(int B, int L, int H, int n_cu);      // the variant the host engines run when none is forced

}  // namespace vcplan
