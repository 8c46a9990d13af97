// The launch planner of vc_attention (see attn_plan.h): host code only, no kernel and no HIP call in this file.
#include <stdio.h>
#include <algorithm>
#include "attn_plan.h"

namespace vcplan {

AttnRequest decode_variant(int variant) {
  return AttnRequest{(variant & 8) != 0, (variant & 4) != 0, (variant & 2) != 0, (variant & 1) != 0, (variant & 16) != 0};
}

int64_t attention64_scratch_bytes(int n_cu) { return (int64_t)n_cu * 2 * PART64_BYTES; }
int64_t attention64_flags_bytes(int n_cu) { return (int64_t)n_cu * 2 * 2 * 4; }
int64_t attention_flags_offset(int n_cu) {
  const int64_t parts = std::max((int64_t)2 * n_cu * 2 * PART_FLOATS * (int64_t)sizeof(float), attention64_scratch_bytes(n_cu));
  return (parts + 255) & ~(int64_t)255;
}
int64_t attention_scratch_bytes(int n_cu) { return attention_flags_offset(n_cu) + ((attention64_flags_bytes(n_cu) + 255) & ~(int64_t)255); }

int attention_variant_by_size(int B, int L, int H, int n_cu) {
  // 28 = 12 + 16: one wave per SIMD, tail split, and - where the stream form of the kernel runs - the tail pieces combined
  // inside the launch (the flag words of ATT_SCRATCH are zeroed by vc_flux_prepare, and only this handle's launches, ordered on
  // one stream, touch it).  Fewer 256-query items than CUs (cfg 1: 168): the same kernel WITHOUT a split (8) - one item per
  // workgroup beats the 32-queries-per-wave kernel down to half the CUs (round 6, cfg 1: 44.6-49.7 vs 56.3-59.4 us per launch
  // in situ; per step +1.7 % on one box, +-0.1 % on another - the q / k norm moves from the pre-pass into the qkv GEMM's
  // epilogue with it; cutting 168 items into 256 short pieces loses 1 %: profiles/r06o_ab_cfg1.log, r06q_ab_cfg1.log)
  const int items = ((L + 255) / 256) * H * B;
  return items >= n_cu ? 28 : 2 * items >= n_cu ? 8 : 3;
}

#define VC_ATTN_FAIL(...) do { snprintf(err, errlen, __VA_ARGS__); return VC_ERR_ARG; } while (0)
int validate_attention(const VcAttention& A, char* err, int errlen) {
  const AttnRequest req = decode_variant(A.variant);
  const int32_t B = A.B, L = A.L, Lpad = A.Lpad, H = A.H;
  const int64_t ld = A.ld, ldo = A.ldo, bstride = A.bstride;
  if (!A.qkv || !A.vt || !A.out) VC_ATTN_FAIL("attention: null pointer");
  if (B <= 0 || L <= 0 || H <= 0) VC_ATTN_FAIL("attention: empty problem B=%d L=%d H=%d", B, L, H);
  if (Lpad < L || Lpad % KVB) VC_ATTN_FAIL("attention: Lpad=%d must be a multiple of %d and >= L=%d", Lpad, KVB, L);
  if (ld % 8 || ldo % 4 || bstride % 8) VC_ATTN_FAIL("attention: strides must keep 16-B row alignment");
  if ((uint64_t)128 * (uint64_t)Lpad >= (1ull << 31)) VC_ATTN_FAIL("attention: Lpad too large");
  if ((uint64_t)(Lpad + KVB) * (uint64_t)ld * 2ull >= (1ull << 32)) VC_ATTN_FAIL("attention: one sample's K rows exceed 32-bit byte offsets (L=%d ld=%ld)", L, (long)ld);
  if (A.q_scale && !req.wave64) VC_ATTN_FAIL("attention: in-kernel QKNorm + RoPE of the queries (q_scale) exists for variants 8 / 12 only");
  if (A.kv_gap && !A.kv_len) VC_ATTN_FAIL("attention: kv_gap needs kv_len");
  if (A.q_scale && !A.rope) VC_ATTN_FAIL("attention: q_scale given without a rope table");
  if (A.q_prescaled && (!req.wave64 || A.q_scale)) VC_ATTN_FAIL("attention: q_prescaled exists for variants 8 / 12 and excludes q_scale");
  // (the 32-queries-per-wave family only: attention64 takes the split with any of its variants)
  if (!req.wave64 && req.tail_split && !(req.four_waves && req.persist)) VC_ATTN_FAIL("attention: the tail split (+4) exists for variant 3 only");
  return VC_OK;
}

// one wave per SIMD, 64 queries per wave (attention64.hip)
static AttnPlan plan_attention64(const VcAttention& A, const AttnRequest& req, int n_cu) {
  AttnPlan p{};
  const int32_t B = A.B, L = A.L, H = A.H;
  // logits bounded by the caller (|x| <= logit_bound in the log2 domain): 2^x, a row's sum over L keys and O stay far inside
  // f32 for bound <= 100, so the softmax needs no running max (kernel header)
  p.bounded = A.logit_bound > 0.0f && A.logit_bound <= 100.0f;
  // bounded logits + prescaled queries (the product's launches wherever this kernel runs): the stream form
  // (its LDS-DMA addresses are kernel-argument base + 32-bit byte offset)
  const bool fits32 = ((uint64_t)B * (uint64_t)A.bstride + (uint64_t)L * (uint64_t)A.ld + 3u * (uint64_t)H * 128u) * 2u < (1ull << 32) &&
                      (uint64_t)B * (uint64_t)H * 128u * (uint64_t)A.Lpad * 2u < (1ull << 32) && L >= 16;
  const bool stream = A.q_prescaled != 0 && !A.q_scale && fits32;
  p.family = stream ? ATTN_64Q_STREAM : ATTN_64Q_ITEM;
  p.threads = 256; p.lds = LDS64;
  p.qblocks = (L + QB - 1) / QB;
  p.items = p.qblocks * H * B;
  p.full_rounds = -1;
  const int G = n_cu;
  const int nkt = (L + KVB - 1) / KVB;
  // the tail split is scheduled per XCD (Sched64): cut where some XCD has tail items and cutting shortens its critical
  // path by more than the merge costs (~4 tiles): plain = one more round of nkt tiles for the workgroups that draw a tail
  // item, split = ceil(tail * nkt / W) tiles for every workgroup of that XCD
  int tail_slots = 0, worst_split = 0;      // tail_slots: the most tail items any XCD has
  if (G % 8 == 0)
    for (int x = 0; x < 8; ++x) {
      const Sched64 sc = sched64(x, G, p.items, nkt);
      tail_slots = std::max(tail_slots, sc.tail);
      worst_split = std::max(worst_split, (int)(((long)sc.tail * nkt + sc.W - 1) / sc.W));
    }
  if (req.tail_split && !A.kv_len && tail_slots > 0 && A.scratch && A.scratch_bytes >= attention64_scratch_bytes(n_cu) && worst_split + 4 < nkt) {
    const bool has_flags = A.scratch_bytes >= attention_scratch_bytes(n_cu);       // the whole buffer, flag words at its end
    p.full_rounds = p.items / G; p.tail_items = p.items - p.full_rounds * G; p.tail_units = p.tail_items * nkt;
    // variant bit 16 (stream form only): the pieces are combined inside the launch - the caller vouches that the flag words at
    // the end of the scratch were zero once and that nothing but these launches, one at a time, touches the scratch
    p.inmerge = stream && req.inmerge && has_flags;
    p.grid = G;
    // 16 blocks (8 XCDs x 2 query blocks) per tail slot that any XCD fills
    p.merge_grid = p.inmerge ? 0 : 16 * tail_slots;
    p.scratch_need = p.inmerge ? attention_scratch_bytes(n_cu) : attention64_scratch_bytes(n_cu);
  } else {
    p.grid = std::min(p.items, G);
  }
  return p;
}

// 32 queries per wave (attention.hip)
static AttnPlan plan_attention32(const VcAttention& A, const AttnRequest& req, int n_cu) {
  AttnPlan p{};
  const int32_t L = A.L;
  p.family = req.four_waves ? ATTN_32Q_4W : ATTN_32Q_8W;
  p.lds = LDS32;
  p.full_rounds = -1;
  if (req.four_waves) {  // 4 waves x 32 queries, two workgroups per CU
    p.threads = 256;
    p.qblocks = (L + 127) / 128;
    p.items = p.qblocks * A.H * A.B;
    const int G = 2 * n_cu;
    const int nkt = (L + KVB - 1) / KVB;
    const int rounds = p.items / G, tail = p.items - rounds * G;
    // cut the tail only where it shortens the critical path by more than the merge costs (~3 tiles): plain = one more
    // round of nkt tiles for the blocks that draw a tail item, split = ceil(tail * nkt / G) tiles for every block
    const int split_tiles = (int)(((long)tail * nkt + G - 1) / G);
    if (req.tail_split && !A.kv_len && tail > 0 && A.scratch && A.scratch_bytes >= attention_scratch_bytes(n_cu) && split_tiles + 3 < nkt) {
      p.full_rounds = rounds; p.tail_items = tail; p.tail_units = tail * nkt;
      p.grid = G;
      p.merge_grid = tail;      // one workgroup per tail item
      p.scratch_need = attention_scratch_bytes(n_cu);
    } else {
      p.grid = std::min(p.items, req.persist ? G : p.items);
    }
  } else {  // 8 waves x 32 queries
    p.threads = 512;
    p.qblocks = (L + 255) / 256;
    p.items = p.qblocks * A.H * A.B;
    p.grid = std::min(p.items, req.persist ? n_cu : p.items);
  }
  return p;
}

AttnPlan plan_attention(const VcAttention& A, int n_cu) {
  const AttnRequest req = decode_variant(A.variant);
  AttnPlan p = req.wave64 ? plan_attention64(A, req, n_cu) : plan_attention32(A, req, n_cu);
  p.flags_offset = attention_flags_offset(n_cu);
  return p;
}

int attention_plan_words(const VcAttention& A, int n_cu, int32_t out[16], char* err, int errlen) {
  std::fill(out, out + 16, 0);
  out[0] = attention_variant_by_size(A.B, A.L, A.H, n_cu);
  const int rc = validate_attention(A, err, errlen);
  if (rc != VC_OK) return rc;
  const AttnPlan p = plan_attention(A, n_cu);
  const int32_t words[14] = {p.family, p.bounded, p.grid, p.threads, p.lds, p.qblocks, p.items, p.full_rounds, p.tail_items, p.tail_units,
                             p.inmerge, p.merge_grid, (int32_t)p.flags_offset, (int32_t)p.scratch_need};
  std::copy(words, words + 14, out + 1);
  return VC_OK;
}

}  // namespace vcplan
