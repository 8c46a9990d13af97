// The launch planner of vc_gemm (see gemm_plan.h): host code only, no kernel and no HIP call in this file.
#include <stdio.h>
#include "gemm_plan.h"

namespace vcplan {

TileRequest decode_tile_cfg(int w) {
  return TileRequest{w & 15, (w >> 4) & 3, (w >> 8) & 255, (w >> 16) & 15, (w & VC_GEMM_NO_SPLIT) != 0, (w & VC_GEMM_NO_SPLITK) != 0,
                     (w & VC_GEMM_PERSIST) != 0, (w & VC_GEMM_STREAMK) != 0, (w & VC_GEMM_PREFER_STREAMK) != 0, (w & VC_GEMM_STREAMK_ANY_K) != 0};
}

// plain main loop: every tile; ping-pong: 256x256, 256x192, 256x288; ping-pong with loader waves: 256x128, 256x192
bool tile_form_exists(int tile, int pp) {
  return tile >= 1 && tile <= 5 && (pp == 0 || (pp == 1 && tile >= 3) || (pp == 2 && (tile == 2 || tile == 4)));
}

#define VC_GEMM_FAIL(...) do { snprintf(err, errlen, __VA_ARGS__); return VC_ERR_ARG; } while (0)
int validate_gemm(VcGemmArgs& a, char* err, int errlen) {
  if (a.nprob < 1 || a.nprob > VC_GEMM_MAX_PROBLEMS) VC_GEMM_FAIL("gemm: nprob must be 1..%d", VC_GEMM_MAX_PROBLEMS);
  for (int i = 0; i < a.nprob; ++i) {
    VcGemmProblem& p = a.p[i];
    p.m_begin = 0;
    if (p.M <= 0 || p.N <= 0 || p.K <= 0) VC_GEMM_FAIL("gemm: empty problem %d (M=%d N=%d K=%d)", i, p.M, p.N, p.K);
    if (p.K % BK) VC_GEMM_FAIL("gemm: K=%d must be a multiple of %d", p.K, BK);
    if (p.N % 8 || p.ldc % 8 || p.lda % 8) VC_GEMM_FAIL("gemm: need N, ldc, lda multiples of 8 (N=%d ldc=%ld lda=%ld)", p.N, (long)p.ldc, (long)p.lda);
    if (!p.A || !p.W || !p.C) VC_GEMM_FAIL("gemm: null operand");
    if (p.a_rpb < 0 || p.c_rpb < 0 || p.a_bstride % 8 || p.c_bstride % 8 || (p.c_rpb > 0 && p.res && p.ldres != p.ldc))
      VC_GEMM_FAIL("gemm: bad batch-strided row description");
    const uint64_t a_batches = p.a_rpb > 0 ? (uint64_t)((p.M + p.a_rpb - 1) / p.a_rpb) * (uint64_t)p.a_bstride : 0;
    const uint64_t a_rows = (uint64_t)(p.a_rpb > 0 ? p.a_rpb : p.M) * (uint64_t)p.lda;
    if (a_batches >= (1ull << 32) || a_rows >= (1ull << 32) || (uint64_t)p.N * (uint64_t)p.ldw >= (1ull << 32) || (p.ldw != 0 && p.ldw < p.K) || p.ldw % 8)
      VC_GEMM_FAIL("gemm: operand exceeds 32-bit element offsets");
    // the loader-wave kernels address A with 32-bit BYTE offsets against the operand, W with byte offsets against its n-tile
    // (the largest element offset of A the kernel forms, + one K-tile: batch-strided rows may overlap or leave gaps, so both
    // terms count - advisor r04)
    const uint64_t a_last = p.a_rpb > 0 ? (uint64_t)((p.M - 1) / p.a_rpb) * (uint64_t)p.a_bstride + (uint64_t)(p.a_rpb - 1) * (uint64_t)p.lda
                                        : (uint64_t)(p.M - 1) * (uint64_t)p.lda;
    if (a_last + (uint64_t)p.K + 64 >= (1ull << 31) || (uint64_t)288 * (uint64_t)p.ldw >= (1ull << 31))
      VC_GEMM_FAIL("gemm: A operand spanning 4 GB or more (2^31 bf16 elements; or a W row stride beyond 7 M elements) is not supported");
    if (a.epi == VC_EPI_GATE_RES && (!p.res || !p.gate || p.rows_per_batch <= 0 || p.ldres % 8 || p.gate_bstride % 8 || a.gate_step_stride % 8))
      VC_GEMM_FAIL("gemm: gate/residual epilogue needs res, gate, rows_per_batch");
    const bool head_permuted = a.epi == VC_EPI_QKV && p.kn_heads != 0, fused_norm = p.kn_scale || p.qn_scale;
    if (head_permuted && (p.kn_heads < 0 || p.N != 384 * p.kn_heads || (p.vt && p.vt_col0 != 256 * p.kn_heads) || p.vt_rpb <= 0 ||
                          (fused_norm && (!p.kn_rope || p.vt_row0 < 0 || p.kn_rope_bstride < 0))))
      VC_GEMM_FAIL("gemm: head-permuted qkv needs N = 3 * 128 * kn_heads (N=%d kn_heads=%d), vt_col0 = 2 * 128 * kn_heads, the row geometry "
                   "vt_rpb / vt_row0, and with kn_scale / qn_scale a rope table", p.N, p.kn_heads);
    if (!head_permuted && (p.kn_heads != 0 || fused_norm || p.qn_prescale))
      VC_GEMM_FAIL("gemm: kn_heads / kn_scale / qn_scale belong to VC_EPI_QKV with head-permuted weights");
    if (p.qn_prescale && !p.qn_scale) VC_GEMM_FAIL("gemm: qn_prescale without qn_scale");
    if (a.epi == VC_EPI_QKV && p.vt && (p.vt_rpb <= 0 || p.vt_col0 < 0 || p.vt_col0 % 8 || p.vt_col0 >= p.N || p.vt_row0 < 0 ||
                                        p.vt_lpad < p.vt_row0 + p.vt_rpb || p.vt_bstride < (int64_t)(p.N - p.vt_col0) * p.vt_lpad))
      VC_GEMM_FAIL("gemm: bad V^T description (vt_col0=%d vt_rpb=%d vt_row0=%d vt_lpad=%d vt_bstride=%ld)", p.vt_col0, p.vt_rpb, p.vt_row0, p.vt_lpad, (long)p.vt_bstride);
  }
  if (a.epi < 0 || a.epi > VC_EPI_QKV) VC_GEMM_FAIL("gemm: unknown epilogue %d", a.epi);
  if (a.batch < 0 || a.batch > 65535) VC_GEMM_FAIL("gemm: batch must be 0..65535");
  if (a.batch > 1 && a.epi != VC_EPI_BIAS) VC_GEMM_FAIL("gemm: batch > 1 supports VC_EPI_BIAS only");
  for (int i = 0; a.batch > 1 && i < a.nprob; ++i) {
    const VcGemmProblem& p = a.p[i];
    if (p.a_zstride % 8 || p.w_zstride % 8 || p.c_zstride % 8 || p.a_zstride < 0 || p.w_zstride < 0 || p.c_zstride < 0 || p.a_rpb || p.c_rpb ||
        (uint64_t)a.batch * (uint64_t)p.a_zstride >= (1ull << 40) || (uint64_t)a.batch * (uint64_t)p.w_zstride >= (1ull << 40))
      VC_GEMM_FAIL("gemm: batch strides must be non-negative multiples of 8 elements (plain rows only)");
  }
  return VC_OK;
}

long tiles_of(const VcGemmArgs& a, int tile) {
  const Tile& t = TILES[tile];
  long tiles = 0;
  for (int i = 0; i < a.nprob; ++i) {
    const int rows = a.p[i].M - a.p[i].m_begin;
    if (rows > 0) tiles += (long)((rows + t.bm - 1) / t.bm) * ((a.p[i].N + t.bn - 1) / t.bn);
  }
  return tiles;
}

namespace {

constexpr int STREAMK_MIN_K = 6144;     // the stream remainder is not offered below this K (the partial traffic outweighs the short tiles)
constexpr Tile T192 = TILES[LW192.tile];

struct Priced { GemmPlan plan; double cost; };      // plan.tile1 == 0: no such plan
constexpr Priced NO_PLAN{GemmPlan{0, 0, 0, 0, 0}, 1e300};

// what the 256x192 tiling leaves beyond whole rounds of the CUs: total = rounds * n_cu + rem
struct Remainder { long total, rounds, rem; bool same_k; };
Remainder remainder_of(const VcGemmArgs& a, long n_cu) {
  const long total = tiles_of(a, LW192.tile);
  bool same_k = true;
  for (int i = 1; i < a.nprob; ++i) same_k = same_k && a.p[i].K == a.p[0].K;
  return Remainder{total, total / n_cu, total % n_cu, same_k};
}

Priced best_tile(const VcGemmArgs& a, long n_cu) {
  Priced best = NO_PLAN;
  for (const Candidate& c : CANDIDATES) {
    const Tile& t = TILES[c.tile];
    const long rounds = (tiles_of(a, c.tile) + n_cu * t.per_cu - 1) / (n_cu * t.per_cu);
    const double cost = rounds * (t.per_cu * (double)t.bm * t.bn * ((double)a.p[0].K + c.ovh) / c.eff);
    if (cost < best.cost) best = Priced{GemmPlan{0, c.tile, c.pp, 0, 0}, cost};
  }
  return best;
}

// a fixed tile is taken literally
GemmPlan fixed_plan(const TileRequest& req) { return GemmPlan{0, req.tile, req.pp, 0, 0}; }

// the 256x192 loader-wave tile with the remainder tiles cut S ways along K
GemmPlan forced_splitk_plan(const Remainder& r, int S) {
  GemmPlan pl{0, LW192.tile, LW192.pp, 0, 0};
  if (r.rem > 0) { pl.sk_S = S; pl.sk_tiles = (int)r.rem; }
  return pl;
}

// stream form: n work items share the remainder's K-iterations evenly (each >= ~12 iterations, at most one per CU)
GemmPlan forced_stream_plan(const VcGemmArgs& a, const Remainder& r, long n_cu) {
  GemmPlan pl{0, LW192.tile, LW192.pp, 0, 0};
  if (r.rem > 0) {
    long n = r.rem * (a.p[0].K / BK) / 12;
    n = n < r.rem ? r.rem : n > n_cu ? n_cu : n;
    pl.sk_stream = (int)n; pl.sk_tiles = (int)r.rem;
  }
  return pl;
}

// heads are normalised inside the epilogue: every head must lie in one 192-wide tile
// (tile1 == 0: no fused head norm in this call)
GemmPlan qkv_head_plan(const VcGemmArgs& a, const TileRequest& req) {
  for (int i = 0; i < a.nprob; ++i)
    if (a.epi == VC_EPI_QKV && (a.p[i].kn_scale || a.p[i].qn_scale)) return GemmPlan{0, LW192.tile, req.fixed() ? req.pp : LW192.pp, 0, 0};
  return NO_PLAN.plan;
}

// SPLIT-K REMAINDER: the 256x192 tiles are R whole rounds of the CUs plus r tiles - run those r as r * S slices of K / S
// (S <= 8, r * S <= CUs: ONE short round) that leave f32 partial tiles for a small second launch, instead of a second round
// at r / CUs fill or a narrower tile for everything.  Priced in the units of best_tile (one 256x192 tile of K = 15360 on its CU
// = 8.2e8 units = 255 us: 3.2e6 units per us): a slice pays its own prologue and the partial store instead of an epilogue
// (+150), the partials are written and read once at ~4 TB/s, the second launch costs a dependent kernel boundary (~3 us).
// Taken at >= 7 % under the best one-launch plan: SDEdit stage (L = 4608: 288 tiles = 256 + 32 x 8 slices, K = 12288 /
// 15360) and cfg 1 (L = 1664: 112 tiles x 2 slices); never at K = 3072 (the partial traffic outweighs 1 / S of a short tile).
Priced splitk_remainder(const VcGemmArgs& a, const Remainder& r, long n_cu, const Priced& whole) {
  const long R = r.rounds, rem = r.rem;
  const int nk = a.p[0].K / BK;
  int S = rem > 0 ? (int)(n_cu / rem) : 0;
  if (S > 8) S = 8;
  if (S > nk / 8) S = nk / 8;
  const double bytes = (double)rem * S * T192.bm * T192.bn * 4;
  if (S >= 2 && r.same_k && bytes <= (double)a.splitk_ws_bytes) {
    const double area = (double)T192.bm * T192.bn / LW192.eff;
    const double cost = R * area * (a.p[0].K + LW192.ovh) + area * ((double)a.p[0].K / S + LW192.ovh + 150.0) + (2.0 * bytes / 4e6 + 3.0) * 3.2e6;
    if (cost < 0.93 * whole.cost) return Priced{forced_splitk_plan(r, S), cost};
  }
  return NO_PLAN;
}

// STREAM REMAINDER: more than half a round of tiles beyond the whole rounds (no uniform S >= 2 fits one round): every CU takes
// f = rem / CUs of a tile's K-iterations, at most two segments, <= 3 partial tiles per remainder tile.  Decided by measurement,
// not by the model (which prices a partly filled round at its full length; under the power cap it costs ~0.85 of one at 81 %
// fill): interleaved whole steps, profiles/r05d_ab_*.log - cfg 3's N = 3072 launches (416 tiles = 256 + 160, f = 0.625: instead
// of the row cut into 256 + 240 narrower tiles) +1.7 % per step, all of it from K >= 12288 (K = 3072 included: +0.0 %);
// cfg 5's (464 = 256 + 208, f = 0.81: instead of a second round at 81 % fill) -1.2 %, with K = 3072 -2.1 %.  Taken for
// 0.5 < f <= 0.7 and K >= STREAMK_MIN_K.
bool stream_remainder(const VcGemmArgs& a, const TileRequest& req, const Remainder& r, long n_cu, const Priced& whole) {
  if (r.rounds >= 1 && 2 * r.rem > n_cu && r.same_k && (a.p[0].K >= STREAMK_MIN_K || req.streamk_any_k) &&
      (double)n_cu * 2 * T192.bm * T192.bn * 4 <= (double)a.splitk_ws_bytes) {
    // (advisor r05: only where the one-launch plan would have chosen the 256x192 tile itself - at N = 256 or 4096 a 192-wide
    // tile wastes columns and another tile may cost far less than any remainder scheme on this one)
    return req.prefer_streamk || req.streamk_any_k || (10 * r.rem <= 7 * n_cu && whole.plan.tile1 == LW192.tile);
  }
  return false;
}

// Block-round quantisation: cut problem 0's rows where the 256x192 tiles above the cut are (nearly) whole rounds of the 256
// CUs and price the remainder with the tile that suits it.  The two launches follow each other on the stream (the first
// has a flat tail by construction); a cut is taken when the model says it saves >= 10 % and both launches fill their rounds.
// The model over-credits by an order of magnitude: under the board's power limit a partly filled round runs at a higher
// clock, so quantisation costs far less than its fill factor.  Interleaved A/B, steps/s with / without cuts: L = 6656 (the
// N = 3072 launches: 416 tiles -> 256 + 240, model -12.7 % per launch) 9.846 / 9.804 = +0.4 %; L = 7424 (N = 12288 launches
// cut at 6144 rows, model -6.3 %) 8.683 / 8.693 = -0.1 % - hence the 10 % bar.
Priced row_cut(const VcGemmArgs& a, int force_cut, long n_cu, const Priced& whole) {
  Priced cut = NO_PLAN;
  double best = force_cut > 0 ? 1e300 : 0.90 * whole.cost;
  const int tn = (a.p[0].N + T192.bn - 1) / T192.bn;
  const int mt_all = (a.p[0].M + 255) / 256;
  for (int mt = 1; mt <= mt_all; ++mt) {
    if (force_cut > 0 && mt != force_cut) continue;
    const int rows = mt * 256 < a.p[0].M ? mt * 256 : a.p[0].M;
    if (rows == a.p[0].M && a.nprob == 1) break;            // nothing left for the second launch
    const long tiles1 = (long)mt * tn, rounds1 = (tiles1 + n_cu - 1) / n_cu;
    if (force_cut == 0 && tiles1 < 0.97 * (double)n_cu * rounds1) continue;
    const double t1 = rounds1 * ((double)T192.bm * T192.bn * ((double)a.p[0].K + LW192.ovh) / LW192.eff);
    VcGemmArgs rest = a;
    rest.p[0].m_begin = rows;
    const Priced rp = best_tile(rest, n_cu);
    // the remainder must fill its own rounds too: a half-empty second launch loses more than the model credits it with
    // (measured: L = 4608 cut into 4096 + 512 rows, 144 - 192 tiles in the second launch: -0.7 % steps/s)
    const int per_cu = TILES[rp.plan.tile1].per_cu;
    const long tiles2 = tiles_of(rest, rp.plan.tile1), slots2 = (tiles2 + n_cu * per_cu - 1) / (n_cu * per_cu) * n_cu * per_cu;
    if (force_cut == 0 && tiles2 < 0.9 * slots2) continue;
    if (t1 + rp.cost < best) { best = t1 + rp.cost; cut = Priced{GemmPlan{rows, LW192.tile, LW192.pp, rp.plan.tile1, rp.plan.pp1}, best}; }
  }
  return cut;
}

}  // namespace

GemmPlan plan_gemm(const VcGemmArgs& a, const TileRequest& req, int n_cu_) {
  if (a.batch > 1) return GemmPlan{0, 1, 0, 0, 0};          // Z instances per problem: the 128x128 tile (grid (tiles, Z))
  const long n_cu = n_cu_;
  const Remainder r = remainder_of(a, n_cu);
  if (req.streamk) return forced_stream_plan(a, r, n_cu);
  if (req.force_splitk >= 2) return forced_splitk_plan(r, req.force_splitk > 8 ? 8 : req.force_splitk);
  const GemmPlan heads = qkv_head_plan(a, req);
  if (heads.tile1 != 0) return heads;
  if (req.fixed()) return fixed_plan(req);
  // auto: the best one-launch tile, unless a remainder scheme on the 256x192 tile or a row cut beats it
  const Priced whole = best_tile(a, n_cu);
  const bool may_split_k = !req.no_splitk && a.splitk_ws && a.epi != VC_EPI_QKV;
  const Priced sk = may_split_k ? splitk_remainder(a, r, n_cu, whole) : NO_PLAN;
  if (may_split_k && sk.plan.sk_S == 0 && stream_remainder(a, req, r, n_cu, whole)) return forced_stream_plan(a, r, n_cu);
  const Priced cut = (!req.no_split || req.force_cut > 0) ? row_cut(a, req.force_cut, n_cu, whole) : NO_PLAN;
  if (sk.plan.sk_S > 1 && (cut.plan.cut == 0 || sk.cost <= cut.cost)) return sk.plan;
  return cut.plan.cut == 0 ? whole.plan : cut.plan;
}

int plan_launches(const VcGemmArgs& a, const GemmPlan& pl, Launch out[2]) {
  out[0] = Launch{a, pl.tile1, pl.pp1, pl.sk_S, pl.sk_stream};
  if (pl.cut == 0) return 1;
  out[0].args.nprob = 1;
  out[0].args.p[0].M = pl.cut;                                 // rows [0, cut) of problem 0 on the 256x192 loader-wave tile
  out[1] = Launch{a, pl.tile2, pl.pp2, 0, 0};
  out[1].args.p[0].m_begin = pl.cut;
  return 2;
}

}  // namespace vcplan
