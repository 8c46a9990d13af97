// The launch planner of vc_gemm: everything that DECIDES (argument checks, tile choice, row cut, split-K / stream remainder,
// the expansion of a plan into launches) and nothing that launches.  Host code only, a pure function of the argument shapes,
// the tile_cfg word and the CU count: gemm_plan.hip makes no HIP call, and vc_gemm_plan answers without a GPU.
// gemm.hip holds the kernels and turns each Launch into an instantiation.
#pragma once
#include "../../include/vcloze_hip.h"

namespace vcplan {

constexpr int BK = 64;      // K-tile of every kernel

// tile shapes by tile number 1..5 (include/vcloze_hip.h); per_cu = resident workgroups per CU the cost model counts with
struct Tile { int bm, bn, per_cu; };
constexpr Tile TILES[6] = {{0, 0, 0}, {128, 128, 2}, {256, 128, 1}, {256, 256, 1}, {256, 192, 1}, {256, 288, 1}};

// Cost model fitted on MI355X (M=3968 FLUX shapes): time = block-rounds on 256 CUs x (tile area x (K + fixed
// prologue/epilogue charge) / streaming efficiency of that tile).  Candidates: 128x128 simple loop (2 blocks per
// CU; small or skinny problems), 256x192 with loader waves (1 block per CU), which beat the 256x256 / 256x192
// ping-pong and the 256x288 tiles on every FLUX shape in an interleaved A/B (tools/gemm_ab.py; those stay
// selectable by number), and its 256x128 sibling.  For M <= 4096, 256x192 gives N=3072 / 9216 / 12288 exactly
// 1 / 3 / 4 rounds.
struct Candidate { int tile, pp; double eff, ovh; };
constexpr Candidate LW192{4, 2, 0.94, 350.0};       // 256x192 with loader waves: the tile of row cuts, split-K and stream remainders
constexpr Candidate CANDIDATES[3] = {{1, 0, 0.55, 500.0}, LW192,
                                     {2, 2, 0.84, 350.0}};       // 256x128 with loaders: more blocks when M is short (L = 1664: 168 vs 112)

// the tile_cfg word of vc_gemm, decoded once (bit layout: include/vcloze_hip.h)
struct TileRequest {
  int tile, pp;                         // 0, 0 = chosen by the cost model; pp: 0 plain main loop, 1 ping-pong, 2 ping-pong with loader waves
  int force_cut, force_splitk;          // tests / A-B: cut problem 0 at row force_cut * 256; VC_GEMM_SPLITK(S)
  bool no_split, no_splitk, persist, streamk, prefer_streamk, streamk_any_k;
  bool fixed() const { return tile != 0 || pp != 0; }
};
TileRequest decode_tile_cfg(int tile_cfg);
bool tile_form_exists(int tile, int pp);      // is (tile, main-loop form) one of the instantiated kernels?

// The launch plan of one vc_gemm call: cut = first row of the second launch (0 = one launch); tile / pp of the two launches.
struct GemmPlan { int cut, tile1, pp1, tile2, pp2, sk_S = 0, sk_tiles = 0, sk_stream = 0; };
// one launch of a plan: the arguments it covers (after a cut: rows [0, cut) of problem 0, then everything from row cut on)
struct Launch { VcGemmArgs args; int tile, pp, splitk_S, stream_items; };

int validate_gemm(VcGemmArgs& a, char* err, int errlen);      // (also normalises m_begin = 0)
long tiles_of(const VcGemmArgs& a, int tile);
GemmPlan plan_gemm(const VcGemmArgs& a, const TileRequest& req, int n_cu);
int plan_launches(const VcGemmArgs& a, const GemmPlan& pl, Launch out[2]);      // -> number of launches (1 or 2)

}  // namespace vcplan
