// The Flux handle (include/vcloze_hip.h: vc_flux_*): its state, and the few functions its three units call across each other -
//   flux_weights.hip  what is bound: the weight and LoRA tables, their resolution per block, a checkpoint as stored (vc_flux_load_*)
//   flux_engine.hip   what is launched: the workspace, the plan of an evaluation and of a step, its capture, prepare / forward / profile
//   flux_sample.hip   what a solver does: one trajectory core and the fixed-grid, adaptive, stochastic and multistep samplers on top of it
// Host code only.  The types live in a NAMED namespace: all three units must see the same Flux.
#pragma once
#include "common.h"
#include "vcloze_internal.h"
#include "engine_core.h"
#include "flux_keys.h"
#include "flux_rules.h"
#include "monitor_sites.h"
#include <math.h>
#include <string.h>
#include <string>
#include <unordered_map>
#include <vector>

namespace vcflux {

// a bound LoRA pair (vc_flux_bind_lora): lora_A [rank, in], lora_B [out, rank], lora_B's bias [out] or null
struct Lora {
  const void* a = nullptr; const void* b = nullptr; const void* bb = nullptr;
  int rank = 0, out = 0, in = 0;
  int64_t lda = 0, ldb = 0;
};

struct Lin {
  const void* w = nullptr;
  const void* b = nullptr;
  int N = 0, K = 0;
  int64_t ldw = 0;
};

// bound: the block's own logit bound, 1.02 sqrt(128) log2(e) max|query_norm.scale| max|key_norm.scale| (both streams of a double block)
struct DoubleW { Lin qkv[2], proj[2], mlp0[2], mlp2[2]; const void* qs[2]; const void* ks[2]; int64_t mod[2]; float bound; };  // [0] = img, [1] = txt
struct SingleW { Lin qkv, mlp, lin2; const void* qs; const void* ks; int64_t mod; float bound; };

struct Buffers {   // the workspace carve-up
  bf16_t *XI, *XT, *X, *XH, *QKV, *VT, *CAT, *HID, *TXT0, *XIN, *V, *XS, *COND, *MOD, *TEMB, *H1, *TVEC, *GVEC, *YVEC, *VEC, *GE, *GH, *YH, *KS, *YIN;
  float *ROPE, *TS, *DTS, *G32, *FREQS, *XS32;
  int32_t *STEP, *KVLEN, *KVGAP;
  bf16_t *SC_P = nullptr, *SC_R = nullptr, *SC_RS = nullptr;      // step cache (carved only while it is on)
  bf16_t *LY = nullptr, *LY2 = nullptr, *LH = nullptr, *LSCALE = nullptr;   // un-merged LoRA mode (carved only while it is on)
  int64_t ly_elems = 0, lh_elems = 0, lscale_elems = 0;
  float *SC_PART = nullptr, *SC_METRIC = nullptr;
  bf16_t* AD_K = nullptr;                                          // adaptive solve (carved only while option adaptive is on)
  float *AD_Y0 = nullptr, *AD_Y1 = nullptr, *AD_DT = nullptr, *AD_OUT = nullptr, *AD_PART = nullptr;
  float *SD_Y = nullptr, *SD_XHAT = nullptr, *SD_K1 = nullptr, *SD_TAB = nullptr;   // stochastic sampler (carved only while option sde is on)
  uint64_t* SD_RNG = nullptr;
  float *MS_Y = nullptr, *MS_TAB = nullptr;                        // multistep solve (carved only while option multistep is on)
  bf16_t* MS_HIST = nullptr;
  float *FM_U = nullptr, *FM_T = nullptr, *FM_PART = nullptr;      // vc_flux_eval_loss (carved only while option eval_loss is on): u_t, t, the sum's partials
  void* ATT_SCRATCH = nullptr;
  int64_t att_scratch_bytes = 0;
  void* SK_WS = nullptr;               // f32 partial tiles of split-K GEMM remainders (VcGemmArgs.splitk_ws)
  int64_t sk_ws_bytes = 0;
};

// vc_flux_set_option: every option of the plan, once.  OPTIONS below is the table that sets, clamps and compares them
struct Options {
  int attn_variant = -1, tile_cfg = 0, fuse_qnorm = 2, fuse_vt = 1, qkv_heads = 0, fuse_knorm = 0, logit_bound_milli = 0, mlp_first = 0, splitk = 1;
  int lora_mode = 0;
  int adaptive = 0;
  int sde = 0;
  int eval_loss = 0;
  int multistep = 0;
};
enum Clamp { ANY, BOOL, AT_LEAST_0, ZERO_TO_2, ZERO_OR_H };
#define OPT(name, clamp) {#name, &Options::name, clamp}
struct OptionRule { const char* name; int Options::*member; Clamp clamp; };
inline constexpr OptionRule OPTIONS[] = {      // (inline: ONE table for the three units that include this header)
    OPT(attn_variant, ANY),      OPT(tile_cfg, ANY),   OPT(fuse_qnorm, ZERO_TO_2),
    OPT(fuse_vt, BOOL),          OPT(qkv_heads, ZERO_OR_H),      // the bound qkv weights (linear1's first 3D rows) are head-permuted (vcloze_hip.h)
    OPT(fuse_knorm, BOOL),       OPT(logit_bound_milli, AT_LEAST_0),
    OPT(mlp_first, BOOL),        OPT(splitk, BOOL),              // split-K remainders (VcGemmArgs.splitk_ws) where the launcher's model takes them
    OPT(lora_mode, BOOL),                                        // 1: every Linear runs un-merged (flux_engine.hip: lora_linear)
    OPT(adaptive, BOOL),                                         // 1: the workspace holds the adaptive solve's buffers (vc_flux_sample_dopri5)
    OPT(sde, BOOL),                                              // 1: ... the stochastic sampler's (vc_flux_sample_sde)
    OPT(eval_loss, BOOL),                                        // 1: ... the flow-matching loss's (vc_flux_eval_loss)
    OPT(multistep, BOOL),                                        // 1: ... the multistep solve's (vc_flux_sample_multistep)
};
#undef OPT
inline bool operator==(const Options& a, const Options& b) {
  for (const auto& o : OPTIONS) if (a.*o.member != b.*o.member) return false;
  return true;
}

// what a trajectory runs with, latched ONCE where it begins (flux_sample.hip: begin_trajectory): the step's plan, its capture key and
// the solver's update read it and nothing else
// codes of the solvers that have no VC_SOLVER_* code (vc_solver_evals keeps refusing them)
constexpr int SOLVER_SDE_EULER = 101, SOLVER_SDE_HEUN = 102;     // the stochastic sampler (one captured step per method)
constexpr int SOLVER_RK = 103;         // the adaptive solve (vc_flux_sample_dopri5, vc_flux_sample_rk): ONE code, the pair is Trajectory::rk (VC_RK_*)
constexpr int SOLVER_MULTISTEP = 104;  // the Adams-Bashforth solve: ONE code and one captured step, the order lives in the table
struct Trajectory {
  int method = VC_SOLVER_EULER;        // VC_SOLVER_*, or one of the codes above
  int evals = 1;                       // replays of the captured evaluation per step
  int rk = 0;                          // SOLVER_RK: the VC_RK_* pair whose stage node the step ends with (0 otherwise)
  bool state_f32 = false;              // the state is stepped in f32 (XS32; XS is its bf16 shadow)
  bool cached = false;                 // the step cache steers it: a step is head + one of two tails
};

struct Flux : Buffers {
  VcFluxConfig cfg{};
  int D = 0, H = 0, mlp = 0;
  int64_t n_mod = 0;
  std::unordered_map<std::string, Lin> bound;
  std::unordered_map<std::string, int64_t> mod_off;
  // un-merged LoRA mode: the bound pairs by module path; resolved, the pair of the Linear whose weight rows start at an address
  // (linear1's two row ranges and the rows of every modulation Linear inside the stacked matrix have their own), and the
  // modulation Linears one by one, in stacking order
  std::unordered_map<std::string, Lora> lora;
  std::unordered_map<const void*, Lora> lora_of;
  std::vector<std::pair<Lin, int64_t>> mods;
  // vc_flux_load_*: the state_dict keys of this configuration (flux_keys.h) and the caller's tensors recorded under them, by key index
  vckeys::Table keys;
  struct Loaded { const void* p; int f32; int64_t shape[2]; };
  std::unordered_map<int, Loaded> loaded;
  float lora_scale = 1.0f;
  bool scale_stale = false;            // the scale changed after vc_flux_prepare ran txt_in / vector_in / guidance_in with the old one
  // per-block taps (vc_flux_set_tap): the caller's buffer of tap i, or null - in the order of monitor_sites.h (vcmon::tap_*)
  std::vector<void*> taps;
  // the numerics monitor (vc_flux_set_monitor): the caller's setting, read where a step is issued or captured.  mon_evals: evaluations
  // logged since the log was zeroed; mon_paused: vc_flux_profile issues its evaluations without the monitor's launches
  int mon_level = 0, mon_cap = 0, mon_evals = 0, mon_B = 0;   // mon_B: the prepared B the caller sized the log for (0: set before a prepare)
  VcStat* mon_log = nullptr;
  float* mon_scratch = nullptr;
  bool mon_paused = false;
  int mon_sites() const { return vcmon::site_count(mon_level, cfg.depth, cfg.depth_single_blocks); }
  bool in_flight = false;              // between vc_flux_sample_begin* and vc_flux_sample_end
  // resolved at prepare time
  bool resolved = false;
  Lin img_in, txt_in, time_in[2], vector_in[2], guidance_in[2], final_lin, modulation;
  std::vector<DoubleW> dbl;
  std::vector<SingleW> sgl;
  int64_t final_mod = 0;
  Options opt;
  int n_cu = 256;
  // prepared geometry + workspace carve-up
  bool prepared = false;
  bool ws_sized = false;     // vc_flux_workspace_bytes / vc_flux_prepare have answered with the current carve-up
  int B = 0, T = 0, N = 0, L = 0, Lp = 0, S = 0;
  bool ragged = false, gapped = false;
  std::vector<int32_t> n_img;          // per prepared sample: the valid image rows, kv_len - T clamped to [0, N] (vc_flux_eval_loss)
  char* base = nullptr;
  // a captured step: ONE graph (g[0]), or with the step cache on three - head, tail-compute, tail-reuse (an entry of `graphs` is a
  // whole step, so a cached trajectory never evicts a graph of its own).  step: the one of the sample in flight
  struct Step { hipGraphExec_t g[3] = {nullptr, nullptr, nullptr}; int nodes[3] = {0, 0, 0}; } step;      // nodes: of each graph (vc_flux_step_nodes)
  struct DropStep {
    void operator()(const Step& st) const { for (auto ge : st.g) if (ge) (void)hipGraphExecDestroy(ge); }
  };
  struct Key {
    char* base; int B, T, N, S, ragged, gapped, variant, state_f32, method, cache; Options opt; hipStream_t s;   // variant: resolved
    int cfg; uint32_t cfg_bits;          // true CFG on, and the bits of its scale: a kernel argument of the captured combine
    std::vector<void*> taps;             // the tap set: every tap is a copy node of the captured step
    int mon_level, mon_cap; void* mon_log; void* mon_scratch;      // the monitor: every site is a node of the captured step
    int rk;                              // SOLVER_RK: the pair (a kernel argument of the captured stage node), 0 otherwise
    bool operator==(const Key& o) const {
      return base == o.base && B == o.B && T == o.T && N == o.N && S == o.S && ragged == o.ragged && gapped == o.gapped &&
             variant == o.variant && state_f32 == o.state_f32 && method == o.method && cache == o.cache && opt == o.opt && s == o.s &&
             cfg == o.cfg && cfg_bits == o.cfg_bits && taps == o.taps && mon_level == o.mon_level && mon_cap == o.mon_cap &&
             mon_log == o.mon_log && mon_scratch == o.mon_scratch && rk == o.rk;
    }
  } key{};
  // captured steps, most recently used first (a two-stage pipeline alternates between two geometries)
  PlanCache<Key, Step, 4, DropStep> graphs;
  // sampling state
  int steps_total = 0, steps_done = 0;
  Trajectory traj;                     // of the last trajectory begun
  // step cache.  sc_threshold / sc_max: the caller's setting (vc_flux_set_step_cache), which sizes the workspace
  // at once and steers a trajectory from its sample_begin on (traj.cached, sc_thr, sc_lim)
  float sc_threshold = 0.0f; int sc_max = 0;
  bool sc_on() const { return sc_threshold > 0.0f && sc_max != 0; }
  bool ws_cache = false;               // the prepared workspace holds SC_P / SC_R / SC_RS
  bool sc_have = false;                // a P (and R) of this trajectory exists
  float sc_thr = 0.0f; int sc_lim = 0, sc_run = 0;   // sc_run: evaluations reused in a row
  int sc_computed = 0, sc_reused = 0;
  std::vector<float> sc_metrics;       // m of every evaluation of the trajectory (NaN where no P existed)
  float* sc_host = nullptr;            // pinned: the head graph's last node copies the metric here
  // true CFG (Flux.forward_with_cfg, model.py:126-145).  cfg_on / cfg_scale: the caller's setting (vc_flux_set_cfg), which steers a
  // trajectory from its sample_begin on (cfg_active, cfg_s)
  bool cfg_on = false, cfg_active = false;
  float cfg_scale = 1.0f, cfg_s = 1.0f;
  // the adaptive solves (vc_flux_sample_dopri5, vc_flux_sample_rk): the pinned words its norms are read from, and the log of the last run
  float* ad_host = nullptr;
  struct Attempt { double t, dt; float ratio; int accepted; };
  std::vector<Attempt> ad_log;
  int ad_evals = 0;
  // host staging (pinned), reused once the copies that read it have completed
  char* pinned = nullptr;
  size_t pinned_bytes = 0, pinned_used = 0;
  hipEvent_t staged = nullptr;
  bool staged_pending = false;
  // vc_flux_profile: HIP-event pairs around the launches of one evaluation (off outside that call)
  struct ProfRec { int kind, epi, n, k; double flops, bytes; size_t e0; };
  bool prof_on = false;
  std::vector<hipEvent_t> prof_ev;
  size_t prof_used = 0;
  std::vector<ProfRec> prof_recs;
};

// where the trajectory keeps its ODE state (in the caller's dtype), and the bf16 rows the next evaluation reads: the state itself
// for a bf16 Euler step, XS as the bf16 shadow of an f32 Euler state, else YIN - the stage input of every other solver
inline void* ode_state(Flux& f) { return f.traj.state_f32 ? (void*)f.XS32 : (void*)f.XS; }
inline int64_t ode_state_bytes(const Flux& f) { return (int64_t)f.B * f.N * f.cfg.out_channels * (f.traj.state_f32 ? 4 : 2); }
inline bf16_t* next_input(Flux& f) { return f.traj.method == VC_SOLVER_EULER ? f.XS : f.YIN; }

// ---- what the units call across each other.  They report as the launchers do, into (err, errlen): Err is a type of each unit's own
// flux_weights.hip
int resolve(Flux& f, char* err, int errlen);                 // the bound set -> the per-block tables (vc_flux_prepare)
// flux_engine.hip
void drop_graph(Flux& f);                                    // every captured step holds the pointers of the bound set
int d2d(void* dst, const void* src, int64_t bytes, hipStream_t s, char* err, int errlen);
// host tables -> pinned staging -> HBM: begin (waits for the copies of the last use), take, send ..., end
int stage_begin(Flux& f, size_t bytes, char* err, int errlen);
template <class T> T* stage_take(Flux& f, size_t count) {
  T* p = (T*)(f.pinned + f.pinned_used);
  f.pinned_used += (count * sizeof(T) + 255) & ~(size_t)255;
  return p;
}
int stage_send(Flux& f, void* dst, const void* staged, size_t bytes, hipStream_t s, char* err, int errlen);
int stage_end(Flux& f, hipStream_t s, char* err, int errlen);
int time_precompute(Flux& f, int S, int timesteps_is_bf16, hipStream_t s, char* err, int errlen);   // TS rows -> MOD rows
int fresh_scale(const Flux& f, const char* what, char* err, int errlen);
int monitor_fits(Flux& f, const char* what, char* err, int errlen);
int ode_update(Flux& f, const void* v, const int32_t* step_ptr, hipStream_t s, char* err, int errlen);
// piece `piece` of a step of f.traj: the whole step (0), or cached its head (0), tail-compute (1), tail-reuse (2); with `update` the
// solver's update behind the evaluation.  step_graph captures every piece on `s` (f.step), behind one un-captured run of each
int step_piece(Flux& f, int piece, bool update, hipStream_t s, char* err, int errlen);
int step_graph(Flux& f, hipStream_t s, char* err, int errlen);

}  // namespace vcflux
