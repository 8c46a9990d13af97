// Handle API of include/vcloze_hip.h: Flux.forward (models/model.py:85-124) and the fixed-grid solver loop around it
// (transport/integrators.py:106-120: Euler, and midpoint / rk4 as E evaluations per step) as launch plans over the kernels of this library.  Host code only: it ORDERS launches
// (once per geometry, under stream capture, for the sampling loop); nothing here touches a tensor element except the RoPE
// angle table, which math.py:102-109 computes in float64 on the host as well.
//
// Workspace (caller's device memory), bf16 unless noted; B samples, T text / N image tokens, L = T + N, D hidden, S = max_steps
// (model EVALUATIONS: solver steps * evaluations per step):
//   XI [B*N, D] / XT [B*T, D]  residual streams of the DoubleStream blocks      X   [B*L, D]  joint stream of the SingleStream blocks
//   XH [B*L, D]   LayerNorm+modulate output (GEMM A operand)                     QKV [B*L, 3D] "B L (K H D)" rows, joint order
//   VT [B, H, 128, Lp]  V transposed per head (Lp = L rounded up to 64, padding zeroed once)
//   CAT [B*L, D+mlp]    attn | gelu(mlp) = linear2's input; CAT[:, :D] is also the DoubleStream attention output
//   HID [B*L, mlp]      MLP hidden of the DoubleStream blocks (image rows first)
//   MOD [S*B, n_mod]    every modulation vector of every block for every evaluation (row s*B + b, evaluation order)
//   XS / COND / XIN / V the ODE state, the conditioning columns, x || cond, the velocity
//   KS [3][B*N*out] / YIN   k1..k3 of an rk4 step / the input state of the next evaluation (midpoint, rk4); every solver's update
//                           is ONE kernel (ode_stage_kernel, elementwise.hip) behind ONE call (ode_update below)
//                           with true CFG on (vc_flux_set_cfg) one more kernel in front of it: V's first half <- uncond + s * (cond - uncond),
//                           in place (cfg_combine_kernel, elementwise.hip); no buffer of its own
//   SC_P / SC_R / SC_RS [B*N, D]  only with the step cache on (vc_flux_set_step_cache), behind everything else: P and R of the last
//                           computed evaluation, and a scratch that holds r = h1 - h0 until the decision and h1 after it
//   AD_K [7][B*N*out] / AD_Y0 / AD_Y1 (f32)  only with option adaptive 1, behind the step cache's: k1..k7, the state and the step's
//                           end state of the adaptive solve (vc_flux_sample_dopri5, dopri5.hip), its dt, norms and reduction scratch
//   SD_Y / SD_XHAT / SD_K1 (f32) / SD_TAB / SD_RNG  only with option sde 1, behind the adaptive solve's: the state, x-hat and K1 of the
//                           stochastic sampler (vc_flux_sample_sde, rng.hip), its coefficient table ([S + 1][VC_SDE_ROW] f32) and the
//                           seed / offset words its update reads
//   LY / LY2 / LH / LSCALE  only in the un-merged LoRA mode (option lora_mode 1), behind everything else: base_out, base_out + lora
//                           and lora_A(x) of the Linear being run, and the lora scale as a bf16 vector (the gate operand of the
//                           gated-residual epilogue that adds the lora branch; refilled by vc_flux_set_lora_scale)
#include "common.h"
#include "vcloze_internal.h"
#include "engine_core.h"
#include "flux_keys.h"
#include "monitor_sites.h"
#include <math.h>
#include <string.h>
#include <string>
#include <unordered_map>
#include <vector>

namespace {

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
};
enum Clamp { ANY, BOOL, AT_LEAST_0, ZERO_TO_2, ZERO_OR_H };
#define OPT(name, clamp) {#name, &Options::name, clamp}
constexpr struct { const char* name; int Options::*member; Clamp clamp; } OPTIONS[] = {
    OPT(attn_variant, ANY),      OPT(tile_cfg, ANY),   OPT(fuse_qnorm, ZERO_TO_2),
    OPT(fuse_vt, BOOL),          OPT(qkv_heads, ZERO_OR_H),      // the bound qkv weights (linear1's first 3D rows) are head-permuted (vcloze_hip.h)
    OPT(fuse_knorm, BOOL),       OPT(logit_bound_milli, AT_LEAST_0),
    OPT(mlp_first, BOOL),        OPT(splitk, BOOL),              // split-K remainders (VcGemmArgs.splitk_ws) where the launcher's model takes them
    OPT(lora_mode, BOOL),                                        // 1: every Linear runs un-merged (lora_linear below)
    OPT(adaptive, BOOL),                                         // 1: the workspace holds the adaptive solve's buffers (vc_flux_sample_dopri5)
    OPT(sde, BOOL),                                              // 1: ... the stochastic sampler's (vc_flux_sample_sde)
};
#undef OPT
inline bool operator==(const Options& a, const Options& b) {
  for (const auto& o : OPTIONS) if (a.*o.member != b.*o.member) return false;
  return true;
}

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
  char* base = nullptr;
  // a captured step: ONE graph (g[0]), or with the step cache on three - head, tail-compute, tail-reuse (an entry of `graphs` is a
  // whole step, so a cached trajectory never evicts a graph of its own).  step: the one of the sample in flight
  struct Step { hipGraphExec_t g[3] = {nullptr, nullptr, nullptr}; int nodes[3] = {0, 0, 0}; } step;      // nodes: of each graph (vc_flux_step_nodes)
  struct DropStep {
    void operator()(const Step& st) const { for (auto ge : st.g) DropExec()(ge); }
  };
  struct Key {
    char* base; int B, T, N, S, ragged, gapped, variant, state_f32, method, cache; Options opt; hipStream_t s;   // variant: resolved
    int cfg; uint32_t cfg_bits;          // true CFG on, and the bits of its scale: a kernel argument of the captured combine
    std::vector<void*> taps;             // the tap set: every tap is a copy node of the captured step
    int mon_level, mon_cap; void* mon_log; void* mon_scratch;      // the monitor: every site is a node of the captured step
    bool operator==(const Key& o) const {
      return base == o.base && B == o.B && T == o.T && N == o.N && S == o.S && ragged == o.ragged && gapped == o.gapped &&
             variant == o.variant && state_f32 == o.state_f32 && method == o.method && cache == o.cache && opt == o.opt && s == o.s &&
             cfg == o.cfg && cfg_bits == o.cfg_bits && taps == o.taps && mon_level == o.mon_level && mon_cap == o.mon_cap &&
             mon_log == o.mon_log && mon_scratch == o.mon_scratch;
    }
  } key{};
  // captured steps, most recently used first (a two-stage pipeline alternates between two geometries)
  PlanCache<Key, Step, 4, DropStep> graphs;
  // sampling state
  int steps_total = 0, steps_done = 0;
  bool state_f32 = false;              // the sample in flight steps an f32 state (XS32; XS is its bf16 shadow)
  int method = VC_SOLVER_EULER, evals = 1;   // ... with this solver: `evals` replays of the captured evaluation per step
  // step cache.  sc_threshold / sc_max: the caller's setting (vc_flux_set_step_cache), which sizes the workspace
  // at once and steers a trajectory from its sample_begin on (sc_active, sc_thr, sc_lim)
  float sc_threshold = 0.0f; int sc_max = 0;
  bool sc_on() const { return sc_threshold > 0.0f && sc_max != 0; }
  bool ws_cache = false;               // the prepared workspace holds SC_P / SC_R / SC_RS
  bool sc_active = false, sc_have = false;   // this trajectory runs cached; a P (and R) of this trajectory exists
  float sc_thr = 0.0f; int sc_lim = 0, sc_run = 0;   // sc_run: evaluations reused in a row
  int sc_computed = 0, sc_reused = 0;
  std::vector<float> sc_metrics;       // m of every evaluation of the trajectory (NaN where no P existed)
  float* sc_host = nullptr;            // pinned: the head graph's last node copies the metric here
  // true CFG (Flux.forward_with_cfg, model.py:126-145).  cfg_on / cfg_scale: the caller's setting (vc_flux_set_cfg), which steers a
  // trajectory from its sample_begin on (cfg_active, cfg_s)
  bool cfg_on = false, cfg_active = false;
  float cfg_scale = 1.0f, cfg_s = 1.0f;
  // the adaptive solve (vc_flux_sample_dopri5): the pinned words its norms are read from, and the log of the last run
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

// ---------------------------------------------------------------- workspace
int64_t carve(Buffers& f, const Flux& g, char* base, int B, int T, int N, int S) {
  const int64_t D = g.D, H = g.H, mlp = g.mlp, L = T + N, Lp = (L + 63) / 64 * 64;
  const int64_t in_ch = g.cfg.in_channels, out_ch = g.cfg.out_channels;
  Carver c{base};
  f.XI = c.take<bf16_t>(B * N * D);          f.XT = c.take<bf16_t>(B * T * D);
  f.X = c.take<bf16_t>(B * L * D);           f.XH = c.take<bf16_t>(B * L * D);
  f.QKV = c.take<bf16_t>(B * L * 3 * D);     f.VT = c.take<bf16_t>(B * H * 128 * Lp);
  f.CAT = c.take<bf16_t>(B * L * (D + mlp)); f.HID = c.take<bf16_t>(B * L * mlp);
  f.TXT0 = c.take<bf16_t>(B * T * D);        f.XIN = c.take<bf16_t>(B * N * in_ch);
  f.V = c.take<bf16_t>(B * N * out_ch);      f.XS = c.take<bf16_t>(B * N * out_ch);
  f.COND = c.take<bf16_t>(B * N * (in_ch - out_ch));
  f.MOD = c.take<bf16_t>((int64_t)S * B * g.n_mod);
  f.TEMB = c.take<bf16_t>((int64_t)S * B * 256);
  f.H1 = c.take<bf16_t>((int64_t)S * B * D); f.TVEC = c.take<bf16_t>((int64_t)S * B * D);
  f.VEC = c.take<bf16_t>((int64_t)S * B * D);
  f.GVEC = c.take<bf16_t>(B * D);            f.YVEC = c.take<bf16_t>(B * D);
  f.GE = c.take<bf16_t>(B * 256);            f.GH = c.take<bf16_t>(B * D);  f.YH = c.take<bf16_t>(B * D);
  f.ROPE = c.take<float>(B * L * 128);
  f.TS = c.take<float>((int64_t)S * B);      f.DTS = c.take<float>(S);
  f.G32 = c.take<float>(B);                  f.FREQS = c.take<float>(128);
  f.XS32 = c.take<float>(B * N * out_ch);    // f32 master copy of the ODE state (state_is_bf16 == 0)
  f.KS = c.take<bf16_t>(3 * B * N * out_ch); f.YIN = c.take<bf16_t>(B * N * out_ch);   // midpoint / rk4 stages (vc_ode_stage)
  f.STEP = c.take<int32_t>(1);               f.KVLEN = c.take<int32_t>(B);  f.KVGAP = c.take<int32_t>(2 * B);
  f.att_scratch_bytes = vcplan::attention_scratch_bytes(vc_cu_count());
  f.ATT_SCRATCH = c.take<char>(f.att_scratch_bytes);
  // one split-K scratch serves every geometry of a handle (all its launches are ordered on one stream): a caller-bound one
  // ("splitk_ws", vc_flux_bind_weight) keeps the 100 MB out of every cached workspace (advisor r04); without it, it is carved here
  auto sk = g.bound.find("splitk_ws");
  if (sk != g.bound.end()) { f.SK_WS = const_cast<void*>(sk->second.w); f.sk_ws_bytes = (int64_t)sk->second.N * sk->second.K * 4; }
  else { f.SK_WS = c.take<char>(VC_GEMM_SPLITK_WS_BYTES); f.sk_ws_bytes = VC_GEMM_SPLITK_WS_BYTES; }
  if (g.sc_on()) {    // behind everything else: with the cache off the carve-up and its size are what they always were
    f.SC_P = c.take<bf16_t>(B * N * D); f.SC_R = c.take<bf16_t>(B * N * D); f.SC_RS = c.take<bf16_t>(B * N * D);
    f.SC_PART = c.take<float>((int64_t)B * 2 * VC_RESIDUAL_CHANGE_MAX_BLOCKS); f.SC_METRIC = c.take<float>(1);
  }
  if (g.opt.adaptive) {    // likewise
    const int64_t n = (int64_t)B * N * out_ch;
    f.AD_K = c.take<bf16_t>(7 * n); f.AD_Y0 = c.take<float>(n); f.AD_Y1 = c.take<float>(n);
    f.AD_DT = c.take<float>(1); f.AD_OUT = c.take<float>(4); f.AD_PART = c.take<float>(VC_DOPRI5_MAX_BLOCKS);
  }
  if (g.opt.sde) {         // likewise
    const int64_t n = (int64_t)B * N * out_ch;
    f.SD_Y = c.take<float>(n); f.SD_XHAT = c.take<float>(n); f.SD_K1 = c.take<float>(n);
    f.SD_TAB = c.take<float>(((int64_t)S + 1) * VC_SDE_ROW); f.SD_RNG = c.take<uint64_t>(2);
  }
  if (g.opt.lora_mode) {   // likewise: the widest Linear over the block rows, the modulation Linears over the (evaluation, sample) rows
    const int64_t wide = std::max<int64_t>({3 * D, mlp, D, out_ch}), rows = std::max<int64_t>(B * L, (int64_t)S * B);
    int64_t rank = 64;
    for (const auto& kv : g.lora) rank = std::max<int64_t>(rank, kv.second.rank);
    f.ly_elems = std::max<int64_t>(B * L * wide, (int64_t)S * B * 6 * D);
    f.lh_elems = rows * rank;
    f.lscale_elems = std::max<int64_t>(wide, 6 * D);
    f.LY = c.take<bf16_t>(f.ly_elems); f.LY2 = c.take<bf16_t>(f.ly_elems);
    f.LH = c.take<bf16_t>(f.lh_elems); f.LSCALE = c.take<bf16_t>(f.lscale_elems);
  }
  return c.off;
}

// ---------------------------------------------------------------- weights
int find(Flux& f, const std::string& name, Lin& out, int N, int K, bool need_bias, Err e) {
  auto it = f.bound.find(name);
  if (it == f.bound.end()) FAIL(VC_ERR_STATE, "flux: weight '%s' is not bound", name.c_str());
  out = it->second;
  if (out.N != N || out.K != K) FAIL(VC_ERR_ARG, "flux: weight '%s' is [%d, %d], expected [%d, %d]", name.c_str(), out.N, out.K, N, K);
  if (need_bias && !out.b) FAIL(VC_ERR_ARG, "flux: weight '%s' needs a bias", name.c_str());
  return VC_OK;
}
int find_scale(Flux& f, const std::string& name, const void*& out, Err e) {
  auto it = f.bound.find(name);
  if (it == f.bound.end()) FAIL(VC_ERR_STATE, "flux: scale '%s' is not bound", name.c_str());
  if (it->second.N * it->second.K != 128) FAIL(VC_ERR_ARG, "flux: scale '%s' must hold 128 values", name.c_str());
  out = it->second.w;
  return VC_OK;
}

void layout_modulation(Flux& f) {
  int64_t o = 0;
  for (int i = 0; i < f.cfg.depth; ++i) {
    f.mod_off["double_blocks." + std::to_string(i) + ".img_mod.lin"] = o; o += 6 * f.D;
    f.mod_off["double_blocks." + std::to_string(i) + ".txt_mod.lin"] = o; o += 6 * f.D;
  }
  for (int i = 0; i < f.cfg.depth_single_blocks; ++i) { f.mod_off["single_blocks." + std::to_string(i) + ".modulation.lin"] = o; o += 3 * f.D; }
  f.mod_off["final_layer.adaLN_modulation.1"] = o; o += 2 * f.D;
  f.n_mod = o;
}

// max |scale| of a bound QK-norm scale vector (128 bf16 on the device): read back ONCE, when the weights are resolved
int scale_absmax(const void* dev, double& out, Err e) {
  uint16_t h[128];
  HIP(hipMemcpy(h, dev, sizeof(h), hipMemcpyDeviceToHost), "hipMemcpy (QK-norm scale)");
  out = 0;
  bool nan = false;
  for (int i = 0; i < 128; ++i) {
    uint32_t u = (uint32_t)h[i] << 16;
    float v;
    memcpy(&v, &u, 4);
    const double a = v < 0 ? -(double)v : (double)v;
    if (a != a) nan = true;
    else if (a > out) out = a;
  }
  if (nan) out = 1e30;                 // (no bound: the running-max template)
  return VC_OK;
}
// |q|, |k| <= sqrt(128) max|scale| after QKNorm (RoPE is a rotation), so |128^-0.5 log2(e) q.k| <= this; + 2 % for the six bf16
// roundings on the way (model.py / engine.py compute the same number for the Python-ordered plan)
inline float logit_bound_of(double qmax, double kmax) { return (float)(1.02 * 11.313708498984761 * 1.4426950408889634 * qmax * kmax); }

// the pair bound for module `name` belongs to the Linear `l`, whose rows are [row0, row0 + l.N) of that module's
int attach_lora(Flux& f, const std::string& name, const Lin& l, int row0, Err e) {
  auto it = f.lora.find(name);
  if (it == f.lora.end()) return VC_OK;
  Lora lo = it->second;
  if (lo.in != l.K || row0 + l.N > lo.out)
    FAIL(VC_ERR_ARG, "flux: LoRA pair of '%s' is [%d, r] x [r, %d], its Linear takes %d inputs", name.c_str(), lo.out, lo.in, l.K);
  lo.b = (const bf16_t*)lo.b + (int64_t)row0 * lo.ldb;
  if (lo.bb) lo.bb = (const bf16_t*)lo.bb + row0;
  lo.out = l.N;
  f.lora_of[l.w] = lo;
  return VC_OK;
}

int resolve(Flux& f, Err e) {
  if (f.resolved) return VC_OK;
  const int D = f.D, mlp = f.mlp;
  f.lora_of.clear();
  f.mods.clear();
  TRY(find(f, "img_in", f.img_in, D, f.cfg.in_channels, false, e));
  TRY(find(f, "txt_in", f.txt_in, D, f.cfg.context_in_dim, false, e));
  TRY(find(f, "time_in.in_layer", f.time_in[0], D, 256, false, e));
  TRY(find(f, "time_in.out_layer", f.time_in[1], D, D, false, e));
  TRY(find(f, "vector_in.in_layer", f.vector_in[0], D, f.cfg.vec_in_dim, false, e));
  TRY(find(f, "vector_in.out_layer", f.vector_in[1], D, D, false, e));
  if (f.cfg.guidance_embed) {
    TRY(find(f, "guidance_in.in_layer", f.guidance_in[0], D, 256, false, e));
    TRY(find(f, "guidance_in.out_layer", f.guidance_in[1], D, D, false, e));
  }
  TRY(find(f, "final_layer.linear", f.final_lin, f.cfg.out_channels, D, false, e));
  TRY(find(f, "modulation", f.modulation, (int)f.n_mod, D, false, e));
  f.dbl.assign(f.cfg.depth, DoubleW{});
  for (int i = 0; i < f.cfg.depth; ++i) {
    const std::string pf = "double_blocks." + std::to_string(i) + ".";
    const char* st[2] = {"img", "txt"};
    for (int k = 0; k < 2; ++k) {
      const std::string a = pf + st[k] + "_attn.", m = pf + st[k] + "_mlp.";
      TRY(find(f, a + "qkv", f.dbl[i].qkv[k], 3 * D, D, false, e));
      TRY(find(f, a + "proj", f.dbl[i].proj[k], D, D, false, e));
      TRY(find(f, m + "0", f.dbl[i].mlp0[k], mlp, D, false, e));
      TRY(find(f, m + "2", f.dbl[i].mlp2[k], D, mlp, false, e));
      TRY(find_scale(f, a + "norm.query_norm.scale", f.dbl[i].qs[k], e));
      TRY(find_scale(f, a + "norm.key_norm.scale", f.dbl[i].ks[k], e));
      f.dbl[i].mod[k] = f.mod_off[pf + st[k] + "_mod.lin"];
    }
    double q[2], k2[2];
    for (int k = 0; k < 2; ++k) { TRY(scale_absmax(f.dbl[i].qs[k], q[k], e)); TRY(scale_absmax(f.dbl[i].ks[k], k2[k], e)); }
    f.dbl[i].bound = logit_bound_of(q[0] > q[1] ? q[0] : q[1], k2[0] > k2[1] ? k2[0] : k2[1]);
  }
  f.sgl.assign(f.cfg.depth_single_blocks, SingleW{});
  for (int i = 0; i < f.cfg.depth_single_blocks; ++i) {
    const std::string pf = "single_blocks." + std::to_string(i) + ".";
    Lin l1;
    TRY(find(f, pf + "linear1", l1, 3 * D + mlp, D, false, e));
    SingleW& w = f.sgl[i];
    w.qkv = l1; w.qkv.N = 3 * D;                                  // linear1's rows [0, 3D) -> qkv, the rest -> mlp (layers.py:236)
    w.mlp = l1; w.mlp.N = mlp;
    w.mlp.w = (const bf16_t*)l1.w + (int64_t)3 * D * l1.ldw;
    w.mlp.b = l1.b ? (const void*)((const bf16_t*)l1.b + 3 * D) : nullptr;
    TRY(find(f, pf + "linear2", w.lin2, D, D + mlp, false, e));
    TRY(find_scale(f, pf + "norm.query_norm.scale", w.qs, e));
    TRY(find_scale(f, pf + "norm.key_norm.scale", w.ks, e));
    w.mod = f.mod_off[pf + "modulation.lin"];
    double q, k;
    TRY(scale_absmax(w.qs, q, e)); TRY(scale_absmax(w.ks, k, e));
    w.bound = logit_bound_of(q, k);
  }
  f.final_mod = f.mod_off["final_layer.adaLN_modulation.1"];
  {  // the LoRA pairs (read in lora_mode 1 only)
    const char* plain[] = {"img_in", "txt_in", "final_layer.linear"};
    const Lin* plain_l[] = {&f.img_in, &f.txt_in, &f.final_lin};
    for (int i = 0; i < 3; ++i) TRY(attach_lora(f, plain[i], *plain_l[i], 0, e));
    const char* emb[] = {"time_in", "vector_in", "guidance_in"};
    Lin* emb_l[] = {f.time_in, f.vector_in, f.guidance_in};
    for (int i = 0; i < (f.cfg.guidance_embed ? 3 : 2); ++i) {
      TRY(attach_lora(f, std::string(emb[i]) + ".in_layer", emb_l[i][0], 0, e));
      TRY(attach_lora(f, std::string(emb[i]) + ".out_layer", emb_l[i][1], 0, e));
    }
    for (int i = 0; i < f.cfg.depth; ++i) {
      const std::string pf = "double_blocks." + std::to_string(i) + ".";
      const char* st[2] = {"img", "txt"};
      for (int k = 0; k < 2; ++k) {
        TRY(attach_lora(f, pf + st[k] + "_attn.qkv", f.dbl[i].qkv[k], 0, e));
        TRY(attach_lora(f, pf + st[k] + "_attn.proj", f.dbl[i].proj[k], 0, e));
        TRY(attach_lora(f, pf + st[k] + "_mlp.0", f.dbl[i].mlp0[k], 0, e));
        TRY(attach_lora(f, pf + st[k] + "_mlp.2", f.dbl[i].mlp2[k], 0, e));
      }
    }
    for (int i = 0; i < f.cfg.depth_single_blocks; ++i) {
      const std::string pf = "single_blocks." + std::to_string(i) + ".";
      TRY(attach_lora(f, pf + "linear1", f.sgl[i].qkv, 0, e));          // linear1's two row ranges share lora_A
      TRY(attach_lora(f, pf + "linear1", f.sgl[i].mlp, 3 * D, e));
      TRY(attach_lora(f, pf + "linear2", f.sgl[i].lin2, 0, e));
    }
    // every modulation Linear as the rows of the stacked matrix it owns, in stacking order
    std::vector<std::pair<int64_t, std::string>> order;
    for (const auto& kv : f.mod_off) order.push_back({kv.second, kv.first});
    std::sort(order.begin(), order.end());
    for (size_t i = 0; i < order.size(); ++i) {
      const int64_t off = order[i].first, end = i + 1 < order.size() ? order[i + 1].first : f.n_mod;
      Lin l = f.modulation;
      l.N = (int)(end - off);
      l.w = (const bf16_t*)f.modulation.w + off * f.modulation.ldw;
      l.b = f.modulation.b ? (const void*)((const bf16_t*)f.modulation.b + off) : nullptr;
      TRY(attach_lora(f, order[i].second, l, 0, e));
      f.mods.push_back({l, off});
    }
  }
  f.resolved = true;
  return VC_OK;
}

// ---------------------------------------------------------------- launch helpers
// qkv projections: with fuse_vt the V third leaves the GEMM transposed into VT (EPI_QKV); with head-permuted weights (option
// qkv_heads) C receives the logical columns and, with fuse_knorm, the key heads leave QK-normed and rotated - and with fuse_qnorm
// the query heads too, times the softmax scale (VcGemmProblem.qn_prescale): no pre-pass, no prologue arithmetic in the attention
int attention_variant(const Flux& f);
// (where the one-wave-per-SIMD attention kernel runs: small geometries keep ONE pre-pass launch for q and k - the fused
// epilogue needs the 256x192 tile, which their short M does not fill)
// (the un-merged LoRA mode completes a Linear's output only after a second GEMM: nothing rides the projection's epilogue there)
bool vt_in_gemm(const Flux& f) { return f.opt.fuse_vt && !f.opt.lora_mode; }
bool kn_in_gemm(const Flux& f) {
  return f.opt.fuse_knorm && f.opt.qkv_heads > 0 && !f.opt.lora_mode && vcplan::decode_variant(attention_variant(f)).wave64;
}
bool qn_in_gemm(const Flux& f) { return kn_in_gemm(f) && f.opt.fuse_qnorm >= 2; }
int qkv_epi(const Flux& f) { return vt_in_gemm(f) || f.opt.qkv_heads > 0 ? VC_EPI_QKV : VC_EPI_BIAS; }
void with_vt(Flux& f, VcGemmProblem& p, int rows, int row0, const void* q_scale, const void* k_scale) {
  if (vt_in_gemm(f)) { p.vt = f.VT; p.vt_bstride = (int64_t)f.H * 128 * f.Lp; p.vt_col0 = 2 * f.D; p.vt_lpad = f.Lp; }
  if (f.opt.qkv_heads > 0) {
    p.kn_heads = f.opt.qkv_heads;
    if (kn_in_gemm(f)) { p.kn_scale = k_scale; p.kn_rope = f.ROPE; p.kn_rope_bstride = (int64_t)f.L * 128; }
    if (qn_in_gemm(f)) { p.qn_scale = q_scale; p.qn_prescale = 1; }
  }
  if (vt_in_gemm(f) || f.opt.qkv_heads > 0) { p.vt_rpb = rows; p.vt_row0 = row0; }
}

VcGemmProblem prob(const void* A, int64_t lda, const Lin& w, void* C, int64_t ldc, int M) {
  VcGemmProblem p;
  memset(&p, 0, sizeof(p));
  p.A = A; p.W = w.w; p.bias = w.b; p.C = C;
  p.lda = lda; p.ldw = w.ldw; p.ldc = ldc;
  p.M = M; p.N = w.N; p.K = w.K;
  p.rows_per_batch = M;
  return p;
}
// vc_flux_profile: an event in front of and behind a launch of the plan (one pair per launch, taken from a pool that grows on demand)
int prof_event(Flux& f, hipStream_t s, Err e) {
  if (f.prof_used == f.prof_ev.size()) {
    hipEvent_t ev;
    HIP(hipEventCreate(&ev), "hipEventCreate");
    f.prof_ev.push_back(ev);
  }
  HIP(hipEventRecord(f.prof_ev[f.prof_used++], s), "hipEventRecord");
  return VC_OK;
}
int prof_open(Flux& f, hipStream_t s, int kind, int epi, int n, int k, double flops, double bytes, Err e) {
  if (!f.prof_on) return VC_OK;
  f.prof_recs.push_back(Flux::ProfRec{kind, epi, n, k, flops, bytes, f.prof_used});
  return prof_event(f, s, e);
}
int prof_close(Flux& f, hipStream_t s, Err e) { return f.prof_on ? prof_event(f, s, e) : VC_OK; }

int gemm1(Flux& f, const VcGemmProblem& p, int epi, hipStream_t s, Err e) {     // one problem, no split-K scratch
  VcGemmArgs a;
  memset(&a, 0, sizeof(a));
  a.p[0] = p; a.nprob = 1; a.epi = epi;
  TRY(prof_open(f, s, VC_LAUNCH_GEMM, epi, p.N, p.K, 2.0 * p.M * p.N * p.K, 0, e));
  TRY(vc_gemm_launch(a, f.opt.tile_cfg, s, e.buf, e.len));
  return prof_close(f, s, e);
}

// lora_mode 1: LinearLora.forward with the reference's three roundings (models/modules/lora.py:92-98), then the Linear's epilogue as
// its own pass -
//   y = bf16(x W^T + b);  h = bf16(x A^T);  y = bf16(y + bf16(bf16(h B^T + b_B) * scale));  C = epilogue(y)
// the lora branch joins through the gated-residual epilogue with the scale vector as its gate.  `p` is the problem the merged plan
// would launch with `epi`: its A / C row descriptions, its residual and its gate.  A Linear without a pair runs the first step alone.
int lora_linear(Flux& f, VcGemmProblem p, int epi, const int32_t* step_ptr, int64_t gate_step_stride, hipStream_t s, Err e) {
  if (epi == VC_EPI_QKV) FAIL(VC_ERR_STATE, "flux: lora_mode 1 runs no fused qkv epilogue");
  if (f.B == 1) { p.a_rpb = p.c_rpb = 0; p.a_bstride = p.c_bstride = 0; }        // one sample: plain rows
  const int M = p.M, N = p.N;
  const bool plain = epi == VC_EPI_BIAS;
  auto it = f.lora_of.find(p.W);
  const Lora* lo = it == f.lora_of.end() ? nullptr : &it->second;
  // scratch rows: those of C where C's are batch-strided (a residual must share C's layout), else M plain rows of N
  const bool strided = plain && p.c_rpb > 0;
  const int64_t ldy = strided ? p.ldc : N;
  const int64_t extent = strided ? (int64_t)((M - 1) / p.c_rpb) * p.c_bstride + (int64_t)p.c_rpb * p.ldc : (int64_t)M * N;
  if (extent > f.ly_elems || (lo && ((int64_t)M * lo->rank > f.lh_elems || N > f.lscale_elems)))
    FAIL(VC_ERR_STATE, "flux: the workspace was sized before lora_mode / the LoRA ranks changed: ask vc_flux_workspace_bytes and prepare again");
  VcGemmProblem base = p;
  base.res = nullptr; base.gate = nullptr; base.ldres = 0; base.gate_bstride = 0; base.rows_per_batch = M;
  bf16_t* y = (bf16_t*)p.C;
  if (!(plain && !lo)) { y = f.LY; base.C = y; base.ldc = ldy; if (!strided) { base.c_rpb = 0; base.c_bstride = 0; } }
  TRY(gemm1(f, base, VC_EPI_BIAS, s, e));                                              // base_out
  if (lo) {
    VcGemmProblem a = base;                                                            // lora_A(x)
    a.W = lo->a; a.ldw = lo->lda; a.bias = nullptr; a.N = lo->rank;
    a.C = f.LH; a.ldc = lo->rank; a.c_rpb = 0; a.c_bstride = 0;
    TRY(gemm1(f, a, VC_EPI_BIAS, s, e));
    VcGemmProblem b;                                                                   // base_out + lora_B(.) * scale
    memset(&b, 0, sizeof(b));
    b.A = f.LH; b.lda = lo->rank; b.W = lo->b; b.ldw = lo->ldb; b.bias = lo->bb;
    b.M = M; b.N = N; b.K = lo->rank; b.rows_per_batch = M;
    b.res = y; b.ldres = ldy; b.gate = f.LSCALE;
    if (plain) { b.C = p.C; b.ldc = p.ldc; b.c_rpb = p.c_rpb; b.c_bstride = p.c_bstride; }
    else { b.C = f.LY2; b.ldc = N; }
    TRY(gemm1(f, b, VC_EPI_GATE_RES, s, e));
    y = (bf16_t*)b.C;
  }
  if (plain) return VC_OK;
  const double bytes = 4.0 * M * N;
  if (epi == VC_EPI_GELU || epi == VC_EPI_SILU) {
    TRY(prof_open(f, s, VC_LAUNCH_PASS, epi, N, 0, 0, bytes, e));
    TRY(vc_act2d_launch(y, N, p.C, p.ldc, M, N, epi == VC_EPI_GELU ? 0 : 1, s, e.buf, e.len));
    return prof_close(f, s, e);
  }
  // the gated residual: one pass per sample (the gate is the sample's modulation row)
  const int rpb = p.rows_per_batch;
  for (int r0 = 0; r0 < M; r0 += rpb) {
    const int rows = std::min(rpb, M - r0);
    TRY(prof_open(f, s, VC_LAUNCH_PASS, epi, N, 0, 0, 6.0 * rows * N, e));
    TRY(vc_gate_residual_launch(y + (int64_t)r0 * N, N, (const bf16_t*)p.res + (int64_t)r0 * p.ldres, p.ldres,
                                (const bf16_t*)p.gate + (int64_t)(r0 / rpb) * p.gate_bstride, (bf16_t*)p.C + (int64_t)r0 * p.ldc, p.ldc,
                                rows, N, step_ptr, gate_step_stride, s, e.buf, e.len));
    TRY(prof_close(f, s, e));
  }
  return VC_OK;
}

int gemm(Flux& f, const VcGemmProblem* ps, int n, int epi, const int32_t* step_ptr, int64_t gate_step_stride, hipStream_t s, Err e) {
  if (f.opt.lora_mode) {      // one Linear after the other, as the reference's modules run
    for (int i = 0; i < n; ++i) TRY(lora_linear(f, ps[i], epi, step_ptr, gate_step_stride, s, e));
    return VC_OK;
  }
  VcGemmArgs a;
  memset(&a, 0, sizeof(a));
  for (int i = 0; i < n; ++i) a.p[i] = ps[i];
  a.nprob = n; a.epi = epi; a.step_ptr = step_ptr; a.gate_step_stride = gate_step_stride;
  if (f.opt.splitk) { a.splitk_ws = f.SK_WS; a.splitk_ws_bytes = f.sk_ws_bytes; }   // the launcher's cost model decides
  double flops = 0;
  for (int i = 0; i < n; ++i) flops += 2.0 * ps[i].M * ps[i].N * ps[i].K;
  TRY(prof_open(f, s, VC_LAUNCH_GEMM, epi, ps[0].N, ps[0].K, flops, 0, e));
  TRY(vc_gemm_launch(a, f.opt.tile_cfg, s, e.buf, e.len));
  return prof_close(f, s, e);
}
int lin(Flux& f, const Lin& w, const void* A, int64_t lda, void* C, int64_t ldc, int M, int epi, hipStream_t s, Err e) {
  VcGemmProblem p = prob(A, lda, w, C, ldc, M);
  return gemm(f, &p, 1, epi, nullptr, 0, s, e);
}

struct Ctx {
  const int32_t* step_ptr;
  hipStream_t s;
  int64_t mss;     // MOD step stride (elements); the sample stride is n_mod
};
inline const bf16_t* modp(Flux& f, int64_t off, int idx) { return f.MOD + off + (int64_t)idx * f.D; }

int ln2(Flux& f, const Ctx& c, const DoubleW& w, int idx, Err e) {   // img + txt streams in one launch
  VcLnStream a{f.XI, f.D, f.XH, f.D, modp(f, w.mod[0], idx), modp(f, w.mod[0], idx + 1), f.B * f.N, f.N};
  VcLnStream b{f.XT, f.D, f.XH + (int64_t)f.B * f.N * f.D, f.D, modp(f, w.mod[1], idx), modp(f, w.mod[1], idx + 1), f.B * f.T, f.T};
  TRY(prof_open(f, c.s, VC_LAUNCH_LN_MODULATE, 0, 0, 0, 0, 4.0 * f.B * f.L * f.D, e));      // rows read + written, bf16
  TRY(vc_ln_modulate2_launch(&a, &b, f.n_mod, f.D, c.step_ptr, c.mss, c.s, e.buf, e.len));
  return prof_close(f, c.s, e);
}
int ln1(Flux& f, const Ctx& c, int64_t mod, Err e) {                  // the joint stream X -> XH
  TRY(prof_open(f, c.s, VC_LAUNCH_LN_MODULATE, 0, 0, 0, 0, 4.0 * f.B * f.L * f.D, e));
  TRY(vc_ln_modulate_launch(f.X, f.D, f.XH, f.D, modp(f, mod, 0), modp(f, mod, 1), f.n_mod, f.B * f.L, f.D, f.L, c.step_ptr, c.mss,
                            c.s, e.buf, e.len));
  return prof_close(f, c.s, e);
}

int attention_variant(const Flux& f) {
  if (f.opt.attn_variant >= 0) return f.opt.attn_variant;
  return vcplan::attention_variant_by_size(f.B, f.L, f.H, f.n_cu);
}

// QKNorm + RoPE (+ V^T) and the joint attention over QKV -> CAT[:, :D] (layers.py:165-185 / 236-241)
int attention(Flux& f, const Ctx& c, const void* q1, const void* k1, const void* q2, const void* k2, int split, float block_bound, Err e) {
  const int variant = attention_variant(f);
  const bool fused_q = vcplan::decode_variant(variant).wave64 && f.opt.fuse_qnorm, q_done = qn_in_gemm(f);     // q_done: by the projection's epilogue, prescaled
  const int64_t ld = 3 * f.D, ldo = f.D + f.mlp;
  const int parts = (kn_in_gemm(f) ? 0 : VC_QKN_K) | (fused_q ? 0 : VC_QKN_Q) | (vt_in_gemm(f) ? 0 : VC_QKN_VT);
  if (parts)
    TRY(vc_qknorm_rope_vt_launch(f.QKV, ld, f.L * ld, q1, k1, q2, k2, split, f.ROPE, (int64_t)f.L * 128, f.VT, f.B, f.L, f.Lp, f.H,
                                 parts, c.s, e.buf, e.len));
  VcAttention a;
  memset(&a, 0, sizeof(a));
  a.qkv = f.QKV; a.ld = ld; a.bstride = f.L * ld;
  a.vt = f.VT; a.out = f.CAT; a.ldo = ldo; a.out_bstride = f.L * ldo;
  a.kv_len = f.ragged ? f.KVLEN : nullptr;
  a.kv_gap = f.gapped ? f.KVGAP : nullptr;
  a.B = f.B; a.L = f.L; a.Lpad = f.Lp; a.H = f.H; a.variant = variant;
  a.scratch = f.ATT_SCRATCH; a.scratch_bytes = f.att_scratch_bytes;
  if (q_done) a.q_prescaled = 1;
  else if (fused_q) { a.q_scale = q1; a.q_scale2 = q2; a.split = split; a.rope = f.ROPE; a.rope_bstride = (int64_t)f.L * 128; }
  // option logit_bound_milli > 0 switches the bounded softmax on; every block is then held to ITS OWN bound (never above the
  // caller's): a checkpoint with a few outlier QK-norm scales runs the running-max template in those blocks only
  const float cap = (float)f.opt.logit_bound_milli * 1e-3f;
  a.logit_bound = f.opt.logit_bound_milli > 0 ? (block_bound < cap ? block_bound : cap) : 0.0f;
  if (f.opt.logit_bound_milli > 0 && !(block_bound < 1e30f)) a.logit_bound = 1e30f;       // (non-finite scales: no bound)
  TRY(prof_open(f, c.s, VC_LAUNCH_ATTENTION, variant, 0, 0, 4.0 * f.L * f.L * f.D * f.B, 0, e));     // the attention launch(es) alone
  TRY(vc_attention_launch(a, c.s, e.buf, e.len));
  return prof_close(f, c.s, e);
}

// DoubleStreamBlock (layers.py:158-196) on XI / XT, in place
int double_block(Flux& f, const Ctx& c, const DoubleW& w, Err e) {
  const int B = f.B, T = f.T, N = f.N, L = f.L, D = f.D, mlp = f.mlp;
  const int64_t ldq = 3 * D, ldc = D + mlp;
  bf16_t* XH_I = f.XH; bf16_t* XH_T = f.XH + (int64_t)B * N * D;
  bf16_t* HID_I = f.HID; bf16_t* HID_T = f.HID + (int64_t)B * N * mlp;
  bf16_t* streams[2] = {f.XI, f.XT};
  const int rows[2] = {N, T};
  TRY(ln2(f, c, w, 0, e));
  {  // qkv of both streams into the joint-order QKV rows (text first): C rows are batch-strided
    VcGemmProblem p[2] = {prob(XH_I, D, w.qkv[0], f.QKV + (int64_t)T * ldq, ldq, B * N), prob(XH_T, D, w.qkv[1], f.QKV, ldq, B * T)};
    p[0].c_rpb = N; p[1].c_rpb = T;
    p[0].c_bstride = p[1].c_bstride = (int64_t)L * ldq;
    with_vt(f, p[0], N, T, w.qs[0], w.ks[0]); with_vt(f, p[1], T, 0, w.qs[1], w.ks[1]);
    TRY(gemm(f, p, 2, qkv_epi(f), nullptr, 0, c.s, e));
  }
  TRY(attention(f, c, w.qs[1], w.ks[1], w.qs[0], w.ks[0], T, w.bound, e));   // rows < T: the text stream's scales
  {  // x += gate * proj(attn): A rows are batch-strided views of CAT[:, :D]
    VcGemmProblem p[2] = {prob(f.CAT + (int64_t)T * ldc, ldc, w.proj[0], f.XI, D, B * N), prob(f.CAT, ldc, w.proj[1], f.XT, D, B * T)};
    for (int k = 0; k < 2; ++k) {
      p[k].res = streams[k]; p[k].ldres = D; p[k].gate = modp(f, w.mod[k], 2); p[k].gate_bstride = f.n_mod;
      p[k].rows_per_batch = rows[k]; p[k].a_rpb = rows[k]; p[k].a_bstride = (int64_t)L * ldc;
    }
    TRY(gemm(f, p, 2, VC_EPI_GATE_RES, c.step_ptr, c.mss, c.s, e));
  }
  TRY(ln2(f, c, w, 3, e));
  {
    VcGemmProblem p[2] = {prob(XH_I, D, w.mlp0[0], HID_I, mlp, B * N), prob(XH_T, D, w.mlp0[1], HID_T, mlp, B * T)};
    TRY(gemm(f, p, 2, VC_EPI_GELU, nullptr, 0, c.s, e));
  }
  {
    VcGemmProblem p[2] = {prob(HID_I, mlp, w.mlp2[0], f.XI, D, B * N), prob(HID_T, mlp, w.mlp2[1], f.XT, D, B * T)};
    for (int k = 0; k < 2; ++k) {
      p[k].res = streams[k]; p[k].ldres = D; p[k].gate = modp(f, w.mod[k], 5); p[k].gate_bstride = f.n_mod; p[k].rows_per_batch = rows[k];
    }
    TRY(gemm(f, p, 2, VC_EPI_GATE_RES, c.step_ptr, c.mss, c.s, e));
  }
  return VC_OK;
}

// SingleStreamBlock (layers.py:232-245) on X, in place
int single_block(Flux& f, const Ctx& c, const SingleW& w, Err e) {
  const int M = f.B * f.L, D = f.D, mlp = f.mlp;
  const int64_t ldc = D + mlp;
  TRY(ln1(f, c, w.mod, e));
  {
    VcGemmProblem p = prob(f.XH, D, w.qkv, f.QKV, 3 * D, M);
    with_vt(f, p, f.L, 0, w.qs, w.ks);
    TRY(gemm(f, &p, 1, qkv_epi(f), nullptr, 0, c.s, e));
  }
  // the attention kernel runs right behind the projection that wrote its operands, and the MLP-up GEMM right in front of the
  // linear2 that reads its 97 MB (option mlp_first = the reference's textual order, layers.py:236-243)
  if (f.opt.mlp_first) TRY(lin(f, w.mlp, f.XH, D, f.CAT + D, ldc, M, VC_EPI_GELU, c.s, e));
  TRY(attention(f, c, w.qs, w.ks, nullptr, nullptr, 0, w.bound, e));
  if (!f.opt.mlp_first) TRY(lin(f, w.mlp, f.XH, D, f.CAT + D, ldc, M, VC_EPI_GELU, c.s, e));
  VcGemmProblem p = prob(f.CAT, ldc, w.lin2, f.X, D, M);
  p.res = f.X; p.ldres = D; p.gate = modp(f, w.mod, 2); p.gate_bstride = f.n_mod; p.rows_per_batch = f.L;
  return gemm(f, &p, 1, VC_EPI_GATE_RES, c.step_ptr, c.mss, c.s, e);
}

int d2d(void* dst, const void* src, int64_t bytes, hipStream_t s, Err e) {
  HIP(hipMemcpyAsync(dst, src, (size_t)bytes, hipMemcpyDeviceToDevice, s), "hipMemcpyAsync");
  return VC_OK;
}

// vc_flux_set_monitor: site `site` of the evaluation `*step_ptr` (row 0 without a counter) <- vc_tensor_stats of the B samples of
// rows x cols contiguous elements at x, one launch (two kernels) on the evaluation's own stream
int monitor(Flux& f, int site, const void* x, bool x_f32, int64_t rows, int cols, const int32_t* step_ptr, hipStream_t s, Err e) {
  if (!f.mon_level || f.mon_paused) return VC_OK;
  const int ns = f.mon_sites();
  return vc_tensor_stats_launch(x, x_f32, rows * cols, cols, f.B, rows, cols, f.mon_log + vcmon::log_index(0, site, 0, f.mon_cap, ns, f.B),
                                vcmon::log_row_stride(ns, f.B), step_ptr, f.mon_cap, f.mon_scratch, s, e.buf, e.len);
}
// the log was sized for the B prepared when the monitor was set: another B would run past its rows
int monitor_fits(Flux& f, const char* what, Err e) {
  if (f.mon_level && f.mon_B && f.mon_B != f.B)
    FAIL(VC_ERR_STATE, "%s: the monitor's log was sized for B = %d, the prepared B is %d: ask vc_flux_monitor_bytes and call vc_flux_set_monitor again",
         what, f.mon_B, f.B);
  if (f.mon_level) f.mon_B = f.B;
  return VC_OK;
}
// a tap site: the residual stream `src` ([B * rows, D] bf16) directly behind its block.  vc_flux_set_tap: tap `idx` <- the stream, one
// copy node on the evaluation's own stream; monitor level 2: its statistics, read in place
int tap(Flux& f, int idx, const bf16_t* src, int rows, const int32_t* step_ptr, hipStream_t s, Err e) {
  if ((size_t)idx < f.taps.size() && f.taps[idx]) {
    const int64_t bytes = (int64_t)f.B * rows * f.D * 2;
    TRY(prof_open(f, s, VC_LAUNCH_TAP, 0, 0, 0, 0, 2.0 * bytes, e));       // every tap in ONE launch class
    TRY(d2d(f.taps[idx], src, bytes, s, e));
    TRY(prof_close(f, s, e));
  }
  return f.mon_level >= 2 ? monitor(f, vcmon::site_of_tap(idx), src, false, rows, f.D, step_ptr, s, e) : VC_OK;
}
int tap_double(Flux& f, int i, const int32_t* step_ptr, hipStream_t s, Err e) {
  TRY(tap(f, vcmon::tap_double(i, false), f.XI, f.N, step_ptr, s, e));
  return tap(f, vcmon::tap_double(i, true), f.XT, f.T, step_ptr, s, e);
}

// Flux.forward on `img_rows` (x || cond in XIN when NULL) -> `out` (V when NULL); with `euler` the solver's update behind it
// (ode_update: the Euler step, or a midpoint / rk4 stage combination).  step_ptr counts EVALUATIONS (= steps for Euler).
// in three pieces, which `evaluate` issues back to back (the plan of every evaluation without the step cache) and the cached step
// issues with its own launches in between: the inputs, the blocks from double block `first` on, the last layer + update.
// where the sample in flight keeps its ODE state (in the caller's dtype), and the bf16 rows the next evaluation reads: the state
// itself for a bf16 Euler step, XS as the bf16 shadow of an f32 Euler state, else YIN - the stage input of a midpoint / rk4 step
constexpr int SOLVER_DOPRI5 = 100;     // Flux::method of the adaptive solve: no VC_SOLVER_* code (vc_solver_evals keeps refusing it)
constexpr int SOLVER_SDE_EULER = 101, SOLVER_SDE_HEUN = 102;     // ... of the stochastic sampler: likewise (one captured step per method)
void* ode_state(Flux& f) { return f.state_f32 ? (void*)f.XS32 : (void*)f.XS; }
int64_t ode_state_bytes(const Flux& f) { return (int64_t)f.B * f.N * f.cfg.out_channels * (f.state_f32 ? 4 : 2); }
bf16_t* next_input(Flux& f) { return f.method == VC_SOLVER_EULER ? f.XS : f.YIN; }
// the solver's update behind an evaluation (v = V), or with v null next_input = bf16(state) alone; next_input is not handed over
// where it IS the state (the kernel's pointers are __restrict__)
int ode_update(Flux& f, const void* v, const int32_t* step_ptr, hipStream_t s, Err e) {
  if (f.method == SOLVER_DOPRI5)      // the stage of the adaptive solve is the device-side counter itself
    return vc_dopri5_stage_launch(-1, f.AD_Y0, f.AD_K, v, f.AD_DT, step_ptr, f.AD_Y1, f.YIN, (int64_t)f.B * f.N * f.cfg.out_channels, s,
                                  e.buf, e.len);
  if (f.method == SOLVER_SDE_EULER || f.method == SOLVER_SDE_HEUN)      // the table row of the update is the device-side counter itself
    return vc_sde_stage_launch(-1, f.SD_TAB, f.S + 1, f.SD_Y, v, f.YIN, f.SD_XHAT, f.SD_K1, f.SD_RNG, step_ptr,
                               (int64_t)f.B * f.N * f.cfg.out_channels, s, e.buf, e.len);
  void* y = ode_state(f);
  bf16_t* y_in = next_input(f);
  return vc_ode_update_launch("ode_update", f.method, -1, y, !f.state_f32, v, f.KS, y_in == y ? nullptr : y_in, f.DTS, step_ptr,
                              (int64_t)f.B * f.N * f.cfg.out_channels, s, e.buf, e.len);
}

int eval_inputs(Flux& f, bool concat, const void* img_rows, const int32_t* step_ptr, hipStream_t s, Err e) {
  const int B = f.B, T = f.T, N = f.N, D = f.D;
  const int in_ch = f.cfg.in_channels, out_ch = f.cfg.out_channels;
  if (concat) TRY(vc_concat_cols_launch(next_input(f), out_ch, f.COND, in_ch - out_ch, f.XIN, (int64_t)B * N, s, e.buf, e.len));
  TRY(d2d(f.XT, f.TXT0, (int64_t)B * T * D * 2, s, e));
  TRY(lin(f, f.img_in, img_rows ? img_rows : f.XIN, in_ch, f.XI, D, B * N, VC_EPI_BIAS, s, e));
  TRY(tap(f, vcmon::tap_img_in(), f.XI, N, step_ptr, s, e));
  return tap(f, vcmon::tap_txt_in(), f.XT, T, step_ptr, s, e);
}
int eval_blocks(Flux& f, const Ctx& c, size_t first, Err e) {
  const int B = f.B, T = f.T, N = f.N, L = f.L, D = f.D;
  hipStream_t s = c.s;
  for (size_t i = first; i < f.dbl.size(); ++i) { TRY(double_block(f, c, f.dbl[i], e)); TRY(tap_double(f, (int)i, c.step_ptr, s, e)); }
  for (int b = 0; b < B; ++b) {   // cat((txt, img), 1) per sample (model.py:116)
    TRY(d2d(f.X + (int64_t)b * L * D, f.XT + (int64_t)b * T * D, (int64_t)T * D * 2, s, e));
    TRY(d2d(f.X + ((int64_t)b * L + T) * D, f.XI + (int64_t)b * N * D, (int64_t)N * D * 2, s, e));
  }
  for (size_t i = 0; i < f.sgl.size(); ++i) {
    TRY(single_block(f, c, f.sgl[i], e));
    TRY(tap(f, vcmon::tap_single(f.cfg.depth, (int)i), f.X, L, c.step_ptr, s, e));
  }
  return VC_OK;
}
int eval_output(Flux& f, const Ctx& c, void* out, bool euler, Err e) {
  const int B = f.B, T = f.T, N = f.N, L = f.L, D = f.D;
  const int out_ch = f.cfg.out_channels;
  const int32_t* step_ptr = c.step_ptr;
  hipStream_t s = c.s;
  // LastLayer (layers.py:248-259) on the image rows
  TRY(ln1(f, c, f.final_mod, e));
  VcGemmProblem p = prob(f.XH + (int64_t)T * D, D, f.final_lin, out ? out : f.V, out_ch, B * N);
  p.a_rpb = N; p.a_bstride = (int64_t)L * D;
  TRY(gemm(f, &p, 1, VC_EPI_BIAS, nullptr, 0, s, e));
  TRY(monitor(f, vcmon::SITE_V, out ? out : f.V, false, N, out_ch, step_ptr, s, e));       // the model's output, before any combine
  if (euler) {
    if (f.cfg_active) {     // V is sample-major: its first half is the conditional samples' velocity, combined in place
      const int64_t half = (int64_t)(B / 2) * N * out_ch;
      TRY(vc_cfg_combine_launch(f.V, f.V + half, f.V, half, f.cfg_s, s, e.buf, e.len));
    }
    TRY(ode_update(f, f.V, step_ptr, s, e));
    TRY(monitor(f, vcmon::SITE_X, ode_state(f), f.state_f32, N, out_ch, step_ptr, s, e));
    TRY(vc_step_advance_launch((int32_t*)step_ptr, s, e.buf, e.len));
  }
  return VC_OK;
}
int evaluate(Flux& f, const int32_t* step_ptr, bool concat, const void* img_rows, void* out, bool euler, hipStream_t s, Err e) {
  Ctx c{step_ptr, s, (int64_t)f.B * f.n_mod};
  TRY(eval_inputs(f, concat, img_rows, step_ptr, s, e));
  TRY(eval_blocks(f, c, 0, e));
  return eval_output(f, c, out, euler, e);
}

// ---- the step cache: one Euler evaluation as head + ONE of two tails, chosen by the host from the metric
// head: the plan up to double block 0 (h0 is parked in X, which nothing uses before the streams are joined), then r, the metric and
// its 4-byte copy to pinned host memory
int cache_head(Flux& f, hipStream_t s, Err e) {
  const int64_t nd = (int64_t)f.N * f.D;
  Ctx c{f.STEP, s, (int64_t)f.B * f.n_mod};
  TRY(eval_inputs(f, true, nullptr, f.STEP, s, e));
  TRY(d2d(f.X, f.XI, f.B * nd * 2, s, e));                                   // h0
  TRY(double_block(f, c, f.dbl[0], e));                                      // XI = h1
  TRY(tap_double(f, 0, f.STEP, s, e));
  TRY(vc_residual_change_launch(f.X, f.XI, f.SC_P, f.SC_RS, nullptr, f.SC_METRIC, f.SC_PART, f.B, nd, s, e.buf, e.len));
  HIP(hipMemcpyAsync(f.sc_host, f.SC_METRIC, sizeof(float), hipMemcpyDeviceToHost, s), "hipMemcpyAsync(D2H)");
  return VC_OK;
}
// tail-compute: P <- r, the scratch keeps h1, blocks 1..end, R <- hE - h1, then the last layer and the update as ever
int cache_tail_compute(Flux& f, bool euler, hipStream_t s, Err e) {
  const int64_t nd = (int64_t)f.N * f.D;
  Ctx c{f.STEP, s, (int64_t)f.B * f.n_mod};
  TRY(d2d(f.SC_P, f.SC_RS, f.B * nd * 2, s, e));
  TRY(d2d(f.SC_RS, f.XI, f.B * nd * 2, s, e));
  TRY(eval_blocks(f, c, 1, e));
  TRY(vc_residual_op_launch(0, f.X + (int64_t)f.T * f.D, (int64_t)f.L * f.D, f.SC_RS, nd, f.SC_R, nd, f.B, nd, s, e.buf, e.len));
  return eval_output(f, c, nullptr, euler, e);
}
// tail-reuse: the image rows of X <- h1 + R (its text rows keep the last computed evaluation's: the last layer reads image rows only)
int cache_tail_reuse(Flux& f, bool euler, hipStream_t s, Err e) {
  const int64_t nd = (int64_t)f.N * f.D;
  Ctx c{f.STEP, s, (int64_t)f.B * f.n_mod};
  TRY(vc_residual_op_launch(1, f.XI, nd, f.SC_R, nd, f.X + (int64_t)f.T * f.D, (int64_t)f.L * f.D, f.B, nd, s, e.buf, e.len));
  return eval_output(f, c, nullptr, euler, e);
}

// ---------------------------------------------------------------- host staging
int stage_begin(Flux& f, size_t bytes, Err e) {
  if (f.staged_pending) { HIP(hipEventSynchronize(f.staged), "hipEventSynchronize"); f.staged_pending = false; }
  if (bytes > f.pinned_bytes) {
    if (f.pinned) (void)hipHostFree(f.pinned);
    f.pinned = nullptr; f.pinned_bytes = 0;
    HIP(hipHostMalloc((void**)&f.pinned, bytes, hipHostMallocDefault), "hipHostMalloc");
    f.pinned_bytes = bytes;
  }
  f.pinned_used = 0;
  return VC_OK;
}
template <class T> T* stage_take(Flux& f, size_t count) {
  T* p = (T*)(f.pinned + f.pinned_used);
  f.pinned_used += (size_t)align256((int64_t)(count * sizeof(T)));
  return p;
}
int stage_send(Flux& f, void* dst, const void* staged, size_t bytes, hipStream_t s, Err e) {
  HIP(hipMemcpyAsync(dst, staged, bytes, hipMemcpyHostToDevice, s), "hipMemcpyAsync(H2D)");
  return VC_OK;
}
int stage_end(Flux& f, hipStream_t s, Err e) {
  if (!f.staged) HIP(hipEventCreateWithFlags(&f.staged, hipEventDisableTiming), "hipEventCreate");
  HIP(hipEventRecord(f.staged, s), "hipEventRecord");
  f.staged_pending = true;
  return VC_OK;
}

inline float bf16_round(float v) {   // round-to-nearest-even through bf16 (finite inputs)
  uint32_t u;
  memcpy(&u, &v, 4);
  u += 0x7fffu + ((u >> 16) & 1u);
  u &= 0xffff0000u;
  memcpy(&v, &u, 4);
  return v;
}

// timestep embedding -> time_in MLP -> vec = time + guidance + vector -> every modulation of every (step, sample):
// model.py:102-108 + layers.py:120-126 for all modules in ONE GEMM.  times: rows s*B + b already in TS.
int time_precompute(Flux& f, int S, int timesteps_is_bf16, hipStream_t s, Err e) {
  const int B = f.B, D = f.D, M = S * B;
  TRY(vc_temb_launch(f.TS, f.FREQS, f.TEMB, M, 128, timesteps_is_bf16, s, e.buf, e.len));
  TRY(lin(f, f.time_in[0], f.TEMB, 256, f.H1, D, M, VC_EPI_SILU, s, e));
  TRY(lin(f, f.time_in[1], f.H1, D, f.TVEC, D, M, VC_EPI_BIAS, s, e));
  if (f.cfg.guidance_embed)
    TRY(vc_add3_launch(f.TVEC, f.GVEC, f.YVEC, f.VEC, (int64_t)M * D, (int64_t)B * D, (int64_t)B * D, s, e.buf, e.len));
  else
    TRY(vc_add3_launch(f.TVEC, f.YVEC, nullptr, f.VEC, (int64_t)M * D, (int64_t)B * D, 1, s, e.buf, e.len));
  TRY(vc_silu_launch(f.VEC, f.H1, (int64_t)M * D, s, e.buf, e.len));
  if (!f.opt.lora_mode) return lin(f, f.modulation, f.H1, D, f.MOD, f.n_mod, M, VC_EPI_BIAS, s, e);
  for (const auto& m : f.mods) TRY(lin(f, m.first, f.H1, D, f.MOD + m.second, f.n_mod, M, VC_EPI_BIAS, s, e));   // each on its own columns of MOD
  return VC_OK;
}

void drop_prof(Flux& f) {
  for (auto ev : f.prof_ev) (void)hipEventDestroy(ev);
  f.prof_ev.clear();
}
void drop_graph(Flux& f) {
  f.graphs.clear();
  f.step = Flux::Step{};
}

// the hipGraph of ONE evaluation + the solver's update behind it (Euler: one solver step): everything that depends on the
// evaluation (modulation rows, dt, the stage of a midpoint / rk4 step) is indexed on the device by STEP
int step_graph(Flux& f, hipStream_t s, Err e) {
  Flux::Key k{f.base, f.B, f.T, f.N, f.S, f.ragged, f.gapped, attention_variant(f), f.state_f32, f.method, f.sc_active, f.opt, s,
               f.cfg_active, 0, {}, f.mon_level, f.mon_cap, f.mon_log, f.mon_scratch};
  if (f.cfg_active) memcpy(&k.cfg_bits, &f.cfg_s, 4);
  k.taps = f.taps;
  if (const Flux::Step* hit = f.graphs.find(k)) {
    f.step = *hit; f.key = k;
    return VC_OK;
  }
  f.step = Flux::Step{};
  Flux::Step st;
  int rc = VC_OK;
  if (!f.sc_active) {
    // warm-up outside capture (kernel attributes are set on first launch): one evaluation into V, the state is untouched
    TRY(evaluate(f, f.STEP, true, nullptr, nullptr, false, s, e));
    rc = capture(s, st.g[0], e, [&] { return evaluate(f, f.STEP, true, nullptr, nullptr, true, s, e); }, &st.nodes[0]);
  } else {
    // the same warm-up through the three pieces (P, R and the scratch it writes are rewritten by the trajectory's first evaluation,
    // which always computes, before anything reads them)
    TRY(cache_head(f, s, e));
    TRY(cache_tail_compute(f, false, s, e));
    TRY(cache_tail_reuse(f, false, s, e));
    rc = capture(s, st.g[0], e, [&] { return cache_head(f, s, e); }, &st.nodes[0]);
    if (rc == VC_OK) rc = capture(s, st.g[1], e, [&] { return cache_tail_compute(f, true, s, e); }, &st.nodes[1]);
    if (rc == VC_OK) rc = capture(s, st.g[2], e, [&] { return cache_tail_reuse(f, true, s, e); }, &st.nodes[2]);
  }
  if (rc != VC_OK) {
    Flux::DropStep()(st);          // the graphs of a half-captured step
    return rc;
  }
  f.graphs.insert(k, st);
  f.step = st; f.key = k;
  return VC_OK;
}

// lora_mode 1: what vc_flux_prepare parked in the workspace (txt_in, vector_in, guidance_in) ran with the scale of that moment
int fresh_scale(const Flux& f, const char* what, Err e) {
  if (f.opt.lora_mode && f.scale_stale)
    FAIL(VC_ERR_STATE, "%s: the lora scale changed after vc_flux_prepare, whose txt_in / vector_in / guidance_in projections ran with the old "
                       "one: call vc_flux_prepare again (captured steps are kept)", what);
  return VC_OK;
}

}  // namespace

int vc_flux_create_impl(const VcFluxConfig* cfg, void** handle, char* err, int errlen) {
  Err e{err, errlen};
  if (!cfg || !handle) FAIL(VC_ERR_ARG, "flux_create: null argument");
  if (cfg->hidden_size <= 0 || cfg->num_heads <= 0 || cfg->hidden_size != cfg->num_heads * 128)
    FAIL(VC_ERR_ARG, "flux_create: hidden_size must be num_heads * 128 (the gfx950 attention kernels are specialised for head_dim 128)");
  if (cfg->axes_dim[0] + cfg->axes_dim[1] + cfg->axes_dim[2] != 128 || (cfg->axes_dim[0] | cfg->axes_dim[1] | cfg->axes_dim[2]) & 1)
    FAIL(VC_ERR_ARG, "flux_create: axes_dim must be even and sum to 128");
  if (cfg->in_channels <= cfg->out_channels || cfg->out_channels <= 0 || cfg->depth < 0 || cfg->depth_single_blocks < 0 || cfg->mlp_hidden <= 0)
    FAIL(VC_ERR_ARG, "flux_create: bad channel / depth configuration");
  Flux* f = new Flux();
  f->cfg = *cfg;
  f->D = cfg->hidden_size; f->H = cfg->num_heads; f->mlp = cfg->mlp_hidden;
  layout_modulation(*f);
  f->keys = vckeys::build(*cfg);
  f->taps.assign((size_t)vcmon::tap_count(cfg->depth, cfg->depth_single_blocks), nullptr);
  // without a ROCm device the handle still answers its host-only calls (vc_flux_mod_offset, vc_flux_load_key / _tensor / _bytes,
  // vc_flux_bound); whatever touches the device then fails with the runtime's own error
  int dev = 0;
  hipDeviceProp_t p;
  if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&p, dev) == hipSuccess) {
    f->n_cu = p.multiProcessorCount;
    if (hipEventCreateWithFlags(&f->staged, hipEventDisableTiming) != hipSuccess) { delete f; FAIL(VC_ERR_HIP, "flux_create: hipEventCreate failed"); }
  }
  *handle = f;
  return VC_OK;
}

int vc_flux_destroy_impl(void* handle, char* err, int errlen) {
  HANDLE(Flux, f, "flux");
  if (f.staged_pending) (void)hipEventSynchronize(f.staged);
  drop_graph(f);
  drop_prof(f);
  if (f.pinned) (void)hipHostFree(f.pinned);
  if (f.sc_host) (void)hipHostFree(f.sc_host);
  if (f.ad_host) (void)hipHostFree(f.ad_host);
  if (f.staged) (void)hipEventDestroy(f.staged);
  delete &f;
  return VC_OK;
}

int vc_flux_bind_weight_impl(void* handle, const char* name, const void* w, const void* bias, int32_t rows, int32_t cols, int64_t ldw,
                             char* err, int errlen) {
  HANDLE(Flux, f, "flux");
  if (!name || !w || rows <= 0 || cols <= 0 || ldw < cols) FAIL(VC_ERR_ARG, "flux_bind_weight: bad arguments for '%s'", name ? name : "?");
  // the optional split-K scratch decides whether 100 MB are carved into EVERY workspace: binding it for the first time after a
  // workspace has been sized would silently change the carve-up of buffers the caller already holds (advisor r05)
  if (!strcmp(name, "splitk_ws") && f.ws_sized && f.bound.find("splitk_ws") == f.bound.end())
    FAIL(VC_ERR_STATE, "flux_bind_weight: bind 'splitk_ws' BEFORE the first vc_flux_workspace_bytes / vc_flux_prepare (it changes the size and "
                       "layout of every workspace)");
  Lin l;
  l.w = w; l.b = bias; l.N = rows; l.K = cols; l.ldw = ldw;
  f.bound[name] = l;
  f.resolved = false;
  f.prepared = false;   // the resolved per-block tables are rebuilt by the next vc_flux_prepare
  drop_graph(f);        // a captured step holds the old pointers
  return VC_OK;
}

// ---------------------------------------------------------------- a checkpoint as stored -> the bound set (vc_flux_load_*)
int vc_flux_load_key_impl(void* handle, int32_t index, char* name, int32_t namelen, int64_t* shape, int32_t* ndim, char* err, int errlen) {
  HANDLE(Flux, f, "flux");
  return vckeys::describe(f.keys, index, name, namelen, shape, ndim, err, errlen);
}

int vc_flux_load_tensor_impl(void* handle, const char* key, const void* ptr, int32_t is_f32, const int64_t* shape, int32_t ndim, char* err,
                             int errlen) {
  HANDLE(Flux, f, "flux");
  const int idx = vckeys::find(f.keys, key);
  if (idx < 0) FAIL(VC_ERR_ARG, "flux_load_tensor: key = '%s' is no state_dict key of this model (vc_flux_load_key lists them)", key ? key : "(null)");
  if (!ptr) { f.loaded.erase(idx); return VC_OK; }
  const vckeys::Key& k = f.keys.keys[idx];
  TRY(vckeys::check_shape(k, shape, ndim, err, errlen));
  const bool factor = k.kind == vckeys::LORA_A || k.kind == vckeys::LORA_B || k.kind == vckeys::LORA_B_BIAS;
  if (factor && is_f32)
    FAIL(VC_ERR_ARG, "flux_load_tensor: is_f32 = 1 for '%s': LoRA factors are merged on the bf16 matrix cores and must be stored as bf16", key);
  if (k.kind == vckeys::LORA_A || k.kind == vckeys::LORA_B) {      // one rank per Linear
    const int key0 = f.keys.linears[k.owner].key0;
    auto other = f.loaded.find(key0 + (k.kind == vckeys::LORA_A ? vckeys::LORA_B : vckeys::LORA_A));
    const int64_t rank = shape[k.kind == vckeys::LORA_A ? 0 : 1];
    if (other != f.loaded.end() && other->second.shape[k.kind == vckeys::LORA_A ? 1 : 0] != rank)
      FAIL(VC_ERR_ARG, "flux_load_tensor: rank = %lld of '%s' differs from the rank %lld of the Linear's other factor", (long long)rank, key,
           (long long)other->second.shape[k.kind == vckeys::LORA_A ? 1 : 0]);
  }
  f.loaded[idx] = Flux::Loaded{ptr, is_f32 != 0, {shape[0], ndim > 1 ? shape[1] : 0}};
  return VC_OK;
}

int64_t vc_flux_load_bytes_impl(void* handle) { return handle ? vckeys::arena_bytes(((Flux*)handle)->keys, ((Flux*)handle)->D) : -1; }

int vc_flux_load_finish_impl(void* handle, float lora_scale, void* arena, int64_t arena_bytes, hipStream_t s, char* err, int errlen) {
  HANDLE(Flux, f, "flux");
  const vckeys::Table& t = f.keys;
  // ---- every check before the device is touched
  if (f.opt.lora_mode)
    FAIL(VC_ERR_ARG, "flux_load_finish: option lora_mode = 1 runs un-merged weights (vc_flux_bind_weight + vc_flux_bind_lora); this call merges");
  if (f.in_flight) FAIL(VC_ERR_STATE, "flux_load_finish: the weights cannot change between vc_flux_sample_begin and vc_flux_sample_end");
  const int64_t need = vckeys::arena_bytes(t, f.D);
  if (!aligned256(arena)) FAIL(VC_ERR_ARG, "flux_load_finish: arena must be a 256-byte aligned device pointer");
  if (arena_bytes < need)
    FAIL(VC_ERR_ARG, "flux_load_finish: arena_bytes = %lld, the prepared set takes %lld (vc_flux_load_bytes)", (long long)arena_bytes, (long long)need);
  auto have = [&](int idx) -> const Flux::Loaded* {
    auto it = f.loaded.find(idx);
    return it == f.loaded.end() ? nullptr : &it->second;
  };
  for (size_t i = 0; i < t.keys.size(); ++i)
    if ((t.keys[i].kind == vckeys::WEIGHT || t.keys[i].kind == vckeys::SCALE) && !have((int)i))
      FAIL(VC_ERR_STATE, "flux_load_finish: '%s' was never recorded (vc_flux_load_tensor)", t.keys[i].name.c_str());
  for (const vckeys::Linear& l : t.linears)
    if (!have(l.key0 + vckeys::LORA_A) != !have(l.key0 + vckeys::LORA_B))
      FAIL(VC_ERR_STATE, "flux_load_finish: '%s' was recorded without the Linear's other factor",
           t.keys[l.key0 + (have(l.key0 + vckeys::LORA_A) ? vckeys::LORA_A : vckeys::LORA_B)].name.c_str());
  // ---- the arena: the formula of vc_flux_load_bytes, in its order
  Carver c{(char*)arena};
  std::vector<std::pair<std::string, Lin>> bind;
  std::vector<bf16_t*> wout(t.linears.size()), bout(t.linears.size());
  for (size_t i = 0; i < t.linears.size(); ++i) {
    const vckeys::Linear& l = t.linears[i];
    if (l.mod_off >= 0) continue;
    wout[i] = c.take<bf16_t>((int64_t)l.out * l.in);
    bout[i] = c.take<bf16_t>(l.out);
  }
  bf16_t* mod_w = c.take<bf16_t>(t.n_mod * f.D);
  bf16_t* mod_b = c.take<bf16_t>(t.n_mod);
  const int n_scales = (int)t.scales.size();
  bf16_t* scales = c.take<bf16_t>((int64_t)128 * n_scales);       // 256 bytes each
  float* amax = c.take<float>(n_scales);
  // ---- one merge launch per Linear (a modulation Linear without any bias leaves zeros in the stacked bias, as Flux.prepare does)
  HIP(hipMemsetAsync(mod_b, 0, (size_t)t.n_mod * 2, s), "hipMemsetAsync");
  for (size_t i = 0; i < t.linears.size(); ++i) {
    const vckeys::Linear& l = t.linears[i];
    const Flux::Loaded *w = have(l.key0 + vckeys::WEIGHT), *b = have(l.key0 + vckeys::BIAS), *la = have(l.key0 + vckeys::LORA_A),
                       *lb = have(l.key0 + vckeys::LORA_B), *lbb = have(l.key0 + vckeys::LORA_B_BIAS);
    const int rank = la ? (int)la->shape[0] : 0;
    if (!rank) la = lb = lbb = nullptr;                            // no pair: a conversion / copy (lora_B.bias belongs to the pair)
    const bool mod = l.mod_off >= 0;
    bf16_t* out = mod ? mod_w + l.mod_off * f.D : wout[i];
    bf16_t* bias_out = !(b || lbb) ? nullptr : mod ? mod_b + l.mod_off : bout[i];
    TRY(vc_lora_merge_qkv_launch(w->p, w->f32, l.in, la ? la->p : nullptr, l.in, lb ? lb->p : nullptr, rank, lora_scale, out, mod ? f.D : l.in,
                                 b ? b->p : nullptr, b ? b->f32 : 0, lbb ? lbb->p : nullptr, bias_out, l.out, l.in, rank, l.qkv ? f.H : 0, s,
                                 err, errlen));
    if (!mod) { Lin x; x.w = out; x.b = bias_out; x.N = l.out; x.K = l.in; x.ldw = l.in; bind.push_back({l.name, x}); }
  }
  { Lin x; x.w = mod_w; x.b = mod_b; x.N = (int)t.n_mod; x.K = f.D; x.ldw = f.D; bind.push_back({"modulation", x}); }
  // ---- the scales: one launch (per VC_SCALE_VECTORS of them), one read of their maxima
  for (int i0 = 0; i0 < n_scales; i0 += VC_SCALE_VECTORS) {
    VcScaleVectors v;
    memset(&v, 0, sizeof(v));
    const int n = std::min(VC_SCALE_VECTORS, n_scales - i0);
    for (int i = 0; i < n; ++i) {
      const Flux::Loaded* sc = have(vckeys::find(t, t.scales[i0 + i].c_str()));
      v.src[i] = sc->p; v.f32[i] = (uint8_t)sc->f32;
    }
    TRY(vc_scale_cast_launch(v, n, scales + (int64_t)128 * i0, 128, amax + i0, s, err, errlen));
  }
  std::vector<float> mx(n_scales);
  HIP(hipMemcpyAsync(mx.data(), amax, sizeof(float) * n_scales, hipMemcpyDeviceToHost, s), "hipMemcpyAsync (QK-norm maxima)");
  HIP(hipStreamSynchronize(s), "hipStreamSynchronize");
  // the cap Flux.prepare / Flux.handle() hand over: the largest per-block bound, in thousandths, rounded up; 0 (no bounded softmax
  // anywhere) where a scale is NaN or the bound leaves the option's range.  A double block's four vectors, then a single block's two
  float cap = 0.0f;
  for (int i = 0; i < n_scales;) {
    const int per = i < 4 * f.cfg.depth ? 4 : 2;
    double q = 0, k = 0;
    bool nan = false;
    for (int j = 0; j < per; ++j) {
      const float v = mx[i + j];
      if (v != v) nan = true;
      else if (j % 2 == 0) q = std::max(q, (double)v);
      else k = std::max(k, (double)v);
    }
    cap = std::max(cap, nan ? 1e30f : logit_bound_of(q, k));
    i += per;
  }
  const int milli = cap > 0.0f && cap < 2e6f ? (int)ceil((double)cap * 1000.0) : 0;
  // ---- bind, as vc_flux_bind_weight would
  for (auto& kv : bind) f.bound[kv.first] = kv.second;
  for (int i = 0; i < n_scales; ++i) {
    Lin x; x.w = scales + (int64_t)128 * i; x.b = nullptr; x.N = 1; x.K = 128; x.ldw = 128;
    f.bound[t.scales[i]] = x;
  }
  f.opt.qkv_heads = f.H; f.opt.fuse_knorm = 1; f.opt.logit_bound_milli = milli;
  f.resolved = false;
  f.prepared = false;
  drop_graph(f);
  return VC_OK;
}

int vc_flux_bound_impl(void* handle, const char* name, const void** w, const void** bias, int32_t* rows, int32_t* cols, int64_t* ldw, char* err,
                       int errlen) {
  HANDLE(Flux, f, "flux");
  if (!name) FAIL(VC_ERR_ARG, "flux_bound: null name");
  auto it = f.bound.find(name);
  if (it == f.bound.end()) FAIL(VC_ERR_STATE, "flux_bound: nothing is bound under '%s'", name);
  if (w) *w = it->second.w;
  if (bias) *bias = it->second.b;
  if (rows) *rows = it->second.N;
  if (cols) *cols = it->second.K;
  if (ldw) *ldw = it->second.ldw;
  return VC_OK;
}

int vc_flux_bind_lora_impl(void* handle, const char* name, const void* lora_a, int64_t lda, const void* lora_b, int64_t ldb,
                           const void* lora_b_bias, int32_t out_features, int32_t in_features, int32_t rank, char* err, int errlen) {
  HANDLE(Flux, f, "flux");
  if (!name) FAIL(VC_ERR_ARG, "flux_bind_lora: null name");
  if (!lora_a && !lora_b) {           // unbind
    f.lora.erase(name);
  } else {
    if (!lora_a || !lora_b) FAIL(VC_ERR_ARG, "flux_bind_lora: lora_a and lora_b of '%s' must both be given", name);
    if (rank <= 0 || rank % 64)
      FAIL(VC_ERR_ARG, "flux_bind_lora: rank = %d of '%s' must be a positive multiple of 64, the GEMM's K granularity (zero-pad the factors)", rank, name);
    int out = 0, in = 0;              // what the Linear is: a module of the stacked modulation matrix, or a bound weight
    auto mo = f.mod_off.find(name);
    if (mo != f.mod_off.end()) {
      int64_t end = f.n_mod;
      for (const auto& kv : f.mod_off) if (kv.second > mo->second && kv.second < end) end = kv.second;
      out = (int)(end - mo->second); in = f.D;
    } else {
      auto it = f.bound.find(name);
      if (it == f.bound.end()) FAIL(VC_ERR_STATE, "flux_bind_lora: name = '%s' is no Linear bound by vc_flux_bind_weight (bind the weight first)", name);
      out = it->second.N; in = it->second.K;
    }
    if (out_features != out || in_features != in)
      FAIL(VC_ERR_ARG, "flux_bind_lora: out_features, in_features = %d, %d of '%s', its weight is [%d, %d]", out_features, in_features, name, out, in);
    if (lda < in || ldb < rank || lda % 8 || ldb % 8)
      FAIL(VC_ERR_ARG, "flux_bind_lora: lda = %lld, ldb = %lld of '%s' must be multiples of 8, at least in_features and rank", (long long)lda, (long long)ldb, name);
    Lora lo;
    lo.a = lora_a; lo.b = lora_b; lo.bb = lora_b_bias; lo.rank = rank; lo.out = out; lo.in = in; lo.lda = lda; lo.ldb = ldb;
    f.lora[name] = lo;
  }
  f.resolved = false;
  f.prepared = false;   // the widest rank sizes the workspace
  drop_graph(f);
  return VC_OK;
}

int vc_flux_set_lora_scale_impl(void* handle, float scale, char* err, int errlen) {
  HANDLE(Flux, f, "flux");
  if (!(scale - scale == 0.0f) || bf16_round(scale) != scale)
    FAIL(VC_ERR_ARG, "flux_set_lora_scale: scale = %.9g is not a bf16 value; the un-merged mode applies it as a bf16 vector and would round it "
                     "(merge with vc_lora_merge, which applies any scale in f32)", scale);
  if (f.in_flight)      // the trajectory's modulation rows and its step-invariant projections ran with the old scale
    FAIL(VC_ERR_STATE, "flux_set_lora_scale: scale cannot change between vc_flux_sample_begin and vc_flux_sample_end");
  // host only.  The next vc_flux_prepare writes the value into the scale vector, which keeps its place in that workspace: a step
  // captured there replays with it.  Until then the prepared state is of the old scale and forward / sample_begin refuse it
  if (scale != f.lora_scale && f.prepared) f.scale_stale = true;
  f.lora_scale = scale;
  return VC_OK;
}

// "img_in", "txt_in", "double.{i}.img", "double.{i}.txt", "single.{i}" -> the tap's index
static int tap_index(Flux& f, const char* what, const char* name, size_t& idx, Err e) {
  if (!name) FAIL(VC_ERR_ARG, "%s: null name", what);
  int i = -1, n = 0;
  char st[4] = "";
  if (!strcmp(name, "img_in")) { idx = (size_t)vcmon::tap_img_in(); return VC_OK; }
  if (!strcmp(name, "txt_in")) { idx = (size_t)vcmon::tap_txt_in(); return VC_OK; }
  if (sscanf(name, "double.%d.%3[a-z]%n", &i, st, &n) == 2 && !name[n] && i >= 0 && (!strcmp(st, "img") || !strcmp(st, "txt"))) {
    if (i >= f.cfg.depth) FAIL(VC_ERR_ARG, "%s: name = '%s', the model has %d double blocks", what, name, f.cfg.depth);
    idx = (size_t)vcmon::tap_double(i, st[0] == 't');
    return VC_OK;
  }
  n = 0;
  if (sscanf(name, "single.%d%n", &i, &n) == 1 && !name[n] && i >= 0) {
    if (i >= f.cfg.depth_single_blocks) FAIL(VC_ERR_ARG, "%s: name = '%s', the model has %d single blocks", what, name, f.cfg.depth_single_blocks);
    idx = (size_t)vcmon::tap_single(f.cfg.depth, i);
    return VC_OK;
  }
  FAIL(VC_ERR_ARG, "%s: unknown tap name = '%s' (img_in, txt_in, double.{i}.img, double.{i}.txt, single.{i})", what, name);
}

int vc_flux_set_tap_impl(void* handle, const char* name, void* dst, char* err, int errlen) {
  HANDLE(Flux, f, "flux");
  size_t idx = 0;
  TRY(tap_index(f, "flux_set_tap", name, idx, e));
  if (f.in_flight && f.taps[idx] != dst)      // the captured step of the trajectory keeps copying to the old buffer
    FAIL(VC_ERR_STATE, "flux_set_tap: the tap '%s' cannot change between vc_flux_sample_begin and vc_flux_sample_end", name);
  f.taps[idx] = dst;
  return VC_OK;
}

int vc_flux_set_monitor_impl(void* handle, int32_t level, VcStat* log, int32_t capacity_evals, float* scratch, char* err, int errlen) {
  HANDLE(Flux, f, "flux");
  if (level < 0 || level > 2) FAIL(VC_ERR_ARG, "flux_set_monitor: level = %d (0: off, 1: v and x, 2: those and every tap site)", level);
  if (level == 0) { log = nullptr; scratch = nullptr; capacity_evals = 0; }
  else {
    if (!log || !scratch) FAIL(VC_ERR_ARG, "flux_set_monitor: null log / scratch (vc_flux_monitor_bytes gives their sizes)");
    if ((uintptr_t)log & 15) FAIL(VC_ERR_ARG, "flux_set_monitor: log must be 16-byte aligned (a VcStat is one 16-byte store)");
    if ((uintptr_t)scratch & 3) FAIL(VC_ERR_ARG, "flux_set_monitor: scratch must be 4-byte aligned");
    if (capacity_evals <= 0) FAIL(VC_ERR_ARG, "flux_set_monitor: capacity_evals = %d must be positive", capacity_evals);
  }
  const bool same = level == f.mon_level && log == f.mon_log && scratch == f.mon_scratch && capacity_evals == f.mon_cap;
  if (f.in_flight) {                          // the captured step of the trajectory keeps its nodes and their row capacity
    if (!same) FAIL(VC_ERR_STATE, "flux_set_monitor: the monitor cannot change between vc_flux_sample_begin and vc_flux_sample_end");
    return VC_OK;
  }
  f.mon_evals = 0;                            // a (new) statement about the log: nothing of it is reported until something is logged
  f.mon_B = level && f.prepared ? f.B : 0;
  f.mon_level = level; f.mon_log = log; f.mon_scratch = scratch; f.mon_cap = capacity_evals;
  return VC_OK;
}

int vc_flux_monitor_sites_impl(void* handle, int32_t index, char* name, int32_t namelen, char* err, int errlen) {
  HANDLE(Flux, f, "flux");
  if (!name || namelen <= 0) FAIL(VC_ERR_ARG, "flux_monitor_sites: null / empty name buffer");
  if (!vcmon::site_name(f.mon_level, f.cfg.depth, f.cfg.depth_single_blocks, index, name, namelen))
    FAIL(VC_ERR_ARG, "flux_monitor_sites: index = %d, level %d has %d sites", index, f.mon_level, f.mon_sites());
  return VC_OK;
}

int vc_flux_monitor_bytes_impl(void* handle, int32_t capacity_evals, int64_t* log_bytes, int64_t* scratch_bytes, char* err, int errlen) {
  HANDLE(Flux, f, "flux");
  if (capacity_evals <= 0) FAIL(VC_ERR_ARG, "flux_monitor_bytes: capacity_evals = %d must be positive", capacity_evals);
  if (!f.mon_level) FAIL(VC_ERR_STATE, "flux_monitor_bytes: the monitor is off (the sites of a level size the log: vc_flux_set_monitor first)");
  if (!f.prepared) FAIL(VC_ERR_STATE, "flux_monitor_bytes: call vc_flux_prepare first (the log holds the samples of the prepared geometry)");
  if (log_bytes) *log_bytes = vcmon::log_bytes(capacity_evals, f.mon_sites(), f.B);
  if (scratch_bytes) *scratch_bytes = vcmon::scratch_bytes(f.B);
  return VC_OK;
}

int vc_flux_monitor_report_impl(void* handle, int32_t* first_bad_eval, int32_t* first_bad_site, int32_t* first_bad_sample, int32_t* evals_logged,
                                hipStream_t s, char* err, int errlen) {
  HANDLE(Flux, f, "flux");
  if (!f.mon_level) FAIL(VC_ERR_STATE, "flux_monitor_report: the monitor is off");
  // the rows were written for mon_B samples - the B prepared when they were logged, whatever has been prepared since (evaluations
  // are only ever logged behind monitor_fits, which sets it)
  const int B = f.mon_B, ns = f.mon_sites();
  const int evals = B > 0 ? std::min(f.mon_evals, f.mon_cap) : 0;
  int32_t first = -1;
  if (evals > 0) {      // the scratch is free between two launches of the stream; its first word takes the answer
    TRY(vc_monitor_first_bad_launch(f.mon_log, (int64_t)evals * ns * B, ns, B, (int32_t*)f.mon_scratch, s, e.buf, e.len));
    HIP(hipMemcpyAsync(&first, f.mon_scratch, sizeof(first), hipMemcpyDeviceToHost, s), "hipMemcpyAsync(D2H)");
    HIP(hipStreamSynchronize(s), "hipStreamSynchronize");
  }
  int32_t ev = -1, site = -1, b = -1;
  if (first >= 0) {      // the rank of the entry that was written first -> its site
    vcmon::log_split(first, ns, B, &ev, &site, &b);
    site = vcmon::site_at_rank(site, ns);
  }
  if (first_bad_eval) *first_bad_eval = ev;
  if (first_bad_site) *first_bad_site = site;
  if (first_bad_sample) *first_bad_sample = b;
  if (evals_logged) *evals_logged = evals;
  return VC_OK;
}

int vc_flux_step_nodes_impl(void* handle, int32_t nodes[3], char* err, int errlen) {
  HANDLE(Flux, f, "flux");
  if (!nodes) FAIL(VC_ERR_ARG, "flux_step_nodes: null nodes");
  if (!f.step.g[0]) FAIL(VC_ERR_STATE, "flux_step_nodes: no captured step (vc_flux_sample_begin* on a stream captures one)");
  for (int i = 0; i < 3; ++i) nodes[i] = f.step.nodes[i];
  return VC_OK;
}

int vc_flux_tap_shape_impl(void* handle, const char* name, int64_t* rows, int32_t* cols, char* err, int errlen) {
  HANDLE(Flux, f, "flux");
  size_t idx = 0;
  TRY(tap_index(f, "flux_tap_shape", name, idx, e));
  if (!rows || !cols) FAIL(VC_ERR_ARG, "flux_tap_shape: null rows / cols");
  if (!f.prepared) FAIL(VC_ERR_STATE, "flux_tap_shape: call vc_flux_prepare first (the rows are those of the prepared geometry)");
  const size_t first_single = (size_t)vcmon::tap_single(f.cfg.depth, 0);
  *rows = (int64_t)f.B * (idx >= first_single ? f.L : idx % 2 ? f.T : f.N);
  *cols = f.D;
  return VC_OK;
}

int64_t vc_flux_mod_offset_impl(void* handle, const char* name) {
  if (!handle) return -1;
  Flux& f = *(Flux*)handle;
  if (!name) return f.n_mod;
  auto it = f.mod_off.find(name);
  return it == f.mod_off.end() ? -1 : it->second;
}

int vc_flux_set_option_impl(void* handle, const char* name, int32_t value, char* err, int errlen) {
  HANDLE(Flux, f, "flux");
  if (!name) FAIL(VC_ERR_ARG, "flux_set_option: null name");
  for (const auto& o : OPTIONS) {
    if (strcmp(name, o.name)) continue;
    switch (o.clamp) {
      case BOOL: value = value != 0; break;
      case AT_LEAST_0: value = value > 0 ? value : 0; break;
      case ZERO_TO_2: value = value < 0 ? 0 : value > 2 ? 2 : value; break;
      case ZERO_OR_H: if (value != 0 && value != f.H) FAIL(VC_ERR_ARG, "flux_set_option: qkv_heads must be 0 or num_heads = %d", f.H); break;
      case ANY: break;
    }
    if ((o.member == &Options::lora_mode || o.member == &Options::adaptive || o.member == &Options::sde) && value != f.opt.*o.member) {
      if (f.in_flight)
        FAIL(VC_ERR_STATE, "flux_set_option: %s cannot change between vc_flux_sample_begin and vc_flux_sample_end", o.name);
      f.prepared = false;    // the workspace carve-up differs: vc_flux_workspace_bytes + vc_flux_prepare again
    }
    f.opt.*o.member = value;
    return VC_OK;
  }
  FAIL(VC_ERR_ARG, "flux_set_option: unknown option '%s'", name);
}

const VcFluxConfig* vc_flux_config_impl(void* handle) { return handle ? &((Flux*)handle)->cfg : nullptr; }   // grid_engine.hip reads the geometry

int64_t vc_flux_workspace_bytes_impl(void* handle, int32_t B, int32_t T, int32_t N, int32_t max_steps) {
  if (!handle || B <= 0 || T <= 0 || N <= 0 || max_steps <= 0) return -1;
  Buffers tmp;                    // carve into a scratch copy: the pointers of the live handle stay as they are
  ((Flux*)handle)->ws_sized = true;
  return carve(tmp, *(Flux*)handle, nullptr, B, T, N, max_steps);
}

int vc_flux_prepare_impl(void* handle, const VcFluxInputs* in, void* workspace, int64_t workspace_bytes, hipStream_t s, char* err, int errlen) {
  HANDLE(Flux, f, "flux");
  if (!in || !workspace) FAIL(VC_ERR_ARG, "flux_prepare: null argument");
  f.ws_sized = true;
  const int B = in->B, T = in->T, N = in->N, S = in->max_steps;
  if (B <= 0 || T <= 0 || N <= 0 || S <= 0) FAIL(VC_ERR_ARG, "flux_prepare: B, T, N, max_steps must be positive");
  if (!in->txt || !in->y || !in->img_ids || !in->txt_ids) FAIL(VC_ERR_ARG, "flux_prepare: txt, y, img_ids, txt_ids are required");
  if (f.cfg.guidance_embed && !in->guidance) FAIL(VC_ERR_ARG, "Didn't get guidance strength for guidance distilled model.");
  if (in->kv_gap && !in->kv_len) FAIL(VC_ERR_ARG, "flux_prepare: kv_gap needs kv_len");
  if (!aligned256(workspace)) FAIL(VC_ERR_ARG, "flux_prepare: workspace must be 256-byte aligned");
  TRY(resolve(f, e));
  if (f.opt.lora_mode && f.opt.qkv_heads > 0)
    FAIL(VC_ERR_ARG, "flux_prepare: lora_mode 1 takes the qkv weights in their natural row order (option qkv_heads 0)");
  f.prepared = false;
  f.in_flight = false;
  f.scale_stale = false;
  const int64_t need = carve(f, f, (char*)workspace, B, T, N, S);
  if (workspace_bytes < need) FAIL(VC_ERR_ARG, "flux_prepare: workspace of %lld bytes, %lld needed", (long long)workspace_bytes, (long long)need);
  f.base = (char*)workspace;
  f.ws_cache = f.sc_on();
  f.B = B; f.T = T; f.N = N; f.L = T + N; f.Lp = (f.L + 63) / 64 * 64; f.S = S;
  const int L = f.L, D = f.D;
  // masks
  f.ragged = f.gapped = false;
  for (int b = 0; b < B; ++b) {
    const int kv = in->kv_len ? in->kv_len[b] : L;
    if (kv < 0 || kv > L) FAIL(VC_ERR_ARG, "flux_prepare: kv_len[%d] = %d outside [0, %d]", b, kv, L);
    if (kv < L) f.ragged = true;
    if (in->kv_gap) {
      const int lo = in->kv_gap[2 * b], hi = in->kv_gap[2 * b + 1];
      if (lo < 0 || lo > hi || hi > kv) FAIL(VC_ERR_ARG, "flux_prepare: kv_gap[%d] = (%d, %d) must lie inside [0, kv_len = %d)", b, lo, hi, kv);
      if (hi > lo) f.gapped = true;
    }
  }
  if (f.gapped) f.ragged = true;
  // host tables -> pinned staging -> HBM
  const size_t n_rope = (size_t)B * L * 128;
  TRY(stage_begin(f, (n_rope + 128 + 4 * B + 64) * sizeof(float) + 8 * 256, e));
  float* rope = stage_take<float>(f, n_rope);
  {  // RoPE angles in float64 exactly as math.py:102-109, stored as (cos, sin) f32 per (token, pair).  Position ids take few
     // distinct values per axis (grid rows / columns), so cos / sin are evaluated once per (axis, value, frequency).
    int pair0 = 0;
    std::vector<float> table;
    std::vector<int> slot((size_t)B * L);
    for (int ax = 0; ax < 3; ++ax) {
      const int half = f.cfg.axes_dim[ax] / 2, d = f.cfg.axes_dim[ax];
      std::unordered_map<float, int> seen;
      std::vector<float> values;
      for (int b = 0; b < B; ++b)
        for (int r = 0; r < L; ++r) {
          const float id = r < T ? in->txt_ids[((size_t)b * T + r) * 3 + ax] : in->img_ids[((size_t)b * N + (r - T)) * 3 + ax];
          auto it = seen.find(id);
          if (it == seen.end()) { it = seen.emplace(id, (int)values.size()).first; values.push_back(id); }
          slot[(size_t)b * L + r] = it->second;
        }
      table.resize(values.size() * (size_t)half * 2);
      for (int j = 0; j < half; ++j) {
        const double omega = 1.0 / pow((double)f.cfg.theta, (double)(2 * j) / (double)d);
        for (size_t v = 0; v < values.size(); ++v) {
          const double ang = (double)values[v] * omega;
          table[(v * half + j) * 2] = (float)cos(ang);
          table[(v * half + j) * 2 + 1] = (float)sin(ang);
        }
      }
      for (size_t row = 0; row < (size_t)B * L; ++row)
        memcpy(rope + (row * 64 + pair0) * 2, table.data() + (size_t)slot[row] * half * 2, (size_t)half * 2 * sizeof(float));
      pair0 += half;
    }
  }
  float* freqs = stage_take<float>(f, 128);
  for (int k = 0; k < 128; ++k)   // layers.py:41-43: exp(-ln(10000) * k / 128), the argument formed in f32 as torch forms it
    freqs[k] = (float)exp((double)((float)(-log(10000.0)) * (float)k / 128.0f));
  int32_t* kvl = stage_take<int32_t>(f, B);
  int32_t* gap = stage_take<int32_t>(f, 2 * B);
  float* g32 = stage_take<float>(f, B);
  for (int b = 0; b < B; ++b) {
    kvl[b] = in->kv_len ? in->kv_len[b] : L;
    gap[2 * b] = in->kv_gap ? in->kv_gap[2 * b] : 0;
    gap[2 * b + 1] = in->kv_gap ? in->kv_gap[2 * b + 1] : 0;
    g32[b] = in->guidance ? in->guidance[b] : 0.0f;
  }
  TRY(stage_send(f, f.ROPE, rope, n_rope * sizeof(float), s, e));
  {
    auto it = f.bound.find("timestep_freqs");     // the caller's own table (torch's f32 exp), bit for bit
    if (it != f.bound.end()) {
      if (it->second.N * it->second.K != 128) FAIL(VC_ERR_ARG, "flux_prepare: 'timestep_freqs' must hold 128 f32 values");
      TRY(d2d(f.FREQS, it->second.w, 128 * sizeof(float), s, e));
    } else {
      TRY(stage_send(f, f.FREQS, freqs, 128 * sizeof(float), s, e));
    }
  }
  TRY(stage_send(f, f.KVLEN, kvl, B * sizeof(int32_t), s, e));
  TRY(stage_send(f, f.KVGAP, gap, 2 * B * sizeof(int32_t), s, e));
  TRY(stage_send(f, f.G32, g32, B * sizeof(float), s, e));
  TRY(stage_end(f, s, e));
  HIP(hipMemsetAsync(f.VT, 0, (size_t)B * f.H * 128 * f.Lp * 2, s), "hipMemsetAsync");
  // the flag words of the attention kernel's in-launch combine: zero before the first launch (every launch leaves them zero)
  HIP(hipMemsetAsync((char*)f.ATT_SCRATCH + vcplan::attention_flags_offset(vc_cu_count()), 0, (size_t)vcplan::attention64_flags_bytes(f.n_cu), s), "hipMemsetAsync");
  if (f.opt.lora_mode) TRY(vc_fill_bf16_launch(f.LSCALE, f.lora_scale, f.lscale_elems, s, e.buf, e.len));
  // step-invariant projections
  TRY(lin(f, f.txt_in, in->txt, f.cfg.context_in_dim, f.TXT0, D, B * T, VC_EPI_BIAS, s, e));
  if (f.cfg.guidance_embed) {
    TRY(vc_temb_launch(f.G32, f.FREQS, f.GE, B, 128, in->guidance_is_bf16, s, e.buf, e.len));
    TRY(lin(f, f.guidance_in[0], f.GE, 256, f.GH, D, B, VC_EPI_SILU, s, e));
    TRY(lin(f, f.guidance_in[1], f.GH, D, f.GVEC, D, B, VC_EPI_BIAS, s, e));
  }
  TRY(lin(f, f.vector_in[0], in->y, f.cfg.vec_in_dim, f.YH, D, B, VC_EPI_SILU, s, e));
  TRY(lin(f, f.vector_in[1], f.YH, D, f.YVEC, D, B, VC_EPI_BIAS, s, e));
  f.prepared = true;
  f.steps_total = f.steps_done = 0;
  return VC_OK;
}

int vc_flux_forward_impl(void* handle, const void* img, const float* timesteps, int32_t timesteps_is_bf16, void* out, hipStream_t s,
                         char* err, int errlen) {
  HANDLE(Flux, f, "flux");
  if (!f.prepared) FAIL(VC_ERR_STATE, "flux_forward: call vc_flux_prepare first");
  TRY(fresh_scale(f, "flux_forward", e));
  if (!img || !timesteps || !out) FAIL(VC_ERR_ARG, "flux_forward: null argument");
  TRY(monitor_fits(f, "flux_forward", e));
  TRY(stage_begin(f, f.B * sizeof(float) + 256, e));
  float* ts = stage_take<float>(f, f.B);
  for (int b = 0; b < f.B; ++b) ts[b] = timesteps[b];
  TRY(stage_send(f, f.TS, ts, f.B * sizeof(float), s, e));
  TRY(stage_end(f, s, e));
  TRY(time_precompute(f, 1, timesteps_is_bf16, s, e));
  f.steps_total = f.steps_done = 0;   // MOD now holds this evaluation's rows, not a trajectory's
  f.in_flight = false;
  if (f.mon_level) {      // row 0 of a zeroed log
    TRY(vc_zero_fill_launch(f.mon_log, vcmon::log_bytes(f.mon_cap, f.mon_sites(), f.B), s, e.buf, e.len));
    f.mon_evals = 1;
  }
  return evaluate(f, nullptr, false, img, out, false, s, e);
}

// the f32 times of the `evals` evaluations of the step t0 -> t1 (dt = t1 - t0), each formed in f32 operation by operation as
// torch forms `t0 + half_dt`, `t0 + dt * (1/3)`, `t0 + dt * (2/3)` from 0-dim f32 tensors (no contraction into a fused multiply-add)
void stage_times(int method, float t0, float t1, float dt, float* out) {
#pragma clang fp contract(off)
  out[0] = t0;
  if (method == VC_SOLVER_MIDPOINT) {
    volatile float half_dt = 0.5f * dt;
    out[1] = t0 + half_dt;
  } else if (method == VC_SOLVER_RK4) {
    volatile float a = dt * (float)(1.0 / 3.0), b = dt * (float)(2.0 / 3.0);
    out[1] = t0 + a; out[2] = t0 + b; out[3] = t1;
  }
}

int vc_flux_sample_begin_impl(void* handle, int32_t method, const void* x, const void* cond, const float* t_grid, int32_t n_points,
                              int32_t state_is_bf16, hipStream_t s, char* err, int errlen) {
  HANDLE(Flux, f, "flux");
  const int E = vc_evals_of(method);
  if (!E) FAIL(VC_ERR_ARG, "flux_sample: unknown solver method %d (VC_SOLVER_EULER, VC_SOLVER_MIDPOINT, VC_SOLVER_RK4)", method);
  if (!f.prepared) FAIL(VC_ERR_STATE, "flux_sample: call vc_flux_prepare first");
  TRY(fresh_scale(f, "flux_sample", e));
  if (!x || !cond || !t_grid) FAIL(VC_ERR_ARG, "flux_sample: null argument");
  const int S = n_points - 1, B = f.B;
  if (S < 1 || (int64_t)S * E > f.S)
    FAIL(VC_ERR_ARG, "flux_sample: %d steps of %d evaluation(s), the prepared workspace holds 1..%d evaluations", S, E, f.S);
  const bool cached = f.sc_on();
  if (cached && method != VC_SOLVER_EULER)
    FAIL(VC_ERR_ARG, "flux_sample: the step cache works with VC_SOLVER_EULER only (method %d): turn it off with vc_flux_set_step_cache(handle, 0, 0)", method);
  if (cached && f.dbl.empty()) FAIL(VC_ERR_ARG, "flux_sample: the step cache needs at least one double block");
  if (cached && !f.ws_cache)
    FAIL(VC_ERR_STATE, "flux_sample: the step cache was turned on after vc_flux_prepare: ask vc_flux_workspace_bytes and prepare again");
  if (f.cfg_on) {
    if (B % 2) FAIL(VC_ERR_ARG, "flux_sample: true CFG pairs the first half of the batch with the second: B = %d is odd", B);
    if (cached) FAIL(VC_ERR_ARG, "flux_sample: true CFG does not work with the step cache: turn one off (vc_flux_set_cfg(handle, 0, 0) / vc_flux_set_step_cache(handle, 0, 0))");
    if (!(f.cfg_scale - f.cfg_scale == 0.0f)) FAIL(VC_ERR_ARG, "flux_sample: the cfg_scale set by vc_flux_set_cfg is not finite");
  }
  TRY(monitor_fits(f, "flux_sample", e));
  if (f.mon_level && (int64_t)S * E > f.mon_cap)
    FAIL(VC_ERR_ARG, "flux_sample: %d steps of %d evaluation(s), the monitor's log holds capacity_evals = %d (vc_flux_set_monitor)", S, E, f.mon_cap);
  if (cached && !f.sc_host) HIP(hipHostMalloc((void**)&f.sc_host, 256, hipHostMallocDefault), "hipHostMalloc");
  const int SE = S * E;
  TRY(stage_begin(f, ((size_t)SE * B + S) * sizeof(float) + 512, e));
  float* ts = stage_take<float>(f, (size_t)SE * B);
  float* dts = stage_take<float>(f, S);
  for (int i = 0; i < S; ++i) {
    dts[i] = t_grid[i + 1] - t_grid[i];   // fixed grid: dt = t1 - t0 in f32
    float te[4];
    stage_times(method, t_grid[i], t_grid[i + 1], dts[i], te);
    for (int j = 0; j < E; ++j) {
      // the drift sees t in the state's dtype (torchdiffeq _PerturbFunc); the model sees 1 - t (transport.py:384)
      const float tm = 1.0f - (state_is_bf16 ? bf16_round(te[j]) : te[j]);
      for (int b = 0; b < B; ++b) ts[((size_t)i * E + j) * B + b] = tm;
    }
  }
  TRY(stage_send(f, f.TS, ts, (size_t)SE * B * sizeof(float), s, e));
  TRY(stage_send(f, f.DTS, dts, S * sizeof(float), s, e));
  TRY(stage_end(f, s, e));
  TRY(time_precompute(f, SE, 0, s, e));
  const int64_t n = (int64_t)B * f.N;
  f.state_f32 = !state_is_bf16;
  f.method = method; f.evals = E;
  TRY(d2d(ode_state(f), x, ode_state_bytes(f), s, e));
  // the first evaluation reads bf16(y0)
  if (f.state_f32) TRY(ode_update(f, nullptr, nullptr, s, e));
  else if (next_input(f) != f.XS) TRY(d2d(next_input(f), f.XS, ode_state_bytes(f), s, e));
  TRY(d2d(f.COND, cond, n * (f.cfg.in_channels - f.cfg.out_channels) * 2, s, e));
  HIP(hipMemsetAsync(f.STEP, 0, sizeof(int32_t), s), "hipMemsetAsync");
  f.sc_active = cached; f.sc_thr = f.sc_threshold; f.sc_lim = f.sc_max;
  f.cfg_active = f.cfg_on; f.cfg_s = f.cfg_on ? f.cfg_scale : 1.0f;
  f.sc_have = false; f.sc_run = f.sc_computed = f.sc_reused = 0;
  f.sc_metrics.clear();
  if (s) TRY(step_graph(f, s, e));
  // the monitor's log starts zeroed (behind the warm-up evaluation of a new capture, which logs): a kernel, not a memset node
  if (f.mon_level) TRY(vc_zero_fill_launch(f.mon_log, vcmon::log_bytes(f.mon_cap, f.mon_sites(), B), s, e.buf, e.len));
  f.mon_evals = 0;
  // no P yet: the first metric is read against zeros (and reported as NaN), never against an earlier trajectory's residual
  if (cached) HIP(hipMemsetAsync(f.SC_P, 0, (size_t)n * f.D * 2, s), "hipMemsetAsync");
  f.steps_total = S; f.steps_done = 0;
  f.in_flight = true;
  return VC_OK;
}

// one cached Euler step: head, ONE host read of the metric, the tail the rule picks
static int cached_step(Flux& f, hipStream_t s, Err e) {
  if (s) HIP(hipGraphLaunch(f.step.g[0], s), "hipGraphLaunch");
  else TRY(cache_head(f, s, e));
  HIP(hipStreamSynchronize(s), "hipStreamSynchronize");
  const float m = *(volatile float*)f.sc_host;
  const bool reuse = f.sc_have && m < f.sc_thr && (f.sc_lim < 0 || f.sc_run < f.sc_lim);
  f.sc_metrics.push_back(f.sc_have ? m : NAN);
  if (s) HIP(hipGraphLaunch(f.step.g[reuse ? 2 : 1], s), "hipGraphLaunch");
  else if (reuse) TRY(cache_tail_reuse(f, true, s, e));
  else TRY(cache_tail_compute(f, true, s, e));
  if (reuse) { ++f.sc_reused; ++f.sc_run; }
  else { ++f.sc_computed; f.sc_run = 0; f.sc_have = true; }
  return VC_OK;
}

int vc_flux_sample_steps_impl(void* handle, int32_t n_steps, void* trajectory, hipStream_t s, char* err, int errlen) {
  HANDLE(Flux, f, "flux");
  if (!f.prepared || f.steps_total == 0) FAIL(VC_ERR_STATE, "flux_sample_steps: call vc_flux_sample_begin first");
  if (n_steps < 0 || f.steps_done + n_steps > f.steps_total)
    FAIL(VC_ERR_ARG, "flux_sample_steps: %d more steps after %d of %d", n_steps, f.steps_done, f.steps_total);
  if (s && (!f.step.g[0] || f.key.s != s)) FAIL(VC_ERR_STATE, "flux_sample_steps: the step was captured on another stream");
  const int64_t state_bytes = ode_state_bytes(f);
  for (int i = 0; i < n_steps; ++i) {
    for (int j = 0; j < f.evals; ++j) {      // a step = `evals` replays; the stage is the device-side counter modulo evals
      ++f.mon_evals;
      if (f.sc_active) { TRY(cached_step(f, s, e)); continue; }
      if (s) HIP(hipGraphLaunch(f.step.g[0], s), "hipGraphLaunch");
      else TRY(evaluate(f, f.STEP, true, nullptr, nullptr, true, s, e));
      ++f.sc_computed;
    }
    if (trajectory) TRY(d2d((char*)trajectory + (int64_t)i * state_bytes, ode_state(f), state_bytes, s, e));
    ++f.steps_done;
  }
  return VC_OK;
}

int vc_flux_sample_end_impl(void* handle, void* x_out, hipStream_t s, char* err, int errlen) {
  HANDLE(Flux, f, "flux");
  if (!f.prepared || f.steps_total == 0) FAIL(VC_ERR_STATE, "flux_sample_end: no sample in flight");
  if (!x_out) FAIL(VC_ERR_ARG, "flux_sample_end: null output");
  f.in_flight = false;
  return d2d(x_out, ode_state(f), ode_state_bytes(f), s, e);
}

// ---------------------------------------------------------------- the adaptive solve (vcloze_hip.h: vc_flux_sample_dopri5)
// the times of the seven modulation rows of a step t -> t + dt (row = the device-side counter = the stage of the evaluation): k1's
// own (its evaluation is the last step's seventh), then c2..c6 and t + dt again for k7; the model sees 1 - f32(t)
static int dopri5_rows(Flux& f, double t, double dt, hipStream_t s, Err e) {
  static const double C[7] = {0.0, 1.0 / 5.0, 3.0 / 10.0, 4.0 / 5.0, 8.0 / 9.0, 1.0, 1.0};
  const int B = f.B;
  TRY(stage_begin(f, (size_t)7 * B * sizeof(float) + 1024, e));
  float* ts = stage_take<float>(f, (size_t)7 * B);
  float* hdt = stage_take<float>(f, 1);
  for (int j = 0; j < 7; ++j) {
    const float tm = 1.0f - (float)(t + C[j] * dt);
    for (int b = 0; b < B; ++b) ts[(size_t)j * B + b] = tm;
  }
  *hdt = (float)dt;
  TRY(stage_send(f, f.TS, ts, (size_t)7 * B * sizeof(float), s, e));
  TRY(stage_send(f, f.AD_DT, hdt, sizeof(float), s, e));
  TRY(stage_end(f, s, e));
  return time_precompute(f, 7, 0, s, e);
}
// `count` replays of the captured evaluation (+ its stage node) with the counter starting at `first`
static int dopri5_evals(Flux& f, int first, int count, hipStream_t s, Err e) {
  HIP(hipMemsetD32Async((hipDeviceptr_t)f.STEP, first, 1, s), "hipMemsetD32Async");
  for (int j = 0; j < count; ++j) {
    if (s) HIP(hipGraphLaunch(f.step.g[0], s), "hipGraphLaunch");
    else TRY(evaluate(f, f.STEP, true, nullptr, nullptr, true, s, e));
  }
  f.ad_evals += count;
  return VC_OK;
}
// the first `count` words of AD_OUT -> the host: the ONE synchronisation of an attempt
static int dopri5_read(Flux& f, int count, hipStream_t s, Err e) {
  HIP(hipMemcpyAsync(f.ad_host, f.AD_OUT, count * sizeof(float), hipMemcpyDeviceToHost, s), "hipMemcpyAsync(D2H)");
  HIP(hipStreamSynchronize(s), "hipStreamSynchronize");
  return VC_OK;
}

static int dopri5_run(Flux& f, void* x, const float* t_grid, int n_points, int out_bf16, float rtol, float atol, int max_attempts,
                      void* trajectory, hipStream_t s, Err e) {
  const int64_t n = (int64_t)f.B * f.N * f.cfg.out_channels, out_bytes = n * (out_bf16 ? 2 : 4);
  const volatile float* host = f.ad_host;
  double t = t_grid[0];
  // k1 = f(t0, y0): the counter at 0 stores it (the caller set the rows of t0 with dt = 0: the state the stage node forms is y0)
  TRY(dopri5_evals(f, 0, 1, s, e));
  // the initial step size
  TRY(vc_dopri5_error_ratio_launch(1, f.AD_Y0, nullptr, f.AD_K, nullptr, rtol, atol, f.AD_OUT, f.AD_PART, n, s, e.buf, e.len));
  TRY(vc_dopri5_error_ratio_launch(2, f.AD_Y0, nullptr, f.AD_K, nullptr, rtol, atol, f.AD_OUT + 1, f.AD_PART, n, s, e.buf, e.len));
  TRY(dopri5_read(f, 2, s, e));
  const double d0 = host[0], d1 = host[1];
  if (d0 != d0 || d1 != d1) FAIL(VC_ERR_STATE, "flux_sample_dopri5: the state or the model's output at t_grid[0] is not finite");
  const double h0 = (d0 < 1e-5 || d1 < 1e-5) ? 1e-6 : 0.01 * d0 / d1;
  TRY(dopri5_rows(f, t, h0, s, e));                       // (row 1 stands at t0 + c2 h0; the probe wants t0 + h0: row 5)
  TRY(vc_dopri5_stage_launch(7, f.AD_Y0, f.AD_K, nullptr, f.AD_DT, nullptr, nullptr, f.YIN, n, s, e.buf, e.len));
  TRY(dopri5_evals(f, 5, 1, s, e));                       // its k lands in k6 (and the state it forms is not used)
  // d2 reads the probe from k2: the slots are free until the first attempt
  TRY(d2d(f.AD_K + n, f.AD_K + 5 * n, n * 2, s, e));
  TRY(vc_dopri5_error_ratio_launch(3, f.AD_Y0, nullptr, f.AD_K, nullptr, rtol, atol, f.AD_OUT, f.AD_PART, n, s, e.buf, e.len));
  TRY(dopri5_read(f, 1, s, e));
  const double d2 = (double)host[0] / h0;
  if (d2 != d2) FAIL(VC_ERR_STATE, "flux_sample_dopri5: the model's output at t_grid[0] + h0 is not finite");
  const double dmax = d1 > d2 ? d1 : d2;
  const double h1 = dmax <= 1e-15 ? std::max(1e-6, h0 * 1e-3) : pow(0.01 / dmax, 1.0 / 5.0);
  double dt = std::min(100.0 * h0, h1);
  int next_out = 1;
  while (next_out < n_points) {
    if ((int)f.ad_log.size() >= max_attempts)
      FAIL(VC_ERR_STATE, "flux_sample_dopri5: more than max_attempts = %d attempts (t = %.9g of [%.9g, %.9g], dt = %.3g)", max_attempts, t,
           (double)t_grid[0], (double)t_grid[n_points - 1], dt);
    if (t + dt == t) FAIL(VC_ERR_STATE, "flux_sample_dopri5: the step size underflowed (t = %.17g, dt = %.3g)", t, dt);
    TRY(dopri5_rows(f, t, dt, s, e));
    TRY(vc_dopri5_stage_launch(0, f.AD_Y0, f.AD_K, nullptr, f.AD_DT, nullptr, f.AD_Y1, f.YIN, n, s, e.buf, e.len));   // k1 is in place
    TRY(dopri5_evals(f, 1, 6, s, e));
    TRY(vc_dopri5_error_ratio_launch(0, f.AD_Y0, f.AD_Y1, f.AD_K, f.AD_DT, rtol, atol, f.AD_OUT, f.AD_PART, n, s, e.buf, e.len));
    TRY(dopri5_read(f, 1, s, e));
    const float ratio32 = host[0];
    const double ratio = ratio32;
    const bool accept = ratio <= 1.0;
    f.ad_log.push_back(Flux::Attempt{t, dt, ratio32, accept});
    if (ratio != ratio) FAIL(VC_ERR_STATE, "flux_sample_dopri5: the error ratio of the step at t = %.9g, dt = %.3g is NaN", t, dt);
    if (accept) {
      const double t1 = t + dt;
      for (; next_out < n_points && (double)t_grid[next_out] <= t1; ++next_out) {
        const bool last = next_out == n_points - 1;
        if (!trajectory && !last) continue;
        double theta = ((double)t_grid[next_out] - t) / dt;
        theta = theta < 0.0 ? 0.0 : theta > 1.0 ? 1.0 : theta;
        void* dst = trajectory ? (void*)((char*)trajectory + (int64_t)(next_out - 1) * out_bytes) : x;
        TRY(vc_dopri5_interp_launch(f.AD_Y0, f.AD_Y1, f.AD_K, f.AD_DT, (float)theta, dst, out_bf16, n, s, e.buf, e.len));
        if (trajectory && last) TRY(d2d(x, dst, out_bytes, s, e));
      }
      TRY(d2d(f.AD_Y0, f.AD_Y1, n * 4, s, e));
      TRY(d2d(f.AD_K, f.AD_K + 6 * n, n * 2, s, e));        // first same as last
      t = t1;
    }
    double factor = 10.0;
    if (ratio != 0.0) factor = std::min(10.0, std::max(0.9 / pow(ratio, 1.0 / 5.0), ratio < 1.0 ? 1.0 : 0.2));
    dt *= factor;
  }
  return VC_OK;
}

int vc_flux_sample_dopri5_impl(void* handle, void* x, const void* cond, const float* t_grid, int32_t n_points, int32_t state_is_bf16,
                               float rtol, float atol, int32_t max_attempts, void* trajectory, hipStream_t s, char* err, int errlen) {
  HANDLE(Flux, f, "flux");
  if (!f.prepared) FAIL(VC_ERR_STATE, "flux_sample_dopri5: call vc_flux_prepare first");
  TRY(fresh_scale(f, "flux_sample_dopri5", e));
  if (!x || !cond || !t_grid) FAIL(VC_ERR_ARG, "flux_sample_dopri5: null argument");
  if (f.mon_level)
    FAIL(VC_ERR_ARG, "flux_sample_dopri5: the monitor is on (level %d): the adaptive solve's device-side counter is the stage of an attempt, not "
                     "an evaluation index; turn it off with vc_flux_set_monitor(handle, 0, NULL, 0, NULL)", f.mon_level);
  if (!f.opt.adaptive || !f.AD_K)
    FAIL(VC_ERR_STATE, "flux_sample_dopri5: set vc_flux_set_option(handle, \"adaptive\", 1) before vc_flux_workspace_bytes / vc_flux_prepare "
                       "(the workspace holds no buffers of the adaptive solve)");
  if (f.S < 7) FAIL(VC_ERR_ARG, "flux_sample_dopri5: the workspace was prepared with max_steps = %d, the adaptive solve needs 7", f.S);
  if (n_points < 2) FAIL(VC_ERR_ARG, "flux_sample_dopri5: n_points = %d, at least 2 expected", n_points);
  for (int i = 1; i < n_points; ++i)
    if (!(t_grid[i] > t_grid[i - 1])) FAIL(VC_ERR_ARG, "flux_sample_dopri5: t_grid must increase strictly (index %d)", i);
  if (!(rtol >= 0.0f) || !(atol >= 0.0f) || !(rtol + atol > 0.0f) || !(rtol + atol - (rtol + atol) == 0.0f))
    FAIL(VC_ERR_ARG, "flux_sample_dopri5: rtol = %g and atol = %g must be finite, non-negative and not both zero", rtol, atol);
  if (max_attempts < 1) FAIL(VC_ERR_ARG, "flux_sample_dopri5: max_attempts = %d must be positive", max_attempts);
  if (f.sc_on())
    FAIL(VC_ERR_ARG, "flux_sample_dopri5: the step cache works with VC_SOLVER_EULER only: turn it off with vc_flux_set_step_cache(handle, 0, 0)");
  if (f.cfg_on) {
    if (f.B % 2) FAIL(VC_ERR_ARG, "flux_sample_dopri5: true CFG pairs the first half of the batch with the second: B = %d is odd", f.B);
    if (!(f.cfg_scale - f.cfg_scale == 0.0f)) FAIL(VC_ERR_ARG, "flux_sample_dopri5: the cfg_scale set by vc_flux_set_cfg is not finite");
  }
  if (!f.ad_host) HIP(hipHostMalloc((void**)&f.ad_host, 256, hipHostMallocDefault), "hipHostMalloc");
  const int64_t n = (int64_t)f.B * f.N * f.cfg.out_channels;
  f.in_flight = false;
  f.steps_total = f.steps_done = 0;             // an earlier trajectory's tables are overwritten: steps / end refuse from here on
  f.state_f32 = true;
  f.method = SOLVER_DOPRI5; f.evals = 1;
  f.sc_active = false;
  f.cfg_active = f.cfg_on; f.cfg_s = f.cfg_on ? f.cfg_scale : 1.0f;
  f.ad_log.clear();
  f.ad_evals = 0;
  TRY(vc_dopri5_load_launch(x, state_is_bf16, f.AD_Y0, f.YIN, n, s, e.buf, e.len));
  TRY(d2d(f.COND, cond, (int64_t)f.B * f.N * (f.cfg.in_channels - f.cfg.out_channels) * 2, s, e));
  {  // the warm-up evaluation of a new capture indexes the modulation rows by the counter and reads dt: both defined first
    HIP(hipMemsetAsync(f.STEP, 0, sizeof(int32_t), s), "hipMemsetAsync");
    TRY(dopri5_rows(f, (double)t_grid[0], 0.0, s, e));
  }
  if (s) TRY(step_graph(f, s, e));
  const int rc = dopri5_run(f, x, t_grid, n_points, state_is_bf16 != 0, rtol, atol, max_attempts, trajectory, s, e);
  f.method = VC_SOLVER_EULER;
  return rc;
}

int vc_flux_dopri5_log_impl(void* handle, double* t, double* dt, float* ratio, int32_t* accepted, int32_t capacity, int32_t* attempts,
                            int32_t* evaluations, char* err, int errlen) {
  HANDLE(Flux, f, "flux");
  if (capacity < 0) FAIL(VC_ERR_ARG, "flux_dopri5_log: capacity = %d is negative", capacity);
  const int count = std::min<int>(capacity, (int)f.ad_log.size());
  for (int i = 0; i < count; ++i) {
    if (t) t[i] = f.ad_log[i].t;
    if (dt) dt[i] = f.ad_log[i].dt;
    if (ratio) ratio[i] = f.ad_log[i].ratio;
    if (accepted) accepted[i] = f.ad_log[i].accepted;
  }
  if (attempts) *attempts = (int32_t)f.ad_log.size();
  if (evaluations) *evaluations = f.ad_evals;
  return VC_OK;
}

// ---------------------------------------------------------------- the stochastic sampler (vcloze_hip.h: vc_flux_sample_sde)
int vc_flux_sample_sde_impl(void* handle, const char* method, void* x, const void* cond, const float* t_grid, int32_t n_points, const char* form,
                            double norm, const char* last_step, double last_step_size, uint64_t seed, uint64_t offset, int32_t state_is_bf16,
                            void* trajectory, hipStream_t s, char* err, int errlen) {
  HANDLE(Flux, f, "flux");
  // ---- every check before the device is touched
  if (!f.prepared) FAIL(VC_ERR_STATE, "flux_sample_sde: call vc_flux_prepare first");
  TRY(fresh_scale(f, "flux_sample_sde", e));
  if (!x || !cond || !t_grid) FAIL(VC_ERR_ARG, "flux_sample_sde: null argument");
  if (!f.opt.sde || !f.SD_Y)
    FAIL(VC_ERR_STATE, "flux_sample_sde: set vc_flux_set_option(handle, \"sde\", 1) before vc_flux_workspace_bytes / vc_flux_prepare "
                       "(the workspace holds no buffers of the stochastic sampler)");
  if (f.mon_level)
    FAIL(VC_ERR_ARG, "flux_sample_sde: the monitor is on (level %d): its log is indexed by the evaluations of a fixed-grid trajectory; turn it "
                     "off with vc_flux_set_monitor(handle, 0, NULL, 0, NULL)", f.mon_level);
  if (f.sc_on())
    FAIL(VC_ERR_ARG, "flux_sample_sde: the step cache works with VC_SOLVER_EULER only: turn it off with vc_flux_set_step_cache(handle, 0, 0)");
  int32_t n_evals = 0, n_draws = 0;
  TRY(vc_sde_plan_impl(method, form, norm, last_step, last_step_size, t_grid, n_points, nullptr, nullptr, 0, &n_evals, &n_draws, err, errlen));
  if (n_evals > f.S)
    FAIL(VC_ERR_ARG, "flux_sample_sde: %d evaluations (%d points, method %s), the prepared workspace holds 1..%d evaluations", n_evals, n_points,
         method, f.S);
  if (f.cfg_on) {
    if (f.B % 2) FAIL(VC_ERR_ARG, "flux_sample_sde: true CFG pairs the first half of the batch with the second: B = %d is odd", f.B);
    if (!(f.cfg_scale - f.cfg_scale == 0.0f)) FAIL(VC_ERR_ARG, "flux_sample_sde: the cfg_scale set by vc_flux_set_cfg is not finite");
  }
  const int B = f.B;
  const int64_t n = (int64_t)B * f.N * f.cfg.out_channels;
  if ((unsigned __int128)offset + (unsigned __int128)n_draws * (unsigned __int128)n > ((unsigned __int128)1 << 64))
    FAIL(VC_ERR_ARG, "flux_sample_sde: offset + draws * n leaves the 64-bit stream position (offset=%llu, %d draws of %lld elements)",
         (unsigned long long)offset, n_draws, (long long)n);
  const bool heun = !strcmp(method, "Heun");
  const int n_rows = n_evals + (heun ? 1 : 0), E = heun ? 2 : 1, out_bf16 = state_is_bf16 != 0;
  const int64_t out_bytes = n * (out_bf16 ? 2 : 4);
  // ---- the tables of the whole trajectory: model times, coefficient rows, the stream's seed and offset
  TRY(stage_begin(f, ((size_t)n_evals * B + (size_t)n_rows * VC_SDE_ROW + n_evals) * sizeof(float) + 2 * sizeof(uint64_t) + 4 * 256, e));
  float* ts = stage_take<float>(f, (size_t)n_evals * B);
  float* rows = stage_take<float>(f, (size_t)n_rows * VC_SDE_ROW);
  float* times = stage_take<float>(f, n_evals);
  uint64_t* words = stage_take<uint64_t>(f, 2);
  TRY(vc_sde_plan_impl(method, form, norm, last_step, last_step_size, t_grid, n_points, rows, times, n_rows, nullptr, nullptr, err, errlen));
  for (int j = 0; j < n_evals; ++j)
    for (int b = 0; b < B; ++b) ts[(size_t)j * B + b] = times[j];
  words[0] = seed; words[1] = offset;
  f.in_flight = false;
  f.steps_total = f.steps_done = 0;             // an earlier trajectory's tables are overwritten: steps / end refuse from here on
  TRY(stage_send(f, f.TS, ts, (size_t)n_evals * B * sizeof(float), s, e));
  TRY(stage_send(f, f.SD_TAB, rows, (size_t)n_rows * VC_SDE_ROW * sizeof(float), s, e));
  TRY(stage_send(f, f.SD_RNG, words, 2 * sizeof(uint64_t), s, e));
  TRY(stage_end(f, s, e));
  TRY(time_precompute(f, n_evals, 0, s, e));
  f.state_f32 = true;
  f.method = heun ? SOLVER_SDE_HEUN : SOLVER_SDE_EULER; f.evals = 1;
  f.sc_active = false;
  f.cfg_active = f.cfg_on; f.cfg_s = f.cfg_on ? f.cfg_scale : 1.0f;
  auto run = [&]() -> int {
    TRY(vc_dopri5_load_launch(x, state_is_bf16, f.SD_Y, f.YIN, n, s, e.buf, e.len));      // the F32 state and its bf16 shadow
    TRY(d2d(f.COND, cond, (int64_t)B * f.N * (f.cfg.in_channels - f.cfg.out_channels) * 2, s, e));
    HIP(hipMemsetAsync(f.STEP, 0, sizeof(int32_t), s), "hipMemsetAsync");
    if (s) TRY(step_graph(f, s, e));
    // Heun: draw 0 goes in ahead of the first evaluation (the row behind the evaluations' rows)
    if (heun) TRY(vc_sde_stage_launch(n_evals, f.SD_TAB, f.S + 1, f.SD_Y, nullptr, f.YIN, f.SD_XHAT, f.SD_K1, f.SD_RNG, nullptr, n, s, e.buf, e.len));
    for (int j = 0; j < n_evals; ++j) {
      if (s) HIP(hipGraphLaunch(f.step.g[0], s), "hipGraphLaunch");
      else TRY(evaluate(f, f.STEP, true, nullptr, nullptr, true, s, e));
      // x' after every loop step; the last step's result (or, without one, x' again) as the final row
      const bool step_done = j < (n_points - 1) * E && (j + 1) % E == 0;
      if (trajectory && step_done) TRY(vc_sde_store_launch(f.SD_Y, (char*)trajectory + (int64_t)(j / E) * out_bytes, out_bf16, n, s, e.buf, e.len));
    }
    if (trajectory) TRY(vc_sde_store_launch(f.SD_Y, (char*)trajectory + (int64_t)(n_points - 1) * out_bytes, out_bf16, n, s, e.buf, e.len));
    return vc_sde_store_launch(f.SD_Y, x, out_bf16, n, s, e.buf, e.len);
  };
  const int rc = run();
  f.method = VC_SOLVER_EULER;
  return rc;
}

int vc_flux_set_step_cache_impl(void* handle, float threshold, int32_t max_consecutive, char* err, int errlen) {
  HANDLE(Flux, f, "flux");
  if (threshold != threshold) FAIL(VC_ERR_ARG, "flux_set_step_cache: threshold is NaN");
  f.sc_threshold = threshold > 0.0f ? threshold : 0.0f;
  f.sc_max = max_consecutive;
  return VC_OK;
}

int vc_flux_set_cfg_impl(void* handle, int32_t on, float cfg_scale, char* err, int errlen) {
  HANDLE(Flux, f, "flux");
  f.cfg_on = on != 0;
  f.cfg_scale = cfg_scale;       // held to finite at the next vc_flux_sample_begin*, where the setting takes effect
  return VC_OK;
}

int vc_flux_step_cache_stats_impl(void* handle, int32_t* computed, int32_t* reused, float* metrics, int32_t capacity, char* err, int errlen) {
  HANDLE(Flux, f, "flux");
  if (capacity < 0 || (capacity > 0 && !metrics)) FAIL(VC_ERR_ARG, "flux_step_cache_stats: bad arguments");
  if (computed) *computed = f.sc_computed;
  if (reused) *reused = f.sc_reused;
  const int done = f.sc_computed + f.sc_reused;
  for (int i = 0; i < capacity; ++i) metrics[i] = i < done && i < (int)f.sc_metrics.size() ? f.sc_metrics[i] : NAN;
  return VC_OK;
}

// HIP-event times of the launches of the product's plan, class by class (vcloze_hip.h): `evaluations` evaluations of the sample in
// flight at its current step, issued un-captured on `s` by the same code that the step graph was captured from, no Euler update
// (the trajectory's state, its step counter and its graph are left as they are).
int vc_flux_profile_impl(void* handle, int32_t evaluations, VcFluxLaunchClass* out, int32_t capacity, int32_t* count, hipStream_t s,
                         char* err, int errlen) {
  HANDLE(Flux, f, "flux");
  if (!f.prepared || f.steps_total == 0) FAIL(VC_ERR_STATE, "flux_profile: call vc_flux_sample_begin first");
  if (!out || !count || capacity <= 0 || evaluations <= 0) FAIL(VC_ERR_ARG, "flux_profile: bad argument");
  f.mon_paused = true;                                                 // the trajectory's log keeps its rows
  int rc = evaluate(f, f.STEP, true, nullptr, nullptr, false, s, e);   // warm: caches and clocks as inside a trajectory
  f.prof_recs.clear();
  f.prof_used = 0;
  f.prof_on = true;
  for (int i = 0; i < evaluations && rc == VC_OK; ++i) rc = evaluate(f, f.STEP, true, nullptr, nullptr, false, s, e);
  f.prof_on = false;
  f.mon_paused = false;
  if (rc != VC_OK) return rc;
  HIP(hipStreamSynchronize(s), "hipStreamSynchronize");
  int n = 0;
  for (const auto& r : f.prof_recs) {
    float ms = 0.f;
    HIP(hipEventElapsedTime(&ms, f.prof_ev[r.e0], f.prof_ev[r.e0 + 1]), "hipEventElapsedTime");
    const float us = ms * 1e3f;
    int j = 0;
    while (j < n && !(out[j].kind == r.kind && out[j].epi == r.epi && out[j].n == r.n && out[j].k == r.k)) ++j;
    if (j == n) {
      if (n == capacity) FAIL(VC_ERR_ARG, "flux_profile: more than %d launch classes", capacity);
      memset(&out[n], 0, sizeof(out[n]));
      out[n].kind = r.kind; out[n].epi = r.epi; out[n].n = r.n; out[n].k = r.k;
      out[n].min_us = us; out[n].max_us = us;
      ++n;
    }
    out[j].launches += 1;
    out[j].flops += r.flops;
    out[j].bytes += r.bytes;
    out[j].total_us += us;
    if (us < out[j].min_us) out[j].min_us = us;
    if (us > out[j].max_us) out[j].max_us = us;
  }
  *count = n;
  return VC_OK;
}
