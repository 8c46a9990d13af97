// Handle API of include/vcloze_hip.h: Flux.forward (models/model.py:85-124) and the fixed-grid solver loop around it
// (transport/integrators.py:106-120: Euler, and midpoint / rk4 as E evaluations per step) as launch plans over the kernels of this library.  Host code only: it ORDERS launches
// (once per geometry, under stream capture, for the sampling loop); nothing here touches a tensor element except the RoPE
// angle table, which math.py:102-109 computes in float64 on the host as well (flux_rules.h).  This unit is the launch plan and
// nothing else: what is bound lives in flux_weights.hip, what a solver does in flux_sample.hip, the handle itself in flux_state.h.
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
//   AD_K [7][B*N*out] / AD_Y0 / AD_Y1 (f32)  only with option adaptive 1, behind the step cache's: k1..kS (S <= 7: the pair's stages),
//                           the state and the step's end state of the adaptive solve (vc_flux_sample_dopri5 / vc_flux_sample_rk,
//                           rk_embedded.hip), its dt, norms and reduction scratch
//   SD_Y / SD_XHAT / SD_K1 (f32) / SD_TAB / SD_RNG  only with option sde 1, behind the adaptive solve's: the state, x-hat and K1 of the
//                           stochastic sampler (vc_flux_sample_sde, rng.hip), its coefficient table ([S + 1][VC_SDE_ROW] f32) and the
//                           seed / offset words its update reads
//   FM_U (f32) / FM_T / FM_PART  only with option eval_loss 1, behind the stochastic sampler's: u_t = x1 - x0 of vc_flux_eval_loss
//                           (fm_loss.hip), its B times and the partial sums of its reduction
//   MS_Y (f32) / MS_HIST / MS_TAB  only with option multistep 1, behind the loss's: the state of the Adams-Bashforth solve
//                           (vc_flux_sample_multistep, multistep.hip), its ring of VC_MS_HIST past model outputs ([3][B*N*out] bf16) and
//                           its coefficient table ([S][VC_MS_ROW] f32)
//   LY / LY2 / LH / LSCALE  only in the un-merged LoRA mode (option lora_mode 1), behind everything else: base_out, base_out + lora
//                           and lora_A(x) of the Linear being run, and the lora scale as a bf16 vector (the gate operand of the
//                           gated-residual epilogue that adds the lora branch; refilled by vc_flux_set_lora_scale)
#include "flux_state.h"

namespace vcflux {
namespace {

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
  if (g.opt.eval_loss) {   // likewise
    f.FM_U = c.take<float>((int64_t)B * N * out_ch); f.FM_T = c.take<float>(B);
    f.FM_PART = c.take<float>((int64_t)B * VC_FM_LOSS_MAX_BLOCKS);
  }
  if (g.opt.multistep) {   // likewise
    const int64_t n = (int64_t)B * N * out_ch;
    f.MS_Y = c.take<float>(n); f.MS_HIST = c.take<bf16_t>(VC_MS_HIST * n); f.MS_TAB = c.take<float>((int64_t)S * VC_MS_ROW);
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

// vc_flux_set_monitor: site `site` of the evaluation `*step_ptr` (row 0 without a counter) <- vc_tensor_stats of the B samples of
// rows x cols contiguous elements at x, one launch (two kernels) on the evaluation's own stream
int monitor(Flux& f, int site, const void* x, bool x_f32, int64_t rows, int cols, const int32_t* step_ptr, hipStream_t s, Err e) {
  if (!f.mon_level || f.mon_paused) return VC_OK;
  const int ns = f.mon_sites();
  return vc_tensor_stats_launch(x, x_f32, rows * cols, cols, f.B, rows, cols, f.mon_log + vcmon::log_index(0, site, 0, f.mon_cap, ns, f.B),
                                vcmon::log_row_stride(ns, f.B), step_ptr, f.mon_cap, f.mon_scratch, s, e.buf, e.len);
}
// a tap site: the residual stream `src` ([B * rows, D] bf16) directly behind its block.  vc_flux_set_tap: tap `idx` <- the stream, one
// copy node on the evaluation's own stream; monitor level 2: its statistics, read in place
int tap(Flux& f, int idx, const bf16_t* src, int rows, const int32_t* step_ptr, hipStream_t s, Err e) {
  if ((size_t)idx < f.taps.size() && f.taps[idx]) {
    const int64_t bytes = (int64_t)f.B * rows * f.D * 2;
    TRY(prof_open(f, s, VC_LAUNCH_TAP, 0, 0, 0, 0, 2.0 * bytes, e));       // every tap in ONE launch class
    TRY(d2d(f.taps[idx], src, bytes, s, e.buf, e.len));
    TRY(prof_close(f, s, e));
  }
  return f.mon_level >= 2 ? monitor(f, vcmon::site_of_tap(idx), src, false, rows, f.D, step_ptr, s, e) : VC_OK;
}
int tap_double(Flux& f, int i, const int32_t* step_ptr, hipStream_t s, Err e) {
  TRY(tap(f, vcmon::tap_double(i, false), f.XI, f.N, step_ptr, s, e));
  return tap(f, vcmon::tap_double(i, true), f.XT, f.T, step_ptr, s, e);
}

// Flux.forward in three pieces, which an evaluation issues back to back and the cached step issues with its own launches in
// between: the inputs, the blocks from double block `first` on, the last layer (+ the solver's update).  step_ptr counts EVALUATIONS
// (= steps for Euler).  The inputs: `img_rows`, or without them x || cond of the trajectory (next_input, flux_state.h) through XIN
int eval_inputs(Flux& f, const void* img_rows, const int32_t* step_ptr, hipStream_t s, Err e) {
  const int B = f.B, T = f.T, N = f.N, D = f.D;
  const int in_ch = f.cfg.in_channels, out_ch = f.cfg.out_channels;
  if (!img_rows) TRY(vc_concat_cols_launch(next_input(f), out_ch, f.COND, in_ch - out_ch, f.XIN, (int64_t)B * N, s, e.buf, e.len));
  TRY(d2d(f.XT, f.TXT0, (int64_t)B * T * D * 2, s, e.buf, e.len));
  TRY(lin(f, f.img_in, img_rows ? img_rows : f.XIN, in_ch, f.XI, D, B * N, VC_EPI_BIAS, s, e));
  TRY(tap(f, vcmon::tap_img_in(), f.XI, N, step_ptr, s, e));
  return tap(f, vcmon::tap_txt_in(), f.XT, T, step_ptr, s, e);
}
int eval_blocks(Flux& f, const Ctx& c, size_t first, Err e) {
  const int B = f.B, T = f.T, N = f.N, L = f.L, D = f.D;
  hipStream_t s = c.s;
  for (size_t i = first; i < f.dbl.size(); ++i) { TRY(double_block(f, c, f.dbl[i], e)); TRY(tap_double(f, (int)i, c.step_ptr, s, e)); }
  for (int b = 0; b < B; ++b) {   // cat((txt, img), 1) per sample (model.py:116)
    TRY(d2d(f.X + (int64_t)b * L * D, f.XT + (int64_t)b * T * D, (int64_t)T * D * 2, s, e.buf, e.len));
    TRY(d2d(f.X + ((int64_t)b * L + T) * D, f.XI + (int64_t)b * N * D, (int64_t)N * D * 2, s, e.buf, e.len));
  }
  for (size_t i = 0; i < f.sgl.size(); ++i) {
    TRY(single_block(f, c, f.sgl[i], e));
    TRY(tap(f, vcmon::tap_single(f.cfg.depth, (int)i), f.X, L, c.step_ptr, s, e));
  }
  return VC_OK;
}
// the last layer -> `out` (V when NULL); with `update` true CFG's combine, the update of the trajectory's solver (ode_update) and the
// counter's advance behind it
int eval_output(Flux& f, const Ctx& c, void* out, bool update, Err e) {
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
  if (update) {
    if (f.cfg_active) {    // V is sample-major: its first half is the conditional samples' velocity, combined in place
      const int64_t half = (int64_t)(B / 2) * N * out_ch;
      TRY(vc_cfg_combine_launch(f.V, f.V + half, f.V, half, f.cfg_s, s, e.buf, e.len));
    }
    TRY(ode_update(f, f.V, step_ptr, s, e.buf, e.len));
    TRY(monitor(f, vcmon::SITE_X, ode_state(f), f.traj.state_f32, N, out_ch, step_ptr, s, e));
    TRY(vc_step_advance_launch((int32_t*)step_ptr, s, e.buf, e.len));
  }
  return VC_OK;
}
// the three shapes an evaluation is issued in.  vc_flux_forward: the caller's rows -> the caller's `out`, modulation row 0, no counter
int eval_to_last_layer(Flux& f, const Ctx& c, const void* img_rows, Err e) {
  TRY(eval_inputs(f, img_rows, c.step_ptr, c.s, e));
  return eval_blocks(f, c, 0, e);
}
int forward_rows(Flux& f, const void* img_rows, void* out, hipStream_t s, Err e) {
  Ctx c{nullptr, s, (int64_t)f.B * f.n_mod};
  TRY(eval_to_last_layer(f, c, img_rows, e));
  return eval_output(f, c, out, false, e);
}
// an evaluation of the trajectory at its counter -> V, the state untouched (the warm-up of a capture, vc_flux_profile) ...
int step_eval(Flux& f, hipStream_t s, Err e) {
  Ctx c{f.STEP, s, (int64_t)f.B * f.n_mod};
  TRY(eval_to_last_layer(f, c, nullptr, e));
  return eval_output(f, c, nullptr, false, e);
}
// ... and the step: that evaluation with the update behind it
int step(Flux& f, hipStream_t s, Err e) {
  Ctx c{f.STEP, s, (int64_t)f.B * f.n_mod};
  TRY(eval_to_last_layer(f, c, nullptr, e));
  return eval_output(f, c, nullptr, true, e);
}

// ---- the step cache: one Euler evaluation as head + ONE of two tails, chosen by the host from the metric
// head: the plan up to double block 0 (h0 is parked in X, which nothing uses before the streams are joined), then r, the metric and
// its 4-byte copy to pinned host memory
int cache_head(Flux& f, hipStream_t s, Err e) {
  const int64_t nd = (int64_t)f.N * f.D;
  Ctx c{f.STEP, s, (int64_t)f.B * f.n_mod};
  TRY(eval_inputs(f, nullptr, f.STEP, s, e));
  TRY(d2d(f.X, f.XI, f.B * nd * 2, s, e.buf, e.len));                                   // h0
  TRY(double_block(f, c, f.dbl[0], e));                                      // XI = h1
  TRY(tap_double(f, 0, f.STEP, s, e));
  TRY(vc_residual_change_launch(f.X, f.XI, f.SC_P, f.SC_RS, nullptr, f.SC_METRIC, f.SC_PART, f.B, nd, s, e.buf, e.len));
  HIP(hipMemcpyAsync(f.sc_host, f.SC_METRIC, sizeof(float), hipMemcpyDeviceToHost, s), "hipMemcpyAsync(D2H)");
  return VC_OK;
}
// tail-compute: P <- r, the scratch keeps h1, blocks 1..end, R <- hE - h1, then the last layer and the update as ever
int cache_tail_compute(Flux& f, bool update, hipStream_t s, Err e) {
  const int64_t nd = (int64_t)f.N * f.D;
  Ctx c{f.STEP, s, (int64_t)f.B * f.n_mod};
  TRY(d2d(f.SC_P, f.SC_RS, f.B * nd * 2, s, e.buf, e.len));
  TRY(d2d(f.SC_RS, f.XI, f.B * nd * 2, s, e.buf, e.len));
  TRY(eval_blocks(f, c, 1, e));
  TRY(vc_residual_op_launch(0, f.X + (int64_t)f.T * f.D, (int64_t)f.L * f.D, f.SC_RS, nd, f.SC_R, nd, f.B, nd, s, e.buf, e.len));
  return eval_output(f, c, nullptr, update, e);
}
// tail-reuse: the image rows of X <- h1 + R (its text rows keep the last computed evaluation's: the last layer reads image rows only)
int cache_tail_reuse(Flux& f, bool update, hipStream_t s, Err e) {
  const int64_t nd = (int64_t)f.N * f.D;
  Ctx c{f.STEP, s, (int64_t)f.B * f.n_mod};
  TRY(vc_residual_op_launch(1, f.XI, nd, f.SC_R, nd, f.X + (int64_t)f.T * f.D, (int64_t)f.L * f.D, f.B, nd, s, e.buf, e.len));
  return eval_output(f, c, nullptr, update, e);
}


void drop_prof(Flux& f) {
  for (auto ev : f.prof_ev) (void)hipEventDestroy(ev);
  f.prof_ev.clear();
}
}  // namespace

int d2d(void* dst, const void* src, int64_t bytes, hipStream_t s, char* err, int errlen) {
  Err e{err, errlen};
  HIP(hipMemcpyAsync(dst, src, (size_t)bytes, hipMemcpyDeviceToDevice, s), "hipMemcpyAsync");
  return VC_OK;
}

// the log was sized for the B prepared when the monitor was set: another B would run past its rows
int monitor_fits(Flux& f, const char* what, char* err, int errlen) {
  Err e{err, errlen};
  if (f.mon_level && f.mon_B && f.mon_B != f.B)
    FAIL(VC_ERR_STATE, "%s: the monitor's log was sized for B = %d, the prepared B is %d: ask vc_flux_monitor_bytes and call vc_flux_set_monitor again",
         what, f.mon_B, f.B);
  if (f.mon_level) f.mon_B = f.B;
  return VC_OK;
}
// the solver's update behind an evaluation (v = V), or with v null next_input = bf16(state) alone; next_input is not handed over
// where it IS the state (the kernel's pointers are __restrict__)
int ode_update(Flux& f, const void* v, const int32_t* step_ptr, hipStream_t s, char* err, int errlen) {
  Err e{err, errlen};
  if (f.traj.method == SOLVER_RK)          // the stage of the adaptive solve is the device-side counter itself, the tableau the pair's
    return vc_rk_stage_launch(f.traj.rk, -1, f.AD_Y0, f.AD_K, v, f.AD_DT, step_ptr, f.AD_Y1, f.YIN, (int64_t)f.B * f.N * f.cfg.out_channels, s,
                              e.buf, e.len);
  if (f.traj.method == SOLVER_SDE_EULER || f.traj.method == SOLVER_SDE_HEUN)      // the table row of the update is the device-side counter itself
    return vc_sde_stage_launch(-1, f.SD_TAB, f.S + 1, f.SD_Y, v, f.YIN, f.SD_XHAT, f.SD_K1, f.SD_RNG, step_ptr,
                               (int64_t)f.B * f.N * f.cfg.out_channels, s, e.buf, e.len);
  if (f.traj.method == SOLVER_MULTISTEP)   // likewise: the row holds the order
    return vc_ms_stage_launch(-1, f.MS_TAB, f.S, f.MS_Y, v, f.MS_HIST, f.YIN, step_ptr, (int64_t)f.B * f.N * f.cfg.out_channels, s, e.buf,
                              e.len);
  void* y = ode_state(f);
  bf16_t* y_in = next_input(f);
  return vc_ode_update_launch("ode_update launch", f.traj.method, -1, y, !f.traj.state_f32, v, f.KS, y_in == y ? nullptr : y_in, f.DTS, step_ptr,
                              (int64_t)f.B * f.N * f.cfg.out_channels, s, e.buf, e.len);
}

// ---------------------------------------------------------------- host staging
int stage_begin(Flux& f, size_t bytes, char* err, int errlen) {
  Err e{err, errlen};
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
int stage_send(Flux& f, void* dst, const void* staged, size_t bytes, hipStream_t s, char* err, int errlen) {
  Err e{err, errlen};
  HIP(hipMemcpyAsync(dst, staged, bytes, hipMemcpyHostToDevice, s), "hipMemcpyAsync(H2D)");
  return VC_OK;
}
int stage_end(Flux& f, hipStream_t s, char* err, int errlen) {
  Err e{err, errlen};
  if (!f.staged) HIP(hipEventCreateWithFlags(&f.staged, hipEventDisableTiming), "hipEventCreate");
  HIP(hipEventRecord(f.staged, s), "hipEventRecord");
  f.staged_pending = true;
  return VC_OK;
}
// timestep embedding -> time_in MLP -> vec = time + guidance + vector -> every modulation of every (step, sample):
// model.py:102-108 + layers.py:120-126 for all modules in ONE GEMM.  times: rows s*B + b already in TS.
int time_precompute(Flux& f, int S, int timesteps_is_bf16, hipStream_t s, char* err, int errlen) {
  Err e{err, errlen};
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

void drop_graph(Flux& f) {
  f.graphs.clear();
  f.step = Flux::Step{};
}

int step_piece(Flux& f, int piece, bool update, hipStream_t s, char* err, int errlen) {
  Err e{err, errlen};
  if (!f.traj.cached) return update ? step(f, s, e) : step_eval(f, s, e);
  return piece == 0 ? cache_head(f, s, e) : piece == 1 ? cache_tail_compute(f, update, s, e) : cache_tail_reuse(f, update, s, e);
}

// the hipGraph of ONE evaluation + the solver's update behind it (Euler: one solver step): everything that depends on the
// evaluation (modulation rows, dt, the stage of a midpoint / rk4 step) is indexed on the device by STEP
int step_graph(Flux& f, hipStream_t s, char* err, int errlen) {
  Err e{err, errlen};
  Flux::Key k{f.base, f.B, f.T, f.N, f.S, f.ragged, f.gapped, attention_variant(f), f.traj.state_f32, f.traj.method, f.traj.cached, f.opt, s,
               f.cfg_active, 0, {}, f.mon_level, f.mon_cap, f.mon_log, f.mon_scratch};
  if (f.cfg_active) memcpy(&k.cfg_bits, &f.cfg_s, 4);
  k.taps = f.taps;
  k.rk = f.traj.method == SOLVER_RK ? f.traj.rk : 0;
  if (const Flux::Step* hit = f.graphs.find(k)) {
    f.step = *hit; f.key = k;
    return VC_OK;
  }
  f.step = Flux::Step{};
  Flux::Step st;
  int rc = VC_OK;
  const int pieces = f.traj.cached ? 3 : 1;
  // warm-up outside capture (kernel attributes are set on first launch): one evaluation into V, the state is untouched (cached: through
  // the three pieces - P, R and the scratch it writes are rewritten by the trajectory's first evaluation, which always computes,
  // before anything reads them)
  for (int i = 0; i < pieces; ++i) TRY(step_piece(f, i, false, s, err, errlen));
  for (int i = 0; i < pieces && rc == VC_OK; ++i)
    rc = capture(s, st.g[i], e, [&] { return step_piece(f, i, true, s, err, errlen); }, &st.nodes[i]);
  if (rc != VC_OK) {
    Flux::DropStep()(st);          // the graphs of a half-captured step
    return rc;
  }
  f.graphs.insert(k, st);
  f.step = st; f.key = k;
  return VC_OK;
}

// lora_mode 1: what vc_flux_prepare parked in the workspace (txt_in, vector_in, guidance_in) ran with the scale of that moment
int fresh_scale(const Flux& f, const char* what, char* err, int errlen) {
  Err e{err, errlen};
  if (f.opt.lora_mode && f.scale_stale)
    FAIL(VC_ERR_STATE, "%s: the lora scale changed after vc_flux_prepare, whose txt_in / vector_in / guidance_in projections ran with the old "
                       "one: call vc_flux_prepare again (captured steps are kept)", what);
  return VC_OK;
}

}  // namespace vcflux
using namespace vcflux;

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

// a tap's name -> its index (vcrules::tap_index), or the refusal
static int tap_index(Flux& f, const char* what, const char* name, size_t& idx, Err e) {
  if (!name) FAIL(VC_ERR_ARG, "%s: null name", what);
  switch (vcrules::tap_index(name, f.cfg.depth, f.cfg.depth_single_blocks, &idx)) {
    case vcrules::TAP_OK: return VC_OK;
    case vcrules::TAP_NO_DOUBLE: FAIL(VC_ERR_ARG, "%s: name = '%s', the model has %d double blocks", what, name, f.cfg.depth);
    case vcrules::TAP_NO_SINGLE: FAIL(VC_ERR_ARG, "%s: name = '%s', the model has %d single blocks", what, name, f.cfg.depth_single_blocks);
    case vcrules::TAP_UNKNOWN: break;
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

int vc_flux_plan_count_impl(void* handle) { return handle ? (int)((Flux*)handle)->graphs.size() : -1; }

int vc_flux_tap_shape_impl(void* handle, const char* name, int64_t* rows, int32_t* cols, char* err, int errlen) {
  HANDLE(Flux, f, "flux");
  size_t idx = 0;
  TRY(tap_index(f, "flux_tap_shape", name, idx, e));
  if (!rows || !cols) FAIL(VC_ERR_ARG, "flux_tap_shape: null rows / cols");
  if (!f.prepared) FAIL(VC_ERR_STATE, "flux_tap_shape: call vc_flux_prepare first (the rows are those of the prepared geometry)");
  *rows = (int64_t)f.B * vcrules::tap_rows(idx, f.cfg.depth, f.T, f.N);
  *cols = f.D;
  return VC_OK;
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
    if ((o.member == &Options::lora_mode || o.member == &Options::adaptive || o.member == &Options::sde ||
         o.member == &Options::eval_loss || o.member == &Options::multistep) && value != f.opt.*o.member) {
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
  TRY(resolve(f, e.buf, e.len));
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
  f.n_img.assign((size_t)B, N);
  for (int b = 0; b < B; ++b)
    if (in->kv_len) f.n_img[b] = std::min(std::max(in->kv_len[b] - T, 0), N);
  // host tables -> pinned staging -> HBM
  const size_t n_rope = (size_t)B * L * 128;
  TRY(stage_begin(f, (n_rope + 128 + 4 * B + 64) * sizeof(float) + 8 * 256, e.buf, e.len));
  float* rope = stage_take<float>(f, n_rope);
  vcrules::rope_table(f.cfg.axes_dim, (double)f.cfg.theta, B, T, N, in->txt_ids, in->img_ids, rope);
  float* freqs = stage_take<float>(f, 128);
  vcrules::timestep_freqs(freqs);
  int32_t* kvl = stage_take<int32_t>(f, B);
  int32_t* gap = stage_take<int32_t>(f, 2 * B);
  float* g32 = stage_take<float>(f, B);
  for (int b = 0; b < B; ++b) {
    kvl[b] = in->kv_len ? in->kv_len[b] : L;
    gap[2 * b] = in->kv_gap ? in->kv_gap[2 * b] : 0;
    gap[2 * b + 1] = in->kv_gap ? in->kv_gap[2 * b + 1] : 0;
    g32[b] = in->guidance ? in->guidance[b] : 0.0f;
  }
  TRY(stage_send(f, f.ROPE, rope, n_rope * sizeof(float), s, e.buf, e.len));
  {
    auto it = f.bound.find("timestep_freqs");     // the caller's own table (torch's f32 exp), bit for bit
    if (it != f.bound.end()) {
      if (it->second.N * it->second.K != 128) FAIL(VC_ERR_ARG, "flux_prepare: 'timestep_freqs' must hold 128 f32 values");
      TRY(d2d(f.FREQS, it->second.w, 128 * sizeof(float), s, e.buf, e.len));
    } else {
      TRY(stage_send(f, f.FREQS, freqs, 128 * sizeof(float), s, e.buf, e.len));
    }
  }
  TRY(stage_send(f, f.KVLEN, kvl, B * sizeof(int32_t), s, e.buf, e.len));
  TRY(stage_send(f, f.KVGAP, gap, 2 * B * sizeof(int32_t), s, e.buf, e.len));
  TRY(stage_send(f, f.G32, g32, B * sizeof(float), s, e.buf, e.len));
  TRY(stage_end(f, s, e.buf, e.len));
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
  TRY(fresh_scale(f, "flux_forward", e.buf, e.len));
  if (!img || !timesteps || !out) FAIL(VC_ERR_ARG, "flux_forward: null argument");
  TRY(monitor_fits(f, "flux_forward", e.buf, e.len));
  TRY(stage_begin(f, f.B * sizeof(float) + 256, e.buf, e.len));
  float* ts = stage_take<float>(f, f.B);
  for (int b = 0; b < f.B; ++b) ts[b] = timesteps[b];
  TRY(stage_send(f, f.TS, ts, f.B * sizeof(float), s, e.buf, e.len));
  TRY(stage_end(f, s, e.buf, e.len));
  TRY(time_precompute(f, 1, timesteps_is_bf16, s, e.buf, e.len));
  f.steps_total = f.steps_done = 0;   // MOD now holds this evaluation's rows, not a trajectory's
  f.in_flight = false;
  if (f.mon_level) {      // row 0 of a zeroed log
    TRY(vc_zero_fill_launch(f.mon_log, vcmon::log_bytes(f.mon_cap, f.mon_sites(), f.B), s, e.buf, e.len));
    f.mon_evals = 1;
  }
  return forward_rows(f, img, out, s, e);
}

// ONE evaluation as the flow-matching loss sees it (vcloze_hip.h): the path sample x_t -> XIN beside the cond columns, u_t -> FM_U,
// vc_flux_forward's evaluation of XIN at timesteps 1 - t -> V, the masked squared error of (V, FM_U) -> loss
int vc_flux_eval_loss_impl(void* handle, const void* x1, int32_t x1_is_f32, const void* cond, const float* t, const void* x0, uint64_t seed,
                           uint64_t offset, float* loss, hipStream_t s, char* err, int errlen) {
  HANDLE(Flux, f, "flux");
  if (!f.prepared) FAIL(VC_ERR_STATE, "flux_eval_loss: call vc_flux_prepare first");
  if (!f.opt.eval_loss || !f.FM_U)
    FAIL(VC_ERR_STATE, "flux_eval_loss: set vc_flux_set_option(handle, \"eval_loss\", 1) before vc_flux_workspace_bytes / vc_flux_prepare");
  if (f.cfg_on) FAIL(VC_ERR_STATE, "flux_eval_loss: true CFG is on (vc_flux_set_cfg): the loss is that of Flux.forward, never of forward_with_cfg");
  if (f.in_flight) FAIL(VC_ERR_STATE, "flux_eval_loss: a trajectory is in flight (vc_flux_sample_end first)");
  TRY(fresh_scale(f, "flux_eval_loss", e.buf, e.len));
  if (!x1 || !t || !loss) FAIL(VC_ERR_ARG, "flux_eval_loss: null x1 / t / loss");
  const int B = f.B, N = f.N, in_ch = f.cfg.in_channels, out_ch = f.cfg.out_channels;
  if (!cond) FAIL(VC_ERR_ARG, "flux_eval_loss: img_in takes %d channels, x1 has %d: cond [B, N, %d] is required", in_ch, out_ch, in_ch - out_ch);
  if ((uintptr_t)loss & 3) FAIL(VC_ERR_ARG, "flux_eval_loss: loss must be 4-byte aligned");
  for (int b = 0; b < B; ++b) {
    if (!(t[b] - t[b] == 0.0f)) FAIL(VC_ERR_ARG, "flux_eval_loss: t[%d] is not finite", b);
    if (f.n_img[b] <= 0) FAIL(VC_ERR_ARG, "flux_eval_loss: sample %d has no valid image row (kv_len <= T): it has no loss", b);
  }
  if (!x0 && (uint64_t)B * N * out_ch - 1 > UINT64_MAX - offset) FAIL(VC_ERR_ARG, "flux_eval_loss: offset + B * N * out_channels wraps the 64-bit stream position");
  TRY(monitor_fits(f, "flux_eval_loss", e.buf, e.len));
  // the times: t as the plan takes it - rounded to bf16 for a bf16 x1 (transport.py:129: t.to(x1[0])) - and the model's 1 - t in that dtype
  TRY(stage_begin(f, 2 * (B * sizeof(float) + 256), e.buf, e.len));
  float* tp = stage_take<float>(f, B);
  float* ts = stage_take<float>(f, B);
  auto as_x1 = [&](float v) {   // a value of a tensor of x1's dtype: bf16 rounds to nearest even, as torch's .to(bfloat16)
    if (x1_is_f32) return v;
    uint32_t u;
    memcpy(&u, &v, 4);
    u = (u + 0x7fffu + ((u >> 16) & 1u)) & 0xffff0000u;
    memcpy(&v, &u, 4);
    return v;
  };
  for (int b = 0; b < B; ++b) {
    tp[b] = as_x1(t[b]);
    ts[b] = as_x1(1.0f - tp[b]);      // timesteps = 1 - t, a tensor of t's dtype
  }
  TRY(stage_send(f, f.FM_T, tp, B * sizeof(float), s, e.buf, e.len));
  TRY(stage_send(f, f.TS, ts, B * sizeof(float), s, e.buf, e.len));
  TRY(stage_end(f, s, e.buf, e.len));
  TRY(vc_fm_plan_launch(x1, x1_is_f32, (int64_t)N * out_ch, out_ch, f.FM_T, x0, seed, offset, f.XIN, in_ch, f.FM_U, B, N, out_ch, s, e.buf, e.len));
  HIP(hipMemcpy2DAsync(f.XIN + out_ch, (size_t)in_ch * 2, cond, (size_t)(in_ch - out_ch) * 2, (size_t)(in_ch - out_ch) * 2, (size_t)B * N,
                       hipMemcpyDeviceToDevice, s), "hipMemcpy2DAsync");
  TRY(time_precompute(f, 1, !x1_is_f32, s, e.buf, e.len));
  f.steps_total = f.steps_done = 0;   // MOD now holds this evaluation's rows, not a trajectory's
  if (f.mon_level) {      // row 0 of a zeroed log, as vc_flux_forward
    TRY(vc_zero_fill_launch(f.mon_log, vcmon::log_bytes(f.mon_cap, f.mon_sites(), f.B), s, e.buf, e.len));
    f.mon_evals = 1;
  }
  TRY(forward_rows(f, f.XIN, f.V, s, e));
  return vc_fm_loss_launch(f.V, out_ch, f.FM_U, f.n_img.data(), 1, loss, f.FM_PART, B, N, out_ch, s, e.buf, e.len);
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
  int rc = step_eval(f, s, e);                                        // warm: caches and clocks as inside a trajectory
  f.prof_recs.clear();
  f.prof_used = 0;
  f.prof_on = true;
  for (int i = 0; i < evaluations && rc == VC_OK; ++i) rc = step_eval(f, s, e);
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
