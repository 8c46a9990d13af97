// C ABI of libvcloze_hip.so (declared in include/vcloze_hip.h): argument checks, per-thread error string,
// stream / hipGraph / event helpers.  No torch types cross this boundary.
#include "vcloze_internal.h"
#include "flux_rules.h"
#include <string.h>

static thread_local char g_err[512] = "";
#define ERRBUF g_err, (int)sizeof(g_err)
static inline hipStream_t S(void* s) { return (hipStream_t)s; }
static int hip_fail(const char* what, hipError_t e) {
  snprintf(g_err, sizeof(g_err), "%s: %s", what, hipGetErrorString(e));
  return VC_ERR_HIP;
}

extern "C" {

int vc_abi_version(void) { return VC_ABI_VERSION; }
const char* vc_last_error(void) { return g_err; }
void vc_struct_sizes(int32_t out[7]) {
  out[0] = (int32_t)sizeof(VcGemmProblem); out[1] = (int32_t)sizeof(VcGemmArgs); out[2] = (int32_t)sizeof(VcLnStream);
  out[3] = (int32_t)sizeof(VcAttention); out[4] = (int32_t)sizeof(VcFluxConfig); out[5] = (int32_t)sizeof(VcFluxInputs);
  out[6] = (int32_t)sizeof(VcFluxLaunchClass);
}

int vc_device_count(void) {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) { hip_fail("hipGetDeviceCount", e); return 0; }
  return n;
}
int vc_device_info(int dev, char* name, int namelen, int* cu_count, int64_t* hbm_bytes) {
  hipDeviceProp_t p;
  hipError_t e = hipGetDeviceProperties(&p, dev);
  if (e != hipSuccess) return hip_fail("hipGetDeviceProperties", e);
  if (name && namelen > 0) { strncpy(name, p.gcnArchName, namelen - 1); name[namelen - 1] = 0; }
  if (cu_count) *cu_count = p.multiProcessorCount;
  if (hbm_bytes) *hbm_bytes = (int64_t)p.totalGlobalMem;
  return VC_OK;
}

int vc_gemm(const VcGemmArgs* args, int tile_cfg, void* stream) {
  if (!args) { snprintf(g_err, sizeof(g_err), "gemm: null args"); return VC_ERR_ARG; }
  return vc_gemm_launch(*args, tile_cfg, S(stream), ERRBUF);
}
int vc_gemm_plan(const VcGemmArgs* args, int tile_cfg, int32_t out[8]) {
  if (!args || !out) { snprintf(g_err, sizeof(g_err), "gemm_plan: null argument"); return VC_ERR_ARG; }
  return vc_gemm_plan_impl(*args, tile_cfg, out, ERRBUF);
}
int vc_ln_modulate(const void* x, int64_t ldx, void* y, int64_t ldy, const void* shift, const void* scale,
                   int64_t mod_bstride, int32_t rows, int32_t D, int32_t rows_per_batch, const int32_t* step_ptr,
                   int64_t mod_step_stride, void* stream) {
  return vc_ln_modulate_launch(x, ldx, y, ldy, shift, scale, mod_bstride, rows, D, rows_per_batch, step_ptr,
                               mod_step_stride, S(stream), ERRBUF);
}
int vc_ln_modulate2(const VcLnStream* a, const VcLnStream* b, int64_t mod_bstride, int32_t D, const int32_t* step_ptr,
                    int64_t mod_step_stride, void* stream) {
  return vc_ln_modulate2_launch(a, b, mod_bstride, D, step_ptr, mod_step_stride, S(stream), ERRBUF);
}
int vc_qknorm_rope_vt(void* qkv, int64_t ld, int64_t bstride, const void* q_scale, const void* k_scale,
                      const void* q_scale2, const void* k_scale2, int32_t split, const float* rope,
                      int64_t rope_bstride, void* vt, int32_t B, int32_t L, int32_t Lpad, int32_t H, int32_t parts, void* stream) {
  return vc_qknorm_rope_vt_launch(qkv, ld, bstride, q_scale, k_scale, q_scale2, k_scale2, split, rope, rope_bstride, vt, B, L, Lpad, H,
                                  parts, S(stream), ERRBUF);
}
int vc_attention(const VcAttention* a, void* stream) {
  if (!a) { snprintf(g_err, sizeof(g_err), "attention: null args"); return VC_ERR_ARG; }
  return vc_attention_launch(*a, S(stream), ERRBUF);
}
int vc_attention_plan(const VcAttention* a, int32_t n_cu, int32_t out[16]) {
  if (!a || !out) { snprintf(g_err, sizeof(g_err), "attention_plan: null argument"); return VC_ERR_ARG; }
  return vcplan::attention_plan_words(*a, n_cu > 0 ? n_cu : vc_cu_count(), out, ERRBUF);
}
int64_t vc_attention_scratch_bytes(void) { return vcplan::attention_scratch_bytes(vc_cu_count()); }
int vc_timestep_embedding(const float* t, const float* freqs, void* out_bf16, int32_t n, int32_t half,
                          int32_t round_t_bf16, void* stream) {
  return vc_temb_launch(t, freqs, out_bf16, n, half, round_t_bf16, S(stream), ERRBUF);
}
int vc_silu(const void* x, void* y, int64_t n, void* stream) { return vc_silu_launch(x, y, n, S(stream), ERRBUF); }
int vc_act2d(const void* x, int64_t ldx, void* y, int64_t ldy, int32_t rows, int32_t cols, int32_t act, void* stream) {
  return vc_act2d_launch(x, ldx, y, ldy, rows, cols, act, S(stream), ERRBUF);
}
int vc_gate_residual(const void* y, int64_t ldy, const void* res, int64_t ldres, const void* gate, void* out, int64_t ldo,
                     int32_t rows, int32_t cols, const int32_t* step_ptr, int64_t gate_step_stride, void* stream) {
  return vc_gate_residual_launch(y, ldy, res, ldres, gate, out, ldo, rows, cols, step_ptr, gate_step_stride, S(stream), ERRBUF);
}
int vc_add3(const void* a, const void* b, const void* c, void* y, int64_t n, int64_t bn, int64_t cn, void* stream) {
  return vc_add3_launch(a, b, c, y, n, bn, cn, S(stream), ERRBUF);
}
int vc_copy(void* dst, const void* src, int64_t bytes, void* stream) {
  if (!dst || !src || bytes <= 0) { snprintf(g_err, sizeof(g_err), "copy: bad args"); return VC_ERR_ARG; }
  hipError_t e = hipMemcpyAsync(dst, src, (size_t)bytes, hipMemcpyDeviceToDevice, S(stream));
  return e == hipSuccess ? VC_OK : hip_fail("hipMemcpyAsync", e);
}
int vc_concat_cols(const void* x, int32_t cx, const void* cond, int32_t cc, void* out, int64_t rows, void* stream) {
  return vc_concat_cols_launch(x, cx, cond, cc, out, rows, S(stream), ERRBUF);
}
int vc_euler_step(void* x, const void* v, const float* dts, const int32_t* step_ptr, int64_t n, void* stream) {
  return vc_euler_launch(x, v, dts, step_ptr, n, S(stream), ERRBUF);
}
int vc_euler_step_f32(float* x32, void* shadow, const void* v, const float* dts, const int32_t* step_ptr, int64_t n, void* stream) {
  return vc_euler_f32_launch(x32, shadow, v, dts, step_ptr, n, S(stream), ERRBUF);
}
int vc_solver_evals(int method) {
  if (vc_evals_of(method)) return vc_evals_of(method);
  snprintf(g_err, sizeof(g_err), "solver_evals: unknown method %d (VC_SOLVER_EULER, VC_SOLVER_MIDPOINT, VC_SOLVER_RK4)", method);
  return VC_ERR_ARG;
}
int vc_ode_stage(int32_t method, int32_t stage, void* y, int32_t state_is_bf16, const void* v, void* k, void* y_in,
                 const float* dts, const int32_t* eval_ptr, int64_t n, void* stream) {
  return vc_ode_stage_launch(method, stage, y, state_is_bf16, v, k, y_in, dts, eval_ptr, n, S(stream), ERRBUF);
}
// vc_dopri5_*: the rk launchers at VC_RK_DOPRI5, under their own names in the messages
int vc_dopri5_stage(int32_t stage, const float* y0, void* k, const void* v, const float* dt_ptr, const int32_t* eval_ptr, float* y_stage,
                    void* y_in, int64_t n, void* stream) {
  return vc_rk_stage_launch(VC_RK_DOPRI5, stage, y0, k, v, dt_ptr, eval_ptr, y_stage, y_in, n, S(stream), ERRBUF, "dopri5_stage");
}
int vc_dopri5_error_ratio(int32_t mode, const float* y0, const float* y1, const void* k, const float* dt_ptr, float rtol, float atol,
                          float* out, float* scratch, int64_t n, void* stream) {
  return vc_rk_error_ratio_launch(VC_RK_DOPRI5, mode, y0, y1, k, dt_ptr, rtol, atol, out, scratch, n, S(stream), ERRBUF, "dopri5_error_ratio");
}
int vc_dopri5_interp(const float* y0, const float* y1, const void* k, const float* dt_ptr, float theta, void* out, int32_t out_is_bf16,
                     int64_t n, void* stream) {
  return vc_rk_dense_launch(VC_RK_DOPRI5, y0, y1, k, dt_ptr, theta, out, out_is_bf16, n, S(stream), ERRBUF, "dopri5_interp");
}
int vc_rk_evals(int32_t method, int32_t* start, int32_t* per_attempt, int32_t* order) {
  const int S = vc_rk_stages_of(method);
  if (!S) {
    snprintf(g_err, sizeof(g_err), "rk_evals: unknown method %d (VC_RK_DOPRI5, VC_RK_BOSH3, VC_RK_ADAPTIVE_HEUN)", method);
    return VC_ERR_ARG;
  }
  if (start) *start = 2;
  if (per_attempt) *per_attempt = vcrules::rk_evals_per_attempt(method);
  if (order) *order = vcrules::rk_order(method);
  return VC_OK;
}
int vc_rk_stage(int32_t method, int32_t stage, const float* y0, void* k, const void* v, const float* dt_ptr, const int32_t* eval_ptr,
                float* y_stage, void* y_in, int64_t n, void* stream) {
  return vc_rk_stage_launch(method, stage, y0, k, v, dt_ptr, eval_ptr, y_stage, y_in, n, S(stream), ERRBUF);
}
int vc_rk_error_ratio(int32_t method, int32_t mode, const float* y0, const float* y1, const void* k, const float* dt_ptr, float rtol,
                      float atol, float* out, float* scratch, int64_t n, void* stream) {
  return vc_rk_error_ratio_launch(method, mode, y0, y1, k, dt_ptr, rtol, atol, out, scratch, n, S(stream), ERRBUF);
}
int vc_rk_interp(int32_t method, const float* y0, const float* y1, const void* k, const float* dt_ptr, float theta, void* out,
                 int32_t out_is_bf16, int64_t n, void* stream) {
  return vc_rk_interp_launch(method, y0, y1, k, dt_ptr, theta, out, out_is_bf16, n, S(stream), ERRBUF);
}
int vc_sde_plan(const char* method, const char* form, double norm, const char* last_step, double last_step_size, const float* t_grid,
                int32_t n_points, float* rows, float* times, int32_t capacity, int32_t* n_evals, int32_t* n_draws) {
  return vc_sde_plan_impl(method, form, norm, last_step, last_step_size, t_grid, n_points, rows, times, capacity, n_evals, n_draws, ERRBUF);
}
int vc_ms_plan(int32_t order, const float* t_grid, int32_t n_points, float* rows, float* times, int32_t capacity, int32_t* n_evals) {
  return vc_ms_plan_impl(order, t_grid, n_points, rows, times, capacity, n_evals, ERRBUF);
}
int vc_ms_stage(int32_t eval, const float* table, int32_t n_rows, float* y, const void* v, void* hist, void* y_in, const int32_t* eval_ptr,
                int64_t n, void* stream) {
  return vc_ms_stage_launch(eval, table, n_rows, y, v, hist, y_in, eval_ptr, n, S(stream), ERRBUF);
}
int vc_sde_stage(int32_t eval, const float* table, int32_t n_rows, float* y, const void* v, void* y_in, float* xhat, float* k1,
                 const uint64_t* rng, const int32_t* eval_ptr, int64_t n, void* stream) {
  return vc_sde_stage_launch(eval, table, n_rows, y, v, y_in, xhat, k1, rng, eval_ptr, n, S(stream), ERRBUF);
}
int vc_cfg_combine(const void* cond, const void* uncond, void* out, int64_t n, float cfg_scale, void* stream) {
  return vc_cfg_combine_launch(cond, uncond, out, n, cfg_scale, S(stream), ERRBUF);
}
int vc_step_advance(int32_t* step_ptr, void* stream) { return vc_step_advance_launch(step_ptr, S(stream), ERRBUF); }
int vc_residual_change(const void* h0, const void* h1, const void* p, void* r, float* sums, float* metric, float* scratch, int32_t B,
                       int64_t n, void* stream) {
  return vc_residual_change_launch(h0, h1, p, r, sums, metric, scratch, B, n, S(stream), ERRBUF);
}
int vc_residual_sub(const void* a, int64_t a_bstride, const void* b, int64_t b_bstride, void* out, int64_t out_bstride, int32_t B,
                    int64_t n, void* stream) {
  return vc_residual_op_launch(0, a, a_bstride, b, b_bstride, out, out_bstride, B, n, S(stream), ERRBUF);
}
int vc_residual_add(const void* a, int64_t a_bstride, const void* b, int64_t b_bstride, void* out, int64_t out_bstride, int32_t B,
                    int64_t n, void* stream) {
  return vc_residual_op_launch(1, a, a_bstride, b, b_bstride, out, out_bstride, B, n, S(stream), ERRBUF);
}
void vc_monitor_struct_sizes(int32_t out[1]) { out[0] = (int32_t)sizeof(VcStat); }
int vc_fm_plan(const void* x1, int32_t x1_is_f32, int64_t x1_bstride, int64_t x1_ld, const float* t, const void* x0, uint64_t seed, uint64_t offset,
               void* xt, int64_t xt_ld, float* ut, int32_t B, int64_t rows, int32_t cols, void* stream) {
  return vc_fm_plan_launch(x1, x1_is_f32, x1_bstride, x1_ld, t, x0, seed, offset, xt, xt_ld, ut, B, rows, cols, S(stream), ERRBUF);
}
int vc_fm_loss(const void* out, int64_t out_ld, const float* ut, const int32_t* valid_rows, int32_t valid_on_host, float* loss, float* scratch,
               int32_t B, int64_t rows, int32_t cols, void* stream) {
  return vc_fm_loss_launch(out, out_ld, ut, valid_rows, valid_on_host, loss, scratch, B, rows, cols, S(stream), ERRBUF);
}
int vc_fm_times(const char* snr_type, const float* base, int32_t n, int32_t n_tokens, int32_t do_shift, float* out) {
  return vc_fm_times_impl(snr_type, base, n, n_tokens, do_shift, out, ERRBUF);
}
int vc_tensor_stats(const void* x, int32_t x_is_f32, int64_t bstride, int64_t ld, int32_t B, int64_t rows, int32_t cols, VcStat* out,
                    int64_t out_stride, const int32_t* row_ptr, int32_t capacity, float* scratch, void* stream) {
  return vc_tensor_stats_launch(x, x_is_f32, bstride, ld, B, rows, cols, out, out_stride, row_ptr, capacity, scratch, S(stream), ERRBUF);
}

int vc_sdedit_mix(const void* noise, const void* latent, double strength, void* out, int64_t n, void* stream) {
  return vc_sdedit_mix_launch(noise, latent, strength, out, n, S(stream), ERRBUF);
}
int vc_im2col3x3(const void* src, void* dst, int32_t H, int32_t W, int32_t C, int32_t up, void* stream) {
  return vc_im2col3x3_launch(src, dst, H, W, C, up, S(stream), ERRBUF);
}
int vc_groupnorm(const void* x, const void* gamma, const void* beta, void* y, void* scratch, int64_t scratch_bytes,
                 int64_t HW, int32_t C, int32_t G, float eps, int32_t swish, void* stream) {
  return vc_groupnorm_launch(x, gamma, beta, y, scratch, scratch_bytes, HW, C, G, eps, swish, S(stream), ERRBUF);
}
int vc_softmax_rows(void* x, int64_t ld, int32_t rows, int32_t cols, float scale, const void* bias, int64_t ld_bias,
                    int32_t causal_period, void* stream) {
  return vc_softmax_rows_launch(x, ld, rows, cols, scale, bias, ld_bias, causal_period, S(stream), ERRBUF);
}
int vc_embedding(const int32_t* ids, const void* table, int64_t ld_table, int32_t vocab, void* out, int32_t L, int32_t D, void* stream) {
  return vc_embedding_launch(ids, table, ld_table, vocab, out, L, D, S(stream), ERRBUF);
}
int vc_rmsnorm(const void* x, const void* weight, void* y, int32_t rows, int32_t D, float eps, void* stream) {
  return vc_rownorm_launch(x, weight, nullptr, y, rows, D, eps, 0, S(stream), ERRBUF);
}
int vc_layernorm(const void* x, const void* weight, const void* bias, void* y, int32_t rows, int32_t D, float eps, void* stream) {
  return vc_rownorm_launch(x, weight, bias, y, rows, D, eps, 1, S(stream), ERRBUF);
}
int vc_mul(const void* a, const void* b, void* y, int64_t n, void* stream) { return vc_ewise_launch(a, b, y, n, 0, S(stream), ERRBUF); }
int vc_add(const void* a, const void* b, void* y, int64_t n, void* stream) { return vc_ewise_launch(a, b, y, n, 1, S(stream), ERRBUF); }
int vc_quick_gelu(const void* x, void* y, int64_t n, void* stream) { return vc_ewise_launch(x, nullptr, y, n, 2, S(stream), ERRBUF); }
int vc_t5_relative_buckets(int32_t L, int32_t num_buckets, int32_t max_distance, int32_t* out) {
  return vc_t5_relative_buckets_impl(L, num_buckets, max_distance, out, ERRBUF);
}
int vc_t5_position_bias(const void* table, int64_t ld, int32_t H, int32_t L, int32_t num_buckets, int32_t max_distance, void* out, void* stream) {
  return vc_t5_position_bias_launch(table, ld, H, L, num_buckets, max_distance, out, S(stream), ERRBUF);
}
int vc_clip_embed(const int32_t* ids, const void* tok, int64_t ld_tok, int32_t vocab, const void* pos, int64_t ld_pos, void* out, int32_t L,
                  int32_t Lp, int32_t D, void* stream) {
  return vc_clip_embed_launch(ids, tok, ld_tok, vocab, pos, ld_pos, out, L, Lp, D, S(stream), ERRBUF);
}
int vc_clip_pool(const int32_t* ids, const void* hidden, int64_t ld, int32_t L, int32_t D, int32_t eos_token_id, void* pooled, void* stream) {
  return vc_clip_pool_launch(ids, hidden, ld, L, D, eos_token_id, pooled, S(stream), ERRBUF);
}
int vc_transpose(const void* src, int64_t ld_src, void* dst, int64_t ld_dst, int32_t rows, int32_t cols, void* stream) {
  return vc_transpose_launch(src, ld_src, dst, ld_dst, rows, cols, S(stream), ERRBUF);
}
int vc_nchw_to_nhwc(const void* src, int32_t src_is_f32, void* dst, int32_t C, int32_t Cp, int64_t HW, float div, float add, void* stream) {
  return vc_nchw_to_nhwc_launch(src, src_is_f32, dst, C, Cp, HW, div, add, S(stream), ERRBUF);
}
int vc_nhwc_to_nchw(const void* src, void* dst, int32_t dst_is_f32, int32_t C, int32_t Cp, int64_t HW, void* stream) {
  return vc_nhwc_to_nchw_launch(src, dst, dst_is_f32, C, Cp, HW, S(stream), ERRBUF);
}
int vc_gaussian_sample(const void* moments, int32_t Cp, const void* noise, void* out, int32_t Z, int64_t HW, float scale, float shift, void* stream) {
  return vc_gaussian_sample_launch(moments, Cp, noise, out, Z, HW, scale, shift, S(stream), ERRBUF);
}
int vc_conv3x3(const void* x, const void* w, const void* bias, void* out, int64_t ldc, const void* res, int64_t ldres,
               const void* gate, int32_t H, int32_t W, int32_t C, int32_t O, int32_t mode, void* stream) {
  return vc_conv3x3_launch(x, w, bias, out, ldc, res, ldres, gate, H, W, C, O, mode, S(stream), ERRBUF);
}
int vc_pack_latent(const void* latent, void* tokens, int32_t C, int32_t h, int32_t w, int64_t ld, int32_t col0, void* stream) {
  return vc_pack_latent_launch(latent, tokens, C, h, w, ld, col0, S(stream), ERRBUF);
}
int vc_pack_mask(const void* mask, void* tokens, int32_t H, int32_t W, int64_t ld, int32_t col0, void* stream) {
  return vc_pack_mask_launch(mask, tokens, H, W, ld, col0, S(stream), ERRBUF);
}
int vc_unpack_latent(const void* tokens, int64_t ld, int32_t col0, void* latent, int32_t C, int32_t h, int32_t w, void* stream) {
  return vc_unpack_latent_launch(tokens, ld, col0, latent, C, h, w, S(stream), ERRBUF);
}
int vc_lora_merge(const void* w, int32_t w_is_f32, int64_t ldw, const void* lora_a, int64_t lda, const void* lora_b, int64_t ldb,
                  float scale, void* out, int64_t ldo, const void* bias, int32_t bias_is_f32, const void* lora_b_bias, void* bias_out,
                  int32_t out_features, int32_t in_features, int32_t rank, void* stream) {
  return vc_lora_merge_launch(w, w_is_f32, ldw, lora_a, lda, lora_b, ldb, scale, out, ldo, bias, bias_is_f32, lora_b_bias, bias_out,
                              out_features, in_features, rank, S(stream), ERRBUF);
}
int vc_lora_merge_qkv(const void* w, int32_t w_is_f32, int64_t ldw, const void* lora_a, int64_t lda, const void* lora_b, int64_t ldb,
                      float scale, void* out, int64_t ldo, const void* bias, int32_t bias_is_f32, const void* lora_b_bias, void* bias_out,
                      int32_t out_features, int32_t in_features, int32_t rank, int32_t qkv_heads, void* stream) {
  return vc_lora_merge_qkv_launch(w, w_is_f32, ldw, lora_a, lda, lora_b, ldb, scale, out, ldo, bias, bias_is_f32, lora_b_bias, bias_out,
                                  out_features, in_features, rank, qkv_heads, S(stream), ERRBUF);
}
int vc_randn(void* out, int32_t dtype, int64_t n, uint64_t seed, uint64_t offset, void* stream) {
  return vc_randn_launch(out, dtype, n, seed, offset, S(stream), ERRBUF);
}
int vc_randn_tokens(void* tokens, int32_t C, int32_t h, int32_t w, int64_t ld, int32_t col0, uint64_t seed, uint64_t offset, void* stream) {
  return vc_randn_tokens_launch(tokens, C, h, w, ld, col0, seed, offset, S(stream), ERRBUF);
}
int vc_torch_randn_policy(int64_t n, int32_t sm_count, int32_t threads_per_sm, int32_t* grid, uint64_t* offset_advance) {
  return vc_torch_randn_policy_impl(n, sm_count, threads_per_sm, grid, offset_advance, ERRBUF);
}
int vc_randn_torch(void* out, int32_t dtype, int64_t n, uint64_t seed, uint64_t philox_offset, int32_t sm_count, int32_t threads_per_sm,
                   void* stream) {
  return vc_randn_torch_launch(out, dtype, n, seed, philox_offset, sm_count, threads_per_sm, S(stream), ERRBUF);
}
int vc_randn_torch_tokens(void* tokens, int32_t C, int32_t h, int32_t w, int64_t ld, int32_t col0, uint64_t seed, uint64_t philox_offset,
                          int32_t sm_count, int32_t threads_per_sm, void* stream) {
  return vc_randn_torch_tokens_launch(tokens, C, h, w, ld, col0, seed, philox_offset, sm_count, threads_per_sm, S(stream), ERRBUF);
}

/* ---- handle API (flux_engine.hip) ---- */
int vc_flux_create(const VcFluxConfig* cfg, void** handle) { return vc_flux_create_impl(cfg, handle, ERRBUF); }
int vc_flux_destroy(void* handle) { return vc_flux_destroy_impl(handle, ERRBUF); }
int vc_flux_bind_weight(void* handle, const char* name, const void* w, const void* bias, int32_t rows, int32_t cols, int64_t ldw) {
  return vc_flux_bind_weight_impl(handle, name, w, bias, rows, cols, ldw, ERRBUF);
}
int vc_flux_bind_lora(void* handle, const char* name, const void* lora_a, int64_t lda, const void* lora_b, int64_t ldb,
                      const void* lora_b_bias, int32_t out_features, int32_t in_features, int32_t rank) {
  return vc_flux_bind_lora_impl(handle, name, lora_a, lda, lora_b, ldb, lora_b_bias, out_features, in_features, rank, ERRBUF);
}
int vc_flux_load_key(void* handle, int32_t index, char* name, int32_t namelen, int64_t* shape, int32_t* ndim) {
  return vc_flux_load_key_impl(handle, index, name, namelen, shape, ndim, ERRBUF);
}
int vc_flux_load_tensor(void* handle, const char* key, const void* ptr, int32_t is_f32, const int64_t* shape, int32_t ndim) {
  return vc_flux_load_tensor_impl(handle, key, ptr, is_f32, shape, ndim, ERRBUF);
}
int64_t vc_flux_load_bytes(void* handle) { return vc_flux_load_bytes_impl(handle); }
int vc_flux_load_finish(void* handle, float lora_scale, void* arena, int64_t arena_bytes, void* stream) {
  return vc_flux_load_finish_impl(handle, lora_scale, arena, arena_bytes, S(stream), ERRBUF);
}
int vc_flux_bound(void* handle, const char* name, const void** w, const void** bias, int32_t* rows, int32_t* cols, int64_t* ldw) {
  return vc_flux_bound_impl(handle, name, w, bias, rows, cols, ldw, ERRBUF);
}
int vc_flux_set_lora_scale(void* handle, float scale) { return vc_flux_set_lora_scale_impl(handle, scale, ERRBUF); }
int vc_flux_set_tap(void* handle, const char* name, void* dst) { return vc_flux_set_tap_impl(handle, name, dst, ERRBUF); }
int vc_flux_tap_shape(void* handle, const char* name, int64_t* rows, int32_t* cols) {
  return vc_flux_tap_shape_impl(handle, name, rows, cols, ERRBUF);
}
int64_t vc_flux_mod_offset(void* handle, const char* module_name) { return vc_flux_mod_offset_impl(handle, module_name); }
int vc_flux_set_option(void* handle, const char* name, int32_t value) { return vc_flux_set_option_impl(handle, name, value, ERRBUF); }
int64_t vc_flux_workspace_bytes(void* handle, int32_t B, int32_t T, int32_t N, int32_t max_steps) {
  return vc_flux_workspace_bytes_impl(handle, B, T, N, max_steps);
}
int vc_flux_prepare(void* handle, const VcFluxInputs* in, void* workspace, int64_t workspace_bytes, void* stream) {
  return vc_flux_prepare_impl(handle, in, workspace, workspace_bytes, S(stream), ERRBUF);
}
int vc_flux_forward(void* handle, const void* img, const float* timesteps, int32_t timesteps_is_bf16, void* out, void* stream) {
  return vc_flux_forward_impl(handle, img, timesteps, timesteps_is_bf16, out, S(stream), ERRBUF);
}
int vc_flux_eval_loss(void* handle, const void* x1, int32_t x1_is_f32, const void* cond, const float* t, const void* x0, uint64_t seed,
                      uint64_t offset, float* loss, void* stream) {
  return vc_flux_eval_loss_impl(handle, x1, x1_is_f32, cond, t, x0, seed, offset, loss, S(stream), ERRBUF);
}
int vc_flux_sample_begin(void* handle, const void* x, const void* cond, const float* t_grid, int32_t n_points, int32_t state_is_bf16,
                         void* stream) {
  return vc_flux_sample_begin_impl(handle, VC_SOLVER_EULER, x, cond, t_grid, n_points, state_is_bf16, S(stream), ERRBUF);
}
int vc_flux_sample_begin_ode(void* handle, int32_t method, const void* x, const void* cond, const float* t_grid, int32_t n_points,
                             int32_t state_is_bf16, void* stream) {
  return vc_flux_sample_begin_impl(handle, method, x, cond, t_grid, n_points, state_is_bf16, S(stream), ERRBUF);
}
int vc_flux_sample_steps(void* handle, int32_t n_steps, void* trajectory, void* stream) {
  return vc_flux_sample_steps_impl(handle, n_steps, trajectory, S(stream), ERRBUF);
}
int vc_flux_profile(void* handle, int32_t evaluations, VcFluxLaunchClass* out, int32_t capacity, int32_t* count, void* stream) {
  return vc_flux_profile_impl(handle, evaluations, out, capacity, count, S(stream), ERRBUF);
}
int vc_flux_sample_end(void* handle, void* x_out, void* stream) { return vc_flux_sample_end_impl(handle, x_out, S(stream), ERRBUF); }
int vc_flux_set_step_cache(void* handle, float threshold, int32_t max_consecutive) {
  return vc_flux_set_step_cache_impl(handle, threshold, max_consecutive, ERRBUF);
}
int vc_flux_set_cfg(void* handle, int32_t on, float cfg_scale) { return vc_flux_set_cfg_impl(handle, on, cfg_scale, ERRBUF); }
int vc_flux_step_cache_stats(void* handle, int32_t* computed, int32_t* reused, float* metrics, int32_t capacity) {
  return vc_flux_step_cache_stats_impl(handle, computed, reused, metrics, capacity, ERRBUF);
}
int vc_flux_sample_ode(void* handle, int32_t method, void* x, const void* cond, const float* t_grid, int32_t n_points,
                       int32_t state_is_bf16, void* trajectory, void* stream) {
  int rc = vc_flux_sample_begin_impl(handle, method, x, cond, t_grid, n_points, state_is_bf16, S(stream), ERRBUF);
  if (rc == VC_OK) rc = vc_flux_sample_steps_impl(handle, n_points - 1, trajectory, S(stream), ERRBUF);
  if (rc == VC_OK) rc = vc_flux_sample_end_impl(handle, x, S(stream), ERRBUF);
  return rc;
}
int vc_flux_sample_dopri5(void* handle, void* x, const void* cond, const float* t_grid, int32_t n_points, int32_t state_is_bf16,
                          float rtol, float atol, int32_t max_attempts, void* trajectory, void* stream) {
  return vc_flux_sample_dopri5_impl(handle, x, cond, t_grid, n_points, state_is_bf16, rtol, atol, max_attempts, trajectory, S(stream), ERRBUF);
}
int vc_flux_dopri5_log(void* handle, double* t, double* dt, float* ratio, int32_t* accepted, int32_t capacity, int32_t* attempts,
                       int32_t* evaluations) {
  return vc_flux_dopri5_log_impl(handle, t, dt, ratio, accepted, capacity, attempts, evaluations, ERRBUF);
}
int vc_flux_sample_rk(void* handle, int32_t method, void* x, const void* cond, const float* t_grid, int32_t n_points, int32_t state_is_bf16,
                      float rtol, float atol, int32_t max_attempts, void* trajectory, void* stream) {
  return vc_flux_sample_rk_impl(handle, method, x, cond, t_grid, n_points, state_is_bf16, rtol, atol, max_attempts, trajectory, S(stream), ERRBUF);
}
int vc_flux_rk_log(void* handle, double* t, double* dt, float* ratio, int32_t* accepted, int32_t capacity, int32_t* attempts,
                   int32_t* evaluations) {      // one log serves both adaptive entry points: the last solve's
  return vc_flux_dopri5_log_impl(handle, t, dt, ratio, accepted, capacity, attempts, evaluations, ERRBUF);
}
int vc_flux_sample_multistep(void* handle, int32_t order, void* x, const void* cond, const float* t_grid, int32_t n_points,
                             int32_t state_is_bf16, void* trajectory, void* stream) {
  return vc_flux_sample_multistep_impl(handle, order, x, cond, t_grid, n_points, state_is_bf16, trajectory, S(stream), ERRBUF);
}
int vc_flux_plan_count(void* handle) { return vc_flux_plan_count_impl(handle); }
int vc_flux_sample_sde(void* handle, const char* method, void* x, const void* cond, const float* t_grid, int32_t n_points, const char* form,
                       double norm, const char* last_step, double last_step_size, uint64_t seed, uint64_t offset, int32_t state_is_bf16,
                       void* trajectory, void* stream) {
  return vc_flux_sample_sde_impl(handle, method, x, cond, t_grid, n_points, form, norm, last_step, last_step_size, seed, offset, state_is_bf16,
                                 trajectory, S(stream), ERRBUF);
}
int vc_flux_sample_euler(void* handle, void* x, const void* cond, const float* t_grid, int32_t n_points, int32_t state_is_bf16,
                         void* trajectory, void* stream) {
  return vc_flux_sample_ode(handle, VC_SOLVER_EULER, x, cond, t_grid, n_points, state_is_bf16, trajectory, stream);
}
int vc_flux_step_nodes(void* handle, int32_t nodes[3]) { return vc_flux_step_nodes_impl(handle, nodes, ERRBUF); }
int vc_flux_set_monitor(void* handle, int32_t level, VcStat* log, int32_t capacity_evals, float* scratch) {
  return vc_flux_set_monitor_impl(handle, level, log, capacity_evals, scratch, ERRBUF);
}
int vc_flux_monitor_sites(void* handle, int32_t index, char* name, int32_t namelen) {
  return vc_flux_monitor_sites_impl(handle, index, name, namelen, ERRBUF);
}
int vc_flux_monitor_bytes(void* handle, int32_t capacity_evals, int64_t* log_bytes, int64_t* scratch_bytes) {
  return vc_flux_monitor_bytes_impl(handle, capacity_evals, log_bytes, scratch_bytes, ERRBUF);
}
int vc_flux_monitor_report(void* handle, int32_t* first_bad_eval, int32_t* first_bad_site, int32_t* first_bad_sample, int32_t* evals_logged,
                           void* stream) {
  return vc_flux_monitor_report_impl(handle, first_bad_eval, first_bad_site, first_bad_sample, evals_logged, S(stream), ERRBUF);
}

/* ---- autoencoder handle (vae_engine.hip) ---- */
void vc_vae_struct_sizes(int32_t out[1]) { out[0] = (int32_t)sizeof(VcVaeConfig); }
int vc_vae_create(const VcVaeConfig* cfg, void** handle) { return vc_vae_create_impl(cfg, handle, ERRBUF); }
int vc_vae_destroy(void* handle) { return vc_vae_destroy_impl(handle, ERRBUF); }
int vc_vae_weight_name(void* handle, int32_t index, char* name, int32_t namelen) { return vc_vae_weight_name_impl(handle, index, name, namelen, ERRBUF); }
int vc_vae_bind_weight(void* handle, const char* name, const void* w, const void* bias, int32_t is_f32, const int64_t* shape, int32_t ndim,
                       void* stream) {
  return vc_vae_bind_weight_impl(handle, name, w, bias, is_f32, shape, ndim, S(stream), ERRBUF);
}
int vc_vae_workspace_bytes(void* handle, int32_t H, int32_t W, int32_t which, int64_t* bytes) {
  return vc_vae_workspace_bytes_impl(handle, H, W, which, bytes, ERRBUF);
}
int vc_vae_prepare(void* handle, int32_t H, int32_t W, int32_t which, void* workspace, int64_t workspace_bytes, void* stream) {
  return vc_vae_prepare_impl(handle, H, W, which, workspace, workspace_bytes, S(stream), ERRBUF);
}
int vc_vae_decode(void* handle, const void* latent, int32_t latent_form, int64_t ld, int32_t col0, void* pixels, int32_t pixels_is_f32,
                  void* stream) {
  return vc_vae_decode_impl(handle, latent, latent_form, ld, col0, pixels, pixels_is_f32, S(stream), ERRBUF);
}
int vc_vae_encode(void* handle, const void* pixels, int32_t pixels_is_f32, const void* noise, void* latent, int32_t latent_form,
                  int64_t ld, int32_t col0, void* stream) {
  return vc_vae_encode_impl(handle, pixels, pixels_is_f32, noise, latent, latent_form, ld, col0, S(stream), ERRBUF);
}
int vc_vae_plan_count(void* handle) { return vc_vae_plan_count_impl(handle); }

/* ---- text-encoder handle (text_engine.hip) ---- */
void vc_text_struct_sizes(int32_t out[1]) { out[0] = (int32_t)sizeof(VcTextConfig); }
int vc_text_create(const VcTextConfig* cfg, void** handle) { return vc_text_create_impl(cfg, handle, ERRBUF); }
int vc_text_destroy(void* handle) { return vc_text_destroy_impl(handle, ERRBUF); }
int vc_text_weight_name(void* handle, int32_t index, char* name, int32_t namelen) { return vc_text_weight_name_impl(handle, index, name, namelen, ERRBUF); }
int vc_text_bind_tensor(void* handle, const char* key, const void* ptr, const int64_t* shape, int32_t ndim) {
  return vc_text_bind_tensor_impl(handle, key, ptr, shape, ndim, ERRBUF);
}
int vc_text_workspace_bytes(void* handle, int32_t L, int64_t* bytes) { return vc_text_workspace_bytes_impl(handle, L, bytes, ERRBUF); }
int vc_text_prepare(void* handle, int32_t L, void* workspace, int64_t workspace_bytes, void* stream) {
  return vc_text_prepare_impl(handle, L, workspace, workspace_bytes, S(stream), ERRBUF);
}
int vc_text_encode(void* handle, const int32_t* ids, int32_t n_prompts, void* hidden, void* pooled, void* stream) {
  return vc_text_encode_impl(handle, ids, n_prompts, hidden, pooled, S(stream), ERRBUF);
}
int vc_text_plan_count(void* handle) { return vc_text_plan_count_impl(handle); }

/* ---- the grid: host rules (grid_rules.hip), pixel epilogue (pixels_out.hip), handle (grid_engine.hip) ---- */
int vc_time_grid(int32_t n_points, int32_t n_tokens, double t0, double t1, int32_t do_shift, double time_shifting_factor, float* out) {
  return vc_time_grid_impl(n_points, n_tokens, t0, t1, do_shift, time_shifting_factor, out, ERRBUF);
}
int64_t vc_grid_tokens(int32_t rows, const int32_t* lat_h, const int32_t* lat_w) { return vc_grid_tokens_impl(rows, lat_h, lat_w, ERRBUF); }
int vc_grid_img_ids(int32_t rows, const int32_t* lat_h, const int32_t* lat_w, float* out) {
  return vc_grid_img_ids_impl(rows, lat_h, lat_w, out, ERRBUF);
}
int vc_pixels_out(const void* img, int32_t img_is_f32, int32_t H, int32_t W, int32_t x0, int32_t w, void* out, int32_t out_form,
                  void* stream) {
  return vc_pixels_out_launch(img, img_is_f32, H, W, x0, w, out, out_form, S(stream), ERRBUF);
}
void vc_image_struct_sizes(int32_t out[1]) { out[0] = (int32_t)sizeof(VcImageMetrics); }
int vc_image_compare_scratch_bytes(int32_t C, int32_t H, int32_t W, int64_t* bytes) {
  return vc_image_compare_scratch_bytes_impl(C, H, W, bytes, ERRBUF);
}
int vc_image_compare(const void* a, const void* b, int32_t form, int32_t C, int32_t H, int32_t W, VcImageMetrics* out_dev, void* scratch,
                     int64_t scratch_bytes, void* stream) {
  return vc_image_compare_launch(a, b, form, C, H, W, out_dev, scratch, scratch_bytes, S(stream), ERRBUF);
}
int vc_image_psnr(const VcImageMetrics* m, double* psnr_db) { return vc_image_psnr_impl(m, psnr_db, ERRBUF); }
void vc_grid_struct_sizes(int32_t out[3]) {
  out[0] = (int32_t)sizeof(VcGridConfig); out[1] = (int32_t)sizeof(VcGridJob); out[2] = (int32_t)sizeof(VcGridSdedit);
}
int vc_grid_create(const VcGridConfig* cfg, void** handle) { return vc_grid_create_impl(cfg, handle, ERRBUF); }
int vc_grid_destroy(void* handle) { return vc_grid_destroy_impl(handle, ERRBUF); }
int vc_grid_set_noise(void* handle, int32_t source, int32_t sm_count, int32_t threads_per_sm) {
  return vc_grid_set_noise_impl(handle, source, sm_count, threads_per_sm, ERRBUF);
}
int vc_grid_workspace_bytes(void* handle, const VcGridJob* job, int64_t* bytes) { return vc_grid_workspace_bytes_impl(handle, job, bytes, ERRBUF); }
int vc_grid_sdedit_workspace_bytes(void* handle, const VcGridSdedit* job, int64_t* bytes) {
  return vc_grid_sdedit_workspace_bytes_impl(handle, job, bytes, ERRBUF);
}
int vc_grid_generate(void* handle, const VcGridJob* job, void* workspace, int64_t workspace_bytes, void* const* out_rows, void* stream) {
  return vc_grid_generate_impl(handle, job, workspace, workspace_bytes, out_rows, S(stream), ERRBUF);
}
int vc_grid_sdedit(void* handle, const VcGridSdedit* job, void* workspace, int64_t workspace_bytes, void* const* out_images, void* stream) {
  return vc_grid_sdedit_impl(handle, job, workspace, workspace_bytes, out_images, S(stream), ERRBUF);
}

/* ---- the photo front end: resample.hip, pixels_in.hip, the size rules of grid_rules.hip, two more calls of grid_engine.hip ---- */
int vc_resample_kmax(int32_t in, int32_t out, int32_t filter) { return vc_resample_kmax_impl(in, out, filter, ERRBUF); }
int vc_resample_coeffs(int32_t in, int32_t out, int32_t filter, int32_t* xmin, int32_t* len, int32_t* ki, int32_t kmax) {
  return vc_resample_coeffs_impl(in, out, filter, xmin, len, ki, kmax, ERRBUF);
}
int64_t vc_resample_tmp_bytes(int32_t H, int32_t W, int32_t h, int32_t w, int32_t filter) { return vc_resample_tmp_bytes_impl(H, W, h, w, filter, ERRBUF); }
int vc_resample_u8(const void* src, int32_t H, int32_t W, void* dst, int32_t h, int32_t w, int32_t filter, void* tmp, int64_t tmp_bytes,
                   void* stream) {
  return vc_resample_u8_launch(src, H, W, dst, h, w, filter, tmp, tmp_bytes, S(stream), ERRBUF);
}
int vc_pixels_in(const void* src, int32_t H, int32_t W, int32_t left, int32_t top, void* out, int32_t out_is_f32, int32_t h,
                 int32_t Wrow, int32_t x0, int32_t w, void* stream) {
  return vc_pixels_in_launch(src, H, W, left, top, out, out_is_f32, h, Wrow, x0, w, S(stream), ERRBUF);
}
int vc_mask_fill(void* mask, int32_t h, int32_t Wrow, int32_t x0, int32_t w, int32_t value, void* stream) {
  return vc_mask_fill_launch(mask, h, Wrow, x0, w, value, S(stream), ERRBUF);
}
int vc_fit_size(int32_t w, int32_t h, int32_t resolution, int32_t* nw, int32_t* nh) { return vc_fit_size_impl(w, h, resolution, nw, nh, ERRBUF); }
int vc_grid_layout(int32_t grid_h, int32_t grid_w, const int32_t* cell_w, const int32_t* cell_h, int32_t resolution, VcCellPlan* out) {
  return vc_grid_layout_impl(grid_h, grid_w, cell_w, cell_h, resolution, out, ERRBUF);
}
int vc_upsampling_size(int32_t orig_w, int32_t orig_h, int32_t* w, int32_t* h) { return vc_upsampling_size_impl(orig_w, orig_h, w, h, ERRBUF); }
void vc_photo_struct_sizes(int32_t out[3]) {
  out[0] = (int32_t)sizeof(VcCellPlan); out[1] = (int32_t)sizeof(VcGridPhotos); out[2] = (int32_t)sizeof(VcGridSdeditU8);
}
int vc_grid_photos_workspace_bytes(void* handle, const VcGridPhotos* job, int64_t* bytes) {
  return vc_grid_photos_workspace_bytes_impl(handle, job, bytes, ERRBUF);
}
int vc_grid_sdedit_u8_workspace_bytes(void* handle, const VcGridSdeditU8* job, int64_t* bytes) {
  return vc_grid_sdedit_u8_workspace_bytes_impl(handle, job, bytes, ERRBUF);
}
int vc_grid_generate_photos(void* handle, const VcGridPhotos* job, void* workspace, int64_t workspace_bytes, void* const* out_rows,
                            void* stream) {
  return vc_grid_generate_photos_impl(handle, job, workspace, workspace_bytes, out_rows, S(stream), ERRBUF);
}
int vc_grid_sdedit_u8(void* handle, const VcGridSdeditU8* job, void* workspace, int64_t workspace_bytes, void* const* out_images,
                      void* stream) {
  return vc_grid_sdedit_u8_impl(handle, job, workspace, workspace_bytes, out_images, S(stream), ERRBUF);
}

/* ---- streams / graphs / events ---- */
int vc_stream_create(void** stream) {
  if (!stream) { snprintf(g_err, sizeof(g_err), "stream_create: null"); return VC_ERR_ARG; }
  hipStream_t s;
  hipError_t e = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
  if (e != hipSuccess) return hip_fail("hipStreamCreate", e);
  *stream = (void*)s;
  return VC_OK;
}
int vc_stream_destroy(void* stream) {
  hipError_t e = hipStreamDestroy(S(stream));
  return e == hipSuccess ? VC_OK : hip_fail("hipStreamDestroy", e);
}
int vc_stream_sync(void* stream) {
  hipError_t e = hipStreamSynchronize(S(stream));
  return e == hipSuccess ? VC_OK : hip_fail("hipStreamSynchronize", e);
}
int vc_graph_begin(void* stream) {
  hipError_t e = hipStreamBeginCapture(S(stream), hipStreamCaptureModeThreadLocal);
  return e == hipSuccess ? VC_OK : hip_fail("hipStreamBeginCapture", e);
}
int vc_graph_end(void* stream, void** graph_exec) {
  if (!graph_exec) { snprintf(g_err, sizeof(g_err), "graph_end: null"); return VC_ERR_ARG; }
  hipGraph_t g = nullptr;
  hipError_t e = hipStreamEndCapture(S(stream), &g);
  if (e != hipSuccess) return hip_fail("hipStreamEndCapture", e);
  hipGraphExec_t ge = nullptr;
  e = hipGraphInstantiate(&ge, g, nullptr, nullptr, 0);
  (void)hipGraphDestroy(g);
  if (e != hipSuccess) return hip_fail("hipGraphInstantiate", e);
  *graph_exec = (void*)ge;
  return VC_OK;
}
int vc_graph_launch(void* graph_exec, void* stream) {
  hipError_t e = hipGraphLaunch((hipGraphExec_t)graph_exec, S(stream));
  return e == hipSuccess ? VC_OK : hip_fail("hipGraphLaunch", e);
}
int vc_graph_destroy(void* graph_exec) {
  hipError_t e = hipGraphExecDestroy((hipGraphExec_t)graph_exec);
  return e == hipSuccess ? VC_OK : hip_fail("hipGraphExecDestroy", e);
}
int vc_event_create(void** ev) {
  if (!ev) { snprintf(g_err, sizeof(g_err), "event_create: null"); return VC_ERR_ARG; }
  hipEvent_t e_;
  hipError_t e = hipEventCreate(&e_);
  if (e != hipSuccess) return hip_fail("hipEventCreate", e);
  *ev = (void*)e_;
  return VC_OK;
}
int vc_event_record(void* ev, void* stream) {
  hipError_t e = hipEventRecord((hipEvent_t)ev, S(stream));
  return e == hipSuccess ? VC_OK : hip_fail("hipEventRecord", e);
}
int vc_event_elapsed_ms(void* ev_start, void* ev_stop, float* ms) {
  hipError_t e = hipEventSynchronize((hipEvent_t)ev_stop);
  if (e != hipSuccess) return hip_fail("hipEventSynchronize", e);
  e = hipEventElapsedTime(ms, (hipEvent_t)ev_start, (hipEvent_t)ev_stop);
  return e == hipSuccess ? VC_OK : hip_fail("hipEventElapsedTime", e);
}
int vc_event_destroy(void* ev) {
  hipError_t e = hipEventDestroy((hipEvent_t)ev);
  return e == hipSuccess ? VC_OK : hip_fail("hipEventDestroy", e);
}

}  // extern "C"
