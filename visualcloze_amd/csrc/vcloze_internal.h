// internal launcher declarations shared by the .hip translation units
#pragma once
#include <hip/hip_runtime.h>
#include <stdio.h>
#include "../../include/vcloze_hip.h"
#include "attn_plan.h"

// One-time per-(kernel, device) setup (hipFuncSetAttribute) and per-device properties: the handle API is a public C ABI, a host
// may drive several GPUs from one process, so nothing of this may be remembered per process only.
constexpr int VC_MAX_DEVICES = 64;
inline int vc_device_index() {
  int d = 0;
  (void)hipGetDevice(&d);
  return d >= 0 && d < VC_MAX_DEVICES ? d : 0;
}
struct VcOncePerDevice {
  bool done[VC_MAX_DEVICES] = {};
  bool need() const { return !done[vc_device_index()]; }
  void mark() { done[vc_device_index()] = true; }
};
inline int vc_cu_count() {          // compute units of the CURRENT device
  static int n[VC_MAX_DEVICES] = {};
  const int d = vc_device_index();
  if (n[d] == 0) {
    hipDeviceProp_t p;
    n[d] = hipGetDeviceProperties(&p, d) == hipSuccess && p.multiProcessorCount > 0 ? p.multiProcessorCount : 256;
  }
  return n[d];
}
// the tail of a launcher: VC_OK, or "<what>: <the runtime's message>" in err and VC_ERR_HIP (`what` is the whole prefix, "silu launch")
inline int vc_launch_status(const char* what, char* err, int errlen) {
  const hipError_t e = hipGetLastError();
  if (e == hipSuccess) return VC_OK;
  snprintf(err, errlen, "%s: %s", what, hipGetErrorString(e));
  return VC_ERR_HIP;
}
int vc_gemm_launch(VcGemmArgs a, int tile_cfg, hipStream_t s, char* err, int errlen);
int vc_gemm_plan_impl(VcGemmArgs a, int tile_cfg, int32_t out[8], char* err, int errlen);
int vc_attention_launch(const VcAttention& a, hipStream_t s, char* err, int errlen);
int vc_attention64_launch(const VcAttention& a, const vcplan::AttnPlan& plan, uint64_t* debug_ts, hipStream_t s, char* err, int errlen);
int vc_ln_modulate2_launch(const VcLnStream* a, const VcLnStream* b, int64_t mod_bstride, int32_t D, const int32_t* step_ptr,
                           int64_t mod_step_stride, hipStream_t s, char* err, int errlen);
int vc_ln_modulate_launch(const void* x, int64_t ldx, void* y, int64_t ldy, const void* shift, const void* scale,
                          int64_t mod_bstride, int32_t rows, int32_t D, int32_t rows_per_batch,
                          const int32_t* step_ptr, int64_t mod_step_stride, hipStream_t s, char* err, int errlen);
int vc_qknorm_rope_vt_launch(void* qkv, int64_t ld, int64_t bstride, const void* q_scale, const void* k_scale,
                             const void* q_scale2, const void* k_scale2, int32_t split, const float* rope, int64_t rope_bstride, void* vt, int32_t B, int32_t L, int32_t Lpad,
                             int32_t H, int32_t parts, hipStream_t s, char* err, int errlen);
int vc_temb_launch(const float* t, const float* freqs, void* out, int n, int half, int round_t, hipStream_t s, char* err, int errlen);
int vc_silu_launch(const void* x, void* y, int64_t n, hipStream_t s, char* err, int errlen);
int vc_act2d_launch(const void* x, int64_t ldx, void* y, int64_t ldy, int32_t rows, int32_t cols, int32_t act, hipStream_t s,
                    char* err, int errlen);
int vc_gate_residual_launch(const void* y, int64_t ldy, const void* res, int64_t ldres, const void* gate, void* out, int64_t ldo,
                            int32_t rows, int32_t cols, const int32_t* step_ptr, int64_t gate_step_stride, hipStream_t s,
                            char* err, int errlen);
int vc_add3_launch(const void* a, const void* b, const void* c, void* y, int64_t n, int64_t bn, int64_t cn, hipStream_t s, char* err, int errlen);
int vc_concat_cols_launch(const void* x, int cx, const void* cond, int cc, void* out, int64_t rows, hipStream_t s, char* err, int errlen);
int vc_euler_launch(void* x, const void* v, const float* dts, const int32_t* step_ptr, int64_t n, hipStream_t s, char* err, int errlen);
int vc_euler_f32_launch(float* x32, void* shadow, const void* v, const float* dts, const int32_t* step_ptr, int64_t n, hipStream_t s,
                        char* err, int errlen);
__host__ __device__ inline int vc_evals_of(int method) {   // model evaluations per solver step; 0 = not a VC_SOLVER_*
  return method == VC_SOLVER_EULER ? 1 : method == VC_SOLVER_MIDPOINT ? 2 : method == VC_SOLVER_RK4 ? 4 : 0;
}
int vc_ode_update_launch(const char* what, int method, int stage, void* y, int state_is_bf16, const void* v, void* k, void* y_in,
                         const float* dts, const int32_t* eval_ptr, int64_t n, hipStream_t s, char* err, int errlen);
int vc_ode_stage_launch(int method, int stage, void* y, int state_is_bf16, const void* v, void* k, void* y_in, const float* dts,
                        const int32_t* eval_ptr, int64_t n, hipStream_t s, char* err, int errlen);
int vc_step_advance_launch(int32_t* step_ptr, hipStream_t s, char* err, int errlen);
// rk_embedded.hip: the adaptive solve's kernels with the pair (VC_RK_*) as an argument.  `alias`: the vc_dopri5_* entry point a call
// serves (its name stands in the messages); vc_rk_dense_launch: the pair's dense output, the quartic of Dormand-Prince or the Hermite
// cubic; vc_rk_interp_launch: the public vc_rk_interp, which refuses VC_RK_DOPRI5; vc_dopri5_load_launch: the caller's state -> the
// f32 state and its bf16 shadow
__host__ __device__ inline int vc_rk_stages_of(int method) {   // evaluations k1..kS of a step, the last one first-same-as-last; 0 = not a VC_RK_*
  return method == VC_RK_DOPRI5 ? 7 : method == VC_RK_BOSH3 ? 4 : method == VC_RK_ADAPTIVE_HEUN ? 3 : 0;
}
int vc_rk_stage_launch(int method, int stage, const float* y0, void* k, const void* v, const float* dt_ptr, const int32_t* eval_ptr,
                       float* y_stage, void* y_in, int64_t n, hipStream_t s, char* err, int errlen, const char* alias = nullptr);
int vc_rk_error_ratio_launch(int method, int mode, const float* y0, const float* y1, const void* k, const float* dt_ptr, float rtol, float atol,
                             float* out, float* scratch, int64_t n, hipStream_t s, char* err, int errlen, const char* alias = nullptr);
int vc_rk_dense_launch(int method, const float* y0, const float* y1, const void* k, const float* dt_ptr, float theta, void* out,
                       int out_is_bf16, int64_t n, hipStream_t s, char* err, int errlen, const char* alias = nullptr);
int vc_rk_interp_launch(int method, const float* y0, const float* y1, const void* k, const float* dt_ptr, float theta, void* out,
                        int out_is_bf16, int64_t n, hipStream_t s, char* err, int errlen);
int vc_dopri5_load_launch(const void* x, int x_is_bf16, float* y0, void* y_in, int64_t n, hipStream_t s, char* err, int errlen);
// rng.hip / sde_plan.hip: the stochastic sampler's update, the store of its F32 state in the caller's dtype, and its host rule
int vc_sde_stage_launch(int eval, const float* table, int n_rows, float* y, const void* v, void* y_in, float* xhat, float* k1,
                        const uint64_t* rng, const int32_t* eval_ptr, int64_t n, hipStream_t s, char* err, int errlen);
int vc_sde_store_launch(const float* y, void* out, int out_is_bf16, int64_t n, hipStream_t s, char* err, int errlen);
int vc_sde_plan_impl(const char* method, const char* form, double norm, const char* last_step, double last_step_size, const float* t_grid,
                     int32_t n_points, float* rows, float* times, int32_t capacity, int32_t* n_evals, int32_t* n_draws, char* err, int errlen);
// multistep.hip: the Adams-Bashforth multistep solver's host rule and its update
int vc_ms_plan_impl(int32_t order, const float* t_grid, int32_t n_points, float* rows, float* times, int32_t capacity, int32_t* n_evals,
                    char* err, int errlen);
int vc_ms_stage_launch(int eval, const float* table, int n_rows, float* y, const void* v, void* hist, void* y_in, const int32_t* eval_ptr,
                       int64_t n, hipStream_t s, char* err, int errlen);
int vc_fill_bf16_launch(void* p, float value, int64_t n, hipStream_t s, char* err, int errlen);
int vc_cfg_combine_launch(const void* cond, const void* uncond, void* out, int64_t n, float cfg_scale, hipStream_t s, char* err, int errlen);
int vc_residual_change_launch(const void* h0, const void* h1, const void* p, void* r, float* sums, float* metric, float* scratch,
                              int32_t B, int64_t n, hipStream_t s, char* err, int errlen);
int vc_residual_op_launch(int add, const void* a, int64_t a_bstride, const void* b, int64_t b_bstride, void* out, int64_t out_bstride,
                          int32_t B, int64_t n, hipStream_t s, char* err, int errlen);
// fm_loss.hip: the flow-matching loss's two passes (vc_fm_plan, vc_fm_loss); grid_rules.hip: its training times
int vc_fm_plan_launch(const void* x1, int x1_is_f32, int64_t x1_bstride, int64_t x1_ld, const float* t, const void* x0, uint64_t seed,
                      uint64_t offset, void* xt, int64_t xt_ld, float* ut, int B, int64_t rows, int cols, hipStream_t s, char* err, int errlen);
int vc_fm_loss_launch(const void* out, int64_t out_ld, const float* ut, const int32_t* valid_rows, int valid_on_host, float* loss, float* scratch,
                      int B, int64_t rows, int cols, hipStream_t s, char* err, int errlen);
int vc_fm_times_impl(const char* snr_type, const float* base, int32_t n, int32_t n_tokens, int32_t do_shift, float* out, char* err, int errlen);
// monitor.hip: the numerics monitor's reduction (vc_tensor_stats) and the scan of a log for the entry with nonfinite != 0 that was written first
int vc_tensor_stats_launch(const void* x, int x_is_f32, int64_t bstride, int64_t ld, int B, int64_t rows, int cols, VcStat* out, int64_t out_stride,
                           const int32_t* row_ptr, int capacity, float* scratch, hipStream_t s, char* err, int errlen);
int vc_monitor_first_bad_launch(const VcStat* log, int64_t n, int n_sites, int B, int32_t* out, hipStream_t s, char* err, int errlen);
int vc_pack_latent_launch(const void* in, void* out, int C, int h, int w, int64_t ld, int col0, hipStream_t s, char* err, int errlen);
int vc_pack_mask_launch(const void* in, void* out, int H, int W, int64_t ld, int col0, hipStream_t s, char* err, int errlen);
int vc_unpack_latent_launch(const void* in, int64_t ld, int col0, void* out, int C, int h, int w, hipStream_t s, char* err, int errlen);
int vc_sdedit_mix_launch(const void* noise, const void* latent, double strength, void* out, int64_t n, hipStream_t s, char* err, int errlen);
int vc_im2col3x3_launch(const void* src, void* dst, int H, int W, int C, int up, hipStream_t s, char* err, int errlen);
int vc_groupnorm_launch(const void* x, const void* gamma, const void* beta, void* y, void* scratch, int64_t scratch_bytes,
                        int64_t HW, int C, int G, float eps, int swish, hipStream_t s, char* err, int errlen);
int vc_softmax_rows_launch(void* x, int64_t ld, int rows, int cols, float scale, const void* bias, int64_t ldb, int causal_period,
                           hipStream_t s, char* err, int errlen);
int vc_transpose_launch(const void* src, int64_t lds_, void* dst, int64_t ldd, int R, int Cc, hipStream_t s, char* err, int errlen);
int vc_nchw_to_nhwc_launch(const void* src, int src_f32, void* dst, int C, int Cp, int64_t HW, float div, float add, hipStream_t s, char* err, int errlen);
int vc_nhwc_to_nchw_launch(const void* src, void* dst, int dst_f32, int C, int Cp, int64_t HW, hipStream_t s, char* err, int errlen);
int vc_gaussian_sample_launch(const void* moments, int Cp, const void* noise, void* out, int Z, int64_t HW, float scale, float shift,
                              hipStream_t s, char* err, int errlen);
int vc_vae_weight_relayout_launch(const void* w, int w_f32, void* dst, int O, int I, int kk, int Op, int Ip, hipStream_t s, char* err, int errlen);
int vc_vae_cast_pad_launch(const void* src, int src_f32, void* dst, int n, int n_pad, hipStream_t s, char* err, int errlen);
int vc_zero_fill_launch(void* p, int64_t bytes, hipStream_t s, char* err, int errlen);
int vc_embedding_launch(const int32_t* ids, const void* table, int64_t ldt, int V, void* out, int L, int D, hipStream_t s, char* err, int errlen);
int vc_rownorm_launch(const void* x, const void* w, const void* b, void* y, int rows, int D, float eps, int affine_ln, hipStream_t s, char* err, int errlen);
int vc_ewise_launch(const void* a, const void* b, void* y, int64_t n, int op, hipStream_t s, char* err, int errlen);
// T5's relative-position buckets as kernel arguments: the bucket of distance d >= max_exact is max_exact + #{k : at[k] <= d}
constexpr int VC_T5_MAX_STEPS = 31;      // num_buckets <= 128
struct VcT5Steps { int32_t n; int32_t at[VC_T5_MAX_STEPS]; };
int vc_t5_relative_buckets_impl(int L, int num_buckets, int max_distance, int32_t* out, char* err, int errlen);
int vc_t5_position_bias_launch(const void* table, int64_t ld, int H, int L, int num_buckets, int max_distance, void* out, hipStream_t s,
                               char* err, int errlen);
int vc_clip_embed_launch(const int32_t* ids, const void* tok, int64_t ldt, int V, const void* pos, int64_t ldp, void* out, int L, int Lp, int D,
                         hipStream_t s, char* err, int errlen);
int vc_clip_pool_launch(const int32_t* ids, const void* hidden, int64_t ld, int L, int D, int eos, void* pooled, hipStream_t s, char* err, int errlen);
int vc_conv3x3_launch(const void* x, const void* w, const void* bias, void* out, int64_t ldc, const void* res, int64_t ldres,
                      const void* gate, int H, int W, int C, int O, int mode, hipStream_t s, char* err, int errlen);
int vc_lora_merge_launch(const void* w, int32_t w_is_f32, int64_t ldw, const void* lora_a, int64_t lda, const void* lora_b, int64_t ldb,
                         float scale, void* out, int64_t ldo, const void* bias, int32_t bias_is_f32, const void* lora_b_bias,
                         void* bias_out, int32_t out_features, int32_t in_features, int32_t rank, hipStream_t s, char* err, int errlen);
// the same with the result's rows stored head-permuted (vc_lora_merge_qkv; qkv_heads 0 = vc_lora_merge_launch)
int vc_lora_merge_qkv_launch(const void* w, int32_t w_is_f32, int64_t ldw, const void* lora_a, int64_t lda, const void* lora_b, int64_t ldb,
                             float scale, void* out, int64_t ldo, const void* bias, int32_t bias_is_f32, const void* lora_b_bias,
                             void* bias_out, int32_t out_features, int32_t in_features, int32_t rank, int32_t qkv_heads, hipStream_t s,
                             char* err, int errlen);
// flux_load.hip: n <= VC_SCALE_VECTORS vectors of 128 values (bf16, or f32 where f32[i]) -> bf16 rows of `out` and max|.| of each
constexpr int VC_SCALE_VECTORS = 256;
struct VcScaleVectors { const void* src[VC_SCALE_VECTORS]; uint8_t f32[VC_SCALE_VECTORS]; };
int vc_scale_cast_launch(const VcScaleVectors& v, int n, void* out, int64_t out_stride, float* amax, hipStream_t s, char* err, int errlen);
int vc_randn_launch(void* out, int dtype, int64_t n, uint64_t seed, uint64_t offset, hipStream_t s, char* err, int errlen);
int vc_randn_tokens_launch(void* tokens, int C, int h, int w, int64_t ld, int col0, uint64_t seed, uint64_t offset, hipStream_t s, char* err,
                           int errlen);
// rng_torch.hip: torch's device generator stream.  vc_torch_caps_resolve checks (sm_count, threads_per_sm) and replaces each 0 by the
// current device's value (VC_ERR_HIP without a device)
int vc_torch_caps_resolve(const char* who, int* sm_count, int* threads_per_sm, char* err, int errlen);
int vc_torch_randn_policy_impl(int64_t n, int sm_count, int threads_per_sm, int32_t* grid, uint64_t* offset_advance, char* err, int errlen);
int vc_randn_torch_launch(void* out, int dtype, int64_t n, uint64_t seed, uint64_t offset, int sm_count, int threads_per_sm, hipStream_t s,
                          char* err, int errlen);
int vc_randn_torch_tokens_launch(void* tokens, int C, int h, int w, int64_t ld, int col0, uint64_t seed, uint64_t offset, int sm_count,
                                 int threads_per_sm, hipStream_t s, char* err, int errlen);
int vc_pixels_out_launch(const void* img, int img_is_f32, int H, int W, int x0, int w, void* out, int out_form, hipStream_t s, char* err,
                         int errlen);
// image_metrics.hip: vc_image_compare
int vc_image_compare_scratch_bytes_impl(int C, int H, int W, int64_t* bytes, char* err, int errlen);
int vc_image_compare_launch(const void* a, const void* b, int form, int C, int H, int W, VcImageMetrics* out_dev, void* scratch, int64_t scratch_bytes,
                            hipStream_t s, char* err, int errlen);
int vc_image_psnr_impl(const VcImageMetrics* m, double* psnr_db, char* err, int errlen);
// resample.hip, pixels_in.hip: the photo front end's kernels
int vc_resample_kmax_impl(int in, int out, int filter, char* err, int errlen);
int vc_resample_coeffs_impl(int in, int out, int filter, int32_t* xmin, int32_t* len, int32_t* ki, int kmax, char* err, int errlen);
int64_t vc_resample_tmp_bytes_impl(int H, int W, int h, int w, int filter, char* err, int errlen);
int vc_resample_u8_launch(const void* src, int H, int W, void* dst, int h, int w, int filter, void* tmp, int64_t tmp_bytes, hipStream_t s,
                          char* err, int errlen);
int vc_pixels_in_launch(const void* src, int H, int W, int left, int top, void* out, int out_is_f32, int h, int Wrow, int x0, int w,
                        hipStream_t s, char* err, int errlen);
int vc_mask_fill_launch(void* mask, int h, int Wrow, int x0, int w, int value, hipStream_t s, char* err, int errlen);
// grid_rules.hip: the host rules of one grid (no device)
int vc_fit_size_impl(int32_t w, int32_t h, int32_t resolution, int32_t* nw, int32_t* nh, char* err, int errlen);
int vc_grid_layout_impl(int32_t grid_h, int32_t grid_w, const int32_t* cell_w, const int32_t* cell_h, int32_t resolution, VcCellPlan* out,
                        char* err, int errlen);
int vc_upsampling_size_impl(int32_t orig_w, int32_t orig_h, int32_t* w, int32_t* h, char* err, int errlen);
int vc_time_grid_impl(int32_t n_points, int32_t n_tokens, double t0, double t1, int32_t do_shift, double time_shifting_factor, float* out,
                      char* err, int errlen);
int64_t vc_grid_tokens_impl(int32_t rows, const int32_t* lat_h, const int32_t* lat_w, char* err, int errlen);
int vc_grid_img_ids_impl(int32_t rows, const int32_t* lat_h, const int32_t* lat_w, float* out, char* err, int errlen);

// the Flux handle API: flux_weights.hip (create, bind_*, bound, mod_offset, set_lora_scale, load_*), flux_sample.hip (sample_*,
// dopri5_log, set_step_cache, set_cfg, step_cache_stats), flux_engine.hip (the rest)
const VcFluxConfig* vc_flux_config_impl(void* handle);
int vc_flux_create_impl(const VcFluxConfig* cfg, void** handle, char* err, int errlen);
int vc_flux_destroy_impl(void* handle, char* err, int errlen);
int vc_flux_bind_weight_impl(void* handle, const char* name, const void* w, const void* bias, int32_t rows, int32_t cols, int64_t ldw,
                             char* err, int errlen);
int vc_flux_bind_lora_impl(void* handle, const char* name, const void* lora_a, int64_t lda, const void* lora_b, int64_t ldb,
                           const void* lora_b_bias, int32_t out_features, int32_t in_features, int32_t rank, char* err, int errlen);
int vc_flux_load_key_impl(void* handle, int32_t index, char* name, int32_t namelen, int64_t* shape, int32_t* ndim, char* err, int errlen);
int vc_flux_load_tensor_impl(void* handle, const char* key, const void* ptr, int32_t is_f32, const int64_t* shape, int32_t ndim, char* err,
                             int errlen);
int64_t vc_flux_load_bytes_impl(void* handle);
int vc_flux_load_finish_impl(void* handle, float lora_scale, void* arena, int64_t arena_bytes, hipStream_t s, char* err, int errlen);
int vc_flux_bound_impl(void* handle, const char* name, const void** w, const void** bias, int32_t* rows, int32_t* cols, int64_t* ldw, char* err,
                       int errlen);
int vc_flux_set_lora_scale_impl(void* handle, float scale, char* err, int errlen);
int vc_flux_set_tap_impl(void* handle, const char* name, void* dst, char* err, int errlen);
int vc_flux_tap_shape_impl(void* handle, const char* name, int64_t* rows, int32_t* cols, char* err, int errlen);
int64_t vc_flux_mod_offset_impl(void* handle, const char* name);
int vc_flux_set_option_impl(void* handle, const char* name, int32_t value, char* err, int errlen);
int64_t vc_flux_workspace_bytes_impl(void* handle, int32_t B, int32_t T, int32_t N, int32_t max_steps);
int vc_flux_prepare_impl(void* handle, const VcFluxInputs* in, void* workspace, int64_t workspace_bytes, hipStream_t s, char* err, int errlen);
int vc_flux_forward_impl(void* handle, const void* img, const float* timesteps, int32_t timesteps_is_bf16, void* out, hipStream_t s,
                         char* err, int errlen);
int vc_flux_eval_loss_impl(void* handle, const void* x1, int32_t x1_is_f32, const void* cond, const float* t, const void* x0, uint64_t seed,
                           uint64_t offset, float* loss, hipStream_t s, char* err, int errlen);
int vc_flux_sample_begin_impl(void* handle, int32_t method, const void* x, const void* cond, const float* t_grid, int32_t n_points, int32_t state_is_bf16,
                              hipStream_t s, char* err, int errlen);
int vc_flux_sample_steps_impl(void* handle, int32_t n_steps, void* trajectory, hipStream_t s, char* err, int errlen);
int vc_flux_profile_impl(void* handle, int32_t evaluations, VcFluxLaunchClass* out, int32_t capacity, int32_t* count, hipStream_t s,
                         char* err, int errlen);
int vc_flux_sample_end_impl(void* handle, void* x_out, hipStream_t s, char* err, int errlen);
int vc_flux_set_step_cache_impl(void* handle, float threshold, int32_t max_consecutive, char* err, int errlen);
int vc_flux_set_cfg_impl(void* handle, int32_t on, float cfg_scale, char* err, int errlen);
int vc_flux_step_cache_stats_impl(void* handle, int32_t* computed, int32_t* reused, float* metrics, int32_t capacity, char* err, int errlen);
int vc_flux_sample_dopri5_impl(void* handle, void* x, const void* cond, const float* t_grid, int32_t n_points, int32_t state_is_bf16,
                               float rtol, float atol, int32_t max_attempts, void* trajectory, hipStream_t s, char* err, int errlen);
int vc_flux_dopri5_log_impl(void* handle, double* t, double* dt, float* ratio, int32_t* accepted, int32_t capacity, int32_t* attempts,
                            int32_t* evaluations, char* err, int errlen);
int vc_flux_sample_rk_impl(void* handle, int32_t method, void* x, const void* cond, const float* t_grid, int32_t n_points, int32_t state_is_bf16,
                           float rtol, float atol, int32_t max_attempts, void* trajectory, hipStream_t s, char* err, int errlen);
int vc_flux_sample_multistep_impl(void* handle, int32_t order, void* x, const void* cond, const float* t_grid, int32_t n_points,
                                  int32_t state_is_bf16, void* trajectory, hipStream_t s, char* err, int errlen);
int vc_flux_plan_count_impl(void* handle);
int vc_flux_sample_sde_impl(void* handle, const char* method, void* x, const void* cond, const float* t_grid, int32_t n_points, const char* form,
                            double norm, const char* last_step, double last_step_size, uint64_t seed, uint64_t offset, int32_t state_is_bf16,
                            void* trajectory, hipStream_t s, char* err, int errlen);
int vc_flux_step_nodes_impl(void* handle, int32_t nodes[3], char* err, int errlen);
int vc_flux_set_monitor_impl(void* handle, int32_t level, VcStat* log, int32_t capacity_evals, float* scratch, char* err, int errlen);
int vc_flux_monitor_sites_impl(void* handle, int32_t index, char* name, int32_t namelen, char* err, int errlen);
int vc_flux_monitor_bytes_impl(void* handle, int32_t capacity_evals, int64_t* log_bytes, int64_t* scratch_bytes, char* err, int errlen);
int vc_flux_monitor_report_impl(void* handle, int32_t* first_bad_eval, int32_t* first_bad_site, int32_t* first_bad_sample, int32_t* evals_logged,
                                hipStream_t s, char* err, int errlen);

// vae_engine.hip: the autoencoder handle
int vc_vae_create_impl(const VcVaeConfig* cfg, void** handle, char* err, int errlen);
int vc_vae_destroy_impl(void* handle, char* err, int errlen);
int vc_vae_weight_name_impl(void* handle, int32_t index, char* name, int32_t namelen, char* err, int errlen);
int vc_vae_bind_weight_impl(void* handle, const char* name, const void* w, const void* bias, int32_t is_f32, const int64_t* shape, int32_t ndim,
                            hipStream_t s, char* err, int errlen);
int vc_vae_workspace_bytes_impl(void* handle, int32_t H, int32_t W, int32_t which, int64_t* bytes, char* err, int errlen);
int vc_vae_prepare_impl(void* handle, int32_t H, int32_t W, int32_t which, void* workspace, int64_t workspace_bytes, hipStream_t s,
                        char* err, int errlen);
int vc_vae_decode_impl(void* handle, const void* latent, int32_t latent_form, int64_t ld, int32_t col0, void* pixels, int32_t pixels_is_f32,
                       hipStream_t s, char* err, int errlen);
int vc_vae_encode_impl(void* handle, const void* pixels, int32_t pixels_is_f32, const void* noise, void* latent, int32_t latent_form, int64_t ld,
                       int32_t col0, hipStream_t s, char* err, int errlen);
int vc_vae_plan_count_impl(void* handle);
const VcVaeConfig* vc_vae_config_impl(void* handle);

// text_engine.hip: the text-encoder handle
int vc_text_create_impl(const VcTextConfig* cfg, void** handle, char* err, int errlen);
int vc_text_destroy_impl(void* handle, char* err, int errlen);
int vc_text_weight_name_impl(void* handle, int32_t index, char* name, int32_t namelen, char* err, int errlen);
int vc_text_bind_tensor_impl(void* handle, const char* key, const void* ptr, const int64_t* shape, int32_t ndim, char* err, int errlen);
int vc_text_workspace_bytes_impl(void* handle, int32_t L, int64_t* bytes, char* err, int errlen);
int vc_text_prepare_impl(void* handle, int32_t L, void* workspace, int64_t workspace_bytes, hipStream_t s, char* err, int errlen);
int vc_text_encode_impl(void* handle, const int32_t* ids, int32_t n_prompts, void* hidden, void* pooled, hipStream_t s, char* err, int errlen);
int vc_text_plan_count_impl(void* handle);
const VcTextConfig* vc_text_config_impl(void* handle);

// grid_engine.hip: the grid handle
int vc_grid_create_impl(const VcGridConfig* cfg, void** handle, char* err, int errlen);
int vc_grid_destroy_impl(void* handle, char* err, int errlen);
int vc_grid_set_noise_impl(void* handle, int source, int sm_count, int threads_per_sm, char* err, int errlen);
int vc_grid_workspace_bytes_impl(void* handle, const VcGridJob* job, int64_t* bytes, char* err, int errlen);
int vc_grid_sdedit_workspace_bytes_impl(void* handle, const VcGridSdedit* job, int64_t* bytes, char* err, int errlen);
int vc_grid_generate_impl(void* handle, const VcGridJob* job, void* workspace, int64_t workspace_bytes, void* const* out_rows, hipStream_t s,
                          char* err, int errlen);
int vc_grid_sdedit_impl(void* handle, const VcGridSdedit* job, void* workspace, int64_t workspace_bytes, void* const* out_images,
                        hipStream_t s, char* err, int errlen);
int vc_grid_photos_workspace_bytes_impl(void* handle, const VcGridPhotos* job, int64_t* bytes, char* err, int errlen);
int vc_grid_sdedit_u8_workspace_bytes_impl(void* handle, const VcGridSdeditU8* job, int64_t* bytes, char* err, int errlen);
int vc_grid_generate_photos_impl(void* handle, const VcGridPhotos* job, void* workspace, int64_t workspace_bytes, void* const* out_rows,
                                 hipStream_t s, char* err, int errlen);
int vc_grid_sdedit_u8_impl(void* handle, const VcGridSdeditU8* job, void* workspace, int64_t workspace_bytes, void* const* out_images,
                           hipStream_t s, char* err, int errlen);
