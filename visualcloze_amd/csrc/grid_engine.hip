// Grid handle of include/vcloze_hip.h (vc_grid_*): one grid, pixels and token ids in, pixels out - the tensor path of
// VisualClozeModel.process_images (visualcloze.py:363-434) and of `upsampling` (:184-240) as ONE call each.  Host code only: it
// COMPOSES the library's own entry points - vc_randn / vc_randn_tokens, the autoencoder, text-encoder and Flux handles, vc_pack_mask,
// vc_sdedit_mix, vc_time_grid, vc_grid_img_ids, vc_pixels_out - in the order visualcloze_amd/pipeline.py composes them
// (generate_grid with rng = NoiseStream(seed), upsample_images): the parity twin, same kernels, same operands, same bits.  With
// vc_grid_set_noise(VC_NOISE_TORCH) the draws are vc_randn_torch / vc_randn_torch_tokens instead (twin: rng = TorchNoiseStream(seed)).  The four
// sub-handles are BORROWED; their plan caches keep the captured graphs, this file captures nothing itself.
//
// Workspace (caller's device memory), carved in this order; tok = image tokens of the job, C = Flux out_channels (= 4 z), CW =
// in_channels - out_channels (= 4 z + 256), n = tokens of one sdedit target:
//   VAE     the autoencoder's workspace at the largest item, both halves      T5 CLIP  the text encoders' workspaces
//   FLUX    the Flux handle's workspace (B, T, tok or n, max_evals)            IDS      int32 T5 ids, CLIP ids
//   TXT     bf16 [B, T, ctx]        VEC  bf16 [B, vec]                          COND     bf16 [tok, CW]      X  bf16 [tok, C]
//   ENOISE  bf16 [z, h, w] of the largest item (the DiagonalGaussian draw)     PIN      the item's pixels, staged (plans are keyed
//   PX      bf16 [3, H, W] of the largest item (the decoder's output)                   on workspace addresses only)
//   sdedit only:  LAT NOISE bf16 [tok, C]    ZERO bf16 [3, H, W]    ONES bf16 [H, W]
// The photo calls (vc_grid_generate_photos, vc_grid_sdedit_u8) put their own part in FRONT of that: the row (target) tensors and
// masks they build from 8-bit images, the 8-bit intermediates of the resamples and vc_resample_u8's tmp; the rest is handed to
// vc_grid_generate / vc_grid_sdedit as their workspace.
#include "common.h"
#include "vcloze_internal.h"
#include "engine_core.h"
#include <math.h>
#include <string.h>
#include <vector>

namespace {

struct Grid {
  void *flux = nullptr, *vae = nullptr, *t5 = nullptr, *clip = nullptr;
  int z = 0, C = 0, CW = 0, ctx = 0, vec = 0;
  int noise = VC_NOISE_OWN, sm_count = 0, threads_per_sm = 0;      // vc_grid_set_noise
};

// what both kinds of job come down to
struct Geo {
  bool sdedit = false;
  int items = 0;                       // grid rows / sdedit targets
  int H[VC_GRID_MAX_ROWS] = {}, W[VC_GRID_MAX_ROWS] = {};
  int64_t tok[VC_GRID_MAX_ROWS] = {};  // image tokens per item
  int64_t total = 0;                   // ... of all items
  int B = 1;                           // samples per Flux solve
  int64_t N = 0;                       // image tokens per sample
  int T = 0, clipL = 0, evals = 0, max_evals = 0, pix_f32 = 0, out_form = 0, n_points = 0, method = 0;
  int Hmax = 0, Wmax = 0;              // the item with the most pixels
  uint64_t draws = 0;                  // stream positions the job consumes (VC_NOISE_TORCH: what the generator's offset advances by)
  int sm = 0, tpsm = 0;                // VC_NOISE_TORCH: the grid cap's factors, the device's where the handle holds 0
};

// the stretch of the noise stream a draw of n elements takes: n positions of the library's own, torch's advance of the offset
int draw_span(const Grid& g, const Geo& q, int64_t n, uint64_t* span, Err e) {
  *span = (uint64_t)n;
  if (g.noise != VC_NOISE_TORCH) return VC_OK;
  int32_t grid = 0;
  return vc_torch_randn_policy_impl(n, q.sm, q.tpsm, &grid, span, e.buf, e.len);
}

struct Bufs {
  char *vae = nullptr, *t5 = nullptr, *clip = nullptr, *flux = nullptr, *pin = nullptr;
  int64_t vae_b = 0, t5_b = 0, clip_b = 0, flux_b = 0;
  int32_t *t5_ids = nullptr, *clip_ids = nullptr;
  bf16_t *txt = nullptr, *vec = nullptr, *cond = nullptr, *x = nullptr, *enoise = nullptr, *px = nullptr;
  bf16_t *lat = nullptr, *noise = nullptr, *zero = nullptr, *ones = nullptr;
};

float round_bf16(float v) {            // nearest even, as torch.full(..., dtype=bfloat16) holds the guidance
  uint32_t u;
  memcpy(&u, &v, 4);
  u += 0x7fffu + ((u >> 16) & 1u);
  u &= 0xffff0000u;
  memcpy(&v, &u, 4);
  return v;
}

// the checks both jobs share; everything here is host work
int check_common(const Grid& g, Geo& q, const void* const* pixels, const int32_t* t5_ids, const int32_t* clip_ids, uint64_t offset,
                 float guidance, Err e, const char* what) {
  if (!t5_ids || !clip_ids) FAIL(VC_ERR_ARG, "%s: null t5_ids or clip_ids", what);
  if (q.n_points < 2) FAIL(VC_ERR_ARG, "%s: n_points = %d, at least 2 time points are needed", what, q.n_points);
  if (!vc_evals_of(q.method)) FAIL(VC_ERR_ARG, "%s: unknown method %d (VC_SOLVER_EULER, VC_SOLVER_MIDPOINT, VC_SOLVER_RK4)", what, q.method);
  if (q.out_form != VC_PIXELS_F32 && q.out_form != VC_PIXELS_U8) FAIL(VC_ERR_ARG, "%s: unknown out_form %d (VC_PIXELS_F32, VC_PIXELS_U8)", what, q.out_form);
  if (!(guidance - guidance == 0.0f)) FAIL(VC_ERR_ARG, "%s: guidance is not finite", what);
  const int64_t evals = (int64_t)(q.n_points - 1) * vc_evals_of(q.method);
  if (q.max_evals < 0 || evals > 0x7fffffff) FAIL(VC_ERR_ARG, "%s: max_evals = %d / %lld evaluations out of range", what, q.max_evals, (long long)evals);
  if (q.max_evals && evals > q.max_evals)
    FAIL(VC_ERR_ARG, "%s: (n_points - 1) * vc_solver_evals(method) = %lld evaluations, the workspace is sized for max_evals = %d", what,
         (long long)evals, q.max_evals);
  q.evals = (int)evals;
  if (!q.max_evals) q.max_evals = q.evals;
  q.total = 0;
  q.draws = 0;
  if (g.noise == VC_NOISE_TORCH) {
    if (offset & 3) FAIL(VC_ERR_ARG, "%s: noise_offset = %llu is not a multiple of 4 (VC_NOISE_TORCH: torch.Generator.get_offset())", what, (unsigned long long)offset);
    q.sm = g.sm_count; q.tpsm = g.threads_per_sm;
    TRY(vc_torch_caps_resolve(what, &q.sm, &q.tpsm, e.buf, e.len));
  }
  int64_t best = 0;
  for (int i = 0; i < q.items; ++i) {
    const int H = q.H[i], W = q.W[i];
    if (H <= 0 || W <= 0 || H % 16 || W % 16 || H >= 65536 || W >= 65536)
      FAIL(VC_ERR_ARG, "%s: item %d is %dx%d pixels, positive multiples of 16 below 65536 expected", what, i, H, W);
    if (!pixels[i]) FAIL(VC_ERR_ARG, "%s: null pixels of item %d", what, i);
    if ((uintptr_t)pixels[i] & (q.pix_f32 ? 3 : 1)) FAIL(VC_ERR_ARG, "%s: the pixels of item %d are not aligned to their element size", what, i);
    q.tok[i] = (int64_t)(H / 16) * (W / 16);
    q.total += q.tok[i];
    // generate: encode draw + start noise; sdedit: encode(image), encode(blank), start noise - z * h * w = C/4 * 4 tok elements each
    uint64_t span = 0;
    TRY(draw_span(g, q, (int64_t)g.C * q.tok[i], &span, e));
    q.draws += (uint64_t)(q.sdedit ? 3 : 2) * span;
    if ((int64_t)H * W > best) { best = (int64_t)H * W; q.Hmax = H; q.Wmax = W; }
  }
  if (q.total > 0x7fffffff / 4) FAIL(VC_ERR_ARG, "%s: %lld image tokens are too many", what, (long long)q.total);
  if (offset + q.draws < offset) FAIL(VC_ERR_ARG, "%s: %llu draws at noise_offset %llu leave the 64-bit stream", what, (unsigned long long)q.draws, (unsigned long long)offset);
  return VC_OK;
}

// the carve-up; a null base only adds up.  The sub-handles' own size functions check the lengths and sizes they are asked for.
int carve(const Grid& g, const Geo& q, char* base, Bufs& b, int64_t* need, char* err, int errlen) {
  Err e{err, errlen};
  b = Bufs{};
  for (int i = 0; i < q.items; ++i) {
    int64_t n = 0;
    TRY(vc_vae_workspace_bytes_impl(g.vae, q.H[i], q.W[i], VC_VAE_ENCODER | VC_VAE_DECODER, &n, err, errlen));
    b.vae_b = std::max(b.vae_b, n);
  }
  TRY(vc_text_workspace_bytes_impl(g.t5, q.T, &b.t5_b, err, errlen));
  TRY(vc_text_workspace_bytes_impl(g.clip, q.clipL, &b.clip_b, err, errlen));
  b.flux_b = vc_flux_workspace_bytes_impl(g.flux, q.B, q.T, (int32_t)q.N, q.max_evals);
  if (b.flux_b <= 0) FAIL(VC_ERR_ARG, "grid: vc_flux_workspace_bytes(%d, %d, %lld, %d) failed", q.B, q.T, (long long)q.N, q.max_evals);
  Carver c{base};
  b.vae = c.bytes(b.vae_b);
  b.t5 = c.bytes(b.t5_b);
  b.clip = c.bytes(b.clip_b);
  b.flux = c.bytes(b.flux_b);
  b.t5_ids = c.take<int32_t>(q.T);
  b.clip_ids = c.take<int32_t>(q.clipL);
  b.txt = c.take<bf16_t>((int64_t)q.B * q.T * g.ctx);
  b.vec = c.take<bf16_t>((int64_t)q.B * g.vec);
  b.cond = c.take<bf16_t>(q.total * g.CW);
  b.x = c.take<bf16_t>(q.total * g.C);
  const int64_t pix = (int64_t)q.Hmax * q.Wmax;
  b.enoise = c.take<bf16_t>((int64_t)g.z * (pix / 64));
  b.pin = c.bytes(3 * pix * (q.pix_f32 ? 4 : 2));
  b.px = c.take<bf16_t>(3 * pix);
  if (q.sdedit) {
    b.lat = c.take<bf16_t>(q.total * g.C);
    b.noise = c.take<bf16_t>(q.total * g.C);
    b.zero = c.take<bf16_t>(3 * pix);
    b.ones = c.take<bf16_t>(pix);
  }
  *need = c.off;
  return VC_OK;
}

int geo_of(const Grid& g, const VcGridJob* job, Geo& q, Err e) {
  if (!job) FAIL(VC_ERR_ARG, "grid_generate: null job");
  if (job->rows < 1 || job->rows > VC_GRID_MAX_ROWS) FAIL(VC_ERR_ARG, "grid_generate: rows = %d outside 1..%d", job->rows, VC_GRID_MAX_ROWS);
  q.sdedit = false;
  q.items = job->rows;
  for (int i = 0; i < q.items; ++i) { q.H[i] = job->height[i]; q.W[i] = job->width[i]; }
  q.T = job->t5_len; q.clipL = job->clip_len; q.max_evals = job->max_evals; q.pix_f32 = job->pixels_is_f32 != 0;
  q.out_form = job->out_form; q.n_points = job->n_points; q.method = job->method;
  TRY(check_common(g, q, job->pixels, job->t5_ids, job->clip_ids, job->noise_offset, job->guidance, e, "grid_generate"));
  for (int i = 0; i < q.items; ++i) {
    if (!job->masks[i]) FAIL(VC_ERR_ARG, "grid_generate: null mask of row %d", i);
    if ((uintptr_t)job->masks[i] & 15) FAIL(VC_ERR_ARG, "grid_generate: the mask of row %d must be 16-byte aligned", i);
  }
  if (!(job->time_shifting_factor - job->time_shifting_factor == 0.0)) FAIL(VC_ERR_ARG, "grid_generate: time_shifting_factor is not finite");
  q.B = 1;
  q.N = q.total;
  return VC_OK;
}

int geo_of(const Grid& g, const VcGridSdedit* job, Geo& q, Err e) {
  if (!job) FAIL(VC_ERR_ARG, "grid_sdedit: null job");
  if (job->count < 1 || job->count > VC_GRID_MAX_ROWS) FAIL(VC_ERR_ARG, "grid_sdedit: count = %d outside 1..%d", job->count, VC_GRID_MAX_ROWS);
  if (!(job->strength >= 0.0) || !(job->strength - job->strength == 0.0)) FAIL(VC_ERR_ARG, "grid_sdedit: strength must be finite and not negative");
  q.sdedit = true;
  q.items = job->count;
  for (int i = 0; i < q.items; ++i) { q.H[i] = job->height; q.W[i] = job->width; }
  q.T = job->t5_len; q.clipL = job->clip_len; q.max_evals = job->max_evals; q.pix_f32 = job->pixels_is_f32 != 0;
  q.out_form = job->out_form; q.n_points = job->n_points; q.method = job->method;
  TRY(check_common(g, q, job->pixels, job->t5_ids, job->clip_ids, job->noise_offset, job->guidance, e, "grid_sdedit"));
  q.B = std::min(q.items, VC_GRID_SDEDIT_CHUNK);
  q.N = q.tok[0];
  return VC_OK;
}

// the checks of a run: the job, the outputs, the workspace - all before the device is touched
template <class Job>
int admit(const Grid& g, const Job* job, const int32_t* wanted, void* workspace, int64_t workspace_bytes, void* const* outs, Geo& q, Bufs& b,
          Err e, const char* what) {
  TRY(geo_of(g, job, q, e));
  if (!outs) FAIL(VC_ERR_ARG, "%s: null output list", what);
  for (int i = 0; i < q.items; ++i) {
    if (wanted && !wanted[i]) continue;
    if (!outs[i]) FAIL(VC_ERR_ARG, "%s: null output pointer of item %d", what, i);
    if (q.out_form == VC_PIXELS_F32 && ((uintptr_t)outs[i] & 3)) FAIL(VC_ERR_ARG, "%s: the F32 output of item %d is not 4-byte aligned", what, i);
  }
  if (!aligned256(workspace)) FAIL(VC_ERR_ARG, "%s: the workspace must be a 256-byte aligned device pointer", what);
  int64_t need = 0;
  TRY(carve(g, q, (char*)workspace, b, &need, e.buf, e.len));
  if (workspace_bytes < need) FAIL(VC_ERR_ARG, "%s: workspace too small (%lld < %lld bytes)", what, (long long)workspace_bytes, (long long)need);
  return VC_OK;
}

// T5 and CLIP of the prompt: ids up, one encode each; the results replicated for the B samples of a solve
int encode_prompt(const Grid& g, const Geo& q, const Bufs& b, const int32_t* t5_ids, const int32_t* clip_ids, hipStream_t s, Err e) {
  HIP(hipMemcpyAsync(b.t5_ids, t5_ids, (size_t)q.T * 4, hipMemcpyHostToDevice, s), "hipMemcpyAsync(t5_ids)");
  HIP(hipMemcpyAsync(b.clip_ids, clip_ids, (size_t)q.clipL * 4, hipMemcpyHostToDevice, s), "hipMemcpyAsync(clip_ids)");
  TRY(vc_text_prepare_impl(g.t5, q.T, b.t5, b.t5_b, s, e.buf, e.len));
  TRY(vc_text_encode_impl(g.t5, b.t5_ids, 1, b.txt, nullptr, s, e.buf, e.len));
  TRY(vc_text_prepare_impl(g.clip, q.clipL, b.clip, b.clip_b, s, e.buf, e.len));
  TRY(vc_text_encode_impl(g.clip, b.clip_ids, 1, nullptr, b.vec, s, e.buf, e.len));
  for (int k = 1; k < q.B; ++k) {
    HIP(hipMemcpyAsync(b.txt + (int64_t)k * q.T * g.ctx, b.txt, (size_t)q.T * g.ctx * 2, hipMemcpyDeviceToDevice, s), "hipMemcpyAsync(txt)");
    HIP(hipMemcpyAsync(b.vec + (int64_t)k * g.vec, b.vec, (size_t)g.vec * 2, hipMemcpyDeviceToDevice, s), "hipMemcpyAsync(vec)");
  }
  return VC_OK;
}

// AutoEncoder.encode of one image with its DiagonalGaussian draw from the stream, straight into token columns
int encode_item(const Grid& g, const Geo& q, const Bufs& b, int H, int W, const void* pixels, bool staged, bf16_t* tokens, int64_t ld,
                uint64_t seed, uint64_t& pos, hipStream_t s, Err e) {
  const int64_t n = (int64_t)g.z * (H / 8) * (W / 8);
  uint64_t span = 0;
  TRY(draw_span(g, q, n, &span, e));
  if (g.noise == VC_NOISE_TORCH) TRY(vc_randn_torch_launch(b.enoise, VC_RNG_BF16, n, seed, pos, q.sm, q.tpsm, s, e.buf, e.len));
  else TRY(vc_randn_launch(b.enoise, VC_RNG_BF16, n, seed, pos, s, e.buf, e.len));
  pos += span;
  const void* src = pixels;
  if (staged) {
    HIP(hipMemcpyAsync(b.pin, pixels, (size_t)3 * H * W * (q.pix_f32 ? 4 : 2), hipMemcpyDeviceToDevice, s), "hipMemcpyAsync(pixels)");
    src = b.pin;
  }
  TRY(vc_vae_prepare_impl(g.vae, H, W, VC_VAE_ENCODER | VC_VAE_DECODER, b.vae, b.vae_b, s, e.buf, e.len));
  return vc_vae_encode_impl(g.vae, src, staged ? q.pix_f32 : 0, b.enoise, tokens, VC_VAE_TOKENS, ld, 0, s, e.buf, e.len);
}

// the start noise of one item, [z, H/8, W/8], straight into token rows
int start_noise(const Grid& g, const Geo& q, bf16_t* tokens, int H, int W, uint64_t seed, uint64_t& pos, hipStream_t s, Err e) {
  uint64_t span = 0;
  TRY(draw_span(g, q, (int64_t)g.z * (H / 8) * (W / 8), &span, e));
  if (g.noise == VC_NOISE_TORCH) TRY(vc_randn_torch_tokens_launch(tokens, g.z, H / 8, W / 8, g.C, 0, seed, pos, q.sm, q.tpsm, s, e.buf, e.len));
  else TRY(vc_randn_tokens_launch(tokens, g.z, H / 8, W / 8, g.C, 0, seed, pos, s, e.buf, e.len));
  pos += span;
  return VC_OK;
}

// AutoEncoder.decode from the sampler's token rows, then the pixel epilogue into the caller's buffer
int decode_item(const Grid& g, const Geo& q, const Bufs& b, int H, int W, const bf16_t* tokens, void* out, hipStream_t s, Err e) {
  TRY(vc_vae_prepare_impl(g.vae, H, W, VC_VAE_ENCODER | VC_VAE_DECODER, b.vae, b.vae_b, s, e.buf, e.len));
  TRY(vc_vae_decode_impl(g.vae, tokens, VC_VAE_TOKENS, g.C, 0, b.px, 0, s, e.buf, e.len));
  return vc_pixels_out_launch(b.px, 0, H, W, 0, W, out, q.out_form, s, e.buf, e.len);
}

// one solve of B samples: x [B, N, C] in place, cond [B, N, CW]; B = 1, all-ones masks, zero txt_ids, bf16 guidance (visualcloze.py:413)
int solve(const Grid& g, const Geo& q, const Bufs& b, int B, const float* img_ids, const float* t_grid, float guidance, bf16_t* x,
          const bf16_t* cond, hipStream_t s, Err e) {
  std::vector<float> txt_ids((size_t)B * q.T * 3, 0.0f), gd((size_t)B, round_bf16(guidance));
  VcFluxInputs in;
  memset(&in, 0, sizeof(in));
  in.B = B; in.T = q.T; in.N = (int32_t)q.N; in.max_steps = q.max_evals;
  in.txt = b.txt; in.y = b.vec;
  in.guidance = gd.data(); in.img_ids = img_ids; in.txt_ids = txt_ids.data();
  in.guidance_is_bf16 = 1;
  TRY(vc_flux_prepare_impl(g.flux, &in, b.flux, b.flux_b, s, e.buf, e.len));
  TRY(vc_flux_sample_begin_impl(g.flux, q.method, x, cond, t_grid, q.n_points, 1, s, e.buf, e.len));
  TRY(vc_flux_sample_steps_impl(g.flux, q.n_points - 1, nullptr, s, e.buf, e.len));
  return vc_flux_sample_end_impl(g.flux, x, s, e.buf, e.len);
}

}  // namespace

int vc_grid_create_impl(const VcGridConfig* cfg, void** handle, char* err, int errlen) {
  Err e{err, errlen};
  if (!cfg || !handle) FAIL(VC_ERR_ARG, "grid_create: null argument");
  if (!cfg->flux || !cfg->vae || !cfg->t5 || !cfg->clip) FAIL(VC_ERR_ARG, "grid_create: the flux, vae, t5 and clip handles are all required");
  const VcFluxConfig& f = *vc_flux_config_impl(cfg->flux);
  const VcVaeConfig& v = *vc_vae_config_impl(cfg->vae);
  const VcTextConfig& t = *vc_text_config_impl(cfg->t5);
  const VcTextConfig& c = *vc_text_config_impl(cfg->clip);
  if (t.kind != VC_TEXT_T5 || c.kind != VC_TEXT_CLIP) FAIL(VC_ERR_ARG, "grid_create: t5 must be a VC_TEXT_T5 handle and clip a VC_TEXT_CLIP handle");
  if (v.n_ch_mult != 4 || v.in_channels != 3 || v.out_ch != 3)
    FAIL(VC_ERR_ARG, "grid_create: the grid needs an RGB autoencoder of 8x reduction (n_ch_mult 4), got n_ch_mult %d, %d -> %d channels", v.n_ch_mult,
         v.in_channels, v.out_ch);
  if (4 * v.z_channels != f.out_channels || f.in_channels - f.out_channels != 4 * v.z_channels + 256)
    FAIL(VC_ERR_ARG, "grid_create: Flux channels %d -> %d do not fit 4 * z_channels = %d latent and 256 mask columns", f.in_channels, f.out_channels,
         4 * v.z_channels);
  if (t.d_model != f.context_in_dim || c.d_model != f.vec_in_dim)
    FAIL(VC_ERR_ARG, "grid_create: T5 d_model %d / CLIP d_model %d differ from the Flux context_in_dim %d / vec_in_dim %d", t.d_model, c.d_model,
         f.context_in_dim, f.vec_in_dim);
  Grid* g = new Grid();
  g->flux = cfg->flux; g->vae = cfg->vae; g->t5 = cfg->t5; g->clip = cfg->clip;
  g->z = v.z_channels; g->C = f.out_channels; g->CW = f.in_channels - f.out_channels; g->ctx = f.context_in_dim; g->vec = f.vec_in_dim;
  *handle = g;
  return VC_OK;
}

int vc_grid_destroy_impl(void* handle, char* err, int errlen) {
  HANDLE(Grid, g, "grid");
  delete &g;                 // the sub-handles are the caller's
  return VC_OK;
}

int vc_grid_set_noise_impl(void* handle, int source, int sm_count, int threads_per_sm, char* err, int errlen) {
  HANDLE(Grid, g, "grid");
  if (source != VC_NOISE_OWN && source != VC_NOISE_TORCH) FAIL(VC_ERR_ARG, "grid_set_noise: unknown source %d (VC_NOISE_OWN, VC_NOISE_TORCH)", source);
  if (sm_count < 0 || (threads_per_sm != 0 && threads_per_sm < 256))
    FAIL(VC_ERR_ARG, "grid_set_noise: sm_count = %d, threads_per_sm = %d: 0 (the current device's) or a positive count / at least 256 expected", sm_count,
         threads_per_sm);
  g.noise = source; g.sm_count = sm_count; g.threads_per_sm = threads_per_sm;
  return VC_OK;
}

int vc_grid_workspace_bytes_impl(void* handle, const VcGridJob* job, int64_t* bytes, char* err, int errlen) {
  HANDLE(Grid, g, "grid");
  if (!bytes) FAIL(VC_ERR_ARG, "grid_workspace_bytes: null result pointer");
  Geo q;
  Bufs b;
  TRY(geo_of(g, job, q, e));
  return carve(g, q, nullptr, b, bytes, err, errlen);
}

int vc_grid_sdedit_workspace_bytes_impl(void* handle, const VcGridSdedit* job, int64_t* bytes, char* err, int errlen) {
  HANDLE(Grid, g, "grid");
  if (!bytes) FAIL(VC_ERR_ARG, "grid_sdedit_workspace_bytes: null result pointer");
  Geo q;
  Bufs b;
  TRY(geo_of(g, job, q, e));
  return carve(g, q, nullptr, b, bytes, err, errlen);
}

int vc_grid_generate_impl(void* handle, const VcGridJob* job, void* workspace, int64_t workspace_bytes, void* const* out_rows, hipStream_t s,
                          char* err, int errlen) {
  HANDLE(Grid, g, "grid");
  Geo q;
  Bufs b;
  TRY(admit(g, job, job ? job->decode : nullptr, workspace, workspace_bytes, out_rows, q, b, e, "grid_generate"));
  // host rules first: they can still refuse
  int32_t lh[VC_GRID_MAX_ROWS], lw[VC_GRID_MAX_ROWS];
  for (int i = 0; i < q.items; ++i) { lh[i] = q.H[i] / 8; lw[i] = q.W[i] / 8; }
  std::vector<float> ids((size_t)q.N * 3), t((size_t)q.n_points);
  TRY(vc_grid_img_ids_impl(q.items, lh, lw, ids.data(), err, errlen));
  TRY(vc_time_grid_impl(q.n_points, (int32_t)q.N, 0.0, 1.0, 1, job->time_shifting_factor, t.data(), err, errlen));
  uint64_t pos = job->noise_offset;
  int64_t row0 = 0;
  for (int i = 0; i < q.items; ++i) {          // :377-378 the encodes, :381-389 cond = latent tokens || packed fill mask
    bf16_t* cond = b.cond + row0 * g.CW;
    TRY(encode_item(g, q, b, q.H[i], q.W[i], job->pixels[i], true, cond, g.CW, job->seed, pos, s, e));
    TRY(vc_pack_mask_launch(job->masks[i], cond, q.H[i], q.W[i], g.CW, g.C, s, err, errlen));
    row0 += q.tok[i];
  }
  row0 = 0;
  for (int i = 0; i < q.items; ++i) {          // :394-399 the start noise, row by row
    TRY(start_noise(g, q, b.x + row0 * g.C, q.H[i], q.W[i], job->seed, pos, s, e));
    row0 += q.tok[i];
  }
  TRY(encode_prompt(g, q, b, job->t5_ids, job->clip_ids, s, e));
  TRY(solve(g, q, b, 1, ids.data(), t.data(), job->guidance, b.x, b.cond, s, e));      // :403-420
  row0 = 0;
  for (int i = 0; i < q.items; ++i) {          // :425-432
    if (job->decode[i]) TRY(decode_item(g, q, b, q.H[i], q.W[i], b.x + row0 * g.C, out_rows[i], s, e));
    row0 += q.tok[i];
  }
  if (job->noise_offset_out) *job->noise_offset_out = pos;
  return VC_OK;
}

int vc_grid_sdedit_impl(void* handle, const VcGridSdedit* job, void* workspace, int64_t workspace_bytes, void* const* out_images,
                        hipStream_t s, char* err, int errlen) {
  HANDLE(Grid, g, "grid");
  Geo q;
  Bufs b;
  TRY(admit(g, job, nullptr, workspace, workspace_bytes, out_images, q, b, e, "grid_sdedit"));
  const int H = job->height, W = job->width, K = q.items;
  if (job->strength >= 1.0) {                  // visualcloze.py:180-181: the (resized) input goes back as it is
    for (int k = 0; k < K; ++k) TRY(vc_pixels_out_launch(job->pixels[k], q.pix_f32, H, W, 0, W, out_images[k], q.out_form, s, err, errlen));
    if (job->noise_offset_out) *job->noise_offset_out = job->noise_offset;
    return VC_OK;
  }
  const int32_t lh = H / 8, lw = W / 8;
  const int64_t n = q.N, pix = (int64_t)H * W;
  std::vector<float> ids((size_t)q.B * n * 3), t((size_t)q.n_points);
  TRY(vc_grid_img_ids_impl(1, &lh, &lw, ids.data(), err, errlen));
  for (int k = 1; k < q.B; ++k) memcpy(ids.data() + (size_t)k * n * 3, ids.data(), (size_t)n * 3 * sizeof(float));
  TRY(vc_time_grid_impl(q.n_points, (int32_t)n, job->strength, 1.0, 0, 1.0, t.data(), err, errlen));   // :184-193: un-shifted, from t0 = strength
  HIP(hipMemsetAsync(b.zero, 0, (size_t)(3 * pix * 2), s), "hipMemsetAsync(blank)");
  HIP(hipMemsetD16Async((hipDeviceptr_t)b.ones, 0x3F80, (size_t)pix, s), "hipMemsetD16Async(mask)");     // bf16 1.0: mask = 1 everywhere, :198
  uint64_t pos = job->noise_offset;
  for (int k = 0; k < K; ++k) {                // :200-217 per target: encode(image), encode(blank), noise
    bf16_t* cond = b.cond + k * n * g.CW;
    TRY(encode_item(g, q, b, H, W, job->pixels[k], true, b.lat + k * n * g.C, g.C, job->seed, pos, s, e));
    TRY(encode_item(g, q, b, H, W, b.zero, false, cond, g.CW, job->seed, pos, s, e));
    TRY(vc_pack_mask_launch(b.ones, cond, H, W, g.CW, g.C, s, err, errlen));
    TRY(start_noise(g, q, b.noise + k * n * g.C, H, W, job->seed, pos, s, e));
  }
  TRY(vc_sdedit_mix_launch(b.noise, b.lat, job->strength, b.x, (int64_t)K * n * g.C, s, err, errlen));     // :221, all targets at once
  TRY(encode_prompt(g, q, b, job->t5_ids, job->clip_ids, s, e));
  for (int k0 = 0; k0 < K; k0 += VC_GRID_SDEDIT_CHUNK) {
    const int bs = std::min(VC_GRID_SDEDIT_CHUNK, K - k0);
    TRY(solve(g, q, b, bs, ids.data(), t.data(), job->guidance, b.x + k0 * n * g.C, b.cond + k0 * n * g.CW, s, e));
  }
  for (int k = 0; k < K; ++k) TRY(decode_item(g, q, b, H, W, b.x + k * n * g.C, out_images[k], s, e));   // :237-240
  if (job->noise_offset_out) *job->noise_offset_out = pos;
  return VC_OK;
}

// ---- the photo front end: 8-bit images in.  The layout rule (grid_rules.hip), vc_resample_u8, vc_pixels_in and vc_mask_fill build
// the row tensors in the front part of the workspace, then the job is vc_grid_generate's / vc_grid_sdedit's own.
namespace {

struct PhotoBufs {
  bf16_t* rows[VC_GRID_MAX_ROWS] = {};
  bf16_t* masks[VC_GRID_MAX_ROWS] = {};
  unsigned char *fit = nullptr, *cover = nullptr, *cell = nullptr, *fin = nullptr;
  char* tmp = nullptr;
  int64_t tmp_b = 0;
};

struct PhotoPlan {
  std::vector<VcCellPlan> cells;
  VcGridJob job;                       // the job vc_grid_generate runs: rows, sizes, the pointers into the workspace
};

int64_t tmp_for(int H, int W, int h, int w, int filter) {
  char scratch[8];
  const int64_t n = vc_resample_tmp_bytes_impl(H, W, h, w, filter, scratch, (int)sizeof(scratch));
  return n < 0 ? 0 : n;
}

// the layout and the carve-up of the photo part; a null base only adds up
int plan_photos(const VcGridPhotos* job, char* base, PhotoPlan& pp, PhotoBufs& pb, int64_t* front, Err e) {
  if (!job) FAIL(VC_ERR_ARG, "grid_generate_photos: null job");
  if (!job->images || !job->width || !job->height) FAIL(VC_ERR_ARG, "grid_generate_photos: null images, width or height list");
  if (job->grid_h < 1 || job->grid_h > VC_GRID_MAX_ROWS || job->grid_w < 1 || job->grid_w > VC_GRID_MAX_ROWS)
    FAIL(VC_ERR_ARG, "grid_generate_photos: a grid of %dx%d cells, 1..%d rows and columns expected", job->grid_h, job->grid_w, VC_GRID_MAX_ROWS);
  const int gh = job->grid_h, gw = job->grid_w, n = gh * gw;
  std::vector<int32_t> cw((size_t)n), ch((size_t)n);
  for (int c = 0; c < n; ++c) {
    const bool has = job->images[c] != nullptr;
    if (has && (job->width[c] < 1 || job->height[c] < 1)) FAIL(VC_ERR_ARG, "grid_generate_photos: image %d is %dx%d", c, job->width[c], job->height[c]);
    cw[c] = has ? job->width[c] : 0;
    ch[c] = has ? job->height[c] : 0;
  }
  pp.cells.assign((size_t)n, VcCellPlan{});
  TRY(vc_grid_layout_impl(gh, gw, cw.data(), ch.data(), job->resolution, pp.cells.data(), e.buf, e.len));
  VcGridJob& j = pp.job;
  memset(&j, 0, sizeof(j));
  j.rows = gh;
  j.t5_ids = job->t5_ids; j.clip_ids = job->clip_ids; j.t5_len = job->t5_len; j.clip_len = job->clip_len;
  j.seed = job->seed; j.noise_offset = job->noise_offset; j.noise_offset_out = job->noise_offset_out;
  j.guidance = job->guidance; j.n_points = job->n_points; j.method = job->method; j.out_form = job->out_form; j.max_evals = job->max_evals;
  j.time_shifting_factor = job->time_shifting_factor;
  Carver c{base};
  pb = PhotoBufs{};
  int64_t fit = 0, cover = 0, cell = 0, fin = 0;
  for (int i = 0; i < gh; ++i) {
    int W = 0;
    for (int k = 0; k < gw; ++k) W += pp.cells[i * gw + k].final_w;
    const int H = pp.cells[i * gw].final_h;
    if (H % 16 || W % 16 || W >= 65536) FAIL(VC_ERR_ARG, "grid_generate_photos: row %d comes to %dx%d pixels, multiples of 16 below 65536 expected", i, H, W);
    j.height[i] = H; j.width[i] = W; j.decode[i] = job->decode[i];
    pb.rows[i] = c.take<bf16_t>((int64_t)3 * H * W);
    pb.masks[i] = c.take<bf16_t>((int64_t)H * W);
    j.pixels[i] = pb.rows[i] ? (const void*)pb.rows[i] : (const void*)(uintptr_t)256;    // sizing only: any aligned non-null value
    j.masks[i] = pb.masks[i] ? (const void*)pb.masks[i] : (const void*)(uintptr_t)256;
  }
  for (int k = 0; k < n; ++k) {
    const VcCellPlan& p = pp.cells[k];
    const bool again = p.final_w != p.cell_w || p.final_h != p.cell_h;
    if (!p.present) continue;
    fit = std::max(fit, (int64_t)p.fit_w * p.fit_h * 3);
    cover = std::max(cover, (int64_t)p.cover_w * p.cover_h * 3);
    pb.tmp_b = std::max(pb.tmp_b, tmp_for(ch[k], cw[k], p.fit_h, p.fit_w, VC_FILTER_LANCZOS));
    pb.tmp_b = std::max(pb.tmp_b, tmp_for(p.fit_h, p.fit_w, p.cover_h, p.cover_w, VC_FILTER_BICUBIC));
    if (again) {
      cell = std::max(cell, (int64_t)p.cell_w * p.cell_h * 3);
      fin = std::max(fin, (int64_t)p.final_w * p.final_h * 3);
      pb.tmp_b = std::max(pb.tmp_b, tmp_for(p.cell_h, p.cell_w, p.final_h, p.final_w, VC_FILTER_BICUBIC));
    }
  }
  pb.fit = (unsigned char*)c.bytes(fit);
  pb.cover = (unsigned char*)c.bytes(cover);
  pb.cell = (unsigned char*)c.bytes(cell);
  pb.fin = (unsigned char*)c.bytes(fin);
  pb.tmp = c.bytes(pb.tmp_b);
  *front = c.off;
  return VC_OK;
}

}  // namespace

int vc_grid_photos_workspace_bytes_impl(void* handle, const VcGridPhotos* job, int64_t* bytes, char* err, int errlen) {
  HANDLE(Grid, g, "grid");
  if (!bytes) FAIL(VC_ERR_ARG, "grid_photos_workspace_bytes: null result pointer");
  PhotoPlan pp;
  PhotoBufs pb;
  int64_t front = 0, rest = 0;
  TRY(plan_photos(job, nullptr, pp, pb, &front, e));
  Geo q;
  Bufs b;
  TRY(geo_of(g, &pp.job, q, e));
  TRY(carve(g, q, nullptr, b, &rest, err, errlen));
  *bytes = front + rest;
  return VC_OK;
}

int vc_grid_generate_photos_impl(void* handle, const VcGridPhotos* job, void* workspace, int64_t workspace_bytes, void* const* out_rows,
                                 hipStream_t s, char* err, int errlen) {
  HANDLE(Grid, g, "grid");
  if (!aligned256(workspace)) FAIL(VC_ERR_ARG, "grid_generate_photos: the workspace must be a 256-byte aligned device pointer");
  PhotoPlan pp;
  PhotoBufs pb;
  int64_t front = 0;
  TRY(plan_photos(job, (char*)workspace, pp, pb, &front, e));
  if (workspace_bytes < front) FAIL(VC_ERR_ARG, "grid_generate_photos: workspace too small (%lld < %lld bytes)", (long long)workspace_bytes, (long long)front);
  {                                              // everything vc_grid_generate would refuse, before the device is touched
    Geo q;
    Bufs b;
    TRY(admit(g, &pp.job, pp.job.decode, (char*)workspace + front, workspace_bytes - front, out_rows, q, b, e, "grid_generate_photos"));
  }
  const int gh = job->grid_h, gw = job->grid_w;
  for (int i = 0; i < gh; ++i) {
    const int H = pp.job.height[i], W = pp.job.width[i];
    int x0 = 0;
    for (int k = 0; k < gw; ++k) {
      const int c = i * gw + k;
      const VcCellPlan& p = pp.cells[c];
      if (!p.present) {                          // :339-344 a black cell, to be generated
        TRY(vc_pixels_in_launch(nullptr, 0, 0, 0, 0, pb.rows[i], 0, H, W, x0, p.final_w, s, err, errlen));
      } else {
        // :316,325 LANCZOS to the fitted size, :327-331 bicubic to cover the row's reference size, centre crop
        TRY(vc_resample_u8_launch(job->images[c], job->height[c], job->width[c], pb.fit, p.fit_h, p.fit_w, VC_FILTER_LANCZOS, pb.tmp, pb.tmp_b, s, err, errlen));
        TRY(vc_resample_u8_launch(pb.fit, p.fit_h, p.fit_w, pb.cover, p.cover_h, p.cover_w, VC_FILTER_BICUBIC, pb.tmp, pb.tmp_b, s, err, errlen));
        if (p.final_w == p.cell_w && p.final_h == p.cell_h) {
          TRY(vc_pixels_in_launch(pb.cover, p.cover_h, p.cover_w, p.crop_left, p.crop_top, pb.rows[i], 0, H, W, x0, p.final_w, s, err, errlen));
        } else {                                 // :350-360 the cropped cell resized once more: the crop as bytes first (outside = 0)
          HIP(hipMemsetAsync(pb.cell, 0, (size_t)p.cell_w * p.cell_h * 3, s), "hipMemsetAsync(cell)");
          const int sx = std::max(p.crop_left, 0), sy = std::max(p.crop_top, 0), dx = std::max(-p.crop_left, 0), dy = std::max(-p.crop_top, 0);
          const int cw_ = std::min(p.cover_w - sx, p.cell_w - dx), ch_ = std::min(p.cover_h - sy, p.cell_h - dy);
          if (cw_ > 0 && ch_ > 0)
            HIP(hipMemcpy2DAsync(pb.cell + ((size_t)dy * p.cell_w + dx) * 3, (size_t)p.cell_w * 3, pb.cover + ((size_t)sy * p.cover_w + sx) * 3,
                                 (size_t)p.cover_w * 3, (size_t)cw_ * 3, (size_t)ch_, hipMemcpyDeviceToDevice, s), "hipMemcpy2DAsync(crop)");
          TRY(vc_resample_u8_launch(pb.cell, p.cell_h, p.cell_w, pb.fin, p.final_h, p.final_w, VC_FILTER_BICUBIC, pb.tmp, pb.tmp_b, s, err, errlen));
          TRY(vc_pixels_in_launch(pb.fin, p.final_h, p.final_w, 0, 0, pb.rows[i], 0, H, W, x0, p.final_w, s, err, errlen));
        }
      }
      TRY(vc_mask_fill_launch(pb.masks[i], H, W, x0, p.final_w, p.mask, s, err, errlen));   // :369-374
      x0 += p.final_w;
    }
  }
  return vc_grid_generate_impl(handle, &pp.job, (char*)workspace + front, workspace_bytes - front, out_rows, s, err, errlen);
}

namespace {

struct U8Bufs {
  bf16_t* px[VC_GRID_MAX_ROWS] = {};
  unsigned char* resized = nullptr;
  char* tmp = nullptr;
  int64_t tmp_b = 0;
};

int plan_u8(const VcGridSdeditU8* job, char* base, VcGridSdedit& j, U8Bufs& ub, int64_t* front, Err e) {
  if (!job) FAIL(VC_ERR_ARG, "grid_sdedit_u8: null job");
  if (job->count < 1 || job->count > VC_GRID_MAX_ROWS) FAIL(VC_ERR_ARG, "grid_sdedit_u8: count = %d outside 1..%d", job->count, VC_GRID_MAX_ROWS);
  if (job->cell_h < 1 || job->cell_w < 1 || job->cell_h > 65535 || job->cell_w > 65535)
    FAIL(VC_ERR_ARG, "grid_sdedit_u8: cells of %dx%d pixels, sizes in 1..65535 expected", job->cell_h, job->cell_w);
  const int H = job->height, W = job->width;
  if (H <= 0 || W <= 0 || H % 16 || W % 16 || H >= 65536 || W >= 65536)
    FAIL(VC_ERR_ARG, "grid_sdedit_u8: the target is %dx%d pixels, positive multiples of 16 below 65536 expected", H, W);
  if (!(job->strength >= 0.0) || !(job->strength - job->strength == 0.0)) FAIL(VC_ERR_ARG, "grid_sdedit_u8: strength must be finite and not negative");
  if (job->strength >= 1.0 && job->out_form != VC_PIXELS_U8)
    FAIL(VC_ERR_ARG, "grid_sdedit_u8: strength >= 1 returns the resized 8-bit images: out_form must be VC_PIXELS_U8");
  for (int k = 0; k < job->count; ++k)
    if (!job->pixels[k]) FAIL(VC_ERR_ARG, "grid_sdedit_u8: null pixels of cell %d", k);
  memset(&j, 0, sizeof(j));
  j.count = job->count; j.height = H; j.width = W;
  j.t5_ids = job->t5_ids; j.clip_ids = job->clip_ids; j.t5_len = job->t5_len; j.clip_len = job->clip_len;
  j.seed = job->seed; j.noise_offset = job->noise_offset; j.noise_offset_out = job->noise_offset_out;
  j.guidance = job->guidance; j.n_points = job->n_points; j.method = job->method; j.out_form = job->out_form; j.max_evals = job->max_evals;
  j.strength = job->strength;
  Carver c{base};
  ub = U8Bufs{};
  for (int k = 0; k < job->count; ++k) {
    ub.px[k] = c.take<bf16_t>((int64_t)3 * H * W);
    j.pixels[k] = ub.px[k] ? (const void*)ub.px[k] : (const void*)(uintptr_t)256;
  }
  ub.resized = (unsigned char*)c.bytes((int64_t)3 * H * W);
  ub.tmp_b = tmp_for(job->cell_h, job->cell_w, H, W, VC_FILTER_BICUBIC);
  ub.tmp = c.bytes(ub.tmp_b);
  *front = c.off;
  return VC_OK;
}

}  // namespace

int vc_grid_sdedit_u8_workspace_bytes_impl(void* handle, const VcGridSdeditU8* job, int64_t* bytes, char* err, int errlen) {
  HANDLE(Grid, g, "grid");
  if (!bytes) FAIL(VC_ERR_ARG, "grid_sdedit_u8_workspace_bytes: null result pointer");
  VcGridSdedit j;
  U8Bufs ub;
  int64_t front = 0, rest = 0;
  TRY(plan_u8(job, nullptr, j, ub, &front, e));
  Geo q;
  Bufs b;
  TRY(geo_of(g, &j, q, e));
  TRY(carve(g, q, nullptr, b, &rest, err, errlen));
  *bytes = front + rest;
  return VC_OK;
}

int vc_grid_sdedit_u8_impl(void* handle, const VcGridSdeditU8* job, void* workspace, int64_t workspace_bytes, void* const* out_images,
                           hipStream_t s, char* err, int errlen) {
  HANDLE(Grid, g, "grid");
  if (!aligned256(workspace)) FAIL(VC_ERR_ARG, "grid_sdedit_u8: the workspace must be a 256-byte aligned device pointer");
  VcGridSdedit j;
  U8Bufs ub;
  int64_t front = 0;
  TRY(plan_u8(job, (char*)workspace, j, ub, &front, e));
  if (workspace_bytes < front) FAIL(VC_ERR_ARG, "grid_sdedit_u8: workspace too small (%lld < %lld bytes)", (long long)workspace_bytes, (long long)front);
  {
    Geo q;
    Bufs b;
    TRY(admit(g, &j, nullptr, (char*)workspace + front, workspace_bytes - front, out_images, q, b, e, "grid_sdedit_u8"));
  }
  const int H = j.height, W = j.width;
  if (job->strength >= 1.0) {                    // visualcloze.py:180-182: the resized image goes back as it is
    for (int k = 0; k < j.count; ++k)
      TRY(vc_resample_u8_launch(job->pixels[k], job->cell_h, job->cell_w, out_images[k], H, W, VC_FILTER_BICUBIC, ub.tmp, ub.tmp_b, s, err, errlen));
    if (job->noise_offset_out) *job->noise_offset_out = job->noise_offset;
    return VC_OK;
  }
  for (int k = 0; k < j.count; ++k) {            // :180 Image.resize (bicubic), then ToTensor / Normalize
    TRY(vc_resample_u8_launch(job->pixels[k], job->cell_h, job->cell_w, ub.resized, H, W, VC_FILTER_BICUBIC, ub.tmp, ub.tmp_b, s, err, errlen));
    TRY(vc_pixels_in_launch(ub.resized, H, W, 0, 0, ub.px[k], 0, H, W, 0, W, s, err, errlen));
  }
  return vc_grid_sdedit_impl(handle, &j, (char*)workspace + front, workspace_bytes - front, out_images, s, err, errlen);
}
