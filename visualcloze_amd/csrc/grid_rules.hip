// The host rules of one grid (include/vcloze_hip.h: vc_time_grid, vc_grid_tokens, vc_grid_img_ids): the solver's time points as
// transport.solver_time_grid builds them with torch, and the img_ids of packing.prepare_grid.  Host code only, no device, no HIP
// call.  This file is compiled with -ffp-contract=off (Makefile) and says so again below: the only fused multiply-adds are the ones
// written out, where torch's own kernel fuses.
#include "vcloze_internal.h"
#include <math.h>

#pragma STDC FP_CONTRACT OFF

namespace {
bool finite_d(double v) { return v - v == 0.0; }
}  // namespace

int vc_time_grid_impl(int32_t n_points, int32_t n_tokens, double t0, double t1, int32_t do_shift, double time_shifting_factor, float* out,
                      char* err, int errlen) {
#pragma clang fp contract(off)
  if (!out) { snprintf(err, errlen, "time_grid: null out"); return VC_ERR_ARG; }
  if (n_points < 2) { snprintf(err, errlen, "time_grid: n_points = %d, at least 2 time points are needed", n_points); return VC_ERR_ARG; }
  if (n_tokens < 1) { snprintf(err, errlen, "time_grid: n_tokens = %d must be positive", n_tokens); return VC_ERR_ARG; }
  if (!finite_d(t0) || !finite_d(t1) || !finite_d(time_shifting_factor)) {
    snprintf(err, errlen, "time_grid: t0, t1 and time_shifting_factor must be finite");
    return VC_ERR_ARG;
  }
  if (!(t0 < t1)) { snprintf(err, errlen, "time_grid: t0 = %g >= t1 = %g (the ODE sampler has to be in forward time)", t0, t1); return VC_ERR_ARG; }
  // torch.linspace(t0, t1, n) in f32 (RangeFactoriesKernel.cpp): the two-sided formula, each point one fused multiply-add
  const float start = (float)t0, end = (float)t1;
  const float step = (end - start) / (float)(n_points - 1);
  const int halfway = n_points / 2;
  for (int i = 0; i < n_points; ++i)
    out[i] = i < halfway ? fmaf(step, (float)i, start) : fmaf(-step, (float)(n_points - 1 - i), end);
  if (time_shifting_factor != 0.0) {           // t / (t + f - f * t): Tensor + number, number * Tensor, Tensor - Tensor, Tensor / Tensor
    const float f = (float)time_shifting_factor;
    for (int i = 0; i < n_points; ++i) {
      const float t = out[i];
      const float a = t + f;
      const float b = f * t;
      const float d = a - b;
      out[i] = t / d;
    }
  }
  if (do_shift) {                              // time_shift(mu, 1.0, t) with mu = get_lin_function(y1=0.5, y2=1.15)(n_tokens), Python floats
    const double m = (1.15 - 0.5) / (4096.0 - 256.0);
    const double b = 0.5 - m * 256.0;
    const double mx = m * (double)n_tokens;
    const double mu = mx + b;
    const float E = (float)exp(mu);
    for (int i = 0; i < n_points; ++i) {
      const float u = 1.0f - out[i];           // t = 1 - t
      const float q = 1.0f / u;                // 1 / t: reciprocal (times 1)
      const float r = q - 1.0f;                // (1 / t - 1) ** 1.0
      const float den = E + r;
      const float rec = 1.0f / den;            // number / Tensor = reciprocal * number
      const float v = rec * E;
      out[i] = 1.0f - v;
    }
  }
  return VC_OK;
}

int64_t vc_grid_tokens_impl(int32_t rows, const int32_t* lat_h, const int32_t* lat_w, char* err, int errlen) {
  if (rows < 1 || !lat_h || !lat_w) { snprintf(err, errlen, "grid_tokens: rows = %d must be positive and the sizes given", rows); return VC_ERR_ARG; }
  int64_t n = 0;
  for (int j = 0; j < rows; ++j) {
    const int h = lat_h[j], w = lat_w[j];
    if (h <= 0 || w <= 0 || (h | w) & 1 || h >= 65536 || w >= 65536) {
      snprintf(err, errlen, "grid_tokens: row %d has latent size %dx%d, even positive sizes below 65536 expected", j, h, w);
      return VC_ERR_ARG;
    }
    n += (int64_t)(h / 2) * (w / 2);
  }
  if (n > 0x7fffffff) { snprintf(err, errlen, "grid_tokens: %lld tokens do not fit a 32-bit count", (long long)n); return VC_ERR_ARG; }
  return n;
}

int vc_grid_img_ids_impl(int32_t rows, const int32_t* lat_h, const int32_t* lat_w, float* out, char* err, int errlen) {
  if (!out) { snprintf(err, errlen, "grid_img_ids: null out"); return VC_ERR_ARG; }
  const int64_t n = vc_grid_tokens_impl(rows, lat_h, lat_w, err, errlen);
  if (n < 0) return (int)n;
  float* p = out;
  for (int j = 0; j < rows; ++j)
    for (int y = 0; y < lat_h[j] / 2; ++y)
      for (int x = 0; x < lat_w[j] / 2; ++x) {
        *p++ = (float)(j + 1);
        *p++ = (float)y;
        *p++ = (float)x;
      }
  return VC_OK;
}
