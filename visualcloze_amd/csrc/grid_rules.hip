// The host rules of one grid (include/vcloze_hip.h: vc_time_grid, vc_grid_tokens, vc_grid_img_ids): the solver's time points as
// transport.solver_time_grid builds them with torch, and the img_ids of packing.prepare_grid.  Host code only, no device, no HIP
// call.  This file is compiled with -ffp-contract=off (Makefile) and says so again below: the only fused multiply-adds are the ones
// written out, where torch's own kernel fuses.
#include "vcloze_internal.h"
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>

#pragma STDC FP_CONTRACT OFF

namespace {
bool finite_d(double v) { return v - v == 0.0; }
// time_shift(mu, 1.0, t) of transport/utils.py in torch's f32 operations, mu = get_lin_function(y1=0.5, y2=1.15)(n_tokens) in Python
// floats: E = f32(exp(mu)); the endpoints 0 and 1 go through inf arithmetic as the reference's do
float shift_exp(int32_t n_tokens) {
#pragma clang fp contract(off)
  const double m = (1.15 - 0.5) / (4096.0 - 256.0);
  const double b = 0.5 - m * 256.0;
  const double mx = m * (double)n_tokens;
  const double mu = mx + b;
  return (float)exp(mu);
}
float shift_f32(float E, float t) {
#pragma clang fp contract(off)
  const float u = 1.0f - t;                // t = 1 - t
  const float q = 1.0f / u;                // 1 / t: reciprocal (times 1)
  const float r = q - 1.0f;                // (1 / t - 1) ** 1.0
  const float den = E + r;
  const float rec = 1.0f / den;            // number / Tensor = reciprocal * number
  const float v = rec * E;
  return 1.0f - v;
}
// "<number>" up to `end`: digits, sign, point and exponent only (what Python's float() and strtod read alike), finite
bool plain_number(const char* p, const char* end, double* v) {
  if (p == end || end - p > 63) return false;
  char buf[64];
  for (const char* c = p; c < end; ++c)
    if (!((*c >= '0' && *c <= '9') || *c == '+' || *c == '-' || *c == '.' || *c == 'e' || *c == 'E')) return false;
  memcpy(buf, p, (size_t)(end - p));
  buf[end - p] = 0;
  char* stop = nullptr;
  *v = strtod(buf, &stop);
  return stop == buf + (end - p) && finite_d(*v);
}
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
    const float E = shift_exp(n_tokens);
    for (int i = 0; i < n_points; ++i) out[i] = shift_f32(E, out[i]);
  }
  return VC_OK;
}

// Transport.sample's training times (transport.py:107-129) for Linear + velocity - check_interval gives (0, 1) - from the caller's
// base draws, in torch's f32 operations: "uniform" t = u * f32(t1 - t0) + f32(t0) with (t0, t1) = (0, 1) or "uniform_<t0>_<t1>";
// "lognorm" t = 1 / (1 + exp(-u)) * 1 + 0, the exponential taken in double and rounded once to f32 (the correctly rounded f32
// exponential; torch's vectorised one is within an ulp of it); then time_shift with do_shift
int vc_fm_times_impl(const char* snr_type, const float* base, int32_t n, int32_t n_tokens, int32_t do_shift, float* out, char* err, int errlen) {
#pragma clang fp contract(off)
  if (!snr_type || !base || !out) { snprintf(err, errlen, "fm_times: null snr_type / base / out"); return VC_ERR_ARG; }
  if (n <= 0) { snprintf(err, errlen, "fm_times: n = %d must be positive", n); return VC_ERR_ARG; }
  if (n_tokens < 1) { snprintf(err, errlen, "fm_times: n_tokens = %d must be positive", n_tokens); return VC_ERR_ARG; }
  double t0 = 0.0, t1 = 1.0;
  bool lognorm = false;
  if (!strcmp(snr_type, "lognorm")) lognorm = true;
  else if (!strncmp(snr_type, "uniform_", 8)) {
    const char* a = snr_type + 8;
    const char* mid = strchr(a, '_');
    if (!mid || strchr(mid + 1, '_') || !plain_number(a, mid, &t0) || !plain_number(mid + 1, mid + 1 + strlen(mid + 1), &t1)) {
      snprintf(err, errlen, "fm_times: snr_type '%.64s' is not 'uniform_<t0>_<t1>' with two finite numbers", snr_type);
      return VC_ERR_ARG;
    }
  } else if (strcmp(snr_type, "uniform")) {
    snprintf(err, errlen, "fm_times: Not implemented snr_type '%.64s' ('uniform', 'uniform_<t0>_<t1>', 'lognorm')", snr_type);
    return VC_ERR_ARG;
  }
  const float scale = (float)(t1 - t0), shift = (float)t0;
  for (int i = 0; i < n; ++i) {
    float v = base[i];
    if (lognorm) {
      const float neg = -v;
      const float ex = (float)exp((double)neg);
      const float den = 1.0f + ex;
      v = 1.0f / den;
    }
    const float m = v * scale;
    out[i] = m + shift;
  }
  if (do_shift) {
    const float E = shift_exp(n_tokens);
    for (int i = 0; i < n; ++i) out[i] = shift_f32(E, out[i]);
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

// ---- the photo front end's size rules (include/vcloze_hip.h: vc_fit_size, vc_grid_layout, vc_upsampling_size): Python's float and
// integer arithmetic of visualcloze.py:28-75,298-360,166-180 restated - doubles, truncation by (int), floor division where Python floors
namespace {
int floordiv2(int v) { return v >= 0 ? v / 2 : -((-v + 1) / 2); }
bool side_ok(int v) { return v >= 1 && v <= 65535; }
void fit_size(int w, int h, int resolution, int* nw, int* nh) {
#pragma clang fp contract(off)
  const double ar = (double)w / (double)h;
  const double area = (double)resolution * (double)resolution;
  const int new_h = (int)pow(area / ar, 0.5);
  const int new_w = (int)((double)new_h * ar);
  *nw = std::max(new_w / 16, 1) * 16;
  *nh = std::max(new_h / 16, 1) * 16;
}
}  // namespace

int vc_fit_size_impl(int32_t w, int32_t h, int32_t resolution, int32_t* nw, int32_t* nh, char* err, int errlen) {
  if (!nw || !nh) { snprintf(err, errlen, "fit_size: null result pointer"); return VC_ERR_ARG; }
  if (!side_ok(w) || !side_ok(h) || !side_ok(resolution)) {
    snprintf(err, errlen, "fit_size: size %dx%d and resolution %d must lie in 1..65535", w, h, resolution);
    return VC_ERR_ARG;
  }
  int a, b;
  fit_size(w, h, resolution, &a, &b);
  if (!side_ok(a) || !side_ok(b)) { snprintf(err, errlen, "fit_size: %dx%d at resolution %d gives %dx%d, outside 1..65535", w, h, resolution, a, b); return VC_ERR_ARG; }
  *nw = a;
  *nh = b;
  return VC_OK;
}

int vc_grid_layout_impl(int32_t grid_h, int32_t grid_w, const int32_t* cell_w, const int32_t* cell_h, int32_t resolution, VcCellPlan* out,
                        char* err, int errlen) {
#pragma clang fp contract(off)
  if (!cell_w || !cell_h || !out) { snprintf(err, errlen, "grid_layout: null pointer"); return VC_ERR_ARG; }
  if (grid_h < 1 || grid_h > VC_GRID_MAX_ROWS || grid_w < 1 || grid_w > VC_GRID_MAX_ROWS) {
    snprintf(err, errlen, "grid_layout: a grid of %dx%d cells, 1..%d rows and columns expected", grid_h, grid_w, VC_GRID_MAX_ROWS);
    return VC_ERR_ARG;
  }
  if (!side_ok(resolution)) { snprintf(err, errlen, "grid_layout: resolution %d must lie in 1..65535", resolution); return VC_ERR_ARG; }
  const int n = grid_h * grid_w;
  for (int c = 0; c < n; ++c) {
    const bool absent = cell_w[c] == 0 && cell_h[c] == 0;
    if (!absent && (!side_ok(cell_w[c]) || !side_ok(cell_h[c]))) {
      snprintf(err, errlen, "grid_layout: cell %d is %dx%d, sizes in 1..65535 or 0x0 for an absent image expected", c, cell_w[c], cell_h[c]);
      return VC_ERR_ARG;
    }
    if (absent && c < n - grid_w) { snprintf(err, errlen, "grid_layout: cell %d is absent: every image of the in-context rows is needed", c); return VC_ERR_ARG; }
  }
  std::vector<VcCellPlan> plan((size_t)n);
  int target_w = 0, masked = 0;
  for (int i = 0; i < grid_h; ++i) {
    int ref_w = 0, ref_h = 0;
    for (int j = 0; j < grid_w && !ref_w; ++j)
      if (cell_w[i * grid_w + j]) fit_size(cell_w[i * grid_w + j], cell_h[i * grid_w + j], resolution, &ref_w, &ref_h);
    if (i == grid_h - 1) target_w = ref_w;
    for (int j = 0; j < grid_w; ++j) {
      const int c = i * grid_w + j;
      VcCellPlan p;
      memset(&p, 0, sizeof(p));
      if (cell_w[c]) {
        p.present = 1;
        fit_size(cell_w[c], cell_h[c], resolution, &p.fit_w, &p.fit_h);
        if (p.fit_w <= p.fit_h) {
          p.cover_w = ref_w;
          p.cover_h = (int)((double)ref_w / (double)p.fit_w * (double)p.fit_h);
        } else {
          p.cover_w = (int)((double)ref_h / (double)p.fit_h * (double)p.fit_w);
          p.cover_h = ref_h;
        }
        p.crop_left = floordiv2(p.cover_w - ref_w);
        p.crop_top = floordiv2(p.cover_h - ref_h);
        p.cell_w = ref_w;
        p.cell_h = ref_h;
        if (!side_ok(p.fit_w) || !side_ok(p.fit_h) || !side_ok(p.cover_w) || !side_ok(p.cover_h)) {
          snprintf(err, errlen, "grid_layout: cell %d resizes to %dx%d, then %dx%d: outside 1..65535", c, p.fit_w, p.fit_h, p.cover_w, p.cover_h);
          return VC_ERR_ARG;
        }
      } else {
        p.cell_w = ref_w ? ref_w : resolution;
        p.cell_h = ref_w ? ref_h : resolution;
        p.mask = 1;
        ++masked;
      }
      p.final_w = p.cell_w;
      p.final_h = p.cell_h;
      plan[c] = p;
    }
  }
  if (grid_w > 1 && masked > 1) {                 // the second pass over EVERY cell, new_w running from cell to cell
    int new_w = target_w ? target_w : 384;
    for (int c = 0; c < n; ++c) {
      int new_h = (int)((double)plan[c].cell_h * ((double)new_w / (double)plan[c].cell_w));
      new_w = (int)((double)new_w / 16.0) * 16;
      new_h = (int)((double)new_h / 16.0) * 16;
      if (!side_ok(new_w) || !side_ok(new_h)) {
        snprintf(err, errlen, "grid_layout: the second pass resizes cell %d to %dx%d: outside 1..65535", c, new_w, new_h);
        return VC_ERR_ARG;
      }
      plan[c].final_w = new_w;
      plan[c].final_h = new_h;
    }
  }
  // A row is ONE tensor: its cells must agree in height (the reference's torch.cat fails otherwise) - and in width, because the
  // reference sizes every cell's mask by the row's FIRST cell (:369-371), so with unequal widths its mask would not fit its row.
  // Neither can happen with the rules above as they stand (new_w is a multiple of 16 from the first cell on); the check guards them.
  for (int i = 0; i < grid_h; ++i)
    for (int j = 1; j < grid_w; ++j) {
      const VcCellPlan &a = plan[i * grid_w], &b = plan[i * grid_w + j];
      if (a.final_h != b.final_h || a.final_w != b.final_w) {
        snprintf(err, errlen, "grid_layout: row %d holds cells of %dx%d and %dx%d: they do not make one row tensor", i, a.final_w, a.final_h, b.final_w, b.final_h);
        return VC_ERR_ARG;
      }
    }
  memcpy(out, plan.data(), (size_t)n * sizeof(VcCellPlan));
  return VC_OK;
}

int vc_upsampling_size_impl(int32_t orig_w, int32_t orig_h, int32_t* w, int32_t* h, char* err, int errlen) {
#pragma clang fp contract(off)
  if (!w || !h) { snprintf(err, errlen, "upsampling_size: null result pointer"); return VC_ERR_ARG; }
  const bool none = orig_w == 0 && orig_h == 0;
  if (!none && (!side_ok(orig_w) || !side_ok(orig_h))) {
    snprintf(err, errlen, "upsampling_size: size %dx%d, sizes in 1..65535 or 0x0 for none expected", orig_w, orig_h);
    return VC_ERR_ARG;
  }
  int tw = none ? 1024 : orig_w, th = none ? 1024 : orig_h;
  if ((int64_t)tw * th > 1024 * 1024) {
    const double ar = (double)tw / (double)th;
    const int new_h = (int)pow((double)(1024 * 1024) / ar, 0.5);
    tw = (int)((double)new_h * ar);
    th = new_h;
  }
  *w = tw / 16 * 16;
  *h = th / 16 * 16;
  return VC_OK;
}
