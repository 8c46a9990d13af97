// The host rule of the stochastic sampler (vcloze_hip.h: vc_sde_plan): the grid, the method, the diffusion form and the last step ->
// one coefficient row (mode, h, A, Bc, g) and one model time per evaluation.  No device.  The mathematics is the reference's
// (transport/transport.py:252-298, integrators.py:27-49, ICPlan in transport/path.py) for the Linear path and a velocity model, written
// on v(x, t) = -model(x || cond, 1 - t):  D(x, t) = v + w s = A v - Bc x,  A = 1 + w t / (1 - t),  Bc = w / (1 - t).
// Every coefficient is computed in double, operation by operation as written here (transport.sde_plan is the same expressions in
// Python: the tables are equal bit for bit), and rounded once to f32.  Compiled with floating-point contraction off (Makefile).
#include "vcloze_internal.h"
#include <math.h>
#include <string.h>

namespace {

enum Form { CONSTANT, SBDM, SIGMA, LINEAR, DECREASING, INC_DEC, N_FORMS };
const char* const FORM_NAMES[N_FORMS] = {"constant", "SBDM", "sigma", "linear", "decreasing", "inccreasing-decreasing"};

double diffusion(int form, double norm, double t) {
  switch (form) {
    case CONSTANT: return norm;
    case SBDM: return norm * (1.0 - t) / t;
    case SIGMA: case LINEAR: return norm * (1.0 - t);
    case DECREASING: { const double u = norm * cos(M_PI * t) + 1.0; return 0.25 * (u * u); }
    default: { const double s = sin(M_PI * t); return norm * (s * s); }
  }
}

struct Plan {
  float* rows; float* times; int capacity; int n = 0;
  const char* form; char* err; int errlen;
  // one row; `t` is the time it belongs to (the message of a refusal names it)
  int put(int mode, double h, double A, double Bc, double g, double t, bool timed) {
    const float r[VC_SDE_ROW] = {(float)mode, (float)h, (float)A, (float)Bc, (float)g};
    for (int j = 1; j < VC_SDE_ROW; ++j)
      if (!(r[j] - r[j] == 0.0f)) {
        static const char* const what[VC_SDE_ROW] = {"mode", "h", "A", "Bc", "g"};
        snprintf(err, errlen, "sde_plan: the coefficient %s = %g at t = %.9g is not finite with diffusion form '%s' (SBDM needs t > 0 - a "
                              "sample_eps; every form needs t < 1 - a last step, or an end time below 1)", what[j], (double)r[j], t, form);
        return VC_ERR_ARG;
      }
    if (rows) {
      if (n >= capacity) { snprintf(err, errlen, "sde_plan: capacity = %d rows is too small", capacity); return VC_ERR_ARG; }
      memcpy(rows + (size_t)n * VC_SDE_ROW, r, sizeof(r));
    }
    if (times && timed) {
      if (n >= capacity) { snprintf(err, errlen, "sde_plan: capacity = %d times is too small", capacity); return VC_ERR_ARG; }
      times[n] = 1.0f - (float)t;
    }
    ++n;
    return VC_OK;
  }
};

}  // namespace

int vc_sde_plan_impl(const char* method, const char* form_name, double norm, const char* last_step, double last_step_size, const float* t_grid,
                     int32_t n_points, float* rows, float* times, int32_t capacity, int32_t* n_evals, int32_t* n_draws, char* err, int errlen) {
  if (!method || !form_name || !t_grid) { snprintf(err, errlen, "sde_plan: null method / form / t_grid"); return VC_ERR_ARG; }
  const bool heun = !strcmp(method, "Heun");
  if (!heun && strcmp(method, "Euler")) { snprintf(err, errlen, "sde_plan: unknown method '%s' (Euler, Heun)", method); return VC_ERR_ARG; }
  int form = -1;
  for (int i = 0; i < N_FORMS; ++i) if (!strcmp(form_name, FORM_NAMES[i])) form = i;
  if (!strcmp(form_name, "increasing-decreasing")) form = INC_DEC;
  if (form < 0) {
    snprintf(err, errlen, "sde_plan: unknown diffusion form '%s' (constant, SBDM, sigma, linear, decreasing, inccreasing-decreasing)", form_name);
    return VC_ERR_ARG;
  }
  enum { NONE, MEAN, EULER, TWEEDIE } last = NONE;
  if (last_step && *last_step) {
    if (!strcmp(last_step, "Mean")) last = MEAN;
    else if (!strcmp(last_step, "Euler")) last = EULER;
    else if (!strcmp(last_step, "Tweedie")) last = TWEEDIE;
    else { snprintf(err, errlen, "sde_plan: unknown last step '%s' (Mean, Euler, Tweedie, or NULL for none)", last_step); return VC_ERR_ARG; }
  }
  if (n_points < 2) { snprintf(err, errlen, "sde_plan: n_points = %d, at least 2 expected", n_points); return VC_ERR_ARG; }
  for (int i = 1; i < n_points; ++i)
    if (!(t_grid[i] > t_grid[i - 1])) { snprintf(err, errlen, "sde_plan: t_grid must increase strictly (index %d)", i); return VC_ERR_ARG; }
  const int S = n_points - 1;
  Plan p{rows, times, capacity, 0, FORM_NAMES[form], err, errlen};
  auto A = [&](double w, double t) { return 1.0 + w * t / (1.0 - t); };
  auto Bc = [&](double w, double t) { return w / (1.0 - t); };
  auto step_dt = [&](int i) { return (double)(float)(t_grid[i + 1] - t_grid[i]); };
  auto noise = [&](int i) { return sqrt(2.0 * diffusion(form, norm, (double)t_grid[i]) * step_dt(i)); };
  for (int i = 0; i < S; ++i) {
    const double t = t_grid[i], dt = step_dt(i), w = diffusion(form, norm, t);
    int rc;
    if (!heun) rc = p.put(VC_SDE_EM, dt, A(w, t), Bc(w, t), noise(i), t, true);
    else {
      rc = p.put(VC_SDE_HEUN1, dt, A(w, t), Bc(w, t), 0.0, t, true);
      const double t2 = t + dt, w2 = diffusion(form, norm, t2);
      if (rc == VC_OK) rc = p.put(VC_SDE_HEUN2, 0.5 * dt, A(w2, t2), Bc(w2, t2), i + 1 < S ? noise(i + 1) : 0.0, t2, true);
    }
    if (rc != VC_OK) return rc;
  }
  if (last != NONE) {
    const double t1 = t_grid[S], w = diffusion(form, norm, t1);
    const int rc = last == MEAN ? p.put(VC_SDE_LAST, last_step_size, A(w, t1), Bc(w, t1), 0.0, t1, true)
                                : p.put(VC_SDE_LAST, last == EULER ? last_step_size : 1.0 - t1, 1.0, 0.0, 0.0, t1, true);
    if (rc != VC_OK) return rc;
  }
  if (n_evals) *n_evals = p.n;
  if (n_draws) *n_draws = S;
  if (heun) {     // behind the evaluations' rows: draw 0, injected in front of the first evaluation
    const int rc = p.put(VC_SDE_INJECT, 0.0, 0.0, 0.0, noise(0), t_grid[0], false);
    if (rc != VC_OK) return rc;
  }
  return VC_OK;
}
