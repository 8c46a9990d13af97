// The host arithmetic of the Flux handle, every rule written once: the RoPE and frequency tables of vc_flux_prepare, the model times
// of the fixed-grid and the adaptive solve, the adaptive solve's step-size rules, the logit bounds and the tap-name parser.  Host code
// only, nothing from HIP: flux_engine.hip, flux_weights.hip and flux_sample.hip call it, tests/c_abi/flux_rules_check.cpp runs it
// alone under the sanitizers and tests/test_flux_rules_cpu.py holds what it prints to the Python restatements, bit for bit.
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <unordered_map>
#include <vector>
#include "monitor_sites.h"

// stage_times: no multiply-add may be contracted.  The library's compiler takes the pragma; under another one (the host check is
// built with g++) the volatile temporaries alone hold every product to its own rounding
#if defined(__clang__)
#define VCRULES_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define VCRULES_NO_CONTRACT
#endif

namespace vcrules {

inline float bf16_round(float v) {   // round-to-nearest-even through bf16 (finite inputs)
  uint32_t u;
  memcpy(&u, &v, 4);
  u += 0x7fffu + ((u >> 16) & 1u);
  u &= 0xffff0000u;
  memcpy(&v, &u, 4);
  return v;
}

// ---- vc_flux_prepare's tables
// RoPE angles in float64 exactly as math.py:102-109, stored as (cos, sin) f32 per (token, pair): rope [B * (T + N)][64][2], text rows
// first.  Position ids ([B, T, 3] / [B, N, 3]) take few distinct values per axis (grid rows / columns), so cos / sin are evaluated
// once per (axis, value, frequency).
inline void rope_table(const int32_t axes_dim[3], double theta, int B, int T, int N, const float* txt_ids, const float* img_ids, float* rope) {
  const int L = T + N;
  int pair0 = 0;
  std::vector<float> table;
  std::vector<int> slot((size_t)B * L);
  for (int ax = 0; ax < 3; ++ax) {
    const int half = axes_dim[ax] / 2, d = axes_dim[ax];
    std::unordered_map<float, int> seen;
    std::vector<float> values;
    for (int b = 0; b < B; ++b)
      for (int r = 0; r < L; ++r) {
        const float id = r < T ? txt_ids[((size_t)b * T + r) * 3 + ax] : img_ids[((size_t)b * N + (r - T)) * 3 + ax];
        auto it = seen.find(id);
        if (it == seen.end()) { it = seen.emplace(id, (int)values.size()).first; values.push_back(id); }
        slot[(size_t)b * L + r] = it->second;
      }
    table.resize(values.size() * (size_t)half * 2);
    for (int j = 0; j < half; ++j) {
      const double omega = 1.0 / pow(theta, (double)(2 * j) / (double)d);
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
// layers.py:41-43: exp(-ln(10000) * k / 128), the argument formed in f32 as torch forms it
inline void timestep_freqs(float freqs[128]) {
  for (int k = 0; k < 128; ++k) freqs[k] = (float)exp((double)((float)(-log(10000.0)) * (float)k / 128.0f));
}

// ---- the fixed-grid solve
// the f32 times of the `evals` evaluations of the step t0 -> t1 (dt = t1 - t0), each formed in f32 operation by operation as
// torch forms `t0 + half_dt`, `t0 + dt * (1/3)`, `t0 + dt * (2/3)` from 0-dim f32 tensors (no contraction into a fused multiply-add)
inline void stage_times(int method, float t0, float t1, float dt, float* out) {
  VCRULES_NO_CONTRACT
  out[0] = t0;
  if (method == VC_SOLVER_MIDPOINT) {
    volatile float half_dt = 0.5f * dt;
    out[1] = t0 + half_dt;
  } else if (method == VC_SOLVER_RK4) {
    volatile float a = dt * (float)(1.0 / 3.0), b = dt * (float)(2.0 / 3.0);
    out[1] = t0 + a; out[2] = t0 + b; out[3] = t1;
  }
}
// the tables of a trajectory over t_grid[0..S] with E evaluations per step: dts [S], and ts [S * E][B], the time the model sees at
// every evaluation for every sample
inline void model_times(int method, int E, const float* t_grid, int S, int B, bool state_bf16, float* ts, float* dts) {
  for (int i = 0; i < S; ++i) {
    dts[i] = t_grid[i + 1] - t_grid[i];   // fixed grid: dt = t1 - t0 in f32
    float te[4];
    stage_times(method, t_grid[i], t_grid[i + 1], dts[i], te);
    for (int j = 0; j < E; ++j) {
      // the drift sees t in the state's dtype (torchdiffeq _PerturbFunc); the model sees 1 - t (transport.py:384)
      const float tm = 1.0f - (state_bf16 ? bf16_round(te[j]) : te[j]);
      for (int b = 0; b < B; ++b) ts[((size_t)i * E + j) * B + b] = tm;
    }
  }
}

// ---- the adaptive solve of an embedded pair (vc_flux_sample_dopri5, vc_flux_sample_rk; transport.rk_initial_step / rk_controller are
// the same rules in Python, dopri5_initial_step / dopri5_controller those at order 5): the pair's tableau and order are parameters.
// The controller is torchdiffeq's as recalled, unpinned against real torchdiffeq
// evaluations k1..kS of a step (kS = f(t1, y1) is the next step's k1), model evaluations per attempt (2 more start a solve: k1 and
// the probe of the first step size) and the order the step-size rules take; 0 for an unknown method
inline int rk_stages(int method) { return method == VC_RK_DOPRI5 ? 7 : method == VC_RK_BOSH3 ? 4 : method == VC_RK_ADAPTIVE_HEUN ? 3 : 0; }
inline int rk_evals_per_attempt(int method) { return rk_stages(method) ? rk_stages(method) - 1 : 0; }
inline int rk_order(int method) { return method == VC_RK_DOPRI5 ? 5 : method == VC_RK_BOSH3 ? 3 : method == VC_RK_ADAPTIVE_HEUN ? 2 : 0; }
// the times of the rk_stages(method) modulation rows of a step t -> t + dt (row = the stage of the evaluation): k1's own (its
// evaluation is the last step's last), then c2.. and t + dt again for kS; the model sees 1 - f32(t)
inline void rk_row_times(int method, double t, double dt, float* out) {
  static const double C[3][7] = {{0.0, 1.0 / 5.0, 3.0 / 10.0, 4.0 / 5.0, 8.0 / 9.0, 1.0, 1.0}, {0.0, 1.0 / 2.0, 3.0 / 4.0, 1.0}, {0.0, 1.0, 1.0}};
  for (int j = 0; j < rk_stages(method); ++j) out[j] = 1.0f - (float)(t + C[method][j] * dt);
}
// Hairer's starting step size, split at its two host reads: h0 from d0 = rms(y0 / scale) and d1 = rms(f0 / scale); the first dt
// from h0, d1 and d2 = rms((f(t0 + h0) - f0) / scale) / h0
inline double rk_h0(double d0, double d1) { return (d0 < 1e-5 || d1 < 1e-5) ? 1e-6 : 0.01 * d0 / d1; }
inline double rk_first_dt(int order, double h0, double d1, double d2) {
  const double dmax = d1 > d2 ? d1 : d2;
  const double h1 = dmax <= 1e-15 ? std::max(1e-6, h0 * 1e-3) : pow(0.01 / dmax, 1.0 / order);
  return std::min(100.0 * h0, h1);
}
// the controller behind an attempt of error ratio `ratio`: accepted iff ratio <= 1, and the factor the next dt takes; false (the
// attempt stands as not accepted) for a NaN ratio, which ends the solve
inline bool rk_controller(int order, double ratio, bool* accept, double* factor) {
  *accept = ratio <= 1.0;
  *factor = 10.0;
  if (ratio != ratio) return false;
  if (ratio != 0.0) *factor = std::min(10.0, std::max(0.9 / pow(ratio, 1.0 / order), ratio < 1.0 ? 1.0 : 0.2));
  return true;
}

// ---- the logit bounds of the bounded softmax
// max |scale| of a QK-norm scale vector (128 bf16), as a double; 1e30 where one is NaN (no bound: the running-max template)
inline double scale_absmax(const uint16_t h[128]) {
  double out = 0;
  bool nan = false;
  for (int i = 0; i < 128; ++i) {
    uint32_t u = (uint32_t)h[i] << 16;
    float v;
    memcpy(&v, &u, 4);
    const double a = v < 0 ? -(double)v : (double)v;
    if (a != a) nan = true;
    else if (a > out) out = a;
  }
  return nan ? 1e30 : out;
}
// |q|, |k| <= sqrt(128) max|scale| after QKNorm (RoPE is a rotation), so |128^-0.5 log2(e) q.k| <= this; + 2 % for the six bf16
// roundings on the way (model.py / engine.py compute the same number for the Python-ordered plan)
inline float logit_bound_of(double qmax, double kmax) { return (float)(1.02 * 11.313708498984761 * 1.4426950408889634 * qmax * kmax); }
// the cap Flux.prepare / Flux.handle() hand over: the largest per-block bound over the maxima of the scale vectors in state_dict
// order - a double block's four (query, key of img, then of txt), then a single block's two; 1e30 for a block with a NaN scale
inline float logit_cap(const float* mx, int n_scales, int depth) {
  float cap = 0.0f;
  for (int i = 0; i < n_scales;) {
    const int per = i < 4 * depth ? 4 : 2;
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
  return cap;
}
// ... in thousandths, rounded up (option logit_bound_milli); 0 (no bounded softmax anywhere) where the cap leaves the option's range
inline int logit_cap_milli(float cap) { return cap > 0.0f && cap < 2e6f ? (int)ceil((double)cap * 1000.0) : 0; }

// ---- "img_in", "txt_in", "double.{i}.img", "double.{i}.txt", "single.{i}" -> the tap's index (monitor_sites.h)
enum TapName { TAP_OK = 0, TAP_NO_DOUBLE, TAP_NO_SINGLE, TAP_UNKNOWN };   // TAP_NO_*: a block the model does not have
inline TapName tap_index(const char* name, int depth, int depth_single, size_t* idx) {
  int i = -1, n = 0;
  char st[4] = "";
  if (!strcmp(name, "img_in")) { *idx = (size_t)vcmon::tap_img_in(); return TAP_OK; }
  if (!strcmp(name, "txt_in")) { *idx = (size_t)vcmon::tap_txt_in(); return TAP_OK; }
  if (sscanf(name, "double.%d.%3[a-z]%n", &i, st, &n) == 2 && !name[n] && i >= 0 && (!strcmp(st, "img") || !strcmp(st, "txt"))) {
    if (i >= depth) return TAP_NO_DOUBLE;
    *idx = (size_t)vcmon::tap_double(i, st[0] == 't');
    return TAP_OK;
  }
  n = 0;
  if (sscanf(name, "single.%d%n", &i, &n) == 1 && !name[n] && i >= 0) {
    if (i >= depth_single) return TAP_NO_SINGLE;
    *idx = (size_t)vcmon::tap_single(depth, i);
    return TAP_OK;
  }
  return TAP_UNKNOWN;
}
// the rows of tap `idx` per sample: N and T alternate (img_in, txt_in, then img / txt of every double block), L behind them
inline int tap_rows(size_t idx, int depth, int T, int N) { return idx >= (size_t)vcmon::tap_single(depth, 0) ? T + N : idx % 2 ? T : N; }

}  // namespace vcrules
