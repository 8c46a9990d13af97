// What a solver does with a Flux handle (flux_state.h): ONE trajectory core - the refusals every sampler shares, begin_trajectory and
// replay - and on top of it the fixed-grid loop (vc_flux_sample_begin / _steps / _end), the adaptive solve of an embedded pair (ONE
// loop behind vc_flux_sample_dopri5 and vc_flux_sample_rk, the pair a parameter), the stochastic sampler (vc_flux_sample_sde) and the
// Adams-Bashforth multistep solve (vc_flux_sample_multistep).  An entry point keeps what is its own: its tables, its own refusals and
// its loop.  Host code only; the arithmetic of the tables is flux_rules.h.
#include "flux_state.h"

namespace vcflux {
namespace {

// ---------------------------------------------------------------- the trajectory core
// the shared refusals, `what` the message prefix.  Three groups, because every entry point's own refusals stand between them and
// the first error of a call is part of the ABI's behaviour: the handle and the pointers ...
int refuse_unready(Flux& f, const char* what, const void* x, const void* cond, const float* t_grid, Err e) {
  if (!f.prepared) FAIL(VC_ERR_STATE, "%s: call vc_flux_prepare first", what);
  TRY(fresh_scale(f, what, e.buf, e.len));
  if (!x || !cond || !t_grid) FAIL(VC_ERR_ARG, "%s: null argument", what);
  return VC_OK;
}
// ... the step cache, which only a VC_SOLVER_EULER trajectory runs with (`method`: the caller's VC_SOLVER_* code, which the message
// then names, or NO_SOLVER_CODE where the entry point takes none) ...
constexpr int NO_SOLVER_CODE = -1;
int refuse_cache(Flux& f, const char* what, int method, Err e) {
  if (!f.sc_on()) return VC_OK;
  if (method == NO_SOLVER_CODE)
    FAIL(VC_ERR_ARG, "%s: the step cache works with VC_SOLVER_EULER only: turn it off with vc_flux_set_step_cache(handle, 0, 0)", what);
  if (method != VC_SOLVER_EULER)
    FAIL(VC_ERR_ARG, "%s: the step cache works with VC_SOLVER_EULER only (method %d): turn it off with vc_flux_set_step_cache(handle, 0, 0)", what, method);
  if (f.dbl.empty()) FAIL(VC_ERR_ARG, "%s: the step cache needs at least one double block", what);
  if (!f.ws_cache) FAIL(VC_ERR_STATE, "%s: the step cache was turned on after vc_flux_prepare: ask vc_flux_workspace_bytes and prepare again", what);
  return VC_OK;
}
// ... and true CFG (behind refuse_cache: the cache is on here for a VC_SOLVER_EULER trajectory alone)
int refuse_cfg(Flux& f, const char* what, Err e) {
  if (!f.cfg_on) return VC_OK;
  if (f.B % 2) FAIL(VC_ERR_ARG, "%s: true CFG pairs the first half of the batch with the second: B = %d is odd", what, f.B);
  if (f.sc_on())
    FAIL(VC_ERR_ARG, "%s: true CFG does not work with the step cache: turn one off (vc_flux_set_cfg(handle, 0, 0) / vc_flux_set_step_cache(handle, 0, 0))", what);
  if (!(f.cfg_scale - f.cfg_scale == 0.0f)) FAIL(VC_ERR_ARG, "%s: the cfg_scale set by vc_flux_set_cfg is not finite", what);
  return VC_OK;
}

// the adaptive and the stochastic call overwrite an earlier trajectory's tables: its steps / end / profile refuse from here on
void end_trajectory(Flux& f) {
  f.in_flight = false;
  f.steps_total = f.steps_done = 0;
}

// a trajectory of solver `method` (SOLVER_RK: of the pair `rk`) from the caller's state x begins: the caller's settings are latched (f.traj, true CFG), the state
// and its bf16 shadow, COND and the zeroed counter go in, and with a stream the step is captured.  The caller has put everything
// else the warm-up evaluation of a new capture reads - the modulation rows, its tables - on `s` before
int begin_trajectory(Flux& f, int method, const void* x, int x_is_bf16, const void* cond, hipStream_t s, Err e, int rk = 0) {
  const int64_t rows = (int64_t)f.B * f.N, n = rows * f.cfg.out_channels;
  const bool fixed = vc_evals_of(method) != 0;
  f.traj.method = method; f.traj.evals = fixed ? vc_evals_of(method) : 1;
  f.traj.rk = method == SOLVER_RK ? rk : 0;
  f.traj.state_f32 = !fixed || !x_is_bf16;
  f.traj.cached = f.sc_on();
  f.cfg_active = f.cfg_on; f.cfg_s = f.cfg_on ? f.cfg_scale : 1.0f;
  if (!fixed) {                                 // the f32 state of the solver and its bf16 shadow
    TRY(vc_dopri5_load_launch(x, x_is_bf16, method == SOLVER_RK ? f.AD_Y0 : method == SOLVER_MULTISTEP ? f.MS_Y : f.SD_Y, f.YIN, n, s, e.buf, e.len));
  } else {
    TRY(d2d(ode_state(f), x, ode_state_bytes(f), s, e.buf, e.len));
    // the first evaluation reads bf16(y0)
    if (f.traj.state_f32) TRY(ode_update(f, nullptr, nullptr, s, e.buf, e.len));
    else if (next_input(f) != f.XS) TRY(d2d(next_input(f), f.XS, ode_state_bytes(f), s, e.buf, e.len));
  }
  TRY(d2d(f.COND, cond, rows * (f.cfg.in_channels - f.cfg.out_channels) * 2, s, e.buf, e.len));
  HIP(hipMemsetAsync(f.STEP, 0, sizeof(int32_t), s), "hipMemsetAsync");
  if (s) TRY(step_graph(f, s, e.buf, e.len));
  return VC_OK;
}

// the step (or, cached, piece `piece` of it) once more: its captured graph, or without a stream the launches it was captured from
int replay(Flux& f, hipStream_t s, Err e, int piece = 0) {
  if (!s) return step_piece(f, piece, true, s, e.buf, e.len);
  HIP(hipGraphLaunch(f.step.g[piece], s), "hipGraphLaunch");
  return VC_OK;
}

// ---------------------------------------------------------------- what the solves with tables of their own share
// the refusals: the entry point's workspace option is off or the workspace was prepared without it (`ready`: both hold), and the
// monitor, whose log only a fixed-grid trajectory can index (`why`: the entry point's own sentence)
int refuse_no_buffers(bool ready, const char* what, const char* option, const char* of_what, Err e) {
  if (!ready)
    FAIL(VC_ERR_STATE, "%s: set vc_flux_set_option(handle, \"%s\", 1) before vc_flux_workspace_bytes / vc_flux_prepare "
                       "(the workspace holds no buffers of %s)", what, option, of_what);
  return VC_OK;
}
int refuse_monitor(Flux& f, const char* what, Err e, const char* why = "its log is indexed by the evaluations of a fixed-grid trajectory") {
  if (f.mon_level)
    FAIL(VC_ERR_ARG, "%s: the monitor is on (level %d): %s; turn it off with vc_flux_set_monitor(handle, 0, NULL, 0, NULL)", what, f.mon_level, why);
  return VC_OK;
}

// a staged TS block from one model time per evaluation: tm[j] for each of the B samples of evaluation j
void broadcast_times(const Flux& f, const float* tm, int evals, float* ts) {
  for (int j = 0; j < evals; ++j)
    for (int b = 0; b < f.B; ++b) ts[(size_t)j * f.B + b] = tm[j];
}

// the tail of vc_flux_sample_sde and vc_flux_sample_multistep behind their checks and their plan: the staged tables go out - TS,
// filled here from the plan's `times`, then the solver's own `tabs` (device address, staged copy, bytes) -, the trajectory begins,
// `ahead()` issues what stands in front of the first evaluation, the n_evals evaluations replay and x receives the f32 state Y.
// With a trajectory buffer, row_after(j) names the row that receives Y behind evaluation j - j = -1: ahead of the first one,
// j = n_evals: behind them all once more - or -1 for none.
template <class Ahead, class RowAfter>
int run_tables(Flux& f, int solver, const float* Y, const float* times, float* ts, std::initializer_list<std::tuple<void*, const void*, size_t>> tabs,
               int n_evals, void* x, int state_is_bf16, const void* cond, void* trajectory, Ahead ahead, RowAfter row_after, hipStream_t s, Err e) {
  const int64_t n = (int64_t)f.B * f.N * f.cfg.out_channels, out_bytes = n * (state_is_bf16 ? 2 : 4);
  auto store = [&](int row) {
    return trajectory && row >= 0 ? vc_sde_store_launch(Y, (char*)trajectory + row * out_bytes, state_is_bf16 != 0, n, s, e.buf, e.len) : VC_OK;
  };
  broadcast_times(f, times, n_evals, ts);
  end_trajectory(f);
  TRY(stage_send(f, f.TS, ts, (size_t)n_evals * f.B * sizeof(float), s, e.buf, e.len));
  for (auto [dev, staged, bytes] : tabs) TRY(stage_send(f, dev, staged, bytes, s, e.buf, e.len));
  TRY(stage_end(f, s, e.buf, e.len));
  TRY(time_precompute(f, n_evals, 0, s, e.buf, e.len));
  TRY(begin_trajectory(f, solver, x, state_is_bf16, cond, s, e));
  TRY(ahead());
  for (int j = -1; j <= n_evals; ++j) {
    if (j >= 0 && j < n_evals) TRY(replay(f, s, e));
    TRY(store(row_after(j)));
  }
  return vc_sde_store_launch(Y, x, state_is_bf16 != 0, n, s, e.buf, e.len);
}

}  // namespace
}  // namespace vcflux
using namespace vcflux;

// ---------------------------------------------------------------- the fixed-grid loop
int vc_flux_sample_begin_impl(void* handle, int32_t method, const void* x, const void* cond, const float* t_grid, int32_t n_points,
                              int32_t state_is_bf16, hipStream_t s, char* err, int errlen) {
  HANDLE(Flux, f, "flux");
  const int E = vc_evals_of(method);
  if (!E) FAIL(VC_ERR_ARG, "flux_sample: unknown solver method %d (VC_SOLVER_EULER, VC_SOLVER_MIDPOINT, VC_SOLVER_RK4)", method);
  TRY(refuse_unready(f, "flux_sample", x, cond, t_grid, e));
  const int S = n_points - 1, B = f.B;
  if (S < 1 || (int64_t)S * E > f.S)
    FAIL(VC_ERR_ARG, "flux_sample: %d steps of %d evaluation(s), the prepared workspace holds 1..%d evaluations", S, E, f.S);
  TRY(refuse_cache(f, "flux_sample", method, e));
  TRY(refuse_cfg(f, "flux_sample", e));
  TRY(monitor_fits(f, "flux_sample", e.buf, e.len));
  if (f.mon_level && (int64_t)S * E > f.mon_cap)
    FAIL(VC_ERR_ARG, "flux_sample: %d steps of %d evaluation(s), the monitor's log holds capacity_evals = %d (vc_flux_set_monitor)", S, E, f.mon_cap);
  const bool cached = f.sc_on();
  if (cached && !f.sc_host) HIP(hipHostMalloc((void**)&f.sc_host, 256, hipHostMallocDefault), "hipHostMalloc");
  const int SE = S * E;
  TRY(stage_begin(f, ((size_t)SE * B + S) * sizeof(float) + 512, e.buf, e.len));
  float* ts = stage_take<float>(f, (size_t)SE * B);
  float* dts = stage_take<float>(f, S);
  vcrules::model_times(method, E, t_grid, S, B, state_is_bf16 != 0, ts, dts);
  TRY(stage_send(f, f.TS, ts, (size_t)SE * B * sizeof(float), s, e.buf, e.len));
  TRY(stage_send(f, f.DTS, dts, S * sizeof(float), s, e.buf, e.len));
  TRY(stage_end(f, s, e.buf, e.len));
  TRY(time_precompute(f, SE, 0, s, e.buf, e.len));
  TRY(begin_trajectory(f, method, x, state_is_bf16, cond, s, e));
  // the monitor's log starts zeroed (behind the warm-up evaluation of a new capture, which logs): a kernel, not a memset node
  if (f.mon_level) TRY(vc_zero_fill_launch(f.mon_log, vcmon::log_bytes(f.mon_cap, f.mon_sites(), B), s, e.buf, e.len));
  f.mon_evals = 0;
  // the step cache's run of this trajectory.  No P yet: the first metric is read against zeros (and reported as NaN), never
  // against an earlier trajectory's residual
  f.sc_thr = f.sc_threshold; f.sc_lim = f.sc_max;
  f.sc_have = false; f.sc_run = f.sc_computed = f.sc_reused = 0;
  f.sc_metrics.clear();
  if (cached) HIP(hipMemsetAsync(f.SC_P, 0, (size_t)B * f.N * f.D * 2, s), "hipMemsetAsync");
  f.steps_total = S; f.steps_done = 0;
  f.in_flight = true;
  return VC_OK;
}

// one cached Euler step: head, ONE host read of the metric, the tail the rule picks
static int cached_step(Flux& f, hipStream_t s, Err e) {
  TRY(replay(f, s, e, 0));
  HIP(hipStreamSynchronize(s), "hipStreamSynchronize");
  const float m = *(volatile float*)f.sc_host;
  const bool reuse = f.sc_have && m < f.sc_thr && (f.sc_lim < 0 || f.sc_run < f.sc_lim);
  f.sc_metrics.push_back(f.sc_have ? m : NAN);
  TRY(replay(f, s, e, reuse ? 2 : 1));
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
    for (int j = 0; j < f.traj.evals; ++j) {      // a step = `evals` replays; the stage is the device-side counter modulo evals
      ++f.mon_evals;
      if (f.traj.cached) { TRY(cached_step(f, s, e)); continue; }
      TRY(replay(f, s, e));
      ++f.sc_computed;
    }
    if (trajectory) TRY(d2d((char*)trajectory + (int64_t)i * state_bytes, ode_state(f), state_bytes, s, e.buf, e.len));
    ++f.steps_done;
  }
  return VC_OK;
}

int vc_flux_sample_end_impl(void* handle, void* x_out, hipStream_t s, char* err, int errlen) {
  HANDLE(Flux, f, "flux");
  if (!f.prepared || f.steps_total == 0) FAIL(VC_ERR_STATE, "flux_sample_end: no sample in flight");
  if (!x_out) FAIL(VC_ERR_ARG, "flux_sample_end: null output");
  f.in_flight = false;
  return d2d(x_out, ode_state(f), ode_state_bytes(f), s, e.buf, e.len);
}

// ---------------------------------------------------------------- the adaptive solve (vcloze_hip.h: vc_flux_sample_dopri5, vc_flux_sample_rk)
// ONE loop for every embedded pair: the rows, the stage node, the norm and the dense output take the pair (VC_RK_*), the step-size
// rules its order.  `what` is the entry point's message prefix.  The buffers are the first S of AD_K's seven planes, AD_Y0 / AD_Y1.
// the S modulation rows of a step t -> t + dt (row = the device-side counter = the stage of the evaluation: vcrules::rk_row_times),
// and dt itself
static int rk_rows(Flux& f, int method, double t, double dt, hipStream_t s, Err e) {
  const int B = f.B, S = vcrules::rk_stages(method);
  TRY(stage_begin(f, (size_t)S * B * sizeof(float) + 1024, e.buf, e.len));
  float* ts = stage_take<float>(f, (size_t)S * B);
  float* hdt = stage_take<float>(f, 1);
  float tm[7];
  vcrules::rk_row_times(method, t, dt, tm);
  broadcast_times(f, tm, S, ts);
  *hdt = (float)dt;
  TRY(stage_send(f, f.TS, ts, (size_t)S * B * sizeof(float), s, e.buf, e.len));
  TRY(stage_send(f, f.AD_DT, hdt, sizeof(float), s, e.buf, e.len));
  TRY(stage_end(f, s, e.buf, e.len));
  return time_precompute(f, S, 0, s, e.buf, e.len);
}
// `count` replays of the captured evaluation (+ its stage node) with the counter starting at `first`
static int rk_evals(Flux& f, int first, int count, hipStream_t s, Err e) {
  HIP(hipMemsetD32Async((hipDeviceptr_t)f.STEP, first, 1, s), "hipMemsetD32Async");
  for (int j = 0; j < count; ++j) TRY(replay(f, s, e));
  f.ad_evals += count;
  return VC_OK;
}
// the first `count` words of AD_OUT -> the host: the ONE synchronisation of an attempt
static int rk_read(Flux& f, int count, hipStream_t s, Err e) {
  HIP(hipMemcpyAsync(f.ad_host, f.AD_OUT, count * sizeof(float), hipMemcpyDeviceToHost, s), "hipMemcpyAsync(D2H)");
  HIP(hipStreamSynchronize(s), "hipStreamSynchronize");
  return VC_OK;
}

static int rk_run(Flux& f, const char* what, int method, void* x, const float* t_grid, int n_points, int out_bf16, float rtol, float atol,
                  int max_attempts, void* trajectory, hipStream_t s, Err e) {
  const int64_t n = (int64_t)f.B * f.N * f.cfg.out_channels, out_bytes = n * (out_bf16 ? 2 : 4);
  const int S = vcrules::rk_stages(method), order = vcrules::rk_order(method);
  const volatile float* host = f.ad_host;
  double t = t_grid[0];
  // k1 = f(t0, y0): the counter at 0 stores it (the caller set the rows of t0 with dt = 0: the state the stage node forms is y0)
  TRY(rk_evals(f, 0, 1, s, e));
  // the initial step size
  TRY(vc_rk_error_ratio_launch(method, 1, f.AD_Y0, nullptr, f.AD_K, nullptr, rtol, atol, f.AD_OUT, f.AD_PART, n, s, e.buf, e.len));
  TRY(vc_rk_error_ratio_launch(method, 2, f.AD_Y0, nullptr, f.AD_K, nullptr, rtol, atol, f.AD_OUT + 1, f.AD_PART, n, s, e.buf, e.len));
  TRY(rk_read(f, 2, s, e));
  const double d0 = host[0], d1 = host[1];
  if (d0 != d0 || d1 != d1) FAIL(VC_ERR_STATE, "%s: the state or the model's output at t_grid[0] is not finite", what);
  const double h0 = vcrules::rk_h0(d0, d1);
  TRY(rk_rows(f, method, t, h0, s, e));
  TRY(vc_rk_stage_launch(method, 7, f.AD_Y0, f.AD_K, nullptr, f.AD_DT, nullptr, nullptr, f.YIN, n, s, e.buf, e.len));
  // the probe runs as the LAST stage: its row stands at t0 + h0 (c_S = 1) and its node stores k alone, into k_S
  TRY(rk_evals(f, S - 1, 1, s, e));
  // d2 reads the probe from k2: the slots are free until the first attempt
  if (S - 1 != 1) TRY(d2d(f.AD_K + n, f.AD_K + (int64_t)(S - 1) * n, n * 2, s, e.buf, e.len));
  TRY(vc_rk_error_ratio_launch(method, 3, f.AD_Y0, nullptr, f.AD_K, nullptr, rtol, atol, f.AD_OUT, f.AD_PART, n, s, e.buf, e.len));
  TRY(rk_read(f, 1, s, e));
  const double d2 = (double)host[0] / h0;
  if (d2 != d2) FAIL(VC_ERR_STATE, "%s: the model's output at t_grid[0] + h0 is not finite", what);
  double dt = vcrules::rk_first_dt(order, h0, d1, d2);
  int next_out = 1;
  while (next_out < n_points) {
    if ((int)f.ad_log.size() >= max_attempts)
      FAIL(VC_ERR_STATE, "%s: more than max_attempts = %d attempts (t = %.9g of [%.9g, %.9g], dt = %.3g)", what, max_attempts, t,
           (double)t_grid[0], (double)t_grid[n_points - 1], dt);
    if (t + dt == t) FAIL(VC_ERR_STATE, "%s: the step size underflowed (t = %.17g, dt = %.3g)", what, t, dt);
    TRY(rk_rows(f, method, t, dt, s, e));
    TRY(vc_rk_stage_launch(method, 0, f.AD_Y0, f.AD_K, nullptr, f.AD_DT, nullptr, f.AD_Y1, f.YIN, n, s, e.buf, e.len));   // k1 is in place
    TRY(rk_evals(f, 1, S - 1, s, e));
    TRY(vc_rk_error_ratio_launch(method, 0, f.AD_Y0, f.AD_Y1, f.AD_K, f.AD_DT, rtol, atol, f.AD_OUT, f.AD_PART, n, s, e.buf, e.len));
    TRY(rk_read(f, 1, s, e));
    const float ratio32 = host[0];
    bool accept;
    double factor;
    const bool ok = vcrules::rk_controller(order, ratio32, &accept, &factor);
    f.ad_log.push_back(Flux::Attempt{t, dt, ratio32, accept});
    if (!ok) FAIL(VC_ERR_STATE, "%s: the error ratio of the step at t = %.9g, dt = %.3g is NaN", what, t, dt);
    if (accept) {
      const double t1 = t + dt;
      for (; next_out < n_points && (double)t_grid[next_out] <= t1; ++next_out) {
        const bool last = next_out == n_points - 1;
        if (!trajectory && !last) continue;
        double theta = ((double)t_grid[next_out] - t) / dt;
        theta = theta < 0.0 ? 0.0 : theta > 1.0 ? 1.0 : theta;
        void* dst = trajectory ? (void*)((char*)trajectory + (int64_t)(next_out - 1) * out_bytes) : x;
        TRY(vc_rk_dense_launch(method, f.AD_Y0, f.AD_Y1, f.AD_K, f.AD_DT, (float)theta, dst, out_bf16, n, s, e.buf, e.len));
        if (trajectory && last) TRY(d2d(x, dst, out_bytes, s, e.buf, e.len));
      }
      TRY(d2d(f.AD_Y0, f.AD_Y1, n * 4, s, e.buf, e.len));
      TRY(d2d(f.AD_K, f.AD_K + (int64_t)(S - 1) * n, n * 2, s, e.buf, e.len));        // first same as last
      t = t1;
    }
    dt *= factor;
  }
  return VC_OK;
}

// the refusals of both entry points behind their own first lines, in their order, then the solve
static int rk_solve(Flux& f, const char* what, int method, void* x, const void* cond, const float* t_grid, int n_points, int state_is_bf16,
                    float rtol, float atol, int max_attempts, void* trajectory, hipStream_t s, Err e) {
  const int S = vcrules::rk_stages(method);
  TRY(refuse_unready(f, what, x, cond, t_grid, e));
  TRY(refuse_monitor(f, what, e, "the adaptive solve's device-side counter is the stage of an attempt, not an evaluation index"));
  TRY(refuse_no_buffers(f.opt.adaptive && f.AD_K, what, "adaptive", "the adaptive solve", e));
  if (f.S < S) {                                // (each entry point's own wording)
    if (method == VC_RK_DOPRI5) FAIL(VC_ERR_ARG, "%s: the workspace was prepared with max_steps = %d, the adaptive solve needs 7", what, f.S);
    FAIL(VC_ERR_ARG, "%s: the workspace was prepared with max_steps = %d, method %d needs %d", what, f.S, method, S);
  }
  if (n_points < 2) FAIL(VC_ERR_ARG, "%s: n_points = %d, at least 2 expected", what, n_points);
  for (int i = 1; i < n_points; ++i)
    if (!(t_grid[i] > t_grid[i - 1])) FAIL(VC_ERR_ARG, "%s: t_grid must increase strictly (index %d)", what, i);
  if (!(rtol >= 0.0f) || !(atol >= 0.0f) || !(rtol + atol > 0.0f) || !(rtol + atol - (rtol + atol) == 0.0f))
    FAIL(VC_ERR_ARG, "%s: rtol = %g and atol = %g must be finite, non-negative and not both zero", what, rtol, atol);
  if (max_attempts < 1) FAIL(VC_ERR_ARG, "%s: max_attempts = %d must be positive", what, max_attempts);
  TRY(refuse_cache(f, what, NO_SOLVER_CODE, e));
  TRY(refuse_cfg(f, what, e));
  if (!f.ad_host) HIP(hipHostMalloc((void**)&f.ad_host, 256, hipHostMallocDefault), "hipHostMalloc");
  end_trajectory(f);
  f.ad_log.clear();
  f.ad_evals = 0;
  // the warm-up evaluation of a new capture indexes the modulation rows by the counter and reads dt: both defined first
  TRY(rk_rows(f, method, (double)t_grid[0], 0.0, s, e));
  TRY(begin_trajectory(f, SOLVER_RK, x, state_is_bf16, cond, s, e, method));
  return rk_run(f, what, method, x, t_grid, n_points, state_is_bf16 != 0, rtol, atol, max_attempts, trajectory, s, e);
}

int vc_flux_sample_dopri5_impl(void* handle, void* x, const void* cond, const float* t_grid, int32_t n_points, int32_t state_is_bf16,
                               float rtol, float atol, int32_t max_attempts, void* trajectory, hipStream_t s, char* err, int errlen) {
  HANDLE(Flux, f, "flux");
  return rk_solve(f, "flux_sample_dopri5", VC_RK_DOPRI5, x, cond, t_grid, n_points, state_is_bf16, rtol, atol, max_attempts, trajectory, s, e);
}

// the public route to Dormand-Prince 5(4) is vc_flux_sample_dopri5 alone
int vc_flux_sample_rk_impl(void* handle, int32_t method, void* x, const void* cond, const float* t_grid, int32_t n_points, int32_t state_is_bf16,
                           float rtol, float atol, int32_t max_attempts, void* trajectory, hipStream_t s, char* err, int errlen) {
  HANDLE(Flux, f, "flux");
  if (method == VC_RK_DOPRI5)
    FAIL(VC_ERR_ARG, "flux_sample_rk: VC_RK_DOPRI5 is not solved here: there is one route to Dormand-Prince 5(4), vc_flux_sample_dopri5");
  if (!vcrules::rk_stages(method)) FAIL(VC_ERR_ARG, "flux_sample_rk: unknown method %d (VC_RK_BOSH3, VC_RK_ADAPTIVE_HEUN)", method);
  return rk_solve(f, "flux_sample_rk", method, x, cond, t_grid, n_points, state_is_bf16, rtol, atol, max_attempts, trajectory, s, e);
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
  TRY(refuse_unready(f, "flux_sample_sde", x, cond, t_grid, e));
  TRY(refuse_no_buffers(f.opt.sde && f.SD_Y, "flux_sample_sde", "sde", "the stochastic sampler", e));
  TRY(refuse_monitor(f, "flux_sample_sde", e));
  TRY(refuse_cache(f, "flux_sample_sde", NO_SOLVER_CODE, e));
  int32_t n_evals = 0, n_draws = 0;
  TRY(vc_sde_plan_impl(method, form, norm, last_step, last_step_size, t_grid, n_points, nullptr, nullptr, 0, &n_evals, &n_draws, err, errlen));
  if (n_evals > f.S)
    FAIL(VC_ERR_ARG, "flux_sample_sde: %d evaluations (%d points, method %s), the prepared workspace holds 1..%d evaluations", n_evals, n_points,
         method, f.S);
  TRY(refuse_cfg(f, "flux_sample_sde", e));
  const int B = f.B;
  const int64_t n = (int64_t)B * f.N * f.cfg.out_channels;
  if ((unsigned __int128)offset + (unsigned __int128)n_draws * (unsigned __int128)n > ((unsigned __int128)1 << 64))
    FAIL(VC_ERR_ARG, "flux_sample_sde: offset + draws * n leaves the 64-bit stream position (offset=%llu, %d draws of %lld elements)",
         (unsigned long long)offset, n_draws, (long long)n);
  const bool heun = !strcmp(method, "Heun");
  const int n_rows = n_evals + (heun ? 1 : 0), E = heun ? 2 : 1;
  // ---- the tables of the whole trajectory: model times, coefficient rows, the stream's seed and offset
  TRY(stage_begin(f, ((size_t)n_evals * B + (size_t)n_rows * VC_SDE_ROW + n_evals) * sizeof(float) + 2 * sizeof(uint64_t) + 4 * 256, e.buf, e.len));
  float* ts = stage_take<float>(f, (size_t)n_evals * B);
  float* rows = stage_take<float>(f, (size_t)n_rows * VC_SDE_ROW);
  float* times = stage_take<float>(f, n_evals);
  uint64_t* words = stage_take<uint64_t>(f, 2);
  TRY(vc_sde_plan_impl(method, form, norm, last_step, last_step_size, t_grid, n_points, rows, times, n_rows, nullptr, nullptr, err, errlen));
  words[0] = seed; words[1] = offset;
  // Heun: draw 0 goes in ahead of the first evaluation (the row behind the evaluations' rows)
  auto inject = [&] {
    return heun ? vc_sde_stage_launch(n_evals, f.SD_TAB, f.S + 1, f.SD_Y, nullptr, f.YIN, f.SD_XHAT, f.SD_K1, f.SD_RNG, nullptr, n, s, e.buf, e.len) : VC_OK;
  };
  // x' after every loop step; the last step's result (or, without one, x' again) as the final row
  auto row_after = [&](int j) { return j == n_evals ? n_points - 1 : j >= 0 && j < (n_points - 1) * E && (j + 1) % E == 0 ? j / E : -1; };
  return run_tables(f, heun ? SOLVER_SDE_HEUN : SOLVER_SDE_EULER, f.SD_Y, times, ts,
                    {{f.SD_TAB, rows, (size_t)n_rows * VC_SDE_ROW * sizeof(float)}, {f.SD_RNG, words, 2 * sizeof(uint64_t)}}, n_evals, x,
                    state_is_bf16, cond, trajectory, inject, row_after, s, e);
}

// ---------------------------------------------------------------- the multistep solve (vcloze_hip.h: vc_flux_sample_multistep)
int vc_flux_sample_multistep_impl(void* handle, int32_t order, void* x, const void* cond, const float* t_grid, int32_t n_points,
                                  int32_t state_is_bf16, void* trajectory, hipStream_t s, char* err, int errlen) {
  HANDLE(Flux, f, "flux");
  // ---- every check before the device is touched
  TRY(refuse_unready(f, "flux_sample_multistep", x, cond, t_grid, e));
  TRY(refuse_no_buffers(f.opt.multistep && f.MS_Y, "flux_sample_multistep", "multistep", "the multistep solve", e));
  TRY(refuse_monitor(f, "flux_sample_multistep", e));
  TRY(refuse_cache(f, "flux_sample_multistep", NO_SOLVER_CODE, e));
  int32_t n_evals = 0;
  TRY(vc_ms_plan_impl(order, t_grid, n_points, nullptr, nullptr, 0, &n_evals, err, errlen));
  if (n_evals > f.S)
    FAIL(VC_ERR_ARG, "flux_sample_multistep: %d evaluations (%d points), the prepared workspace holds 1..%d evaluations", n_evals, n_points, f.S);
  TRY(refuse_cfg(f, "flux_sample_multistep", e));
  const int B = f.B;
  // ---- the tables of the whole trajectory: model times and coefficient rows
  TRY(stage_begin(f, ((size_t)n_evals * B + (size_t)n_evals * VC_MS_ROW + n_evals) * sizeof(float) + 3 * 256, e.buf, e.len));
  float* ts = stage_take<float>(f, (size_t)n_evals * B);
  float* rows = stage_take<float>(f, (size_t)n_evals * VC_MS_ROW);
  float* times = stage_take<float>(f, n_evals);
  TRY(vc_ms_plan_impl(order, t_grid, n_points, rows, times, n_evals, nullptr, err, errlen));
  // the start state as row 0, then the state after every step
  return run_tables(f, SOLVER_MULTISTEP, f.MS_Y, times, ts, {{f.MS_TAB, rows, (size_t)n_evals * VC_MS_ROW * sizeof(float)}}, n_evals, x, state_is_bf16,
                    cond, trajectory, [] { return VC_OK; }, [&](int j) { return j < n_evals ? j + 1 : -1; }, s, e);
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
