// The Adams-Bashforth multistep solver (vcloze_hip.h: vc_ms_plan, vc_ms_stage): a fixed-grid, variable-step rule of order 1..4 that
// costs ONE model evaluation per step - the velocities of the last steps are reused.
//   ms_plan   the host rule: the grid and the order -> one row of VC_MS_ROW coefficients and one model time per evaluation.  No device.
//             Every coefficient is computed in double, operation by operation as written here (transport.ms_plan is the same
//             expressions in Python: the tables are equal bit for bit), and rounded once to f32.  Compiled with floating-point
//             contraction off (Makefile).
//   ms_stage  the update: one elementwise pass keyed by the device-side evaluation counter, over the f32 state, the model's bf16
//             output and a ring of VC_MS_HIST past outputs.  Copy-rate kernel (at most 22 bytes read and 14 written per element, a
//             handful of f32 operations): nothing here is tuned beyond 16-byte accesses and a capped grid.  No LDS, no atomics, no
//             waiting on another workgroup.
#include "common.h"
#include "vcloze_internal.h"
#include <string.h>

// ---------------------------------------------------------------- the host rule
// Step i from t_i to t_{i+1} with k = min(order, i + 1) nodes tau_j = t_{i-j}.  In u = (tau - t_i) / h, h = t_{i+1} - t_i, the nodes
// are b_j = (t_{i-j} - t_i) / h (b_0 = 0) and
//   c_{i,j} = h * INT_0^1 PROD_{m != j} (u - b_m) du / PROD_{m != j} (b_j - b_m):
// the numerator is multiplied out factor by factor (m ascending) into monomial coefficients p[d], integrated term by term (d
// ascending), divided by the denominator (a running product, m ascending) and scaled by h.
int vc_ms_plan_impl(int32_t order, const float* t_grid, int32_t n_points, float* rows, float* times, int32_t capacity, int32_t* n_evals,
                    char* err, int errlen) {
  if (order < 1 || order > VC_MS_ROW) { snprintf(err, errlen, "ms_plan: order = %d outside 1..%d", order, VC_MS_ROW); return VC_ERR_ARG; }
  if (!t_grid) { snprintf(err, errlen, "ms_plan: null t_grid"); return VC_ERR_ARG; }
  if (n_points < 2) { snprintf(err, errlen, "ms_plan: n_points = %d, at least 2 expected", n_points); return VC_ERR_ARG; }
  for (int i = 1; i < n_points; ++i)
    if (!(t_grid[i] > t_grid[i - 1])) { snprintf(err, errlen, "ms_plan: t_grid must increase strictly (index %d)", i); return VC_ERR_ARG; }
  const int S = n_points - 1;
  if ((rows || times) && capacity < S) {
    snprintf(err, errlen, "ms_plan: capacity = %d is too small for %d evaluations", capacity, S);
    return VC_ERR_ARG;
  }
  for (int i = 0; i < S; ++i) {
    const int k = order < i + 1 ? order : i + 1;
    const double ti = t_grid[i], h = (double)t_grid[i + 1] - ti;
    double b[VC_MS_ROW];
    for (int m = 0; m < k; ++m) b[m] = ((double)t_grid[i - m] - ti) / h;
    float row[VC_MS_ROW] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int j = 0; j < k; ++j) {
      double p[VC_MS_ROW] = {1.0, 0.0, 0.0, 0.0}, den = 1.0;
      int deg = 0;
      for (int m = 0; m < k; ++m) {
        if (m == j) continue;
        double q[VC_MS_ROW];
        q[deg + 1] = p[deg];
        for (int d = deg; d >= 1; --d) q[d] = p[d - 1] - b[m] * p[d];
        q[0] = -(b[m] * p[0]);
        ++deg;
        for (int d = 0; d <= deg; ++d) p[d] = q[d];
        den = den * (b[j] - b[m]);
      }
      double integral = 0.0;
      for (int d = 0; d <= deg; ++d) integral = integral + p[d] / (double)(d + 1);
      const double c = h * (integral / den);
      row[j] = (float)c;
      if (!(row[j] - row[j] == 0.0f)) {
        snprintf(err, errlen, "ms_plan: the coefficient c[%d][%d] = %g of the step from t = %.9g to %.9g is not finite (order %d)", i, j, c, ti,
                 (double)t_grid[i + 1], order);
        return VC_ERR_ARG;
      }
    }
    if (rows) memcpy(rows + (size_t)i * VC_MS_ROW, row, sizeof(row));
    if (times) times[i] = 1.0f - t_grid[i];
  }
  if (n_evals) *n_evals = S;
  return VC_OK;
}

// ---------------------------------------------------------------- the update
namespace {

constexpr int MS_MAX_BLOCKS = 1024;      // 4 workgroups of 256 per CU of a 256-CU device; the grid-stride loop takes the rest

int grid_for(long total) { return (int)((total + 255) / 256 < MS_MAX_BLOCKS ? (total + 255) / 256 : MS_MAX_BLOCKS); }

struct MsRow { float c0, c1, c2, c3; };
// one element, f32, one operation after the other: the torch expression of transport.multistep_integrate gives the same bits.
// f0..f3 = the drift -v of this evaluation and of the three before it; f_j is read only where c_j != 0
VC_DEV float ms_element(const MsRow& r, float y, float f0, float f1, float f2, float f3) {
#pragma clang fp contract(off)
  float z = r.c0 * f0;
  if (r.c1 != 0.0f) z = z + r.c1 * f1;
  if (r.c2 != 0.0f) z = z + r.c2 * f2;
  float yn = y + z;
  if (r.c3 != 0.0f) yn = yn + r.c3 * f3;
  return yn;
}

// work items: `nvec` chunks of 8 elements (16-byte accesses: the host found every base 16-byte aligned), then the n - 8 nvec single
// elements behind them.  What the row decides (which ring slots are read) is uniform over the grid.  Slot of v_{e-j}: (e - j) mod 3,
// so v_{e-3} lives where v_e goes: every work item reads its elements of that slot BEFORE it stores them, and no other work item
// touches them.  `hist` is read and written through one pointer (not __restrict__)
__global__ __launch_bounds__(256) void ms_stage_kernel(int eval_arg, const float* __restrict__ table, int n_rows, float* __restrict__ y,
                                                       const bf16_t* __restrict__ v, bf16_t* hist, bf16_t* __restrict__ y_in,
                                                       const int* __restrict__ eval_ptr, long n, long nvec) {
  const int ev = eval_arg >= 0 ? eval_arg : *eval_ptr;
  if (ev < 0 || ev >= n_rows) return;                // a counter outside the table: nothing is read or written
  const float* row = table + (long)ev * VC_MS_ROW;
  const MsRow r{row[0], row[1], row[2], row[3]};
  const bool rd1 = r.c1 != 0.0f, rd2 = r.c2 != 0.0f, rd3 = r.c3 != 0.0f;
  const int s0 = ev % VC_MS_HIST;                    // v_e goes here; v_{e-3} is here until then
  const bf16_t* h1 = hist + (long)((ev + 2) % VC_MS_HIST) * n;      // v_{e-1}
  const bf16_t* h2 = hist + (long)((ev + 1) % VC_MS_HIST) * n;      // v_{e-2}
  bf16_t* h3 = hist + (long)s0 * n;                                 // v_{e-3}, then v_e
  const long total = nvec + (n - nvec * 8);
  for (long wi = blockIdx.x * 256L + threadIdx.x; wi < total; wi += gridDim.x * 256L) {
    if (wi < nvec) {
      const long i = wi * 8;
      const f32x4 ya = *(const f32x4*)(y + i), yb = *(const f32x4*)(y + i + 4);
      const u32x4 v0 = *(const u32x4*)(v + i);
      u32x4 v1 = {0, 0, 0, 0}, v2 = {0, 0, 0, 0}, v3 = {0, 0, 0, 0};
      if (rd1) v1 = *(const u32x4*)(h1 + i);
      if (rd2) v2 = *(const u32x4*)(h2 + i);
      if (rd3) v3 = *(const u32x4*)(h3 + i);
      f32x4 yo[2];
      float in8[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const bool hi = e & 1;
        const int w = e >> 1;
        // the drift's sign: exact
        const float f0 = -(hi ? hi_bf(v0[w]) : lo_bf(v0[w])), f1 = -(hi ? hi_bf(v1[w]) : lo_bf(v1[w]));
        const float f2 = -(hi ? hi_bf(v2[w]) : lo_bf(v2[w])), f3 = -(hi ? hi_bf(v3[w]) : lo_bf(v3[w]));
        const float yn = ms_element(r, e < 4 ? ya[e & 3] : yb[e & 3], f0, f1, f2, f3);
        yo[e >> 2][e & 3] = yn; in8[e] = yn;
      }
      *(f32x4*)(y + i) = yo[0]; *(f32x4*)(y + i + 4) = yo[1];
      *(u32x4*)(h3 + i) = v0;                        // behind the read of v_{e-3} above
      u32x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = pack2bf(in8[2 * e], in8[2 * e + 1]);
      *(u32x4*)(y_in + i) = o;
    } else {
      const long i = nvec * 8 + (wi - nvec);
      const bf16_t vi = v[i];
      const float f1 = rd1 ? -bf2f(h1[i]) : 0.0f, f2 = rd2 ? -bf2f(h2[i]) : 0.0f, f3 = rd3 ? -bf2f(h3[i]) : 0.0f;
      const float yn = ms_element(r, y[i], -bf2f(vi), f1, f2, f3);
      y[i] = yn;
      h3[i] = vi;                                    // behind the read of v_{e-3} above
      y_in[i] = f2bf(yn);
    }
  }
}

}  // namespace

int vc_ms_stage_launch(int eval, const float* table, int n_rows, float* y, const void* v, void* hist, void* y_in, const int32_t* eval_ptr,
                       int64_t n, hipStream_t s, char* err, int errlen) {
  if (!table || !y || !v || !hist || !y_in || n <= 0 || n_rows <= 0 || eval >= n_rows || (eval < 0 && !eval_ptr)) {
    snprintf(err, errlen, "ms_stage: bad args (table, y, v, hist, y_in required; n, n_rows >= 1; eval in [0, n_rows), or < 0 with the evaluation "
                          "counter; eval=%d n_rows=%d n=%lld)", eval, n_rows, (long long)n);
    return VC_ERR_ARG;
  }
  if (((uintptr_t)table | (uintptr_t)y | (uintptr_t)eval_ptr) & 3 || ((uintptr_t)v | (uintptr_t)hist | (uintptr_t)y_in) & 1) {
    snprintf(err, errlen, "ms_stage: every buffer must be aligned to its elements (F32 / the counter: 4 bytes, bf16: 2)");
    return VC_ERR_ARG;
  }
  // the ring's planes start n elements apart: all three are 16-byte aligned only where n % 8 == 0
  const bool vec = n % 8 == 0 && !(((uintptr_t)y | (uintptr_t)v | (uintptr_t)hist | (uintptr_t)y_in) & 15);
  const long nvec = vec ? (long)(n / 8) : 0;
  hipLaunchKernelGGL(ms_stage_kernel, dim3(grid_for(nvec + (n - nvec * 8))), dim3(256), 0, s, eval, table, n_rows, y, (const bf16_t*)v,
                     (bf16_t*)hist, (bf16_t*)y_in, (const int*)eval_ptr, (long)n, nvec);
  return vc_launch_status("ms_stage launch", err, errlen);
}
