// csrc/flux_rules.h on the host, alone: the arithmetic the Flux handle does on the host, run at the buffer sizes the engine passes (heap
// buffers of exactly that size: an overrun is an AddressSanitizer report) and printed as hex floats for tests/test_flux_rules_cpu.py, which
// holds every line to the Python restatement.  Built there with -Wall -Werror -fsanitize=address,undefined.
//   flux_rules_check <t_0> ... <t_S>     the time grid of the fixed-grid tables, hex floats
// What has no Python restatement is checked here: the de-duplicated RoPE table against the direct per-element evaluation (the same libm:
// exact), every tap name against monitor_sites.h.  Exit status 0 and a last line "rules ok" = every check held.
#include "flux_rules.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#define CHECK(cond)                                                              \
  do {                                                                           \
    if (!(cond)) {                                                               \
      fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond);   \
      exit(1);                                                                   \
    }                                                                            \
  } while (0)

template <class T> struct Exact {   // a heap buffer of exactly n elements
  T* p;
  explicit Exact(size_t n) : p((T*)malloc(n ? n * sizeof(T) : 1)) { CHECK(p); }
  ~Exact() { free(p); }
};

static void fixed_grid(const std::vector<float>& grid) {
  const int S = (int)grid.size() - 1, B = 2;
  const int methods[3] = {VC_SOLVER_EULER, VC_SOLVER_MIDPOINT, VC_SOLVER_RK4}, evals[3] = {1, 2, 4};
  for (int m = 0; m < 3; ++m)
    for (int bf16 = 0; bf16 < 2; ++bf16) {
      const int E = evals[m];
      Exact<float> ts((size_t)S * E * B), dts(S);
      vcrules::model_times(methods[m], E, grid.data(), S, B, bf16 != 0, ts.p, dts.p);
      printf("times %d %d", methods[m], bf16);
      for (int j = 0; j < S * E; ++j) {
        CHECK(!memcmp(&ts.p[(size_t)j * B], &ts.p[(size_t)j * B + 1], 4));      // one time for every sample
        printf(" %a", (double)ts.p[(size_t)j * B]);
      }
      printf("\ndts %d %d", methods[m], bf16);
      for (int i = 0; i < S; ++i) printf(" %a", (double)dts.p[i]);
      printf("\n");
    }
}

// the adaptive solve's rules at Dormand-Prince: VC_RK_DOPRI5, order 5
static void dopri5() {
  const int order = vcrules::rk_order(VC_RK_DOPRI5);
  CHECK(order == 5 && vcrules::rk_stages(VC_RK_DOPRI5) == 7);
  // (d0, d1, r = rms(f(t0 + h0) - f0)): the ordinary case, d0 < 1e-5, max(d1, d2) <= 1e-15
  const double cases[3][3] = {{0.5, 0.25, ldexp(1.0, -10)}, {ldexp(1.0, -20), 0.25, ldexp(1.0, -12)}, {0.5, ldexp(1.0, -60), 0.0}};
  for (const auto& c : cases) {
    const double h0 = vcrules::rk_h0(c[0], c[1]);
    printf("initial %a %a %a %a %a\n", c[0], c[1], c[2], h0, vcrules::rk_first_dt(order, h0, c[1], c[2] / h0));
  }
  const double ratios[6] = {0.0, 0.5, 1.0, 1.0 + ldexp(1.0, -23), 7.0, 1e-12};
  for (double r : ratios) {
    bool accept = false;
    double factor = 0;
    CHECK(vcrules::rk_controller(order, r, &accept, &factor));
    printf("controller %a %d %a\n", r, (int)accept, factor);
  }
  bool accept = true;
  double factor = 0;
  CHECK(!vcrules::rk_controller(order, std::numeric_limits<double>::quiet_NaN(), &accept, &factor) && !accept);
  printf("controller nan refused\n");
  const double steps[3][2] = {{0.0, 0.0}, {0.0, 1e-6}, {0.3721, 0.0713}};
  for (const auto& st : steps) {
    Exact<float> tm(7);
    vcrules::rk_row_times(VC_RK_DOPRI5, st[0], st[1], tm.p);
    printf("rows %a %a", st[0], st[1]);
    for (int j = 0; j < 7; ++j) printf(" %a", (double)tm.p[j]);
    printf("\n");
  }
}

static void rope() {
  const int32_t axes[3] = {16, 56, 56};
  const int B = 2, T = 3, N = 5, L = T + N;
  const double theta = 10000.0;
  Exact<float> txt((size_t)B * T * 3), img((size_t)B * N * 3), out((size_t)B * L * 128);
  for (int i = 0; i < B * T * 3; ++i) txt.p[i] = 0.0f;                              // repeats
  const float vals[6] = {0.0f, 1.0f, -2.0f, 1.0f, 3.5f, -2.0f};                     // repeats, negative values, a fractional one
  for (int i = 0; i < B * N * 3; ++i) img.p[i] = vals[(i * 5 + i / 3) % 6];
  vcrules::rope_table(axes, theta, B, T, N, txt.p, img.p, out.p);
  for (int b = 0; b < B; ++b)
    for (int r = 0; r < L; ++r) {
      int pair = 0;
      for (int ax = 0; ax < 3; ++ax)
        for (int j = 0; j < axes[ax] / 2; ++j, ++pair) {
          const float id = r < T ? txt.p[((size_t)b * T + r) * 3 + ax] : img.p[((size_t)b * N + (r - T)) * 3 + ax];
          const double ang = (double)id * (1.0 / pow(theta, (double)(2 * j) / (double)axes[ax]));
          const float c = (float)cos(ang), s = (float)sin(ang);
          const float* got = out.p + (((size_t)b * L + r) * 64 + pair) * 2;
          CHECK(!memcmp(got, &c, 4) && !memcmp(got + 1, &s, 4));
        }
      CHECK(pair == 64);
    }
  printf("rope equal %d\n", B * L * 128);
  Exact<float> freqs(128);
  vcrules::timestep_freqs(freqs.p);
  printf("freqs");
  for (int k = 0; k < 128; ++k) printf(" %a", (double)freqs.p[k]);
  printf("\n");
}

static void bounds() {
  const int depth = 2, single = 3, n = 4 * depth + 2 * single;
  const float nan = std::numeric_limits<float>::quiet_NaN();
  for (int c = 0; c < 3; ++c) {       // all-ones scales, one outlier block, a NaN scale
    Exact<float> mx(n);
    for (int i = 0; i < n; ++i) mx.p[i] = 1.0f;
    if (c == 1) { mx.p[4 * depth + 2] = 8.5f; mx.p[4 * depth + 3] = 1.25f; mx.p[2] = 3.0f; }
    if (c == 2) mx.p[5] = nan;
    const float cap = vcrules::logit_cap(mx.p, n, depth);
    printf("cap %d", depth);
    for (int i = 0; i < n; ++i) printf(" %a", (double)mx.p[i]);
    printf(" -> %a %d\n", (double)cap, vcrules::logit_cap_milli(cap));
  }
  CHECK(vcrules::logit_cap_milli(0.0f) == 0 && vcrules::logit_cap_milli(2e6f) == 0 && vcrules::logit_cap_milli(1e30f) == 0);
  Exact<uint16_t> h(128);
  for (int i = 0; i < 128; ++i) h.p[i] = (uint16_t)((0x3f80 + 37 * i) ^ (i % 3 == 0 ? 0x8000 : 0));
  printf("absmax %a\n", vcrules::scale_absmax(h.p));
  h.p[77] = 0x7fc0;
  printf("absmax_nan %a\n", vcrules::scale_absmax(h.p));
}

static int parse(const std::string& name, int depth, int single, size_t* idx) {
  Exact<char> exact(name.size() + 1);                                                // the name in a buffer of its own size
  memcpy(exact.p, name.c_str(), name.size() + 1);
  return (int)vcrules::tap_index(exact.p, depth, single, idx);
}
static void taps() {
  const int depth = 2, single = 3, T = 16, N = 24;
  for (int tap = 0; tap < vcmon::tap_count(depth, single); ++tap) {
    char name[64];
    CHECK(vcmon::tap_name(depth, single, tap, name, sizeof(name)));
    size_t idx = 999;
    CHECK(parse(name, depth, single, &idx) == vcrules::TAP_OK && idx == (size_t)tap);
    const bool dbl = tap < vcmon::tap_single(depth, 0);
    CHECK(vcrules::tap_rows(idx, depth, T, N) == (dbl ? (strstr(name, "txt") ? T : N) : T + N));
    printf("tap %s %d\n", name, tap);
  }
  const char* bad[] = {"double.2.img", "double.0.foo", "single.3", "single.1x", "", "double.-1.img", "single.", "img_in "};
  for (const char* name : bad) {
    size_t idx = 999;
    const int code = parse(name, depth, single, &idx);
    CHECK(code != vcrules::TAP_OK && idx == 999);
    printf("tap_refused '%s' %d\n", name, code);
  }
}

int main(int argc, char** argv) {
  std::vector<float> grid;
  for (int i = 1; i < argc; ++i) grid.push_back(strtof(argv[i], nullptr));
  CHECK(grid.size() >= 2);
  fixed_grid(grid);
  dopri5();
  rope();
  bounds();
  taps();
  printf("rules ok\n");
  return 0;
}
