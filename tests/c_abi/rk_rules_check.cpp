// The rk_* rules of csrc/flux_rules.h on the host, alone: the stage times, the controller and the initial step size of the embedded pairs,
// run at the buffer sizes the engine passes (heap buffers of exactly that size: an overrun is an AddressSanitizer report) and printed as
// hex floats for tests/test_rk_rules_cpu.py, which holds every line to transport.rk_* and passes the inputs in.  Built there with -Wall
// -Werror -fsanitize=address,undefined.
//   rk_rules_check rows <t> <dt> ... | controller <ratio> ... | initial <d0> <d1> <r> ...      (hex floats; any number of groups)
// Dormand-Prince runs through the same rules (VC_RK_DOPRI5, order 5).  Exit status 0 and a last line "rk rules ok" = every check held.
#include "flux_rules.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
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

static const int METHODS[3] = {VC_RK_DOPRI5, VC_RK_BOSH3, VC_RK_ADAPTIVE_HEUN};

static void rows(double t, double dt) {
  for (int m : METHODS) {
    const int S = vcrules::rk_stages(m);
    Exact<float> tm(S);
    vcrules::rk_row_times(m, t, dt, tm.p);
    printf("rows %d %a %a", m, t, dt);
    for (int j = 0; j < S; ++j) printf(" %a", (double)tm.p[j]);
    printf("\n");
  }
}

static void controller(double ratio) {
  for (int m : METHODS) {
    bool accept = true;
    double factor = 0;
    const bool ok = vcrules::rk_controller(vcrules::rk_order(m), ratio, &accept, &factor);
    if (ok) printf("controller %d %a %d %a\n", m, ratio, (int)accept, factor);
    else { CHECK(ratio != ratio && !accept); printf("controller %d nan refused\n", m); }
  }
}

static void initial(double d0, double d1, double r) {
  const double h0 = vcrules::rk_h0(d0, d1);
  for (int m : METHODS) {
    const double dt = vcrules::rk_first_dt(vcrules::rk_order(m), h0, d1, r / h0);
    printf("initial %d %a %a %a %a %a\n", m, d0, d1, r, h0, dt);
  }
}

int main(int argc, char** argv) {
  CHECK(vcrules::rk_stages(VC_RK_DOPRI5) == 7 && vcrules::rk_stages(VC_RK_BOSH3) == 4 && vcrules::rk_stages(VC_RK_ADAPTIVE_HEUN) == 3);
  CHECK(vcrules::rk_evals_per_attempt(VC_RK_DOPRI5) == 6 && vcrules::rk_evals_per_attempt(VC_RK_BOSH3) == 3 &&
        vcrules::rk_evals_per_attempt(VC_RK_ADAPTIVE_HEUN) == 2);
  CHECK(vcrules::rk_order(VC_RK_DOPRI5) == 5 && vcrules::rk_order(VC_RK_BOSH3) == 3 && vcrules::rk_order(VC_RK_ADAPTIVE_HEUN) == 2);
  CHECK(!vcrules::rk_stages(3) && !vcrules::rk_stages(-1) && !vcrules::rk_evals_per_attempt(3) && !vcrules::rk_order(3));
  std::string group;
  std::vector<double> v;
  auto flush = [&] {
    if (group == "rows") { CHECK(v.size() % 2 == 0); for (size_t i = 0; i < v.size(); i += 2) rows(v[i], v[i + 1]); }
    else if (group == "controller") for (double r : v) controller(r);
    else if (group == "initial") { CHECK(v.size() % 3 == 0); for (size_t i = 0; i < v.size(); i += 3) initial(v[i], v[i + 1], v[i + 2]); }
    else CHECK(group.empty() && v.empty());
    v.clear();
  };
  for (int i = 1; i < argc; ++i) {
    if (!strcmp(argv[i], "rows") || !strcmp(argv[i], "controller") || !strcmp(argv[i], "initial")) { flush(); group = argv[i]; }
    else v.push_back(strtod(argv[i], nullptr));
  }
  flush();
  printf("rk rules ok\n");
  return 0;
}
