// csrc/monitor_sites.h on the host, alone: the site enumeration of the numerics monitor (shared with the taps), the byte sizes of its
// log and scratch, and the index arithmetic of the log at the capacity edges.  Built and run by tests/test_monitor_cpu.py with -Wall
// -Werror -fsanitize=address,undefined; exit status 0 and "monitor ok" = every check held.
#include "monitor_sites.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#define CHECK(cond)                                                              \
  do {                                                                           \
    if (!(cond)) {                                                               \
      fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond);   \
      exit(1);                                                                   \
    }                                                                            \
  } while (0)

// the name of a site through an exact-size heap buffer: a write past namelen is an AddressSanitizer report
static std::string site(int level, int depth, int single, int index) {
  char big[64];
  CHECK(vcmon::site_name(level, depth, single, index, big, sizeof(big)));
  const size_t len = strlen(big);
  char* exact = (char*)malloc(len + 1);
  CHECK(vcmon::site_name(level, depth, single, index, exact, (int)len + 1) && !strcmp(exact, big));
  free(exact);
  const int cut = len > 4 ? 4 : 1;          // truncated: cut - 1 characters and a terminator, never more
  char* part = (char*)malloc(cut);
  memset(part, 'x', cut);
  CHECK(vcmon::site_name(level, depth, single, index, part, cut));
  CHECK(strlen(part) == (size_t)cut - 1 && !strncmp(part, big, cut - 1));
  free(part);
  return big;
}

static void check_sites(int depth, int single) {
  const int taps = 2 + 2 * depth + single;
  CHECK(vcmon::tap_count(depth, single) == taps);
  CHECK(vcmon::site_count(0, depth, single) == 0 && vcmon::site_count(-1, depth, single) == 0);
  CHECK(vcmon::site_count(1, depth, single) == 2 && vcmon::site_count(2, depth, single) == 2 + taps);
  char buf[32];
  // level 0 has no site, level 1 has v and x alone
  CHECK(!vcmon::site_name(0, depth, single, 0, buf, sizeof(buf)));
  CHECK(site(1, depth, single, 0) == "v" && site(1, depth, single, 1) == "x" && !vcmon::site_name(1, depth, single, 2, buf, sizeof(buf)));
  // level 2: v, x, then the taps in tap order, each name once, each tap helper landing on its own name
  std::vector<std::string> want = {"v", "x", "img_in", "txt_in"};
  for (int i = 0; i < depth; ++i) { want.push_back("double." + std::to_string(i) + ".img"); want.push_back("double." + std::to_string(i) + ".txt"); }
  for (int i = 0; i < single; ++i) want.push_back("single." + std::to_string(i));
  CHECK((int)want.size() == vcmon::site_count(2, depth, single));
  std::set<std::string> seen;
  for (int s = 0; s < (int)want.size(); ++s) CHECK(site(2, depth, single, s) == want[s] && seen.insert(want[s]).second);
  CHECK(site(2, depth, single, vcmon::site_of_tap(vcmon::tap_img_in())) == "img_in");
  CHECK(site(2, depth, single, vcmon::site_of_tap(vcmon::tap_txt_in())) == "txt_in");
  for (int i = 0; i < depth; ++i) {
    CHECK(site(2, depth, single, vcmon::site_of_tap(vcmon::tap_double(i, false))) == "double." + std::to_string(i) + ".img");
    CHECK(site(2, depth, single, vcmon::site_of_tap(vcmon::tap_double(i, true))) == "double." + std::to_string(i) + ".txt");
  }
  for (int i = 0; i < single; ++i) CHECK(site(2, depth, single, vcmon::site_of_tap(vcmon::tap_single(depth, i))) == "single." + std::to_string(i));
  // the order an evaluation writes its sites in: a permutation of the sites, the taps first in tap order, then v, then x
  for (int level = 1; level <= 2; ++level) {
    const int ns = vcmon::site_count(level, depth, single);
    std::set<int> ranks;
    for (int s = 0; s < ns; ++s) {
      const int r = vcmon::site_rank(s, ns);
      CHECK(r >= 0 && r < ns && ranks.insert(r).second && vcmon::site_at_rank(r, ns) == s);
    }
    CHECK(vcmon::site_rank(vcmon::SITE_V, ns) == ns - 2 && vcmon::site_rank(vcmon::SITE_X, ns) == ns - 1);
    if (level == 2) CHECK(vcmon::site_rank(vcmon::site_of_tap(0), ns) == 0 && vcmon::site_rank(ns - 1, ns) == ns - 3);
  }
  // past either end, null and empty buffers
  CHECK(!vcmon::site_name(2, depth, single, (int)want.size(), buf, sizeof(buf)) && !vcmon::site_name(2, depth, single, -1, buf, sizeof(buf)));
  CHECK(!vcmon::site_name(2, depth, single, 1 << 30, buf, sizeof(buf)));
  CHECK(!vcmon::site_name(2, depth, single, 0, nullptr, 8) && !vcmon::site_name(2, depth, single, 0, buf, 0));
  CHECK(!vcmon::tap_name(depth, single, taps, buf, sizeof(buf)) && !vcmon::tap_name(depth, single, -1, buf, sizeof(buf)));
}

static void check_log(int64_t cap, int ns, int B) {
  const int64_t bytes = vcmon::log_bytes(cap, ns, B);
  CHECK(bytes == cap * ns * B * 16 && bytes % 16 == 0);
  // a log of exactly that many records: every valid index is written once, in layout order, and nothing else is
  std::vector<VcStat> log((size_t)(bytes / (int64_t)sizeof(VcStat)));
  memset(log.data(), 0, (size_t)bytes);
  int64_t next = 0;
  for (int64_t ev = 0; ev < cap; ++ev)
    for (int s = 0; s < ns; ++s)
      for (int b = 0; b < B; ++b) {
        const int64_t i = vcmon::log_index(ev, s, b, cap, ns, B);
        CHECK(i == next++);
        log[(size_t)i].count += 1;
        int32_t e2, s2, b2;
        vcmon::log_split(i, ns, B, &e2, &s2, &b2);
        CHECK(e2 == ev && s2 == s && b2 == b);
      }
  CHECK(next == (int64_t)log.size());
  // what the engine hands the kernel: the base of a site and the row stride; the kernel's row * stride + b lands on log_index
  for (int s = 0; s < ns; ++s)
    CHECK(vcmon::log_index(0, s, 0, cap, ns, B) + (cap - 1) * vcmon::log_row_stride(ns, B) + (B - 1) == vcmon::log_index(cap - 1, s, B - 1, cap, ns, B));
  for (const VcStat& st : log) CHECK(st.count == 1);
  // the edges: the last record is the last index, one past any extent is refused
  CHECK(vcmon::log_index(cap - 1, ns - 1, B - 1, cap, ns, B) == (int64_t)log.size() - 1);
  CHECK(vcmon::log_index(cap, 0, 0, cap, ns, B) == -1 && vcmon::log_index(-1, 0, 0, cap, ns, B) == -1);
  CHECK(vcmon::log_index(0, ns, 0, cap, ns, B) == -1 && vcmon::log_index(0, -1, 0, cap, ns, B) == -1);
  CHECK(vcmon::log_index(0, 0, B, cap, ns, B) == -1 && vcmon::log_index(0, 0, -1, cap, ns, B) == -1);
  CHECK(vcmon::log_index((int64_t)1 << 40, 0, 0, cap, ns, B) == -1);
}

int main() {
  static_assert(sizeof(VcStat) == 16, "VcStat is 16 bytes");
  const int cfgs[][2] = {{2, 2}, {19, 38}, {0, 0}, {0, 3}, {3, 0}, {101, 120}};
  for (const auto& c : cfgs) check_sites(c[0], c[1]);
  check_log(1, 2, 1);
  check_log(4, 10, 2);
  check_log(12, 2 + 2 + 2 * 19 + 38, 4);
  check_log(7, 1, 3);
  // sizes that are not positive have no log; the scratch holds four words per block and sample
  CHECK(vcmon::log_bytes(0, 2, 1) == -1 && vcmon::log_bytes(1, 0, 1) == -1 && vcmon::log_bytes(1, 2, 0) == -1 && vcmon::log_bytes(-3, 2, 1) == -1);
  CHECK(vcmon::log_index(0, 0, 0, 0, 2, 1) == -1);
  CHECK(vcmon::scratch_bytes(1) == 4 * VC_MONITOR_MAX_BLOCKS * 4 && vcmon::scratch_bytes(4) == 4 * vcmon::scratch_bytes(1) && vcmon::scratch_bytes(0) == -1);
  // the full model at the largest trajectory the product runs: 64-bit all the way
  CHECK(vcmon::log_bytes(200, 80, 4) == (int64_t)200 * 80 * 4 * 16);
  CHECK(vcmon::log_bytes((int64_t)1 << 28, 80, 4) == ((int64_t)1 << 28) * 80 * 4 * 16);
  printf("monitor ok\n");
  return 0;
}
