// csrc/plan_cache.h on the host, alone: the most-recently-used list of captured plans behind vc_flux_*, vc_vae_* and vc_text_*
// (include/vcloze_hip.h: "most recently used first").  Plans are ints, "drop" appends to a log.  Built and run by
// tests/test_host_cpu.py with -Wall -Werror -fsanitize=address,undefined; exit status 0 and "plan_cache ok" = every check held.
#include "plan_cache.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CHECK(cond)                                                                                        \
  do {                                                                                                     \
    if (!(cond)) {                                                                                         \
      fprintf(stderr, "%s:%d: capacity %d: CHECK(%s) failed\n", __FILE__, __LINE__, (int)N, #cond);        \
      exit(1);                                                                                             \
    }                                                                                                      \
  } while (0)

struct Log {
  std::vector<int>* dropped;
  void operator()(int plan) const { dropped->push_back(plan); }
};
using Plans = std::vector<int>;

static Plans sorted(Plans v) {
  std::sort(v.begin(), v.end());
  return v;
}

// the documented rule, step by step: key k holds plan 100 + k
template <size_t N> void by_hand() {
  const int n = (int)N;
  Plans dropped, inserted;
  {
    PlanCache<int, int, N, Log> c(Log{&dropped});
    CHECK(c.size() == 0 && c.find(0) == nullptr);
    for (int k = 0; k < n; ++k) {
      c.insert(k, 100 + k);
      inserted.push_back(100 + k);
      CHECK(c.size() == (size_t)k + 1);
    }
    CHECK(dropped.empty());                                  // up to the capacity nothing leaves
    int* hit = c.find(0);                                    // the least recently used entry: a hit moves it to the front ...
    CHECK(hit && *hit == 100 && c.size() == N && dropped.empty());
    CHECK(c.find(999) == nullptr && c.size() == N && dropped.empty());      // a miss: null, nothing dropped, nothing reordered ...
    c.insert(n, 100 + n);                                    // ... so the (capacity + 1)-th entry drops exactly key 1's plan
    inserted.push_back(100 + n);
    CHECK(dropped == Plans({101}) && c.size() == N);
    CHECK(c.find(1) == nullptr);
    hit = c.find(0);                                         // key 0 survived its eviction turn; front again, key 2 is last
    CHECK(hit && *hit == 100);
    c.insert(n + 1, 101 + n);
    inserted.push_back(101 + n);
    CHECK(dropped == Plans({101, 102}) && c.size() == N && c.find(2) == nullptr);
    Plans live;                                              // every other plan is still there, under its key
    for (int k : {0, n, n + 1}) live.push_back(100 + k);
    for (int k = 3; k < n; ++k) live.push_back(100 + k);
    CHECK(live.size() == N);
    for (int p : live) {
      hit = c.find(p - 100);
      CHECK(hit && *hit == p);
    }
    CHECK(dropped.size() == 2);                              // finding drops nothing
    c.clear();                                               // each remaining plan once, none of the two that left before
    CHECK(c.size() == 0 && dropped.size() == 2 + N);
    CHECK(sorted(Plans(dropped.begin() + 2, dropped.end())) == sorted(live));
    CHECK(c.find(0) == nullptr);
    c.clear();                                               // an empty list drops nothing
    CHECK(dropped.size() == 2 + N);
    for (int k = 0; k <= n; ++k) {                           // insert after clear(): the list works as a new one
      c.insert(k, 500 + k);
      inserted.push_back(500 + k);
      CHECK(c.size() == (size_t)std::min(k + 1, n));
      CHECK(dropped.size() == 2 + N + (k == n ? 1 : 0));
    }
    CHECK(dropped.back() == 500);
    hit = c.find(n);
    CHECK(hit && *hit == 500 + n && c.find(0) == nullptr);
  }
  // the list is gone: every plan that ever entered it has been dropped exactly once
  CHECK(sorted(dropped) == sorted(inserted));
}

// the same rule as a model (keys in order of use), driven by a fixed pseudo-random sequence of find / insert / clear
template <size_t N> void against_model() {
  Plans dropped, expect_dropped;
  std::vector<std::pair<int, int>> model;                    // (key, plan), most recently used first
  int next_plan = 1000;
  unsigned rng = 12345u + (unsigned)N;
  {
    PlanCache<int, int, N, Log> c(Log{&dropped});
    for (int step = 0; step < 4000; ++step) {
      rng = rng * 1664525u + 1013904223u;
      const int key = (int)((rng >> 16) % (N + 5));
      const bool wipe = (rng >> 8) % 97 == 0;
      if (wipe) {
        const size_t before = dropped.size();
        c.clear();                                           // in any order: compared as a set
        Plans live;
        for (auto& m : model) live.push_back(m.second);
        CHECK(sorted(Plans(dropped.begin() + before, dropped.end())) == sorted(live));
        expect_dropped.insert(expect_dropped.end(), live.begin(), live.end());
        model.clear();
      } else {
        size_t i = 0;
        while (i < model.size() && model[i].first != key) ++i;
        int* hit = c.find(key);
        if (i < model.size()) {
          CHECK(hit && *hit == model[i].second);
          std::rotate(model.begin(), model.begin() + i, model.begin() + i + 1);
        } else {
          CHECK(hit == nullptr);
          if ((rng >> 4) % 3) {                              // ... and some of the misses stay misses
            const bool evicts = model.size() >= N;
            const int last = evicts ? model.back().second : -1;
            if (evicts) {
              expect_dropped.push_back(last);
              model.pop_back();
            }
            model.insert(model.begin(), {key, next_plan});
            c.insert(key, next_plan++);
            CHECK(dropped.size() == expect_dropped.size() && (!evicts || dropped.back() == last));     // exactly the last one
          }
        }
      }
      CHECK(c.size() == model.size() && c.size() <= N);
      CHECK(dropped.size() == expect_dropped.size());
    }
    const size_t before = dropped.size();
    CHECK(expect_dropped.size() >= 2 * N);                   // the sequence did evict
    c.clear();
    CHECK(c.size() == 0 && dropped.size() == before + model.size());
    Plans tail(dropped.begin() + before, dropped.end()), live;
    for (auto& m : model) live.push_back(m.second);
    CHECK(sorted(tail) == sorted(live));
  }
  Plans all = sorted(dropped);
  CHECK(std::adjacent_find(all.begin(), all.end()) == all.end());        // no plan twice
  CHECK(all.size() == (size_t)(next_plan - 1000));                         // and every plan once
}

int main() {
  by_hand<4>();
  by_hand<8>();
  against_model<4>();
  against_model<8>();
  puts("plan_cache ok");
  return 0;
}
