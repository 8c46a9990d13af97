// A short list of captured plans, most recently used first (include/vcloze_hip.h: "a list of 8, most recently used first").
// Plain C++17, nothing from HIP: tests/c_abi/plan_cache_check.cpp runs it on the host under the sanitizers.
// `drop` releases a Plan; it is called exactly once for every plan that leaves the list (evicted, cleared, or still held when the
// list dies) and never for one that stays.  A key is looked up with find() before it is inserted: insert() does not search.
#pragma once
#include <algorithm>
#include <cstddef>
#include <utility>
#include <vector>

template <class Key, class Plan, size_t Capacity, class Drop>
class PlanCache {
 public:
  explicit PlanCache(Drop drop = Drop()) : drop_(drop) {}
  PlanCache(const PlanCache&) = delete;
  PlanCache& operator=(const PlanCache&) = delete;
  ~PlanCache() { clear(); }
  // the plan of `key` (valid until the next insert / clear), now the most recently used one; null on a miss, which reorders nothing
  Plan* find(const Key& key) {
    for (size_t i = 0; i < list_.size(); ++i)
      if (list_[i].first == key) {
        std::rotate(list_.begin(), list_.begin() + i, list_.begin() + i + 1);
        return &list_.front().second;
      }
    return nullptr;
  }
  // to the front; at capacity the least recently used entry is dropped first
  void insert(const Key& key, const Plan& plan) {
    if (list_.size() >= Capacity) {
      drop_(list_.back().second);
      list_.pop_back();
    }
    list_.insert(list_.begin(), {key, plan});
  }
  void clear() {
    for (auto& entry : list_) drop_(entry.second);
    list_.clear();
  }
  size_t size() const { return list_.size(); }

 private:
  std::vector<std::pair<Key, Plan>> list_;
  Drop drop_;
};
