// slim_sched_check.cpp -- the level schedule of SLIM-BPR sample lists (ganmf_amd/csrc/slim_sched.hpp), checked on the host.
// Built by tests/test_slim_bpr_host.py with -fsanitize=address,undefined.  Every case prints "ok   <name>" and the program ends with
// "all schedules clean"; a broken property prints "FAIL ..." and the exit status is 1.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../ganmf_amd/csrc/slim_sched.hpp"

using ganmf::SlimSchedule;
using ganmf::slim_schedule;

static int g_failed = 0;
#define CHECK(cond, ...)                      \
  do {                                        \
    if (!(cond)) {                            \
      std::printf("FAIL %s:%d ", __FILE__, __LINE__); \
      std::printf(__VA_ARGS__);               \
      std::printf("\n");                      \
      g_failed = 1;                           \
    }                                         \
  } while (0)

// every property the library relies on, against the O(n^2) definition
static void check_list(const char* name, const std::vector<int32_t>& pos, const std::vector<int32_t>& neg, int64_t n_items,
                       int64_t want_levels) {
  const int64_t n = (int64_t)pos.size();
  SlimSchedule s;
  const int64_t levels = slim_schedule(pos.data(), neg.data(), n, n_items, s);
  CHECK(levels >= 0, "%s: refused", name);
  if (levels < 0) return;
  if (want_levels >= 0) CHECK(levels == want_levels, "%s: %lld levels, expected %lld", name, (long long)levels, (long long)want_levels);
  CHECK((int64_t)s.level.size() == n && (int64_t)s.order.size() == n && (int64_t)s.level_start.size() == levels + 1, "%s: sizes", name);
  // the definition: 1 + the largest level of an earlier sample that shares an item
  int64_t top = 0;
  for (int64_t t = 0; t < n; ++t) {
    int32_t want = 1;
    for (int64_t e = 0; e < t; ++e) {
      const bool shares = pos[e] == pos[t] || pos[e] == neg[t] || neg[e] == pos[t] || neg[e] == neg[t];
      if (shares) {
        CHECK(s.level[e] < s.level[t], "%s: sample %lld depends on %lld but is not in a later level", name, (long long)t, (long long)e);
        if (s.level[e] + 1 > want) want = s.level[e] + 1;
      }
    }
    CHECK(s.level[t] == want, "%s: sample %lld has level %d, the definition gives %d", name, (long long)t, s.level[t], want);
    if (s.level[t] > top) top = s.level[t];
  }
  CHECK(top == levels, "%s: the largest level is %lld of %lld", name, (long long)top, (long long)levels);
  // order: a permutation, sorted by level, list order inside a level; level_start delimits the levels
  std::vector<char> seen((size_t)n, 0);
  CHECK(s.level_start[0] == 0 && s.level_start[(size_t)levels] == n, "%s: level_start ends", name);
  for (int64_t l = 0; l < levels; ++l) {
    CHECK(s.level_start[(size_t)l] < s.level_start[(size_t)l + 1], "%s: level %lld is empty", name, (long long)l + 1);
    for (int64_t q = s.level_start[(size_t)l]; q < s.level_start[(size_t)l + 1]; ++q) {
      const int64_t t = s.order[(size_t)q];
      CHECK(t >= 0 && t < n && !seen[(size_t)t], "%s: order is no permutation at %lld", name, (long long)q);
      if (t < 0 || t >= n) continue;
      seen[(size_t)t] = 1;
      CHECK(s.level[(size_t)t] == l + 1, "%s: slot %lld holds a sample of level %d in level %lld", name, (long long)q, s.level[(size_t)t], (long long)l + 1);
      if (q > s.level_start[(size_t)l]) CHECK(s.order[(size_t)q - 1] < t, "%s: list order lost inside level %lld", name, (long long)l + 1);
      // no two samples of a level share an item
      for (int64_t r = s.level_start[(size_t)l]; r < q; ++r) {
        const int64_t e = s.order[(size_t)r];
        CHECK(!(pos[e] == pos[t] || pos[e] == neg[t] || neg[e] == pos[t] || neg[e] == neg[t]), "%s: level %lld holds two samples that share an item", name, (long long)l + 1);
      }
    }
  }
  std::printf("ok   %s: %lld samples, %lld levels\n", name, (long long)n, (long long)levels);
}

int main() {
  // an empty list
  check_list("empty", {}, {}, 10, 0);
  {
    SlimSchedule s;
    CHECK(slim_schedule(nullptr, nullptr, 0, 0, s) == 0 && s.level_start.size() == 1, "empty list with null pointers");
  }
  // independent samples share one level
  check_list("independent", {0, 2, 4, 6, 8}, {1, 3, 5, 7, 9}, 10, 1);
  // one i repeated: a chain of full length
  {
    std::vector<int32_t> pos(40, 3), neg;
    for (int t = 0; t < 40; ++t) neg.push_back(4 + t);
    check_list("repeated i", pos, neg, 64, 40);
  }
  // one sample's i is the next sample's j: a chain of full length
  {
    std::vector<int32_t> pos, neg;
    for (int t = 0; t < 40; ++t) { pos.push_back(t); neg.push_back(t + 1); }      // i_t = t = j_(t-1) ... as j: neg[t] = pos[t + 1]
    check_list("i becomes j", neg, pos, 64, 40);
    check_list("j becomes i", pos, neg, 64, 40);
  }
  // two interleaved chains and a late independent sample
  check_list("two chains", {0, 10, 0, 10, 0, 10, 20}, {1, 11, 2, 12, 3, 13, 21}, 32, 3);
  // random lists at several densities
  uint64_t z = 12345;
  auto next = [&z]() { z = z * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(z >> 33); };
  for (int n_items : {2, 7, 70, 400}) {
    for (int n : {1, 5, 64, 300}) {
      std::vector<int32_t> pos, neg;
      for (int t = 0; t < n; ++t) {
        const int32_t i = (int32_t)(next() % (uint32_t)n_items);
        int32_t j = (int32_t)(next() % (uint32_t)n_items);
        if (j == i) j = (j + 1) % n_items;
        pos.push_back(i);
        neg.push_back(j);
      }
      char name[64];
      std::snprintf(name, sizeof name, "random items=%d n=%d", n_items, n);
      check_list(name, pos, neg, n_items, -1);
    }
  }
  // an id out of range is refused
  {
    SlimSchedule s;
    const int32_t pos[2] = {0, 5}, neg[2] = {1, 2};
    CHECK(slim_schedule(pos, neg, 2, 5, s) == -1, "an item id == n_items must be refused");
    const int32_t neg2[2] = {1, -1};
    CHECK(slim_schedule(pos, neg2, 2, 8, s) == -1, "a negative item id must be refused");
    std::printf("ok   out of range\n");
  }
  if (g_failed) return 1;
  std::printf("all schedules clean\n");
  return 0;
}
