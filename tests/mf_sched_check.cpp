// mf_sched_check.cpp -- the level schedule of one mini-batch of MF-BPR / FunkSVD samples (ganmf_amd/csrc/mf_sched.hpp), checked on the
// host.  Built by tests/test_mf_sgd_host.py with -fsanitize=address,undefined.  Every case prints "ok   <name>" and the program ends
// with "all schedules clean"; a broken property prints "FAIL ..." and the exit status is 1.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../ganmf_amd/csrc/mf_sched.hpp"

using ganmf::MfSchedule;
using ganmf::MfScheduler;

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

typedef std::vector<int32_t> Ids;

// two samples conflict when they name one user, or one item in either role; neg empty: FunkSVD (no j)
static bool shares(const Ids& users, const Ids& pos, const Ids& neg, int64_t a, int64_t b) {
  if (users[a] == users[b] || pos[a] == pos[b]) return true;
  if (neg.empty()) return false;
  return pos[a] == neg[b] || neg[a] == pos[b] || neg[a] == neg[b];
}

// every property the library relies on, against the O(n^2) definition; the scheduler is the caller's: its tables carry over
static void check_list(MfScheduler& sch, const char* name, const Ids& users, const Ids& pos, const Ids& neg, int64_t want_levels) {
  const int64_t n = (int64_t)users.size();
  MfSchedule s;
  const int64_t levels = sch.schedule(users.data(), pos.data(), neg.empty() ? nullptr : neg.data(), n, s);
  CHECK(levels >= 0, "%s: refused", name);
  if (levels < 0) return;
  if (want_levels >= 0) CHECK(levels == want_levels, "%s: %lld levels, expected %lld", name, (long long)levels, (long long)want_levels);
  CHECK((int64_t)s.level.size() == n && (int64_t)s.order.size() == n && (int64_t)s.level_start.size() == levels + 1, "%s: sizes", name);
  int64_t top = 0;
  for (int64_t t = 0; t < n; ++t) {
    int32_t want = 1;
    for (int64_t e = 0; e < t; ++e) {
      if (shares(users, pos, neg, e, t)) {
        CHECK(s.level[e] < s.level[t], "%s: sample %lld depends on %lld but is not in a later level", name, (long long)t, (long long)e);
        if (s.level[e] + 1 > want) want = s.level[e] + 1;
      }
    }
    CHECK(s.level[t] == want, "%s: sample %lld has level %d, the definition gives %d", name, (long long)t, s.level[t], want);
    if (s.level[t] > top) top = s.level[t];
  }
  CHECK(top == levels, "%s: the largest level is %lld of %lld", name, (long long)top, (long long)levels);
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
      for (int64_t r = s.level_start[(size_t)l]; r < q; ++r)
        CHECK(!shares(users, pos, neg, s.order[(size_t)r], t), "%s: level %lld holds two samples that share a row", name, (long long)l + 1);
    }
  }
  std::printf("ok   %s: %lld samples, %lld levels\n", name, (long long)n, (long long)levels);
}

int main() {
  MfScheduler sch(64, 64);
  check_list(sch, "empty", {}, {}, {}, 0);
  {
    MfSchedule s;
    CHECK(sch.schedule(nullptr, nullptr, nullptr, 0, s) == 0 && s.level_start.size() == 1, "empty list with null pointers");
  }
  // the two id spaces are apart: user 3 and item 3 are different rows
  check_list(sch, "independent", {0, 1, 2, 3}, {3, 2, 1, 0}, {7, 6, 5, 4}, 1);
  check_list(sch, "independent funk", {0, 1, 2, 3}, {3, 2, 1, 0}, {}, 1);
  // consecutive samples share the user only, the positive only, and one's negative is the next one's positive
  check_list(sch, "shared user", {5, 5, 5, 5}, {0, 1, 2, 3}, {10, 11, 12, 13}, 4);
  check_list(sch, "shared user funk", {5, 5, 5, 5}, {0, 1, 2, 3}, {}, 4);
  check_list(sch, "shared positive", {0, 1, 2, 3}, {9, 9, 9, 9}, {10, 11, 12, 13}, 4);
  check_list(sch, "shared positive funk", {0, 1, 2, 3}, {9, 9, 9, 9}, {}, 4);
  check_list(sch, "j becomes i", {0, 1, 2, 3}, {20, 21, 22, 23}, {21, 22, 23, 24}, 4);
  check_list(sch, "i becomes j", {0, 1, 2, 3}, {21, 22, 23, 24}, {20, 21, 22, 23}, 4);
  // a negative is no row of FunkSVD: the same ids without j are independent
  check_list(sch, "j ignored by funk", {0, 1, 2, 3}, {20, 21, 22, 23}, {}, 1);
  {      // one row in every sample of a batch: as many levels as samples
    Ids users(40, 7), pos, neg;
    for (int t = 0; t < 40; ++t) { pos.push_back(t); neg.push_back(63 - t % 20); }
    check_list(sch, "one user in every sample", users, pos, neg, 40);
  }
  check_list(sch, "two chains", {0, 10, 0, 10, 0, 10, 20}, {1, 11, 2, 12, 3, 13, 21}, {31, 32, 33, 34, 35, 36, 37}, 3);
  // the tables are clean after every batch: the same batch twice, and after a refused one, gives the same schedule
  check_list(sch, "again after other batches", {0, 1, 2, 3}, {3, 2, 1, 0}, {7, 6, 5, 4}, 1);
  {
    MfSchedule s;
    const int32_t users[3] = {1, 2, 64}, pos[3] = {1, 2, 3}, neg[3] = {4, 5, 6};
    CHECK(sch.schedule(users, pos, neg, 3, s) == -1, "a user id == n_users must be refused");
    const int32_t users2[3] = {1, 2, 3}, pos2[3] = {1, 2, -1};
    CHECK(sch.schedule(users2, pos2, neg, 3, s) == -1, "a negative item id must be refused");
    const int32_t neg2[3] = {4, 5, 64};
    CHECK(sch.schedule(users2, pos, neg2, 3, s) == -1, "a negative-item id == n_items must be refused");
    CHECK(sch.schedule(users2, pos, nullptr, 3, s) == 1, "without j the same ids are fine");
    std::printf("ok   out of range\n");
  }
  check_list(sch, "clean after a refusal", {1, 2, 3}, {1, 2, 3}, {4, 5, 6}, 1);
  // random batches at several densities, with and without j, through ONE scheduler
  uint64_t z = 12345;
  auto next = [&z]() { z = z * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(z >> 33); };
  for (int n_users : {1, 5, 50}) {
    for (int n_items : {2, 7, 60}) {
      MfScheduler rs(n_users, n_items);
      for (int n : {1, 5, 64, 300}) {
        for (int with_j = 0; with_j < 2; ++with_j) {
          Ids users, pos, neg;
          for (int t = 0; t < n; ++t) {
            const int32_t i = (int32_t)(next() % (uint32_t)n_items);
            int32_t j = (int32_t)(next() % (uint32_t)n_items);
            if (j == i) j = (j + 1) % n_items;
            users.push_back((int32_t)(next() % (uint32_t)n_users));
            pos.push_back(i);
            if (with_j) neg.push_back(j);
          }
          char name[80];
          std::snprintf(name, sizeof name, "random users=%d items=%d n=%d j=%d", n_users, n_items, n, with_j);
          check_list(rs, name, users, pos, neg, n_users == 1 ? n : -1);
        }
      }
    }
  }
  if (g_failed) return 1;
  std::printf("all schedules clean\n");
  return 0;
}
