// level_sched_check.cpp -- the level schedule of SGD sample lists (ganmf_amd/csrc/level_sched.hpp), checked on the host with the columns
// of SLIM-BPR ({pos, neg} over the items) and of MF-BPR / FunkSVD ({users, pos[, neg]} over users + items).  Built by
// tests/test_level_sched_host.py with -fsanitize=address,undefined.  Every case prints "ok   <name>" and the program ends with
// "all schedules clean"; a broken property prints "FAIL ..." and the exit status is 1.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../ganmf_amd/csrc/level_sched.hpp"

using ganmf::LevelColumn;
using ganmf::LevelSchedule;
using ganmf::LevelScheduler;

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

// a list by columns; an empty id vector is a column the list does not have (FunkSVD's j)
struct List {
  std::vector<Ids> ids;
  std::vector<int64_t> base, rows;
  void add(const Ids& v, int64_t b, int64_t r) {
    // (so an "empty" list reaches the scheduler with ONE column; the null-pointer calls beside those cases pass the empty list with
    // the trainers' 2 and 3 columns)
    if (v.empty() && !ids.empty()) return;
    ids.push_back(v); base.push_back(b); rows.push_back(r);
  }
  int64_t n() const { return (int64_t)ids[0].size(); }
  std::vector<LevelColumn> columns() const {
    std::vector<LevelColumn> c;
    for (size_t q = 0; q < ids.size(); ++q) c.push_back({ids[q].data(), base[q], rows[q]});
    return c;
  }
  // the definition of a conflict: two samples share a key
  bool shares(int64_t a, int64_t b) const {
    for (size_t x = 0; x < ids.size(); ++x)
      for (size_t y = 0; y < ids.size(); ++y)
        if (base[x] + ids[x][(size_t)a] == base[y] + ids[y][(size_t)b]) return true;
    return false;
  }
};

static List slim_list(const Ids& pos, const Ids& neg, int64_t n_items) {
  List l;
  l.add(pos, 0, n_items);
  l.add(neg, 0, n_items);
  return l;
}
static List mf_list(const Ids& users, const Ids& pos, const Ids& neg, int64_t n_users, int64_t n_items) {
  List l;
  l.add(users, 0, n_users);
  l.add(pos, n_users, n_items);
  l.add(neg, n_users, n_items);
  return l;
}

// every property the library relies on, against the O(n^2) definition; the scheduler is the caller's: its table carries over
static void check_list(LevelScheduler& sch, const char* name, const List& list, int64_t want_levels) {
  const int64_t n = list.n();
  LevelSchedule s;
  const int64_t levels = sch.schedule(list.columns(), n, s);
  CHECK(levels >= 0, "%s: refused", name);
  if (levels < 0) return;
  if (want_levels >= 0) CHECK(levels == want_levels, "%s: %lld levels, expected %lld", name, (long long)levels, (long long)want_levels);
  CHECK((int64_t)s.level.size() == n && (int64_t)s.order.size() == n && (int64_t)s.level_start.size() == levels + 1, "%s: sizes", name);
  // the definition: 1 + the largest level of an earlier sample that shares a key
  int64_t top = 0;
  for (int64_t t = 0; t < n; ++t) {
    int32_t want = 1;
    for (int64_t e = 0; e < t; ++e) {
      if (list.shares(e, t)) {
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
      // no two samples of a level share a key
      for (int64_t r = s.level_start[(size_t)l]; r < q; ++r)
        CHECK(!list.shares(s.order[(size_t)r], t), "%s: level %lld holds two samples that share a row", name, (long long)l + 1);
    }
  }
  std::printf("ok   %s: %lld samples, %lld levels\n", name, (long long)n, (long long)levels);
}

static uint64_t g_z;
static uint32_t next() {
  g_z = g_z * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)(g_z >> 33);
}

// ---- one key space: the items of SLIM-BPR's (pos, neg) ---------------------------------------------------------------------------------
static void item_lists() {
  std::printf("-- columns {pos, neg} over the items\n");
  auto check = [](const char* name, const Ids& pos, const Ids& neg, int64_t n_items, int64_t want) {
    LevelScheduler sch(n_items);
    check_list(sch, name, slim_list(pos, neg, n_items), want);
  };
  // an empty list
  check("empty", {}, {}, 10, 0);
  {
    LevelScheduler sch(0);
    LevelSchedule s;
    CHECK(sch.schedule({{nullptr, 0, 0}, {nullptr, 0, 0}}, 0, s) == 0 && s.level_start.size() == 1, "empty list with null pointers");
  }
  // independent samples share one level
  check("independent", {0, 2, 4, 6, 8}, {1, 3, 5, 7, 9}, 10, 1);
  // one i repeated: a chain of full length
  {
    Ids pos(40, 3), neg;
    for (int t = 0; t < 40; ++t) neg.push_back(4 + t);
    check("repeated i", pos, neg, 64, 40);
  }
  // one sample's i is the next sample's j: a chain of full length
  {
    Ids pos, neg;
    for (int t = 0; t < 40; ++t) { pos.push_back(t); neg.push_back(t + 1); }      // i_t = t = j_(t-1) ... as j: neg[t] = pos[t + 1]
    check("i becomes j", neg, pos, 64, 40);
    check("j becomes i", pos, neg, 64, 40);
  }
  // two interleaved chains and a late independent sample
  check("two chains", {0, 10, 0, 10, 0, 10, 20}, {1, 11, 2, 12, 3, 13, 21}, 32, 3);
  // random lists at several densities
  g_z = 12345;
  for (int n_items : {2, 7, 70, 400}) {
    for (int n : {1, 5, 64, 300}) {
      Ids pos, neg;
      for (int t = 0; t < n; ++t) {
        const int32_t i = (int32_t)(next() % (uint32_t)n_items);
        int32_t j = (int32_t)(next() % (uint32_t)n_items);
        if (j == i) j = (j + 1) % n_items;
        pos.push_back(i);
        neg.push_back(j);
      }
      char name[64];
      std::snprintf(name, sizeof name, "random items=%d n=%d", n_items, n);
      check(name, pos, neg, n_items, -1);
    }
  }
  // an id out of range is refused
  {
    LevelSchedule s;
    const int32_t pos[2] = {0, 5}, neg[2] = {1, 2};
    LevelScheduler five(5), eight(8);
    CHECK(five.schedule({{pos, 0, 5}, {neg, 0, 5}}, 2, s) == -1, "an item id == n_items must be refused");
    const int32_t neg2[2] = {1, -1};
    CHECK(eight.schedule({{pos, 0, 8}, {neg2, 0, 8}}, 2, s) == -1, "a negative item id must be refused");
    std::printf("ok   out of range\n");
  }
}

// ---- two id spaces in one key space: users, then items at base n_users; ONE scheduler through every case --------------------------------
static void user_item_lists() {
  std::printf("-- columns {users, pos[, neg]} over users + items\n");
  LevelScheduler sch(64 + 64);
  auto check = [&sch](const char* name, const Ids& users, const Ids& pos, const Ids& neg, int64_t want) {
    check_list(sch, name, mf_list(users, pos, neg, 64, 64), want);
  };
  check("empty", {}, {}, {}, 0);
  {
    LevelSchedule s;
    CHECK(sch.schedule({{nullptr, 0, 64}, {nullptr, 64, 64}, {nullptr, 64, 64}}, 0, s) == 0 && s.level_start.size() == 1,
          "empty list with null pointers");
  }
  // the two id spaces are apart: user 3 and item 3 are different rows
  check("independent", {0, 1, 2, 3}, {3, 2, 1, 0}, {7, 6, 5, 4}, 1);
  check("independent funk", {0, 1, 2, 3}, {3, 2, 1, 0}, {}, 1);
  // consecutive samples share the user only, the positive only, and one's negative is the next one's positive
  check("shared user", {5, 5, 5, 5}, {0, 1, 2, 3}, {10, 11, 12, 13}, 4);
  check("shared user funk", {5, 5, 5, 5}, {0, 1, 2, 3}, {}, 4);
  check("shared positive", {0, 1, 2, 3}, {9, 9, 9, 9}, {10, 11, 12, 13}, 4);
  check("shared positive funk", {0, 1, 2, 3}, {9, 9, 9, 9}, {}, 4);
  check("j becomes i", {0, 1, 2, 3}, {20, 21, 22, 23}, {21, 22, 23, 24}, 4);
  check("i becomes j", {0, 1, 2, 3}, {21, 22, 23, 24}, {20, 21, 22, 23}, 4);
  // a negative is no row of FunkSVD: the same ids without j are independent
  check("j ignored by funk", {0, 1, 2, 3}, {20, 21, 22, 23}, {}, 1);
  {      // one row in every sample of a batch: as many levels as samples
    Ids users(40, 7), pos, neg;
    for (int t = 0; t < 40; ++t) { pos.push_back(t); neg.push_back(63 - t % 20); }
    check("one user in every sample", users, pos, neg, 40);
  }
  check("two chains", {0, 10, 0, 10, 0, 10, 20}, {1, 11, 2, 12, 3, 13, 21}, {31, 32, 33, 34, 35, 36, 37}, 3);
  // the table is clean after every batch: the same batch twice, and after a refused one, gives the same schedule
  check("again after other batches", {0, 1, 2, 3}, {3, 2, 1, 0}, {7, 6, 5, 4}, 1);
  {
    LevelSchedule s;
    const int32_t users[3] = {1, 2, 64}, pos[3] = {1, 2, 3}, neg[3] = {4, 5, 6};
    CHECK(sch.schedule({{users, 0, 64}, {pos, 64, 64}, {neg, 64, 64}}, 3, s) == -1, "a user id == n_users must be refused");
    const int32_t users2[3] = {1, 2, 3}, pos2[3] = {1, 2, -1};
    CHECK(sch.schedule({{users2, 0, 64}, {pos2, 64, 64}, {neg, 64, 64}}, 3, s) == -1, "a negative item id must be refused");
    const int32_t neg2[3] = {4, 5, 64};
    CHECK(sch.schedule({{users2, 0, 64}, {pos, 64, 64}, {neg2, 64, 64}}, 3, s) == -1, "a negative-item id == n_items must be refused");
    CHECK(sch.schedule({{users2, 0, 64}, {pos, 64, 64}}, 3, s) == 1, "without j the same ids are fine");
    std::printf("ok   out of range\n");
  }
  check("clean after a refusal", {1, 2, 3}, {1, 2, 3}, {4, 5, 6}, 1);
  // random batches at several densities, with and without j, through ONE scheduler
  g_z = 12345;
  for (int n_users : {1, 5, 50}) {
    for (int n_items : {2, 7, 60}) {
      LevelScheduler rs(n_users + n_items);
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
          check_list(rs, name, mf_list(users, pos, neg, n_users, n_items), n_users == 1 ? n : -1);
        }
      }
    }
  }
}

int main() {
  item_lists();
  user_item_lists();
  if (g_failed) return 1;
  std::printf("all schedules clean\n");
  return 0;
}
