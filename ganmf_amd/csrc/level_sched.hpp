// level_sched.hpp -- the level schedule of an SGD sample list (slim_bpr.hpp, mf_sgd.hpp; lib/sgd_train.inc).  Plain C++, no device code:
// the library and tests/level_sched_check.cpp share it.
//
// A sample reads and writes a few rows of the model (parameters and optimiser state) and nothing else; a row has a key in ONE key space.
// SLIM-BPR's (u, i, j) names rows i and j of S: the columns {pos, neg} over n_items keys.  MF-BPR's names row u of the user matrix and
// rows i and j of the item matrix: the columns {users, pos, neg} over n_users + n_items keys, the items at base n_users.  FunkSVD has
// no j: two columns.  A sample has to run behind the last earlier sample that named any of its keys, and behind nothing else:
//     level[t] = 1 + max over the sample's keys of last[key]          (last[key]: the level of the last earlier sample that named it,
// 0 for a key nobody has named).  Two samples of one level share no key, so a level is one grid; the levels run in order, one launch
// each, and the launch boundary is the only synchronisation there is.  The table lives in the object and is cleared entry by entry
// after a list: a list costs O(n), whatever n_keys.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace ganmf {

struct LevelSchedule {
  std::vector<int32_t> level;          // [n] 1-based level of every sample
  std::vector<int64_t> order;          // [n] positions 0 .. n - 1 sorted by level, list order kept inside a level
  std::vector<int64_t> level_start;    // [n_levels + 1] order[level_start[l], level_start[l + 1]) is level l + 1
};

constexpr int LEVEL_MAX_COLUMNS = 4;

struct LevelColumn {
  const int32_t* ids;      // [n] one id of every sample
  int64_t base;            // key = base + id
  int64_t rows;            // ids lie in [0, rows)
};

class LevelScheduler {
 public:
  explicit LevelScheduler(int64_t n_keys) : last_((size_t)std::max<int64_t>(n_keys, 0), 0) {}

  // Returns the number of levels (0 for an empty list), -1 when an id is out of range (nothing is left behind in the table).
  int64_t schedule(const std::vector<LevelColumn>& cols, int64_t n, LevelSchedule& out) {
    switch (cols.size()) {      // the trainers' two counts as constants: the loops over the columns unroll (a third less host time)
      case 2: return run<2>(cols, n, out);
      case 3: return run<3>(cols, n, out);
      default: return run<0>(cols, n, out);
    }
  }

 private:
  template <int N_COLS>      // 0: any count up to LEVEL_MAX_COLUMNS
  int64_t run(const std::vector<LevelColumn>& cols, int64_t n, LevelSchedule& out) {
    out.level.assign((size_t)std::max<int64_t>(n, 0), 0);
    out.order.assign((size_t)std::max<int64_t>(n, 0), 0);
    out.level_start.assign(1, 0);
    if (n <= 0) return 0;
    if (cols.size() > (size_t)LEVEL_MAX_COLUMNS) return -1;
    const int n_cols = N_COLS ? N_COLS : (int)cols.size();
    LevelColumn col[LEVEL_MAX_COLUMNS] = {};
    for (size_t c = 0; c < cols.size(); ++c) col[c] = cols[c];
    for (int c = 0; c < n_cols; ++c)      // (a column outside the table, or one no id of the n > 0 can lie in: the caller's mistake)
      if (col[c].base < 0 || col[c].rows < 1 || col[c].base + col[c].rows > (int64_t)last_.size()) return -1;
    int32_t* last = last_.data();
    int32_t* level = out.level.data();
    int32_t top = 0;
    int64_t done = 0;
    bool bad = false;
    for (; done < n; ++done) {
      int64_t key[LEVEL_MAX_COLUMNS];      // (read before the table is written: the ids are int32 like the table)
      int32_t lv = 0;
      for (int c = 0; c < n_cols; ++c) {
        const int64_t id = col[c].ids[done];
        bad |= id < 0 || id >= col[c].rows;
        key[c] = col[c].base + (bad ? 0 : id);
        lv = std::max(lv, last[key[c]]);
      }
      if (bad) break;
      ++lv;
      level[done] = lv;
      for (int c = 0; c < n_cols; ++c) last[key[c]] = lv;
      top = std::max(top, lv);
    }
    for (int64_t t = 0; t < done; ++t)      // the table is zero again for the next list
      for (int c = 0; c < n_cols; ++c) last[col[c].base + col[c].ids[t]] = 0;
    if (bad) return -1;
    out.level_start.assign((size_t)top + 1, 0);
    for (int64_t t = 0; t < n; ++t) ++out.level_start[(size_t)out.level[(size_t)t]];      // counts at [level], level >= 1
    for (int32_t l = 1; l <= top; ++l) out.level_start[(size_t)l] += out.level_start[(size_t)l - 1];
    // level_start[l] is now the END of level l; a stable counting sort fills every level from its start
    std::vector<int64_t> at((size_t)top + 1, 0);
    for (int32_t l = 1; l <= top; ++l) at[(size_t)l] = out.level_start[(size_t)l - 1];
    for (int64_t t = 0; t < n; ++t) out.order[(size_t)at[(size_t)out.level[(size_t)t]]++] = t;
    return top;
  }

  std::vector<int32_t> last_;      // level of the last sample of the list that named the key
};

}  // namespace ganmf
