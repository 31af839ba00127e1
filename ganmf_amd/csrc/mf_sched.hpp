// mf_sched.hpp -- the level schedule of one mini-batch of an SGD matrix-factorisation sample list (mf_sgd.hpp; lib/abi_mf_sgd.inc).
// Plain C++: the library and tests/mf_sched_check.cpp share it.
//
// The rule of slim_sched.hpp with keys in two id spaces.  A sample (u, i, j) reads and writes row u of the user matrix and rows i and
// j of the item matrix (factors, optimiser state, biases), nothing else; FunkSVD has no j (neg == nullptr).  It has to run behind the
// last earlier sample of its batch that named u, behind the last one that named i (as its i or its j) and behind the last one that
// named j:
//     level[t] = 1 + max(last_user[u], last_item[i], last_item[j])
// with 0 for a row nobody has named.  Two samples of one level share no row, so a level is one grid; the launch boundary is the only
// synchronisation.  The two tables live in the object and are cleared entry by entry after a batch: a batch costs O(count).
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace ganmf {

struct MfSchedule {
  std::vector<int32_t> level;          // [n] 1-based level of every sample
  std::vector<int64_t> order;          // [n] positions 0 .. n - 1 sorted by level, list order kept inside a level
  std::vector<int64_t> level_start;    // [n_levels + 1] order[level_start[l], level_start[l + 1]) is level l + 1
};

class MfScheduler {
 public:
  MfScheduler(int64_t n_users, int64_t n_items)
      : last_user_((size_t)std::max<int64_t>(n_users, 0), 0), last_item_((size_t)std::max<int64_t>(n_items, 0), 0) {}

  // Returns the number of levels (0 for an empty batch), -1 when an id is out of range (nothing is left behind in the tables).
  int64_t schedule(const int32_t* users, const int32_t* pos, const int32_t* neg, int64_t n, MfSchedule& out) {
    const int64_t n_users = (int64_t)last_user_.size(), n_items = (int64_t)last_item_.size();
    out.level.assign((size_t)std::max<int64_t>(n, 0), 0);
    out.order.assign((size_t)std::max<int64_t>(n, 0), 0);
    out.level_start.assign(1, 0);
    if (n <= 0) return 0;
    int32_t top = 0;
    int64_t done = 0;
    bool bad = false;
    for (; done < n; ++done) {
      const int32_t u = users[done], i = pos[done], j = neg ? neg[done] : 0;
      if (u < 0 || u >= n_users || i < 0 || i >= n_items || j < 0 || j >= n_items) { bad = true; break; }
      int32_t lv = std::max(last_user_[(size_t)u], last_item_[(size_t)i]);
      if (neg) lv = std::max(lv, last_item_[(size_t)j]);
      ++lv;
      out.level[(size_t)done] = lv;
      last_user_[(size_t)u] = lv;
      last_item_[(size_t)i] = lv;
      if (neg) last_item_[(size_t)j] = lv;
      top = std::max(top, lv);
    }
    for (int64_t t = 0; t < done; ++t) {      // the tables are zero again for the next batch
      last_user_[(size_t)users[t]] = 0;
      last_item_[(size_t)pos[t]] = 0;
      if (neg) last_item_[(size_t)neg[t]] = 0;
    }
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

 private:
  std::vector<int32_t> last_user_, last_item_;
};

}  // namespace ganmf
