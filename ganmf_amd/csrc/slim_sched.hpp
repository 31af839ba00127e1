// slim_sched.hpp -- the level schedule of a SLIM-BPR sample list (slim_bpr.hpp; lib/abi_slim.inc).  Plain C++, no HIP: the library
// and tests/slim_sched_check.cpp share it.
//
// A sample (user, i, j) of the dense, non-symmetric storage reads and writes rows i and j of S and the optimiser state of i and j,
// nothing else.  It therefore has to run behind the last earlier sample that named i (as its i or its j) and behind the last one that
// named j, and behind nothing else:
//     level[t] = 1 + max(level of the last earlier sample that named pos[t], level of the last earlier sample that named neg[t])
// with 0 for an item nobody has named.  Two samples of one level share no item, so a level is one grid; the levels run in order, one
// launch each, and the launch boundary is the only synchronisation there is.  O(n + n_items) time and memory.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace ganmf {

struct SlimSchedule {
  std::vector<int32_t> level;          // [n] 1-based level of every sample
  std::vector<int64_t> order;          // [n] the samples sorted by level, list order kept inside a level
  std::vector<int64_t> level_start;    // [n_levels + 1] order[level_start[l], level_start[l + 1]) is level l + 1
};

// Returns the number of levels (0 for an empty list), -1 when an item id is outside [0, n_items).
inline int64_t slim_schedule(const int32_t* pos, const int32_t* neg, int64_t n, int64_t n_items, SlimSchedule& out) {
  out.level.assign((size_t)std::max<int64_t>(n, 0), 0);
  out.order.assign((size_t)std::max<int64_t>(n, 0), 0);
  out.level_start.assign(1, 0);
  if (n <= 0) return 0;
  std::vector<int32_t> last((size_t)std::max<int64_t>(n_items, 0), 0);      // level of the last sample that named the item
  int32_t top = 0;
  for (int64_t t = 0; t < n; ++t) {
    const int32_t i = pos[t], j = neg[t];
    if (i < 0 || i >= n_items || j < 0 || j >= n_items) return -1;
    const int32_t lv = 1 + std::max(last[(size_t)i], last[(size_t)j]);
    out.level[(size_t)t] = lv;
    last[(size_t)i] = lv;
    last[(size_t)j] = lv;
    top = std::max(top, lv);
  }
  out.level_start.assign((size_t)top + 1, 0);
  for (int64_t t = 0; t < n; ++t) ++out.level_start[(size_t)out.level[(size_t)t]];      // counts at [level], level >= 1
  for (int32_t l = 1; l <= top; ++l) out.level_start[(size_t)l] += out.level_start[(size_t)l - 1];
  // level_start[l] is now the END of level l; a stable counting sort fills every level from its start
  std::vector<int64_t> at((size_t)top + 1, 0);
  for (int32_t l = 1; l <= top; ++l) at[(size_t)l] = out.level_start[(size_t)l - 1];
  for (int64_t t = 0; t < n; ++t) out.order[(size_t)at[(size_t)out.level[(size_t)t]]++] = t;
  return top;
}

}  // namespace ganmf
