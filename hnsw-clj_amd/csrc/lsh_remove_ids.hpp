// lsh_remove_ids.hpp -- what hnswgpu_lsh_remove decides about the caller's id list on the host, before anything is enqueued: every
// id lies in [0, n), and how many DISTINCT rows the list names (the list may repeat and come in any order).  Plain C++, no device:
// tools/lsh_remove_ids_check.cpp compiles it alone.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace hg {

// The position of the first id outside [0, n), or -1 when there is none; then *distinct = the rows the list names.
inline int64_t lsh_remove_check_ids(const int32_t *rows, int64_t m, int64_t n, int64_t *distinct) {
    for (int64_t i = 0; i < m; i++)
        if (rows[i] < 0 || rows[i] >= n) return i;
    std::vector<int32_t> sorted(rows, rows + (m > 0 ? m : 0));
    std::sort(sorted.begin(), sorted.end());
    *distinct = std::unique(sorted.begin(), sorted.end()) - sorted.begin();
    return -1;
}

}  // namespace hg
