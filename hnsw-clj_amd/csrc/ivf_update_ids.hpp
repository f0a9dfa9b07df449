// ivf_update_ids.hpp -- what hnswgpu_ivf_update decides about the caller's id list on the host, before anything is enqueued: every
// id lies in [0, n), no id is named twice, and the SLOTS of the call -- slot s is the s-th smallest id.  The one sort serves both:
// equal ids end up adjacent, and the sorted order is the row-id order the movers join their new lists in.  Plain C++, no device:
// tools/ivf_update_ids_check.cpp compiles it alone.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace hg {

// 0 and uid[s] = the s-th smallest id, from[s] = its position in `ids`; or 1 with *at = the position of the first id outside
// [0, n); or 2 with *at = the position of the second mention of the lowest id that is named twice (*first = its first mention).
inline int ivf_update_slots(const int32_t *ids, int64_t m, int64_t n, std::vector<int32_t> &uid, std::vector<int32_t> &from, int64_t *at,
                            int64_t *first) {
    for (int64_t i = 0; i < m; i++)
        if (ids[i] < 0 || ids[i] >= n) {
            *at = i;
            return 1;
        }
    std::vector<int64_t> order(static_cast<size_t>(m > 0 ? m : 0));
    for (int64_t i = 0; i < m; i++) order[i] = i;
    std::sort(order.begin(), order.end(), [ids](int64_t a, int64_t b) { return ids[a] != ids[b] ? ids[a] < ids[b] : a < b; });
    for (int64_t s = 1; s < m; s++)
        if (ids[order[s]] == ids[order[s - 1]]) {
            *first = order[s - 1];
            *at = order[s];
            return 2;
        }
    uid.resize(order.size());  // (distinct ids in [0, n): m <= n < 2^31, positions fit)
    from.resize(order.size());
    for (int64_t s = 0; s < m; s++) {
        uid[s] = ids[order[s]];
        from[s] = static_cast<int32_t>(order[s]);
    }
    return 0;
}

}  // namespace hg
