// What hnswgpu_ivf_update decides about its id list on the host (hnsw-clj_amd/csrc/ivf_update_ids.hpp), exercised without a device:
// the range check names the first offending position, an id named twice is refused with both positions, and the slots are the ids
// ascending with the positions they came from.  Meant for a sanitizer build:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/ivf_update_ids_check.cpp -o ivf_update_ids_check
//   ./ivf_update_ids_check
#include <stdio.h>
#include <stdlib.h>

#include <numeric>
#include <random>
#include <vector>

#include "../hnsw-clj_amd/csrc/ivf_update_ids.hpp"

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            fprintf(stderr, "%s:%d: %s is false\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                       \
        }                                                                  \
    } while (0)

int main() {
    std::vector<int32_t> uid, from;
    int64_t at = -7, first = -7;
    // nothing named: no slots, and a null list is never read
    CHECK(hg::ivf_update_slots(nullptr, 0, 10, uid, from, &at, &first) == 0 && uid.empty() && from.empty());
    {
        const std::vector<int32_t> v = {7, 2, 9, 0};
        CHECK(hg::ivf_update_slots(v.data(), 4, 10, uid, from, &at, &first) == 0);
        CHECK((uid == std::vector<int32_t>{0, 2, 7, 9}) && (from == std::vector<int32_t>{3, 1, 0, 2}));
        CHECK(hg::ivf_update_slots(v.data(), 4, 9, uid, from, &at, &first) == 1 && at == 2);   // n == 9: the 9 at position 2
        CHECK(hg::ivf_update_slots(v.data(), 1, 0, uid, from, &at, &first) == 1 && at == 0);   // an empty index has no rows to name
    }
    {
        const std::vector<int32_t> v = {0, 5, -1, 11, 5};
        CHECK(hg::ivf_update_slots(v.data(), 5, 10, uid, from, &at, &first) == 1 && at == 2);  // the FIRST offender, before any repeat
        const std::vector<int32_t> w = {4, 8, 3, 8, 3, 3};
        CHECK(hg::ivf_update_slots(w.data(), 6, 10, uid, from, &at, &first) == 2 && first == 2 && at == 4);   // the lowest repeated id
        CHECK(hg::ivf_update_slots(w.data(), 3, 10, uid, from, &at, &first) == 0 && (uid == std::vector<int32_t>{3, 4, 8}));
    }
    {
        const std::vector<int32_t> v = {2147483645, 0, 2147483646};
        CHECK(hg::ivf_update_slots(v.data(), 3, 2147483647LL, uid, from, &at, &first) == 0 && uid[2] == 2147483646 && from[2] == 2);
        CHECK(hg::ivf_update_slots(v.data(), 3, 2147483646LL, uid, from, &at, &first) == 1 && at == 2);
    }
    std::mt19937 rng(1);
    for (int round = 0; round < 200; round++) {  // permutations of distinct ids; then one id repeated
        const int64_t n = 1 + rng() % 300, m = 1 + rng() % n;
        std::vector<int32_t> all(n);
        std::iota(all.begin(), all.end(), 0);
        std::shuffle(all.begin(), all.end(), rng);
        std::vector<int32_t> v(all.begin(), all.begin() + m);
        CHECK(hg::ivf_update_slots(v.data(), m, n, uid, from, &at, &first) == 0 && (int64_t)uid.size() == m);
        for (int64_t s = 0; s < m; s++) CHECK(v[from[s]] == uid[s] && (s == 0 || uid[s - 1] < uid[s]));
        if (m > 1) {
            const int64_t a = rng() % m, b = (a + 1 + rng() % (m - 1)) % m;
            v[b] = v[a];
            CHECK(hg::ivf_update_slots(v.data(), m, n, uid, from, &at, &first) == 2 && first == std::min(a, b) && at == std::max(a, b));
        }
    }
    printf("ivf_update_ids_check: ok\n");
    return 0;
}
