// What hnswgpu_lsh_remove decides about its id list on the host (hnsw-clj_amd/csrc/lsh_remove_ids.hpp), exercised without a device:
// the range check names the first offending position, the distinct count ignores order and repeats.  Meant for a sanitizer build:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/lsh_remove_ids_check.cpp -o lsh_remove_ids_check
//   ./lsh_remove_ids_check
#include <stdio.h>
#include <stdlib.h>

#include <random>
#include <set>
#include <vector>

#include "../hnsw-clj_amd/csrc/lsh_remove_ids.hpp"

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            fprintf(stderr, "%s:%d: %s is false\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                       \
        }                                                                  \
    } while (0)

int main() {
    int64_t d = -7;
    // nothing named: nothing distinct, and a null list is never read
    CHECK(hg::lsh_remove_check_ids(nullptr, 0, 10, &d) == -1 && d == 0);
    {
        const std::vector<int32_t> v = {3, 1, 3, 9, 0, 1, 3};
        CHECK(hg::lsh_remove_check_ids(v.data(), (int64_t)v.size(), 10, &d) == -1 && d == 4);
        d = -7;  // n == 9: the 9 at position 3 is out of range, and *distinct is not written
        CHECK(hg::lsh_remove_check_ids(v.data(), (int64_t)v.size(), 9, &d) == 3 && d == -7);
    }
    {
        const std::vector<int32_t> v = {0, 5, -1, 11};
        CHECK(hg::lsh_remove_check_ids(v.data(), 4, 10, &d) == 2);   // the FIRST offender
        CHECK(hg::lsh_remove_check_ids(v.data(), 2, 10, &d) == -1 && d == 2);
        CHECK(hg::lsh_remove_check_ids(v.data(), 1, 0, &d) == 0);    // an empty index has no rows to name
    }
    {
        const std::vector<int32_t> v = {2147483646, 0, 2147483646};
        CHECK(hg::lsh_remove_check_ids(v.data(), 3, 2147483647LL, &d) == -1 && d == 2);
        CHECK(hg::lsh_remove_check_ids(v.data(), 3, 2147483646LL, &d) == 0);
    }
    std::mt19937 rng(1);
    for (int round = 0; round < 200; round++) {  // against std::set, lists longer and shorter than n
        const int64_t n = 1 + rng() % 300, m = rng() % 700;
        std::vector<int32_t> v(m);
        std::set<int32_t> s;
        for (auto &x : v) {
            x = (int32_t)(rng() % n);
            s.insert(x);
        }
        CHECK(hg::lsh_remove_check_ids(v.data(), m, n, &d) == -1 && d == (int64_t)s.size());
        if (m > 0) {
            const int64_t at = rng() % m;
            v[at] = (rng() & 1) ? (int32_t)n : -1 - (int32_t)(rng() % 5);
            int64_t first = at;
            for (int64_t i = 0; i < at; i++)
                if (v[i] < 0 || v[i] >= n) first = std::min(first, i);
            CHECK(hg::lsh_remove_check_ids(v.data(), m, n, &d) == first);
        }
    }
    printf("lsh_remove_ids_check: ok\n");
    return 0;
}
