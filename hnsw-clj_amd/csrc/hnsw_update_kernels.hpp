// hnsw_update_kernels.hpp -- rows of a live HNSW graph take new values (hnsw.hip: hnswgpu_hnsw_update).  The device chain of the
// call's first half, the UNLINK: the mark mask of the call's ids U (lsh_remove_mark_kernel / lsh_remove_rank_kernel of
// remove_kernels.hpp: the rank scan turns the mask into keep bits and counts the rows outside U), the call's rows and their norms
// scattered into copies of the base and the norms (here), and hnswgpu_hnsw_remove's repair with NOTHING renumbered: the list pass,
// the scan, gather, distances, sort, selection and scatter of hnsw_remove_kernels.hpp, the list pass and the scatter instantiated
// with RENUM = false -- an untouched list is copied to its place, a list of a row of U is cleared, a list that holds a member of
// U is selected again from the old graph under the OLD ids.  The staged graph has the shape of the old one (levels and up_off are
// the handle's own: no row's level changes), so HnswRemoveArgs is filled with n1 = n0, blocks1 = blocks0, new_upoff = old_upoff.
// What is here writes rows only: a wave per row of the call, float4 copies, every index checked before its store, no atomics,
// no loop that is not bounded by ld.  The ids of a call are distinct (checked on the host), so no two waves write one row.
// Included by hnsw.hip only.
#pragma once
#include "hnsw_remove_kernels.hpp"

namespace hg {

// words of HnswRemoveArgs::r.gate the host of hnswgpu_hnsw_update compares with what it knows in advance
constexpr int kHnswUpdateGateKept = 2 * kRemoveMaxTables;     // rows outside U by the rank scan: n - m, so m rows are marked
constexpr int kHnswUpdateGateSeen = kHnswRemoveGateRows;      // layer-0 lists of rows outside U the list pass copied or counted: n - m
constexpr int kHnswUpdateGateCleared = kHnswRemoveGateCleared;  // lists of rows of U the list pass cleared: m + their levels summed

struct HnswUpdateRows {
    int64_t n, m, ld;
    const int32_t *ids;   // [m] the call's ids in the caller's order, each in [0, n), distinct (checked on the host)
    const float *stage;   // [m][ld] the caller's rows in the caller's order, padding columns zero
    const float *snorms;  // [m] their norms (row_norms_kernel, as hnswgpu_create)
    float *base, *norms;  // copies of the handle's base and norms
};

// One wave per row of the call: staged row i and its norm replace those of row ids[i] in the copies.
static __global__ __launch_bounds__(kWG) void hnsw_update_rows_kernel(HnswUpdateRows a) {
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t i = static_cast<int64_t>(blockIdx.x) * kNWave + (threadIdx.x >> 6);
    if (i >= a.m) return;  // (wave-uniform)
    const int64_t r = a.ids[i];
    if (r < 0 || r >= a.n) return;  // (the host has refused such a call)
    const float4 *sp = reinterpret_cast<const float4 *>(a.stage + i * a.ld);
    float4 *dp = reinterpret_cast<float4 *>(a.base + r * a.ld);
    for (int64_t j = lane; j < a.ld / 4; j += kWave) dp[j] = sp[j];
    if (lane == 0) a.norms[r] = a.snorms[i];
}

}  // namespace hg
