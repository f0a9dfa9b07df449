// parts_kernels.hpp -- the small kernels around a forest launch (hnswgpu_hnsw_search_parts, hnsw.hip): a handle whose rows are
// grouped into parts, every part with an HNSW sub-graph of its own (the reference's partitioned_hnsw.clj:149-196 and
// ivf_hnsw.clj:286-325 on ONE handle).  The traversal itself is hnsw_search_kernel / hnsw_wave_kernel with an item table
// (kernels.hpp, HnswArgs::items); what is here fills that table from the caller's probe table and puts the per-item counters into
// the caller's layout.  No host pass and no read-back on the path.
#pragma once
#include "kernels.hpp"

namespace hg {

// Work item r * nq + q is (query q, its r-th probe): the [nshard][nq][k_in] layout of merge_shards_kernel, the probe being the
// shard, so that the merge keeps the earlier probe first among equal distances.
// parts[p] = (first row, entry row or -1 for an empty part, top level, rows); probes: [nq][nprobe] part ids, -1 = skip, null =
// every part in order (nprobe = nparts).  An id outside [0, nparts) is a skip.
__global__ __launch_bounds__(256) void parts_items_kernel(const int32_t *probes, int32_t nq, int32_t nprobe, const int4 *parts,
                                                          int32_t nparts, int4 *items) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= static_cast<int64_t>(nq) * nprobe) return;
    const int32_t r = static_cast<int32_t>(i / nq), q = static_cast<int32_t>(i % nq);
    const int32_t p = probes ? probes[static_cast<int64_t>(q) * nprobe + r] : r;
    int4 it = make_int4(q, -1, 0, 0);
    if (p >= 0 && p < nparts) {
        const int4 pt = parts[p];
        it = make_int4(q, pt.y, pt.z, pt.x);
    }
    items[i] = it;
}

// counters [nprobe][nq][2] (by item) -> the caller's [nq][nprobe][2]
__global__ __launch_bounds__(256) void parts_stats_kernel(const int64_t *by_item, int32_t nq, int32_t nprobe, int64_t *out) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= static_cast<int64_t>(nq) * nprobe) return;
    const int64_t r = i / nq, q = i % nq;
    out[2 * (q * nprobe + r)] = by_item[2 * i];
    out[2 * (q * nprobe + r) + 1] = by_item[2 * i + 1];
}

}  // namespace hg
