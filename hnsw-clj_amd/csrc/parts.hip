// parts.hip -- the instantiations of the two traversal kernels that read an item table (HnswArgs::items): the forest launches of
// hnswgpu_hnsw_search_parts (hnsw.hip: hnsw_parts_enqueue).  A translation unit of its own, like wave.hip and solo.hip, so that
// the families compile side by side; the instantiations of plain launches are untouched by the item table.
// Reference: partitioned_hnsw.clj:149-196, ivf_hnsw.clj:286-325 (many small graphs, each searched by search-knn).
#include "engine.hpp"
#include "wave_kernels.hpp"

namespace hg {

template <int N, int R, bool L>
static HnswKernelFn parts_kernel(const HnswLaunchPlan &p) {
    if (p.kernel == HnswKernel::Wave)
        return p.vis_global ? &hnsw_wave_kernel<N, R, L, true, true> : &hnsw_wave_kernel<N, R, L, false, true>;
    if (p.vis_global)
        return p.nw == 1 ? &hnsw_search_kernel<N, R, L, 1, true, false, true>
                         : (p.nw == 2 ? &hnsw_search_kernel<N, R, L, 2, true, false, true> : &hnsw_search_kernel<N, R, L, 4, true, false, true>);
    return p.nw == 1 ? &hnsw_search_kernel<N, R, L, 1, false, false, true>
                     : (p.nw == 2 ? &hnsw_search_kernel<N, R, L, 2, false, false, true> : &hnsw_search_kernel<N, R, L, 4, false, false, true>);
}

// Search or Wave, as the plan says (a forest launch is never planned on the helper or the several-CU kernel)
HnswKernelFn hnsw_parts_kernel_for(const HnswLaunchPlan &p, const HnswArgs &a) {
    if (p.kernel != HnswKernel::Search && p.kernel != HnswKernel::Wave) return nullptr;
    const bool l2 = a.metric == METRIC_L2;
#define PICK(N, R, RF) HG_HNSW_ROWS_IN_FLIGHT(parts_kernel, N, R, RF)
    HG_HNSW_ROWS(p.nch, 2, PICK);
#undef PICK
}

}  // namespace hg
