// solo.hip -- the instantiations of the small-launch HNSW traversal that spreads ONE query over several CUs (solo_kernels.hpp).
// Reference: search-layer-ultra / search-knn, src/hnsw/ultra_fast.clj:151-212, 346-374 (the same traversal, same results).
#include "engine.hpp"
#include "solo_kernels.hpp"

namespace hg {

// (the int8 test stays off on this path -- hnsw_launch_plan --, and every instance takes both row counts of the table: R rows in
// flight per trip of the sequencer's own gathers, RH of a helper wave)
HnswKernelFn hnsw_solo_kernel_for(const HnswLaunchPlan &p, const HnswArgs &a) {
    const bool l2 = a.metric == METRIC_L2;
#define PICK(N, R, RH) return l2 ? &hnsw_solo_kernel<N, R, RH, true> : &hnsw_solo_kernel<N, R, RH, false>
    HG_HNSW_ROWS(p.nch, 4, PICK);
#undef PICK
}

}  // namespace hg
