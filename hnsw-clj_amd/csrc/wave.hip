// wave.hip -- the instantiations of the one-wave-per-query HNSW traversal of large launches (wave_kernels.hpp).
// Reference: search-layer-ultra / search-knn, src/hnsw/ultra_fast.clj:151-212, 346-374 (the same traversal, same results).
#include "engine.hpp"
#include "order_kernels.hpp"
#include "wave_kernels.hpp"

namespace hg {

template <int N, int R, bool L>
static HnswKernelFn wave_kernel(const HnswLaunchPlan &p) {
    return p.vis_global ? &hnsw_wave_kernel<N, R, L, true> : &hnsw_wave_kernel<N, R, L, false>;
}

HnswKernelFn hnsw_wave_kernel_for(const HnswLaunchPlan &p, const HnswArgs &a) {
    const bool l2 = a.metric == METRIC_L2;
#define PICK(N, R, RF) HG_HNSW_ROWS_IN_FLIGHT(wave_kernel, N, R, RF)
    HG_HNSW_ROWS(p.nch, 2, PICK);
#undef PICK
}

// The order of an ordered launch (order_kernels.hpp): keys, then the counting sort -- two launches in front of the traversal
int launch_hnsw_order(int nch, const OrderArgs &a, hipStream_t st) {
    const int blocks = (a.nq + kOrderQ - 1) / kOrderQ;
#define CALL(N, R, L) hipLaunchKernelGGL((hnsw_order_key_kernel<N>), dim3(blocks), dim3(kOrderWaves * kWave), 0, st, a)
    HG_DISPATCH(nch, false, CALL);
#undef CALL
    HG_HIP(hipGetLastError());
    hipLaunchKernelGGL(hnsw_order_sort_kernel<kOrderSortWG>, dim3(1), dim3(kOrderSortWG), 0, st, a.keys, a.nq, a.order);
    HG_HIP(hipGetLastError());
    return 0;
}

}  // namespace hg
