// dense.hip -- the int8 bounds of a whole batch on the matrix cores (dense_kernels.hpp), and the instantiations of the
// one-wave-per-query traversal that read them from the table (wave_kernels.hpp: DENSE).
#include "engine.hpp"
#include "dense_kernels.hpp"
#include "wave_kernels.hpp"

namespace hg {

template <int N, int R, bool L>
static HnswKernelFn wave_dense_kernel(const HnswLaunchPlan &p) {
    return p.vis_global ? &hnsw_wave_kernel<N, R, L, true, false, true> : &hnsw_wave_kernel<N, R, L, false, false, true>;
}

// (the rows in flight of the rejection test's cell: a plan with the table has the test on.  768-float rows, nch 3: two or four,
// the plan's choice -- without the query code and the int8 loop four rows fit 128 VGPRs: hnsw_launch_plan, dense_rows)
HnswKernelFn hnsw_wave_dense_kernel_for(const HnswLaunchPlan &p, const HnswArgs &a) {
    const bool l2 = a.metric == METRIC_L2;
    if (p.nch == 3 && p.dense_rows == 4) return l2 ? wave_dense_kernel<3, 4, true>(p) : wave_dense_kernel<3, 4, false>(p);
#define PICK(N, R, RF) return l2 ? wave_dense_kernel<N, RF, true>(p) : wave_dense_kernel<N, RF, false>(p)
    HG_HNSW_ROWS(p.nch, 2, PICK);
#undef PICK
}

size_t hnsw_dense_code_bytes(int nch, int32_t nq) {
    return (sizeof(uint32_t) * 2 * kWave * nch * static_cast<size_t>(nq) + 255) & ~static_cast<size_t>(255);
}

int64_t hnsw_dense_ld(int64_t n) { return (n + kDenseLd - 1) / kDenseLd * kDenseLd; }

// Query codes, then the table: two launches in front of the traversal.  codes: hnsw_dense_code_bytes + nq QueryScal.
int launch_hnsw_dense(const hnswgpu_index *idx, const float *d_Q, int64_t qld, int32_t nq, void *codes, float *lb, int64_t lb_ld,
                      hipStream_t st) {
    QueryCodeArgs c;
    c.Q = d_Q;
    c.qld = qld;
    c.dim = idx->dim;
    c.nq = nq;
    c.qcode = static_cast<uint32_t *>(codes);
    c.qscal = reinterpret_cast<QueryScal *>(static_cast<char *>(codes) + hnsw_dense_code_bytes(idx->nch, nq));
    const int blocks = (nq + kNWave - 1) / kNWave;
#define CALL(N, R, L) hipLaunchKernelGGL((hnsw_query_code_kernel<N>), dim3(blocks), dim3(kWG), 0, st, c)
    HG_DISPATCH(idx->nch, false, CALL);
#undef CALL
    HG_HIP(hipGetLastError());
    DenseArgs d;
    d.qcode = c.qcode;
    d.qscal = c.qscal;
    d.qrows = idx->d_qrows;
    d.qmeta = idx->d_qmeta;
    d.lb = lb;
    d.lb_ld = lb_ld;
    d.n = idx->n;
    d.nq = nq;
    d.kbytes = 4 * kWave * idx->nch;
    dense_tiling(d);
    const int64_t places = dense_walk_places(d);
    // one persistent workgroup per CU, a multiple of 8 of them: each stays on one XCD of the walk
    const unsigned grid = static_cast<unsigned>(std::min<int64_t>(places, std::max(8, idx->cus / 8 * 8)));
    // (a workgroup steps its place by the grid once past the last one: that sum stays an int too)
    HG_REQUIRE(places < (1LL << 31) - grid, HNSWGPU_ELIMIT, "too many tiles for one bounds launch");
    d.nvt = static_cast<int32_t>(places);
    static bool attr_done[3][64] = {};
#define CALL(M)                                                                                                              \
    do {                                                                                                                     \
        if (attr_needed(attr_done[M]))                                                                                       \
            HG_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&hnsw_dense_bounds_kernel<M>),                         \
                                       hipFuncAttributeMaxDynamicSharedMemorySize, kDenseLds));                              \
        hipLaunchKernelGGL((hnsw_dense_bounds_kernel<M>), dim3(grid), dim3(kDenseWG), kDenseLds, st, d);                     \
    } while (0)
    static_assert(METRIC_COS == 0 && METRIC_L2 == 1 && METRIC_DOT == 2, "attr_done");
    switch (idx->metric) {
        case METRIC_L2: CALL(METRIC_L2); break;
        case METRIC_DOT: CALL(METRIC_DOT); break;
        default: CALL(METRIC_COS); break;
    }
#undef CALL
    HG_HIP(hipGetLastError());
    return 0;
}

}  // namespace hg
