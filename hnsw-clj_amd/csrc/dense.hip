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

int64_t hnsw_dense_ld(int64_t n) { return (n + kDenseTR - 1) / kDenseTR * kDenseTR; }

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
    d.metric = idx->metric;
    d.nqt = (nq + kDenseTQ - 1) / kDenseTQ;
    d.nrt = static_cast<int32_t>((idx->n + kDenseTR - 1) / kDenseTR);
    d.rp = std::max(1, std::min(kDensePanel, d.nrt / 8));  // (few rows: narrower panels, so that every XCD has one)
    d.nsp = (d.nrt + d.rp - 1) / d.rp;
    const int64_t grid = 8LL * ((d.nsp + 7) / 8) * d.nqt * d.rp;
    HG_REQUIRE(grid < (1LL << 31), HNSWGPU_ELIMIT, "too many tiles for one bounds launch");
    hipLaunchKernelGGL(hnsw_dense_bounds_kernel, dim3(static_cast<unsigned>(grid)), dim3(kWG), 0, st, d);
    HG_HIP(hipGetLastError());
    return 0;
}

}  // namespace hg
