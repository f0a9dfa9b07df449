// pcaf.hip -- P-HNSW on one handle (src/hnsw/ann/dimreduct/pcaf.clj): the random projection, the projected rows and their
// norms as state of an ordinary cosine handle, and search-pcaf-parallel for a batch in three launches (C ABI:
// include/hnswgpu.h, "P-HNSW"; kernels: pcaf_kernels.hpp).
#include <string.h>

#include <cmath>
#include <vector>

#include "engine.hpp"
#include "javarandom.hpp"
#include "ivf_update_ids.hpp"
#include "lsh_remove_ids.hpp"
#include "pcaf_kernels.hpp"
#include "pcaf_mutate_kernels.hpp"

namespace hg {

constexpr size_t kPcafLdsMax = 160 * 1024;   // LDS of a gfx950 workgroup
constexpr int32_t kPcafSlice = 65536;        // queries (rows of hnswgpu_pcaf_project) per pass over the scratch buffers

static int pcaf_tp(int32_t T) { return (T + 7) & ~7; }

// X [m][dim] (row stride xld, device) -> out [m][Tp], norms [m]; with `dst` (device, [m]) row r goes to row dst[r] of out / norms,
// which hold n_dst rows (the MAP form of the kernel: hnswgpu_pcaf_update)
static int launch_pcaf_project(const hnswgpu_index *idx, const float *P, int32_t T, const float *X, int64_t xld, int64_t m, float *out,
                               float *norms, hipStream_t st, const int32_t *dst = nullptr, int64_t n_dst = 0) {
    if (m <= 0) return 0;
    PcafProjectArgs a;
    a.X = X;
    a.xld = xld;
    a.m = m;
    a.dim = idx->dim;
    a.vec = (xld % 4 == 0 && reinterpret_cast<uintptr_t>(X) % 16 == 0) ? 1 : 0;
    a.P = P;
    a.pld = idx->ld;
    a.T = T;
    a.Tp = pcaf_tp(T);
    a.out = out;
    a.norms = norms;
    a.dst = dst;
    a.n_dst = n_dst;
    const dim3 grid(static_cast<unsigned>((m + kPcafProjRows - 1) / kPcafProjRows));
    const int nt = (a.Tp + 31) / 32;
#define CALL(NT)                                                                                       \
    do {                                                                                               \
        if (dst) hipLaunchKernelGGL((pcaf_project_kernel<NT, true>), grid, dim3(kWG), 0, st, a);       \
        else hipLaunchKernelGGL((pcaf_project_kernel<NT, false>), grid, dim3(kWG), 0, st, a);          \
    } while (0)
    if (nt <= 1) CALL(1);
    else if (nt <= 2) CALL(2);
    else if (nt <= 4) CALL(4);
    else CALL(8);
#undef CALL
    HG_HIP(hipGetLastError());
    return 0;
}

// The shape of a filter launch.  Waves per workgroup: as many of 8, 4, 2, 1 as the LDS holds (a wave's row buffer is
// 32 (Tp + 4) floats beside the query block and the 2 kf keys per query).  Slabs: whole steps of nw * 32 rows, as many slabs as
// give every CU a workgroup at the batch's number of query blocks -- at T = 100 a workgroup takes most of a CU's LDS, so more
// workgroups than CUs would queue, and every slab costs the merge kf more keys per query.  `masked`: the launch is
// pcaf_filter_masked_kernel's, whose waves keep their id buffers beside the rest (pcaf_filter_masked_lds).
struct PcafFilterPlan {
    int nw;
    size_t lds;
    int64_t slab_rows;
    int32_t nslabs;
};
static PcafFilterPlan pcaf_filter_plan(const hnswgpu_index *idx, int32_t nq, int32_t kf, bool masked) {
    const auto lds = [&](int nw) { return masked ? pcaf_filter_masked_lds(idx->pcaf_Tp, kf, nw) : pcaf_filter_lds(idx->pcaf_Tp, kf, nw); };
    PcafFilterPlan p;
    p.nw = 8;
    while (p.nw > 1 && lds(p.nw) > kPcafLdsMax) p.nw >>= 1;
    p.lds = lds(p.nw);
    const int64_t step = p.nw * 32, steps = (idx->n + step - 1) / step, qblocks = (nq + 31) / 32;
    const int64_t want = std::max<int64_t>(1, (idx->cus + qblocks - 1) / qblocks);
    p.slab_rows = std::max<int64_t>(1, (steps + want - 1) / want) * step;
    p.nslabs = static_cast<int32_t>((idx->n + p.slab_rows - 1) / p.slab_rows);
    return p;
}

static int launch_pcaf_filter(const PcafFilterArgs &a, const PcafFilterPlan &p, hipStream_t st) {
    const int nv = a.Tp / 8;
    const dim3 grid(static_cast<unsigned>(static_cast<int64_t>((a.nq + 31) / 32) * a.nslabs)), block(p.nw * kWave);
#define CALL(NV)                                                                                                             \
    do {                                                                                                                     \
        static bool attr_done[64] = {};                                                                                      \
        if (attr_needed(attr_done))                                                                                          \
            HG_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&pcaf_filter_kernel<NV>),                              \
                                       hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(kPcafLdsMax)));          \
        hipLaunchKernelGGL((pcaf_filter_kernel<NV>), grid, block, p.lds, st, a);                                             \
    } while (0)
    if (nv <= 4) CALL(4);
    else if (nv <= 8) CALL(8);
    else if (nv <= 13) CALL(13);
    else if (nv <= 16) CALL(16);
    else if (nv <= 24) CALL(24);
    else CALL(32);
#undef CALL
    HG_HIP(hipGetLastError());
    return 0;
}

// the same grid and NV over pcaf_filter_masked_kernel, x the form of the mask (a.allow_stride != 0: one mask per query)
static int launch_pcaf_filter_masked(const PcafMaskedArgs &a, const PcafFilterPlan &p, hipStream_t st) {
    const int nv = a.Tp / 8;
    const bool each = a.allow_stride != 0;
    const dim3 grid(static_cast<unsigned>(static_cast<int64_t>((a.nq + 31) / 32) * a.nslabs)), block(p.nw * kWave);
#define CALLE(NV, E)                                                                                                         \
    do {                                                                                                                     \
        static bool attr_done[64] = {};                                                                                      \
        if (attr_needed(attr_done))                                                                                          \
            HG_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&pcaf_filter_masked_kernel<NV, E>),                    \
                                       hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(kPcafLdsMax)));          \
        hipLaunchKernelGGL((pcaf_filter_masked_kernel<NV, E>), grid, block, p.lds, st, a);                                   \
    } while (0)
#define CALL(NV)                  \
    do {                          \
        if (each) CALLE(NV, true); \
        else CALLE(NV, false);    \
    } while (0)
    if (nv <= 4) CALL(4);
    else if (nv <= 8) CALL(8);
    else if (nv <= 13) CALL(13);
    else if (nv <= 16) CALL(16);
    else if (nv <= 24) CALL(24);
    else CALL(32);
#undef CALL
#undef CALLE
    HG_HIP(hipGetLastError());
    return 0;
}

static int launch_pcaf_refine(int nch, const PcafRefineArgs &a, int32_t nq, hipStream_t st) {
#define CALL(N, R, L) hipLaunchKernelGGL((pcaf_refine_kernel<N>), dim3(nq), dim3(kWG), 0, st, a)
    HG_DISPATCH(nch, false, CALL);
#undef CALL
    HG_HIP(hipGetLastError());
    return 0;
}

static const char *pcaf_other_state(const hnswgpu_index *idx) {
    if (idx->nparts > 0) return "an HNSW forest";
    if (idx->has_graph) return "an HNSW graph";
    if (idx->nlist > 0) return "IVF lists";
    if (idx->lsh_tables > 0) return "LSH tables";
    return nullptr;
}

// What a build or an install stages: the handle takes it over only when every step has succeeded.
struct PcafStaged {
    float *proj = nullptr, *low = nullptr, *lnorms = nullptr;
    ~PcafStaged() {
        void *ptrs[] = {proj, low, lnorms};
        for (void *p : ptrs)
            if (p) (void)hipFree(p);
    }
};

// The rows of a handle in all their pieces as hnswgpu_pcaf_add / _remove / _update stage them (the projection stays the
// handle's): what is left in it when it goes out of scope is freed -- the staged arrays on an early return, the handle's old ones
// behind the swap.
struct PcafStagedRows {
    float *base = nullptr, *norms = nullptr, *low = nullptr, *lnorms = nullptr;
    uint32_t *qrows = nullptr;
    float4 *qmeta = nullptr;
    ~PcafStagedRows() {
        void *ptrs[] = {base, norms, low, lnorms, qrows, qmeta};
        for (void *p : ptrs)
            if (p) (void)hipFree(p);
    }
    // room for n rows (none for n == 0: the empty handle pcaf_install leaves has null arrays)
    int alloc(const hnswgpu_index *idx, int64_t n) {
        if (n <= 0) return 0;
        const size_t nn = static_cast<size_t>(n);
        HG_HIP(hipMalloc(reinterpret_cast<void **>(&base), sizeof(float) * nn * idx->ld));
        HG_HIP(hipMalloc(reinterpret_cast<void **>(&norms), sizeof(float) * nn));
        HG_HIP(hipMalloc(reinterpret_cast<void **>(&low), sizeof(float) * nn * idx->pcaf_Tp));
        HG_HIP(hipMalloc(reinterpret_cast<void **>(&lnorms), sizeof(float) * nn));
        return 0;
    }
    // the first n0 rows' four pieces as the handle has them: copied on the device, never computed again
    int copy_old(const hnswgpu_index *idx, int64_t n0, hipStream_t st) {
        if (n0 <= 0) return 0;
        const size_t nn = static_cast<size_t>(n0);
        HG_HIP(hipMemcpyAsync(base, idx->d_base, sizeof(float) * nn * idx->ld, hipMemcpyDeviceToDevice, st));
        HG_HIP(hipMemcpyAsync(norms, idx->d_norms, sizeof(float) * nn, hipMemcpyDeviceToDevice, st));
        HG_HIP(hipMemcpyAsync(low, idx->d_pcaf_low, sizeof(float) * nn * idx->pcaf_Tp, hipMemcpyDeviceToDevice, st));
        HG_HIP(hipMemcpyAsync(lnorms, idx->d_pcaf_lnorms, sizeof(float) * nn, hipMemcpyDeviceToDevice, st));
        return 0;
    }
    void swap_into(hnswgpu_index *idx, int64_t n) {
        std::swap(idx->d_base, base);  // (what the handle had goes with this object)
        std::swap(idx->d_norms, norms);
        std::swap(idx->d_qrows, qrows);
        std::swap(idx->d_qmeta, qmeta);
        std::swap(idx->d_pcaf_low, low);
        std::swap(idx->d_pcaf_lnorms, lnorms);
        idx->n = n;
    }
};

// m host rows [m][dim] -> dst [m][ld] on the device, padding zero (what hnswgpu_create does with its base)
static int pcaf_upload_rows(const hnswgpu_index *idx, const float *rows, int64_t m, float *dst, hipStream_t st) {
    const size_t mm = static_cast<size_t>(m);
    if (idx->ld == idx->dim) {  // one run of bytes: a 2-D copy of the same rows from pageable memory took 9 us a row on an MI355X
        HG_HIP(hipMemcpyAsync(dst, rows, sizeof(float) * mm * idx->dim, hipMemcpyHostToDevice, st));
        return 0;
    }
    HG_HIP(hipMemsetAsync(dst, 0, sizeof(float) * mm * idx->ld, st));
    HG_HIP(hipMemcpy2DAsync(dst, sizeof(float) * idx->ld, rows, sizeof(float) * idx->dim, sizeof(float) * idx->dim, mm,
                            hipMemcpyHostToDevice, st));
    return 0;
}

// P: [T][dim] on the host
static int pcaf_install(hnswgpu_index *idx, Call &call, const float *P, int32_t T, hipStream_t st) {
    const char *other = pcaf_other_state(idx);
    HG_REQUIRE(!other, HNSWGPU_ESTATE, "index holds %s: P-HNSW state goes on a handle that holds rows only", other);
    const int64_t n = idx->n, ld = idx->ld;
    const int Tp = pcaf_tp(T);
    PcafStaged s;
    HG_HIP(hipMalloc(reinterpret_cast<void **>(&s.proj), sizeof(float) * T * ld));
    if (ld != idx->dim) HG_HIP(hipMemsetAsync(s.proj, 0, sizeof(float) * T * ld, st));
    HG_HIP(hipMemcpy2DAsync(s.proj, sizeof(float) * ld, P, sizeof(float) * idx->dim, sizeof(float) * idx->dim, T, hipMemcpyHostToDevice, st));
    if (n > 0) {
        HG_HIP(hipMalloc(reinterpret_cast<void **>(&s.low), sizeof(float) * n * Tp));
        HG_HIP(hipMalloc(reinterpret_cast<void **>(&s.lnorms), sizeof(float) * n));
        HG_TRY(launch_pcaf_project(idx, s.proj, T, idx->d_base, ld, n, s.low, s.lnorms, st));
    }
    std::vector<float> keep(P, P + static_cast<size_t>(T) * idx->dim);
    HG_TRY(call.quiesce());  // the upload is done, and no search reads the old state any more
    std::swap(idx->d_pcaf_proj, s.proj);  // (what the handle had goes with `s`)
    std::swap(idx->d_pcaf_low, s.low);
    std::swap(idx->d_pcaf_lnorms, s.lnorms);
    idx->h_pcaf_proj.swap(keep);
    idx->pcaf_T = T;
    idx->pcaf_Tp = Tp;
    return 0;
}

static int check_pcaf_shape(const hnswgpu_index *idx, int32_t T) {
    HG_REQUIRE(idx, HNSWGPU_EINVAL, "idx is null");
    HG_REQUIRE(idx->metric == METRIC_COS, HNSWGPU_EINVAL, "P-HNSW needs a cosine handle (pcaf.clj uses cosine in both phases)");
    HG_REQUIRE(T >= 1, HNSWGPU_EINVAL, "n_components must be >= 1");
    HG_REQUIRE(T <= kPcafMaxT, HNSWGPU_ELIMIT, "n_components > %d is not supported", kPcafMaxT);
    return 0;
}

#define HG_PCAF_STATE(idx) \
    HG_REQUIRE((idx)->pcaf_T > 0, HNSWGPU_ESTATE, "index has no P-HNSW state (call hnswgpu_pcaf_build / hnswgpu_set_pcaf first)")

// d_Q [nq][dim] -> d_ids / d_dist [nq][k] on `st`; only enqueues: projection, filter, merge + refine per slice of queries.
// d_allow: null -- the unfiltered search; else the mask of query q is d_allow + q * allow_stride ((n + 31) / 32 words; stride 0:
// one mask for the call) and the filter is the masked one.  Projection, key scratch and refine are the same either way.
static int pcaf_search_enqueue(hnswgpu_index *idx, const float *d_Q, int32_t nq, int32_t k, int32_t kf, const uint32_t *d_allow,
                               int64_t allow_stride, int32_t *d_ids, float *d_dist, hipStream_t st) {
    const int Tp = idx->pcaf_Tp;
    const int32_t slice = std::min(nq, kPcafSlice);
    const PcafFilterPlan plan = pcaf_filter_plan(idx, slice, kf, d_allow != nullptr);
    HG_TRY(idx->s_pcaf_q.ensure(sizeof(float) * static_cast<size_t>(slice) * (Tp + 1)));
    HG_TRY(idx->s_pcaf_keys.ensure(sizeof(uint64_t) * static_cast<size_t>(slice) * plan.nslabs * kf));
    float *qlow = idx->s_pcaf_q.as<float>(), *qnorms = qlow + static_cast<size_t>(slice) * Tp;
    for (int32_t q0 = 0; q0 < nq; q0 += slice) {
        const int32_t m = std::min(slice, nq - q0);
        const float *Qs = d_Q + static_cast<int64_t>(q0) * idx->dim;
        HG_TRY(launch_pcaf_project(idx, idx->d_pcaf_proj, idx->pcaf_T, Qs, idx->dim, m, qlow, qnorms, st));
        PcafMaskedArgs f;
        f.rows = idx->d_pcaf_low;
        f.row_norms = idx->d_pcaf_lnorms;
        f.n = idx->n;
        f.Q = qlow;
        f.q_norms = qnorms;
        f.nq = m;
        f.Tp = Tp;
        f.kf = kf;
        f.slab_rows = plan.slab_rows;
        f.nslabs = plan.nslabs;
        f.keys = idx->s_pcaf_keys.as<uint64_t>();
        f.allow = d_allow ? d_allow + static_cast<int64_t>(q0) * allow_stride : nullptr;
        f.allow_stride = allow_stride;
        HG_TRY(d_allow ? launch_pcaf_filter_masked(f, plan, st) : launch_pcaf_filter(f, plan, st));
        PcafRefineArgs r;
        r.keys = f.keys;
        r.nslabs = plan.nslabs;
        r.kf = kf;
        r.k = k;
        r.rows = idx->d_base;
        r.row_norms = idx->d_norms;
        r.ld = idx->ld;
        r.Q = Qs;
        r.qld = idx->dim;
        r.dim = idx->dim;
        r.out_ids = d_ids + static_cast<int64_t>(q0) * k;
        r.out_dist = d_dist + static_cast<int64_t>(q0) * k;
        HG_TRY(launch_pcaf_refine(idx->nch, r, m, st));
    }
    return 0;
}

// Everything hnswgpu_pcaf_search* checks before the lock; *kf: min(k_filter, 3 k) (pcaf.clj:236), not yet clamped to n
static int check_pcaf_search(const hnswgpu_index *idx, const void *Q, int32_t nq, int32_t k, int32_t k_filter, const void *ids,
                             const void *dist, int32_t *kf) {
    HG_REQUIRE(idx, HNSWGPU_EINVAL, "idx is null");
    HG_REQUIRE(nq >= 0, HNSWGPU_EINVAL, "nq < 0");
    HG_REQUIRE(k >= 1, HNSWGPU_EINVAL, "k must be >= 1");
    HG_REQUIRE(k <= 1024, HNSWGPU_ELIMIT, "k > 1024 is not supported");
    HG_REQUIRE(nq == 0 || (Q && ids && dist), HNSWGPU_EINVAL, "null argument");
    *kf = static_cast<int32_t>(std::min<int64_t>(k_filter <= 0 ? 32 : k_filter, 3 * static_cast<int64_t>(k)));  // (:122, :236)
    return 0;
}

}  // namespace hg

using namespace hg;

extern "C" {

int hnswgpu_pcaf_build(hnswgpu_index *idx, int32_t n_components, int64_t seed) {
    HG_TRY(check_pcaf_shape(idx, n_components));
    // (create-random-projection, :33-45: row by row, float(gaussian) * float(1 / sqrt(target-dim)))
    std::vector<float> P(static_cast<size_t>(n_components) * idx->dim);
    const float scale = static_cast<float>(1.0 / std::sqrt(static_cast<double>(n_components)));
    JavaRandom rng(seed);
    for (float &p : P) p = scale * static_cast<float>(rng.next_gaussian());
    hipStream_t st = idx->stream;
    Call call;
    HG_TRY(call.open(idx, st));
    HG_TRY(pcaf_install(idx, call, P.data(), n_components, st));
    HG_TRY(call.sync());
    return call.close();
}

int hnswgpu_set_pcaf(hnswgpu_index *idx, const float *projection, int32_t n_components) {
    HG_TRY(check_pcaf_shape(idx, n_components));
    HG_REQUIRE(projection, HNSWGPU_EINVAL, "null argument");
    hipStream_t st = idx->stream;
    Call call;
    HG_TRY(call.open(idx, st));
    HG_TRY(pcaf_install(idx, call, projection, n_components, st));
    HG_TRY(call.sync());
    return call.close();
}

int hnswgpu_pcaf_sizes(hnswgpu_index *idx, int32_t *n_components) {
    HG_REQUIRE(idx, HNSWGPU_EINVAL, "idx is null");
    std::lock_guard<std::mutex> lk(idx->mu);
    if (n_components) *n_components = idx->pcaf_T;
    return 0;
}

int hnswgpu_pcaf_get(hnswgpu_index *idx, float *projection, float *low_rows) {
    HG_REQUIRE(idx, HNSWGPU_EINVAL, "idx is null");
    hipStream_t st = idx->stream;
    Call call;
    HG_TRY(call.open(idx, st));
    HG_PCAF_STATE(idx);
    if (projection) memcpy(projection, idx->h_pcaf_proj.data(), sizeof(float) * idx->h_pcaf_proj.size());
    if (low_rows && idx->n > 0)
        HG_HIP(hipMemcpy2DAsync(low_rows, sizeof(float) * idx->pcaf_T, idx->d_pcaf_low, sizeof(float) * idx->pcaf_Tp,
                                sizeof(float) * idx->pcaf_T, idx->n, hipMemcpyDeviceToHost, st));
    HG_TRY(call.sync());
    return call.close();
}

int hnswgpu_pcaf_project(hnswgpu_index *idx, const float *X, int64_t m, float *out) {
    HG_REQUIRE(idx, HNSWGPU_EINVAL, "idx is null");
    HG_REQUIRE(m >= 0, HNSWGPU_EINVAL, "m < 0");
    HG_REQUIRE(m == 0 || (X && out), HNSWGPU_EINVAL, "null argument");
    if (m == 0) return 0;
    hipStream_t st = idx->stream;
    Call call;
    HG_TRY(call.open(idx, st));
    HG_PCAF_STATE(idx);
    const int T = idx->pcaf_T, Tp = idx->pcaf_Tp;
    const int32_t slice = static_cast<int32_t>(std::min<int64_t>(m, kPcafSlice));
    HG_TRY(idx->s_pcaf_q.ensure(sizeof(float) * static_cast<size_t>(slice) * (Tp + 1)));
    float *low = idx->s_pcaf_q.as<float>(), *norms = low + static_cast<size_t>(slice) * Tp;
    for (int64_t r0 = 0; r0 < m; r0 += slice) {
        const int32_t c = static_cast<int32_t>(std::min<int64_t>(slice, m - r0));
        HG_TRY(upload_queries(idx, X + r0 * idx->dim, c, st));
        HG_TRY(launch_pcaf_project(idx, idx->d_pcaf_proj, T, idx->s_q.as<float>(), idx->dim, c, low, norms, st));
        HG_HIP(hipMemcpy2DAsync(out + r0 * T, sizeof(float) * T, low, sizeof(float) * Tp, sizeof(float) * T, c, hipMemcpyDeviceToHost, st));
    }
    HG_TRY(call.sync());
    return call.close();
}

int hnswgpu_pcaf_search_dev(hnswgpu_index *idx, const float *d_Q, int32_t nq, int32_t k, int32_t k_filter, int32_t *d_out_ids,
                            float *d_out_dist, void *stream) {
    int32_t kf;
    HG_TRY(check_pcaf_search(idx, d_Q, nq, k, k_filter, d_out_ids, d_out_dist, &kf));
    if (nq == 0) return 0;
    HG_REQUIRE(idx->n > 0, HNSWGPU_ESTATE, "empty index: use the host entry point");
    hipStream_t st = static_cast<hipStream_t>(stream);
    Call call;
    HG_TRY(call.open(idx, st));
    HG_PCAF_STATE(idx);
    kf = static_cast<int32_t>(std::min<int64_t>(kf, idx->n));
    HG_REQUIRE(kf <= kPcafMaxKf, HNSWGPU_ELIMIT, "min(k_filter, 3 k, n) > %d is not supported", kPcafMaxKf);
    HG_TRY(pcaf_search_enqueue(idx, d_Q, nq, k, kf, nullptr, 0, d_out_ids, d_out_dist, st));
    return call.close();
}

int hnswgpu_pcaf_search(hnswgpu_index *idx, const float *Q, int32_t nq, int32_t k, int32_t k_filter, int32_t *out_ids,
                        float *out_dist) {
    int32_t kf;
    HG_TRY(check_pcaf_search(idx, Q, nq, k, k_filter, out_ids, out_dist, &kf));
    if (nq == 0) return 0;
    const int64_t cnt = static_cast<int64_t>(nq) * k;
    hipStream_t st = idx->stream;
    Call call;
    HG_TRY(call.open(idx, st));
    HG_PCAF_STATE(idx);
    if (idx->n == 0) {
        fill_empty(out_ids, out_dist, cnt);
        return call.close();
    }
    kf = static_cast<int32_t>(std::min<int64_t>(kf, idx->n));
    HG_REQUIRE(kf <= kPcafMaxKf, HNSWGPU_ELIMIT, "min(k_filter, 3 k, n) > %d is not supported", kPcafMaxKf);
    HG_TRY(call.stage_in(Q, nq, k));
    HG_TRY(pcaf_search_enqueue(idx, idx->s_q.as<float>(), nq, k, kf, nullptr, 0, idx->s_ids.as<int32_t>(), idx->s_outd.as<float>(), st));
    HG_TRY(call.stage_out(out_ids, out_dist, cnt));
    return call.close();
}

// ---- filtered search: the allow-mask through the low-dimensional filter (pcaf_filter_masked_kernel; the contract:
// include/hnswgpu.h) ----
// One body for both forms of the mask: Single is stride 0, Each stride (n + 31) / 32.  Device arrays: enqueues only, reads
// nothing back -- kf is clamped to n, not to the passing rows, so nothing needs a count.
static int pcaf_filtered_dev(hnswgpu_index *idx, MaskForm form, const float *d_Q, int32_t nq, int32_t k, int32_t k_filter,
                             const uint32_t *d_allow, int32_t *d_out_ids, float *d_out_dist, void *stream) {
    int32_t kf;
    HG_TRY(check_pcaf_search(idx, d_Q, nq, k, k_filter, d_out_ids, d_out_dist, &kf));
    if (nq == 0) return 0;
    HG_REQUIRE(d_allow, HNSWGPU_EINVAL, "allow is null");
    HG_REQUIRE(idx->n > 0, HNSWGPU_ESTATE, "empty index: use the host entry point");
    hipStream_t st = static_cast<hipStream_t>(stream);
    Call call;
    HG_TRY(call.open(idx, st));
    HG_PCAF_STATE(idx);
    kf = static_cast<int32_t>(std::min<int64_t>(kf, idx->n));
    HG_REQUIRE(kf <= kPcafMaxKf, HNSWGPU_ELIMIT, "min(k_filter, 3 k, n) > %d is not supported", kPcafMaxKf);
    const int64_t stride = form == MaskForm::Each ? (idx->n + 31) / 32 : 0;
    HG_TRY(pcaf_search_enqueue(idx, d_Q, nq, k, kf, d_allow, stride, d_out_ids, d_out_dist, st));
    return call.close();
}

// Host arrays.  One caller's batch, its mask -- Each: its [nq][W] masks -- staged whole as hnswgpu_lsh_search_filtered_each
// stages its own: masks differ between callers, so the call takes no part in the call combiner.
static int pcaf_filtered_host(hnswgpu_index *idx, MaskForm form, const float *Q, int32_t nq, int32_t k, int32_t k_filter,
                              const uint32_t *allow, int32_t *out_ids, float *out_dist) {
    int32_t kf;
    HG_TRY(check_pcaf_search(idx, Q, nq, k, k_filter, out_ids, out_dist, &kf));
    if (nq == 0) return 0;
    HG_REQUIRE(allow, HNSWGPU_EINVAL, "allow is null");
    const int64_t cnt = static_cast<int64_t>(nq) * k;
    hipStream_t st = idx->stream;
    Call call;
    HG_TRY(call.open(idx, st));
    HG_PCAF_STATE(idx);
    if (idx->n == 0) {  // (an empty index has no mask words)
        fill_empty(out_ids, out_dist, cnt);
        return call.close();
    }
    kf = static_cast<int32_t>(std::min<int64_t>(kf, idx->n));
    HG_REQUIRE(kf <= kPcafMaxKf, HNSWGPU_ELIMIT, "min(k_filter, 3 k, n) > %d is not supported", kPcafMaxKf);
    HG_TRY(call.stage_in(Q, nq, k));
    HG_TRY(call.stage_mask(allow, form, nq));
    const int64_t stride = form == MaskForm::Each ? (idx->n + 31) / 32 : 0;
    HG_TRY(pcaf_search_enqueue(idx, idx->s_q.as<float>(), nq, k, kf, idx->s_fmask.as<uint32_t>(), stride, idx->s_ids.as<int32_t>(),
                               idx->s_outd.as<float>(), st));
    HG_TRY(call.stage_out(out_ids, out_dist, cnt));
    return call.close();
}

int hnswgpu_pcaf_search_filtered_dev(hnswgpu_index *idx, const float *d_Q, int32_t nq, int32_t k, int32_t k_filter,
                                     const uint32_t *d_allow, int32_t *d_out_ids, float *d_out_dist, void *stream) {
    return pcaf_filtered_dev(idx, MaskForm::Single, d_Q, nq, k, k_filter, d_allow, d_out_ids, d_out_dist, stream);
}
int hnswgpu_pcaf_search_filtered(hnswgpu_index *idx, const float *Q, int32_t nq, int32_t k, int32_t k_filter, const uint32_t *allow,
                                 int32_t *out_ids, float *out_dist) {
    return pcaf_filtered_host(idx, MaskForm::Single, Q, nq, k, k_filter, allow, out_ids, out_dist);
}
int hnswgpu_pcaf_search_filtered_each_dev(hnswgpu_index *idx, const float *d_Q, int32_t nq, int32_t k, int32_t k_filter,
                                          const uint32_t *d_allow_each, int32_t *d_out_ids, float *d_out_dist, void *stream) {
    return pcaf_filtered_dev(idx, MaskForm::Each, d_Q, nq, k, k_filter, d_allow_each, d_out_ids, d_out_dist, stream);
}
int hnswgpu_pcaf_search_filtered_each(hnswgpu_index *idx, const float *Q, int32_t nq, int32_t k, int32_t k_filter,
                                      const uint32_t *allow_each, int32_t *out_ids, float *out_dist) {
    return pcaf_filtered_host(idx, MaskForm::Each, Q, nq, k, k_filter, allow_each, out_ids, out_dist);
}

// ---- rows join, leave and take new values on a live handle (pcaf_mutate_kernels.hpp; the contract: include/hnswgpu.h) ----
// One rule behind all three: afterwards the handle holds, bit for bit, what hnswgpu_create(the rows it should now hold) +
// hnswgpu_set_pcaf(the same projection) holds.  It can, because a row's projection and norm from pcaf_project_kernel depend on the
// row's values and the projection alone.  Failure-atomic as the siblings (hnswgpu_lsh_add): every array a call makes is STAGED
// and goes with `nw` on an early return; the handle's fields change only behind the last step (idx->mu is held and the streams
// are quiesced: no caller sees a state in between).

// Rows join: ids n .. n + m - 1.  One chain on the handle's stream: base / norms / int8 rows grow as in hnswgpu_lsh_add, the
// projected rows and their norms grow behind device copies of the old ones -- the plain projection kernel reads the new rows
// where they sit in the grown base and writes at new_low + n0 * Tp, new_lnorms + n0.
int hnswgpu_pcaf_add(hnswgpu_index *idx, const float *rows, int64_t m) {
    HG_REQUIRE(idx, HNSWGPU_EINVAL, "idx is null");
    HG_REQUIRE(m >= 0, HNSWGPU_EINVAL, "m must be >= 0");
    HG_REQUIRE(rows || m == 0, HNSWGPU_EINVAL, "rows is null");
    if (m == 0) return 0;
    hipStream_t st = idx->stream;
    Call call;
    HG_TRY(call.open(idx, st));
    HG_PCAF_STATE(idx);
    const int64_t n0 = idx->n, n1 = n0 + m, ld = idx->ld;
    HG_REQUIRE(n1 < 2147483647LL, HNSWGPU_ELIMIT, "the index must hold fewer than 2^31 rows");
    HG_TRY(call.quiesce());
    PcafStagedRows nw;
    auto grow = [&]() -> int {
        HG_TRY(nw.alloc(idx, n1));
        HG_TRY(nw.copy_old(idx, n0, st));
        HG_TRY(pcaf_upload_rows(idx, rows, m, nw.base + n0 * ld, st));
        HG_TRY(launch_norms(idx->nch, nw.base + n0 * ld, ld, m, nw.norms + n0, st));
        if (idx->d_qrows) HG_TRY(quantize_rows(idx, nw.base, n1, &nw.qrows, &nw.qmeta, st));  // (all rows again: one pass over the base)
        HG_TRY(launch_pcaf_project(idx, idx->d_pcaf_proj, idx->pcaf_T, nw.base + n0 * ld, ld, m, nw.low + n0 * idx->pcaf_Tp,
                                   nw.lnorms + n0, st));
        HG_HIP(hipStreamSynchronize(st));  // (the upload has read `rows`; a failing step shows before the takeover)
        return 0;
    };
    const int rc = grow();
    if (rc != 0) {
        (void)hipStreamSynchronize(st);  // (nothing of the chain is in flight when `nw` frees what it staged)
        return rc;
    }
    nw.swap_into(idx, n1);
    return call.close();
}

// Rows leave; the kept rows are renumbered densely in their old order.  One chain: mark, rank (remove_kernels.hpp, as
// hnswgpu_ivf_remove reuses them: tables = 0), then ONE pass that moves a kept row's four pieces to its rank.  Only the m ids go
// up; ONE readback: the rank scan's total, which gates the takeover.
int hnswgpu_pcaf_remove(hnswgpu_index *idx, const int32_t *rows, int64_t m, int64_t *n_after) {
    HG_REQUIRE(idx, HNSWGPU_EINVAL, "idx is null");
    HG_REQUIRE(m >= 0, HNSWGPU_EINVAL, "m must be >= 0");
    HG_REQUIRE(rows || m == 0, HNSWGPU_EINVAL, "rows is null");
    if (m == 0) {  // nothing to remove: nothing happens, whatever the handle holds
        std::lock_guard<std::mutex> lk(idx->mu);
        if (n_after) *n_after = idx->n;
        return 0;
    }
    hipStream_t st = idx->stream;
    Call call;
    HG_TRY(call.open(idx, st));
    HG_PCAF_STATE(idx);
    const int64_t n0 = idx->n;
    int64_t distinct = 0, bad = -1;
    try {
        bad = lsh_remove_check_ids(rows, m, n0, &distinct);  // on the host array, before anything is enqueued
    } catch (const std::bad_alloc &) {  // (its sorted copy of the ids)
        set_error("host allocation failed");
        return HNSWGPU_ENOMEM;
    }
    HG_REQUIRE(bad < 0, HNSWGPU_EINVAL, "rows[%lld] = %d is not a row of the index (n = %lld)", (long long)bad, rows[bad], (long long)n0);
    const int64_t n1 = n0 - distinct;
    HG_TRY(call.quiesce());
    PcafStagedRows nw;
    auto shrink = [&]() -> int {
        HG_TRY(nw.alloc(idx, n1));
        // scratch, 16-byte sections: [gate | keep] zeroed, then word_rank and the call's ids
        PcafRemoveArgs a;
        memset(&a, 0, sizeof(a));
        a.r.n0 = n0;
        a.r.n1 = n1;
        a.r.m = m;
        a.r.W = (n0 + 31) / 32;
        a.r.ld = idx->ld;
        auto sect = [](size_t bytes) { return (bytes + 15) / 16 * 16; };
        const size_t o_keep = sect(sizeof(int64_t) * kLshRemoveGate), o_rank = o_keep + sect(sizeof(uint32_t) * a.r.W),
                     o_ids = o_rank + sect(sizeof(uint32_t) * a.r.W), bytes = o_ids + sect(sizeof(int32_t) * m);
        HG_TRY(idx->s_misc.ensure(bytes));
        char *s = idx->s_misc.as<char>();
        HG_HIP(hipMemsetAsync(s, 0, o_rank, st));
        HG_HIP(hipMemcpyAsync(s + o_ids, rows, sizeof(int32_t) * static_cast<size_t>(m), hipMemcpyHostToDevice, st));
        a.r.gate = reinterpret_cast<int64_t *>(s);
        a.r.keep = reinterpret_cast<uint32_t *>(s + o_keep);
        a.r.word_rank = reinterpret_cast<uint32_t *>(s + o_rank);
        a.r.rows = reinterpret_cast<const int32_t *>(s + o_ids);
        a.r.old_base = idx->d_base;
        a.r.old_norms = idx->d_norms;
        a.r.new_base = nw.base;
        a.r.new_norms = nw.norms;
        a.Tp = idx->pcaf_Tp;
        a.old_low = idx->d_pcaf_low;
        a.old_lnorms = idx->d_pcaf_lnorms;
        a.new_low = nw.low;
        a.new_lnorms = nw.lnorms;
        hipLaunchKernelGGL(lsh_remove_mark_kernel, dim3(static_cast<unsigned>((m + kWG - 1) / kWG)), dim3(kWG), 0, st, a.r);
        hipLaunchKernelGGL(lsh_remove_rank_kernel, dim3(1), dim3(kWG), 0, st, a.r);
        if (n1 > 0) hipLaunchKernelGGL(pcaf_remove_rows_kernel, dim3(static_cast<unsigned>((n0 + kNWave - 1) / kNWave)), dim3(kWG), 0, st, a);
        HG_HIP(hipGetLastError());
        if (idx->d_qrows && n1 > 0) HG_TRY(quantize_rows(idx, nw.base, n1, &nw.qrows, &nw.qmeta, st));  // (as add: one pass over the new base)
        // ---- the one readback
        int64_t kept = -1;
        HG_HIP(hipMemcpyAsync(&kept, a.r.gate + 2 * kRemoveMaxTables, sizeof(kept), hipMemcpyDeviceToHost, st));
        HG_HIP(hipStreamSynchronize(st));
        HG_REQUIRE(kept == n1, HNSWGPU_EHIP, "the mask keeps %lld rows, not %lld", (long long)kept, (long long)n1);
        return 0;
    };
    const int rc = shrink();
    if (rc != 0) {
        (void)hipStreamSynchronize(st);  // (nothing of the chain is in flight when `nw` frees what it staged)
        return rc;
    }
    nw.swap_into(idx, n1);  // (n1 == 0: null arrays -- the empty handle with its projection that hnswgpu_pcaf_add grows again)
    if (n_after) *n_after = n1;
    return call.close();
}

// Rows take new values under their ids.  One chain: the call's ids and rows go up once (the rows into a staging matrix [m][ld],
// padding zero); their norms by the kernel hnswgpu_create uses; device copies of the four arrays; pcaf_update_place_kernel puts
// the staged rows and norms where the ids name, and the MAP form of the projection kernel projects the staged rows straight into
// the copies of the projected rows and their norms.  Every slot writes its own row only: the result does not depend on the order
// of `ids` or on the split of calls.
int hnswgpu_pcaf_update(hnswgpu_index *idx, const int32_t *ids, const float *rows, int64_t m) {
    HG_REQUIRE(idx, HNSWGPU_EINVAL, "idx is null");
    HG_REQUIRE(m >= 0, HNSWGPU_EINVAL, "m must be >= 0");
    HG_REQUIRE(ids || m == 0, HNSWGPU_EINVAL, "ids is null");
    HG_REQUIRE(rows || m == 0, HNSWGPU_EINVAL, "rows is null");
    if (m == 0) return 0;  // nothing to update: nothing happens, whatever the handle holds
    hipStream_t st = idx->stream;
    Call call;
    HG_TRY(call.open(idx, st));
    HG_PCAF_STATE(idx);
    const int64_t n = idx->n, ld = idx->ld;
    std::vector<int32_t> uid, from;
    int64_t at = -1, first = -1;
    int verdict;
    try {
        verdict = ivf_update_slots(ids, m, n, uid, from, &at, &first);  // on the host array, before anything is enqueued
    } catch (const std::bad_alloc &) {  // (its sorted copy of the ids)
        set_error("host allocation failed");
        return HNSWGPU_ENOMEM;
    }
    HG_REQUIRE(verdict != 1, HNSWGPU_EINVAL, "ids[%lld] = %d is not a row of the index (n = %lld)", (long long)at, ids[at], (long long)n);
    HG_REQUIRE(verdict != 2, HNSWGPU_EINVAL, "ids[%lld] = %d is named twice (first at ids[%lld]): two values for one row have no winner",
               (long long)at, ids[at], (long long)first);
    HG_TRY(call.quiesce());
    PcafStagedRows nw;
    auto update = [&]() -> int {
        const size_t mm = static_cast<size_t>(m);
        HG_TRY(nw.alloc(idx, n));
        // scratch.  s_misc: the call's ids (slot s of the call is its s-th id as it came).  s_misc2: the staging matrix | its norms.
        auto sect = [](size_t bytes) { return (bytes + 15) / 16 * 16; };
        HG_TRY(idx->s_misc.ensure(sizeof(int32_t) * mm));
        HG_TRY(idx->s_misc2.ensure(sect(sizeof(float) * mm * ld) + sizeof(float) * mm));
        PcafUpdateArgs a;
        a.n = n;
        a.m = m;
        a.ld = ld;
        a.ids = idx->s_misc.as<int32_t>();
        float *stage = idx->s_misc2.as<float>();
        float *snorms = reinterpret_cast<float *>(idx->s_misc2.as<char>() + sect(sizeof(float) * mm * ld));
        a.stage = stage;
        a.snorms = snorms;
        a.new_base = nw.base;
        a.new_norms = nw.norms;
        HG_HIP(hipMemcpyAsync(idx->s_misc.p, ids, sizeof(int32_t) * mm, hipMemcpyHostToDevice, st));
        HG_TRY(pcaf_upload_rows(idx, rows, m, stage, st));
        HG_TRY(launch_norms(idx->nch, stage, ld, m, snorms, st));
        HG_TRY(nw.copy_old(idx, n, st));
        hipLaunchKernelGGL(pcaf_update_place_kernel, dim3(static_cast<unsigned>((m + kNWave - 1) / kNWave)), dim3(kWG), 0, st, a);
        HG_HIP(hipGetLastError());
        HG_TRY(launch_pcaf_project(idx, idx->d_pcaf_proj, idx->pcaf_T, stage, ld, m, nw.low, nw.lnorms, st, a.ids, n));
        if (idx->d_qrows) HG_TRY(quantize_rows(idx, nw.base, n, &nw.qrows, &nw.qmeta, st));  // (as add: one pass over the new base)
        HG_HIP(hipStreamSynchronize(st));  // (the uploads have read `ids` and `rows`; a failing step shows before the takeover)
        return 0;
    };
    const int rc = update();
    if (rc != 0) {
        (void)hipStreamSynchronize(st);  // (nothing of the chain is in flight when `nw` frees what it staged)
        return rc;
    }
    nw.swap_into(idx, n);
    return call.close();
}

}  // extern "C"
