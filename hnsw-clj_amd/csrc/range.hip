// range.hip -- hnswgpu_range_search / hnswgpu_range_search_dev: every row within a radius of each query, exact, as CSR
// (lims, ids, distances).  The kernels and the reasons for their shape: range_kernels.hpp.  One body for both entries.
// hnswgpu_range_search_filtered[_each][_dev]: the same under an allow-mask, one per call or one per query, by a gathered scan
// and a gathered fill over the masks' pass lists (range_filtered_kernels.hpp).  One body for the four entries.
// hnswgpu_ivf_range_search[_dev]: the rows of each query's PROBED IVF lists within its radius, in candidate-stream order, by a
// list-major scan over the pairs filed by list (ivf_range_kernels.hpp).  One chain for both entries.
#include <string.h>

#include <functional>

#include "engine.hpp"
#include "ivf_range_kernels.hpp"
#include "range_filtered_kernels.hpp"
#include "range_kernels.hpp"

namespace hg {

static int launch_range_scan(int nch, const RangeArgs &a, int64_t blocks, hipStream_t st) {
    HG_REQUIRE(blocks > 0 && blocks < 2147483647LL, HNSWGPU_ELIMIT, "range scan grid too large (%lld blocks)", (long long)blocks);
    const size_t lds = range_scan_lds_bytes(a.ld, a.tq);
    const bool l2 = a.metric == METRIC_L2;
#define CALL(N, R, L)                                                                                          \
    do {                                                                                                       \
        static bool rs_attr_done[64] = {};                                                                     \
        if (attr_needed(rs_attr_done))                                                                         \
            HG_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&range_scan_kernel<N, R, L>),           \
                                       hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));              \
        hipLaunchKernelGGL((range_scan_kernel<N, R, L>), dim3(static_cast<unsigned>(blocks)), dim3(kTileThreads), lds, st, a); \
    } while (0)
    HG_DISPATCH(nch, l2, CALL);
#undef CALL
    HG_HIP(hipGetLastError());
    return 0;
}

static int launch_range_fill(int nch, const RangeArgs &a, hipStream_t st) {
    const bool l2 = a.metric == METRIC_L2;
    const dim3 grid(static_cast<unsigned>(a.nblk), static_cast<unsigned>(a.nq));
#define CALL(N, R, L) hipLaunchKernelGGL((range_fill_kernel<N, L>), grid, dim3(kWG), 0, st, a)
    HG_DISPATCH(nch, l2, CALL);
#undef CALL
    HG_HIP(hipGetLastError());
    return 0;
}

// Slices of whole query groups: scan into the slice's hit words, counts, lims, and -- unless the call only counts -- fill and
// sort.  Everything is enqueued on `st`; the running total lives at d_run and nothing is read back.
static int range_enqueue(hnswgpu_index *idx, const float *d_Q, int32_t nq, const float *d_radius, int32_t flags, int64_t *d_lims,
                         int32_t *d_ids, float *d_dist, int64_t cap, unsigned long long *d_run, hipStream_t st) {
    const int64_t n = idx->n, W = (n + 31) / 32;
    const int tq = group_queries_of(idx->ld);
    const int64_t G = (static_cast<int64_t>(nq) + tq - 1) / tq;
    // a slice's hit words stay within the budget (at least one group; at most 65535 queries: a query is a blockIdx.y)
    const int64_t budget = std::max<int64_t>(0, tune(HNSWGPU_TUNE_FILTER_EACH_MB, 2048)) << 20;
    const int64_t group_bytes = static_cast<int64_t>(tq) * W * static_cast<int64_t>(sizeof(uint32_t));
    const int64_t gps = std::max<int64_t>(1, std::min<int64_t>(budget / group_bytes, 65535 / tq));
    const int64_t slice_q = std::min<int64_t>(gps * tq, nq);
    HG_TRY(idx->s_rhits.ensure(sizeof(uint32_t) * static_cast<size_t>(slice_q) * static_cast<size_t>(W)));
    HG_TRY(pad_queries(idx, d_Q, idx->dim, nq, st));
    for (int64_t g0 = 0; g0 < G; g0 += gps) {
        const int64_t q0 = g0 * tq;
        const int32_t nb = static_cast<int32_t>(std::min<int64_t>((g0 + gps) * tq, nq) - q0);
        const int32_t ng = (nb + tq - 1) / tq;
        RangeArgs a;
        memset(&a, 0, sizeof(a));
        a.rows = idx->d_base;
        a.row_norms = idx->d_norms;
        a.ld = idx->ld;
        a.n = n;
        a.metric = idx->metric;
        a.Qp = idx->s_qp.as<float>() + q0 * idx->ld;
        a.q_norms = idx->s_qn.as<float>() + q0;
        a.radius = d_radius + q0;
        a.nq = nb;
        a.tq = tq;
        a.ngroups = ng;
        a.nwords = W;
        a.hits = idx->s_rhits.as<uint32_t>();
        // chunks of whole 256-row tiles, about 2048 workgroups in all: a workgroup stages its query group once per chunk
        const int64_t tiles = (n + kTileRows - 1) / kTileRows;
        const int64_t want = std::max<int64_t>(1, std::min<int64_t>(tiles, (2048 + ng - 1) / ng));
        a.chunk_rows = (tiles + want - 1) / want * kTileRows;
        const int64_t nchunks = (n + a.chunk_rows - 1) / a.chunk_rows;
        hipEvent_t e0;
        prof_begin(idx, PROF_IVF_SCAN, st, &e0);
        HG_TRY(launch_range_scan(idx->nch, a, nchunks * ng, st));
        prof_end(idx, PROF_IVF_SCAN, st, e0);
        HG_TRY(mask_counts(idx, a.hits, n, nb, st, &a.blk, &a.nblk, &a.qtot));
        HG_REQUIRE(a.nblk == (W + kRangeFillWords - 1) / kRangeFillWords, HNSWGPU_EHIP, "the count pass and the fill pass disagree about a block");
        a.run = d_run;
        a.first = g0 == 0;
        a.lims = d_lims + q0;
        a.out_ids = d_ids;
        a.out_dist = d_dist;
        a.cap = cap;
        hipLaunchKernelGGL(range_lims_kernel, dim3(1), dim3(kRangeSortThreads), 0, st, a);
        HG_HIP(hipGetLastError());
        if (!d_ids) continue;  // count only
        HG_TRY(launch_range_fill(idx->nch, a, st));
        if (flags & HNSWGPU_RANGE_BY_DISTANCE) {
            hipLaunchKernelGGL(range_sort_kernel, dim3(static_cast<unsigned>(nb)), dim3(kRangeSortThreads), 0, st, a);
            HG_HIP(hipGetLastError());
        }
    }
    return 0;
}

static int check_range_args(const hnswgpu_index *idx, const void *Q, int32_t nq, const void *radius, int32_t flags, const void *lims,
                            const void *ids, const void *dist, int64_t cap) {
    HG_REQUIRE(idx, HNSWGPU_EINVAL, "idx is null");
    HG_REQUIRE(nq >= 0, HNSWGPU_EINVAL, "nq < 0");
    HG_REQUIRE((flags & ~HNSWGPU_RANGE_BY_DISTANCE) == 0, HNSWGPU_EINVAL, "unknown flag bits: %d", flags);
    HG_REQUIRE(cap >= 0, HNSWGPU_EINVAL, "cap < 0");
    HG_REQUIRE((ids == nullptr) == (dist == nullptr), HNSWGPU_EINVAL, "out_ids and out_dist: both or neither");
    HG_REQUIRE(ids || cap == 0, HNSWGPU_EINVAL, "a count-only call (no output arrays) takes cap == 0");
    HG_REQUIRE(nq == 0 || (Q && radius && lims), HNSWGPU_EINVAL, "null argument");
    return 0;
}

// ---- under an allow-mask ---------------------------------------------------------------------------------------------------
static int launch_range_gather_scan(int nch, MaskForm form, const RangeGatherArgs &a, int64_t blocks, hipStream_t st) {
    HG_REQUIRE(blocks > 0 && blocks < 2147483647LL, HNSWGPU_ELIMIT, "range scan grid too large (%lld blocks)", (long long)blocks);
    const size_t lds = range_scan_lds_bytes(a.r.ld, a.r.tq);
    const bool l2 = a.r.metric == METRIC_L2;
#define CALLE(N, R, L, E)                                                                                                 \
    do {                                                                                                                  \
        static bool rg_attr_done[64] = {};                                                                                \
        if (attr_needed(rg_attr_done))                                                                                    \
            HG_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&range_gather_scan_kernel<N, R, L, E>),            \
                                       hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));                         \
        hipLaunchKernelGGL((range_gather_scan_kernel<N, R, L, E>), dim3(static_cast<unsigned>(blocks)), dim3(kTileThreads), lds, st, a); \
    } while (0)
#define CALL(N, R, L)                                     \
    do {                                                  \
        if (form == MaskForm::Each) CALLE(N, R, L, true); \
        else CALLE(N, R, L, false);                       \
    } while (0)
    HG_DISPATCH(nch, l2, CALL);
#undef CALL
#undef CALLE
    HG_HIP(hipGetLastError());
    return 0;
}

static int launch_range_fill_gather(int nch, const RangeGatherArgs &a, hipStream_t st) {
    const bool l2 = a.r.metric == METRIC_L2;
    const dim3 grid(static_cast<unsigned>(a.r.nblk), static_cast<unsigned>(a.r.nq));
#define CALL(N, R, L) hipLaunchKernelGGL((range_fill_gather_kernel<N, L>), grid, dim3(kWG), 0, st, a)
    HG_DISPATCH(nch, l2, CALL);
#undef CALL
    HG_HIP(hipGetLastError());
    return 0;
}

// range_enqueue over pass lists.  Single: the call's mask is compacted once, before the slices.  Each: d_allow is [nq][W] and
// every slice compacts the unions of ITS groups; the slice budget covers their lists and words (8 n bytes per group) and their
// union masks beside the hit words.  Nothing is read back: lists and grids are sized by n, the lists' lengths stay in s_rcnt.
static int range_filtered_enqueue(hnswgpu_index *idx, MaskForm form, const float *d_Q, int32_t nq, const float *d_radius, int32_t flags,
                                  const uint32_t *d_allow, int64_t *d_lims, int32_t *d_ids, float *d_dist, int64_t cap,
                                  unsigned long long *d_run, hipStream_t st) {
    const bool each = form == MaskForm::Each;
    const int64_t n = idx->n, W = (n + 31) / 32;
    const int tq = group_queries_of(idx->ld);
    const int64_t G = (static_cast<int64_t>(nq) + tq - 1) / tq;
    const int64_t budget = std::max<int64_t>(0, tune(HNSWGPU_TUNE_FILTER_EACH_MB, 2048)) << 20;
    const int64_t group_bytes = static_cast<int64_t>(tq) * W * static_cast<int64_t>(sizeof(uint32_t)) + (each ? 8 * n + 4 * W : 0);
    const int64_t gps = std::max<int64_t>(1, std::min<int64_t>(budget / group_bytes, 65535 / tq));
    const int64_t slice_q = std::min<int64_t>(gps * tq, nq);
    HG_TRY(idx->s_rhits.ensure(sizeof(uint32_t) * static_cast<size_t>(slice_q) * static_cast<size_t>(W)));
    HG_TRY(idx->s_rcnt.ensure(sizeof(unsigned long long) * static_cast<size_t>(each ? (slice_q + tq - 1) / tq : 1)));
    HG_TRY(pad_queries(idx, d_Q, idx->dim, nq, st));
    RangeGatherArgs ga;
    memset(&ga, 0, sizeof(ga));
    ga.cnt = idx->s_rcnt.as<unsigned long long>();
    if (!each) HG_TRY(mask_lists_dev(idx, form, d_allow, nq, tq, st, idx->s_rcnt.as<unsigned long long>(), &ga.pass, &ga.uw));
    for (int64_t g0 = 0; g0 < G; g0 += gps) {
        const int64_t q0 = g0 * tq;
        const int32_t nb = static_cast<int32_t>(std::min<int64_t>((g0 + gps) * tq, nq) - q0);
        const int32_t ng = (nb + tq - 1) / tq;
        if (each) {
            HG_TRY(mask_lists_dev(idx, form, d_allow + q0 * W, nb, tq, st, idx->s_rcnt.as<unsigned long long>(), &ga.pass, &ga.uw));
            ga.lstride = n;
        }
        RangeArgs &a = ga.r;
        memset(&a, 0, sizeof(a));
        a.rows = idx->d_base;
        a.row_norms = idx->d_norms;
        a.ld = idx->ld;
        a.n = n;
        a.metric = idx->metric;
        a.Qp = idx->s_qp.as<float>() + q0 * idx->ld;
        a.q_norms = idx->s_qn.as<float>() + q0;
        a.radius = d_radius + q0;
        a.nq = nb;
        a.tq = tq;
        a.ngroups = ng;
        a.nwords = W;
        a.hits = idx->s_rhits.as<uint32_t>();
        // the unfiltered scan's grid: chunks of whole tiles of the n positions a list can hold, about 2048 workgroups in all.  The
        // kernel cuts its list -- p positions, known on the device alone -- into as many chunks itself.
        const int64_t tiles = (n + kTileRows - 1) / kTileRows;
        const int64_t want = std::max<int64_t>(1, std::min<int64_t>(tiles, (2048 + ng - 1) / ng));
        a.chunk_rows = (tiles + want - 1) / want * kTileRows;
        ga.nchunks = static_cast<int32_t>((n + a.chunk_rows - 1) / a.chunk_rows);
        hipEvent_t e0;
        prof_begin(idx, PROF_IVF_SCAN, st, &e0);
        HG_TRY(launch_range_gather_scan(idx->nch, form, ga, static_cast<int64_t>(ga.nchunks) * ng, st));
        prof_end(idx, PROF_IVF_SCAN, st, e0);
        HG_TRY(mask_counts(idx, a.hits, n, nb, st, &a.blk, &a.nblk, &a.qtot));
        HG_REQUIRE(a.nblk == (W + kRangeFillWords - 1) / kRangeFillWords, HNSWGPU_EHIP, "the count pass and the fill pass disagree about a block");
        a.run = d_run;
        a.first = g0 == 0;
        a.lims = d_lims + q0;
        a.out_ids = d_ids;
        a.out_dist = d_dist;
        a.cap = cap;
        hipLaunchKernelGGL(range_lims_kernel, dim3(1), dim3(kRangeSortThreads), 0, st, a);
        HG_HIP(hipGetLastError());
        if (!d_ids) continue;  // count only
        HG_TRY(launch_range_fill_gather(idx->nch, ga, st));
        if (flags & HNSWGPU_RANGE_BY_DISTANCE) {
            hipLaunchKernelGGL(range_sort_kernel, dim3(static_cast<unsigned>(nb)), dim3(kRangeSortThreads), 0, st, a);
            HG_HIP(hipGetLastError());
        }
    }
    return 0;
}

static int range_filtered_dev(hnswgpu_index *idx, MaskForm form, const float *d_Q, int32_t nq, const float *d_radius, int32_t flags,
                              const uint32_t *d_allow, int64_t *d_lims, int32_t *d_out_ids, float *d_out_dist, int64_t cap, void *stream) {
    HG_TRY(check_range_args(idx, d_Q, nq, d_radius, flags, d_lims, d_out_ids, d_out_dist, cap));
    HG_REQUIRE(d_allow, HNSWGPU_EINVAL, "allow is null");
    if (nq == 0) return 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    Call call;
    HG_TRY(call.open(idx, st));
    if (idx->n == 0) {
        hipLaunchKernelGGL(range_zero_lims_kernel, dim3((nq + 1 + 255) / 256), dim3(256), 0, st, d_lims, static_cast<int64_t>(nq) + 1);
        HG_HIP(hipGetLastError());
        return call.close();
    }
    HG_TRY(idx->s_rmeta.ensure(sizeof(unsigned long long)));
    HG_TRY(range_filtered_enqueue(idx, form, d_Q, nq, d_radius, flags, d_allow, d_lims, d_out_ids, d_out_dist, cap,
                                  idx->s_rmeta.as<unsigned long long>(), st));
    return call.close();
}

// Host arrays.  One caller's staged batch, its mask -- Each: its [nq][W] masks -- staged whole: no part in the call combiner.
static int range_filtered_host(hnswgpu_index *idx, MaskForm form, const float *Q, int32_t nq, const float *radius, int32_t flags,
                               const uint32_t *allow, int64_t *lims, int32_t *out_ids, float *out_dist, int64_t cap) {
    HG_TRY(check_range_args(idx, Q, nq, radius, flags, lims, out_ids, out_dist, cap));
    HG_REQUIRE(allow, HNSWGPU_EINVAL, "allow is null");
    if (nq == 0) {
        if (lims) lims[0] = 0;
        return 0;
    }
    if (idx->n == 0) {
        memset(lims, 0, sizeof(int64_t) * (static_cast<size_t>(nq) + 1));
        return 0;
    }
    hipStream_t st = idx->stream;
    Call call;
    HG_TRY(call.open(idx, st));
    HG_TRY(upload_queries(idx, Q, nq, st));
    HG_TRY(call.stage_mask(allow, form, nq));
    // s_rmeta: [running total][lims: nq + 1][radii: nq]
    const size_t lims_bytes = sizeof(int64_t) * (static_cast<size_t>(nq) + 1);
    HG_TRY(idx->s_rmeta.ensure(sizeof(unsigned long long) + lims_bytes + sizeof(float) * static_cast<size_t>(nq)));
    unsigned long long *d_run = idx->s_rmeta.as<unsigned long long>();
    int64_t *d_lims = reinterpret_cast<int64_t *>(d_run + 1);
    float *d_radius = reinterpret_cast<float *>(d_lims + nq + 1);
    HG_HIP(hipMemcpyAsync(d_radius, radius, sizeof(float) * static_cast<size_t>(nq), hipMemcpyHostToDevice, st));
    if (out_ids) {
        HG_TRY(idx->s_ids.ensure(sizeof(int32_t) * static_cast<size_t>(cap)));
        HG_TRY(idx->s_outd.ensure(sizeof(float) * static_cast<size_t>(cap)));
    }
    HG_TRY(range_filtered_enqueue(idx, form, idx->s_q.as<float>(), nq, d_radius, flags, idx->s_fmask.as<uint32_t>(), d_lims,
                                  out_ids ? idx->s_ids.as<int32_t>() : nullptr, out_ids ? idx->s_outd.as<float>() : nullptr, cap, d_run, st));
    HG_HIP(hipMemcpyAsync(lims, d_lims, lims_bytes, hipMemcpyDeviceToHost, st));
    HG_TRY(call.sync());
    const int64_t total = lims[nq];
    if (out_ids && total > cap) {
        (void)call.close();
        set_error("the result holds %lld entries, the arrays %lld: lims is complete, size the arrays by lims[nq]", (long long)total, (long long)cap);
        return HNSWGPU_ELIMIT;
    }
    if (out_ids && total > 0) HG_TRY(call.stage_out(out_ids, out_dist, total));
    return call.close();
}

// ---- through the IVF lists (ivf_range_kernels.hpp) ---------------------------------------------------------------------------
static int launch_ivf_range_scan(int nch, const IvfRangeArgs &a, hipStream_t st) {
    const size_t lds = range_scan_lds_bytes(a.r.ld, a.r.tq);
    const bool l2 = a.r.metric == METRIC_L2;
#define CALL(N, R, L)                                                                                              \
    do {                                                                                                           \
        static bool ir_attr_done[64] = {};                                                                         \
        if (attr_needed(ir_attr_done))                                                                             \
            HG_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&ivf_range_scan_kernel<N, R, L>),           \
                                       hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 512));            \
        hipLaunchKernelGGL((ivf_range_scan_kernel<N, R, L>), dim3(static_cast<unsigned>(a.max_items)), dim3(kTileThreads), lds, st, a); \
    } while (0)
    HG_DISPATCH(nch, l2, CALL);
#undef CALL
    HG_HIP(hipGetLastError());
    return 0;
}

static int launch_ivf_range_fill(int nch, const IvfRangeArgs &a, hipStream_t st) {
    const bool l2 = a.r.metric == METRIC_L2;
    const dim3 grid(static_cast<unsigned>(a.r.nblk), static_cast<unsigned>(a.r.nq), kIvfRangeFillParts);
#define CALL(N, R, L) hipLaunchKernelGGL((ivf_range_fill_kernel<N, L>), grid, dim3(kWG), 0, st, a)
    HG_DISPATCH(nch, l2, CALL);
#undef CALL
    HG_HIP(hipGetLastError());
    return 0;
}

// What the host decides for one call, from its mirror of the list offsets alone (nothing is read back).  Wq, the words of a
// query's hit mask: a list starts a fresh word, so the np probes of a query own at most the np largest ceil(len / 32) -- routed
// probes are distinct lists; a caller's table may name the longest list in every column.  chunk_rows: whole tiles, about 2048
// workgroups over the blocks of pairs; max_items bounds the device's work list: a list with c pairs has ceil(c / tq) blocks,
// so all lists together at most npairs / tq + (lists with a pair), each over at most the chunks of the longest list.
struct IvfRangePlan {
    int64_t Wq, chunk_rows, slice_q, max_items;
};
static int ivf_range_plan(const hnswgpu_index *idx, int32_t nq, int32_t np, bool given, IvfRangePlan *p) {
    const int tq = group_queries_of(idx->ld);
    std::vector<int64_t> w(static_cast<size_t>(idx->nlist));
    for (int l = 0; l < idx->nlist; l++) w[l] = (idx->h_listoff[l + 1] - idx->h_listoff[l] + 31) / 32;
    const int64_t wmax = *std::max_element(w.begin(), w.end());
    int64_t Wq = 0;
    if (given) {
        Wq = wmax * np;
    } else {
        std::partial_sort(w.begin(), w.begin() + np, w.end(), std::greater<int64_t>());
        for (int j = 0; j < np; j++) Wq += w[j];
    }
    p->Wq = std::max<int64_t>(Wq, 1);
    HG_REQUIRE(p->Wq * 32 < 2147483647LL, HNSWGPU_ELIMIT, "a query's probed lists hold too many rows (%lld words of hit bits)", (long long)p->Wq);
    // a slice's hit words, woff rows and pair order stay within the budget (at least one group; at most 65535 queries)
    const int64_t budget = std::max<int64_t>(0, tune(HNSWGPU_TUNE_FILTER_EACH_MB, 2048)) << 20;
    const int64_t group_bytes = static_cast<int64_t>(tq) * static_cast<int64_t>(sizeof(uint32_t)) * (p->Wq + 2 * static_cast<int64_t>(np) + 1);
    const int64_t gps = std::max<int64_t>(1, std::min<int64_t>(budget / group_bytes, 65535 / tq));
    p->slice_q = std::min<int64_t>(gps * tq, nq);
    const int64_t npairs = p->slice_q * np;
    HG_REQUIRE(npairs < 2147483647LL, HNSWGPU_ELIMIT, "too many (query, list) pairs in a slice (%lld)", (long long)npairs);
    const int64_t tiles = std::max<int64_t>(1, (idx->max_list_len + kTileRows - 1) / kTileRows);
    const int64_t blocks = npairs / tq + std::min<int64_t>(idx->nlist, npairs);
    const int64_t want = std::max<int64_t>(1, std::min<int64_t>(tiles, (2048 + blocks - 1) / blocks));
    p->chunk_rows = (tiles + want - 1) / want * kTileRows;
    p->max_items = blocks * ((idx->max_list_len + p->chunk_rows - 1) / p->chunk_rows);
    HG_REQUIRE(p->max_items < 2147483647LL, HNSWGPU_ELIMIT, "range scan grid too large (%lld blocks)", (long long)p->max_items);
    p->max_items = std::max<int64_t>(p->max_items, 1);
    return 0;
}

static size_t align16(size_t x) { return (x + 15) & ~static_cast<size_t>(15); }

// s_ivr: [the call's probe table: nq * np][a slice's woff rows: slice_q * (np + 1)][pair order: slice_q * np][items][their number]
struct IvfRangeScratch {
    int32_t *table, *woff, *order, *nitems;
    IvfRangeItem *items;
};
static int ivf_range_scratch(hnswgpu_index *idx, int32_t nq, int32_t np, const IvfRangePlan &p, IvfRangeScratch *s) {
    const size_t o_woff = align16(sizeof(int32_t) * static_cast<size_t>(nq) * np);
    const size_t o_order = o_woff + align16(sizeof(int32_t) * static_cast<size_t>(p.slice_q) * (np + 1));
    const size_t o_items = o_order + align16(sizeof(int32_t) * static_cast<size_t>(p.slice_q) * np);
    const size_t o_nit = o_items + sizeof(IvfRangeItem) * static_cast<size_t>(p.max_items);
    HG_TRY(idx->s_ivr.ensure(o_nit + 16));
    char *b = idx->s_ivr.as<char>();
    s->table = reinterpret_cast<int32_t *>(b);
    s->woff = reinterpret_cast<int32_t *>(b + o_woff);
    s->order = reinterpret_cast<int32_t *>(b + o_order);
    s->items = reinterpret_cast<IvfRangeItem *>(b + o_items);
    s->nitems = reinterpret_cast<int32_t *>(b + o_nit);
    return 0;
}

// range_enqueue over the lists: per slice of whole query groups the slice's pairs are filed by list (a pair's queries lie in
// one slice), scanned list-major into the slice's hit words in stream space, counted, and -- unless the call only counts --
// filled and sorted.  s.table holds the call's probe table.  Everything is enqueued on `st`; nothing is read back.
static int ivf_range_enqueue(hnswgpu_index *idx, const float *d_Q, int32_t nq, const float *d_radius, int32_t np, const IvfRangePlan &p,
                             const IvfRangeScratch &s, int32_t flags, int64_t *d_lims, int32_t *d_ids, float *d_dist, int64_t cap,
                             unsigned long long *d_run, hipStream_t st) {
    const int tq = group_queries_of(idx->ld);
    HG_TRY(idx->s_rhits.ensure(sizeof(uint32_t) * static_cast<size_t>(p.slice_q) * static_cast<size_t>(p.Wq)));
    HG_TRY(pad_queries(idx, d_Q, idx->dim, nq, st));
    static bool wl_attr_done[64] = {};
    const size_t wl_lds = ivf_range_worklist_lds_bytes(idx->nlist);
    if (wl_lds > 32 * 1024 && attr_needed(wl_attr_done))
        HG_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&ivf_range_worklist_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   static_cast<int>(ivf_range_worklist_lds_bytes(kIvfRangeMaxLists))));
    for (int64_t q0 = 0; q0 < nq; q0 += p.slice_q) {
        const int32_t nb = static_cast<int32_t>(std::min<int64_t>(p.slice_q, nq - q0));
        IvfRangeArgs ia;
        memset(&ia, 0, sizeof(ia));
        RangeArgs &a = ia.r;
        a.rows = idx->d_lrows;
        a.row_norms = idx->d_lnorms;
        a.ld = idx->ld;
        a.n = idx->n;
        a.metric = idx->metric;
        a.Qp = idx->s_qp.as<float>() + q0 * idx->ld;
        a.q_norms = idx->s_qn.as<float>() + q0;
        a.radius = d_radius + q0;
        a.nq = nb;
        a.tq = tq;
        a.ngroups = (nb + tq - 1) / tq;
        a.chunk_rows = p.chunk_rows;
        a.nwords = p.Wq;
        a.hits = idx->s_rhits.as<uint32_t>();
        ia.listoff = idx->d_listoff;
        ia.listids = idx->d_listids;
        ia.nlist = idx->nlist;
        ia.probes = s.table + q0 * np;
        ia.nprobe = np;
        ia.woff = s.woff;
        ia.order = s.order;
        ia.items = s.items;
        ia.nitems = s.nitems;
        ia.max_items = static_cast<int32_t>(p.max_items);
        const int64_t npairs = static_cast<int64_t>(nb) * np;
        hipLaunchKernelGGL(ivf_range_offsets_kernel, dim3((nb + kNWave - 1) / kNWave), dim3(kWG), 0, st, ia);
        HG_HIP(hipGetLastError());
        HG_TRY(launch_pair_order(idx, ia.probes, npairs, s.order, st));
        hipLaunchKernelGGL(ivf_range_worklist_kernel, dim3(1), dim3(kIvfRangeListThreads), wl_lds, st, ia);
        HG_HIP(hipGetLastError());
        hipEvent_t e0;
        prof_begin(idx, PROF_IVF_SCAN, st, &e0);
        HG_TRY(launch_ivf_range_scan(idx->nch, ia, st));
        prof_end(idx, PROF_IVF_SCAN, st, e0);
        HG_TRY(mask_counts(idx, a.hits, p.Wq * 32, nb, st, &a.blk, &a.nblk, &a.qtot));
        HG_REQUIRE(a.nblk == (p.Wq + kRangeFillWords - 1) / kRangeFillWords, HNSWGPU_EHIP, "the count pass and the fill pass disagree about a block");
        a.run = d_run;
        a.first = q0 == 0;
        a.lims = d_lims + q0;
        a.out_ids = d_ids;
        a.out_dist = d_dist;
        a.cap = cap;
        hipLaunchKernelGGL(range_lims_kernel, dim3(1), dim3(kRangeSortThreads), 0, st, a);
        HG_HIP(hipGetLastError());
        if (!d_ids) continue;  // count only
        HG_TRY(launch_ivf_range_fill(idx->nch, ia, st));
        if (flags & HNSWGPU_RANGE_BY_DISTANCE) {
            hipLaunchKernelGGL(range_sort_kernel, dim3(static_cast<unsigned>(nb)), dim3(kRangeSortThreads), 0, st, a);
            HG_HIP(hipGetLastError());
        }
    }
    return 0;
}

static int launch_ivf_range_probes(const int32_t *src, int32_t src_np, int32_t *dst, int32_t dst_np, int32_t nq, int32_t nlist, hipStream_t st) {
    const int64_t cnt = static_cast<int64_t>(nq) * dst_np;
    hipLaunchKernelGGL(ivf_range_probes_kernel, dim3(static_cast<unsigned>((cnt + 255) / 256)), dim3(256), 0, st, src, src_np, dst, dst_np,
                       static_cast<int64_t>(nq), nlist);
    HG_HIP(hipGetLastError());
    return 0;
}

static int check_ivf_range_args(const hnswgpu_index *idx, const void *Q, int32_t nq, const void *radius, int32_t nprobe, int32_t flags,
                                const void *lims, const void *ids, const void *dist, int64_t cap) {
    HG_TRY(check_range_args(idx, Q, nq, radius, flags, lims, ids, dist, cap));
    HG_REQUIRE(nprobe >= 1, HNSWGPU_EINVAL, "need nprobe >= 1");
    HG_REQUIRE(nprobe <= kIvfRangeMaxProbe, HNSWGPU_ELIMIT, "nprobe > %d is not supported", kIvfRangeMaxProbe);
    return 0;
}
// under the handle's lock: the lists may have been replaced since any earlier look
static int check_ivf_range_handle(const hnswgpu_index *idx) {
    HG_REQUIRE(idx->nlist > 0, HNSWGPU_ESTATE, "index has no IVF lists (call hnswgpu_ivf_build / hnswgpu_set_ivf)");
    HG_REQUIRE(idx->d_glistoff == nullptr, HNSWGPU_ESTATE, "a shard of a larger IVF index (hnswgpu_set_ivf_shard) holds a part of every list: range search through the lists is refused");
    HG_REQUIRE(idx->nlist <= kIvfRangeMaxLists, HNSWGPU_ELIMIT, "more than %d lists are not supported", kIvfRangeMaxLists);
    return 0;
}

// The probe table into s.table -- routed, or the caller's with the ids outside [0, nlist) as skips -- and, where asked for, out
// to d_out_probes [nq][nprobe]; then the slices.  One body for both entries: device arrays throughout.
static int ivf_range_chain(hnswgpu_index *idx, const float *d_Q, int32_t nq, const float *d_radius, int32_t nprobe, const int32_t *d_probes,
                           int32_t flags, int64_t *d_lims, int32_t *d_ids, float *d_dist, int64_t cap, int32_t *d_out_probes,
                           unsigned long long *d_run, hipStream_t st) {
    const int32_t np = d_probes ? nprobe : std::min(nprobe, idx->nlist);
    IvfRangePlan p;
    IvfRangeScratch s;
    HG_TRY(ivf_range_plan(idx, nq, np, d_probes != nullptr, &p));
    HG_TRY(ivf_range_scratch(idx, nq, np, p, &s));
    if (d_probes) HG_TRY(launch_ivf_range_probes(d_probes, np, s.table, np, nq, idx->nlist, st));
    else HG_TRY(ivf_route_table(idx, d_Q, nq, np, s.table, st));
    if (d_out_probes) HG_TRY(launch_ivf_range_probes(s.table, np, d_out_probes, nprobe, nq, idx->nlist, st));
    return ivf_range_enqueue(idx, d_Q, nq, d_radius, np, p, s, flags, d_lims, d_ids, d_dist, cap, d_run, st);
}

}  // namespace hg

using namespace hg;

int hnswgpu_range_search_dev(hnswgpu_index *idx, const float *d_Q, int32_t nq, const float *d_radius, int32_t flags, int64_t *d_lims,
                             int32_t *d_out_ids, float *d_out_dist, int64_t cap, void *stream) {
    HG_TRY(check_range_args(idx, d_Q, nq, d_radius, flags, d_lims, d_out_ids, d_out_dist, cap));
    if (nq == 0) return 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    Call call;
    HG_TRY(call.open(idx, st));
    if (idx->n == 0) {
        hipLaunchKernelGGL(range_zero_lims_kernel, dim3((nq + 1 + 255) / 256), dim3(256), 0, st, d_lims, static_cast<int64_t>(nq) + 1);
        HG_HIP(hipGetLastError());
        return call.close();
    }
    HG_TRY(idx->s_rmeta.ensure(sizeof(unsigned long long)));
    HG_TRY(range_enqueue(idx, d_Q, nq, d_radius, flags, d_lims, d_out_ids, d_out_dist, cap, idx->s_rmeta.as<unsigned long long>(), st));
    return call.close();
}

int hnswgpu_range_search(hnswgpu_index *idx, const float *Q, int32_t nq, const float *radius, int32_t flags, int64_t *lims,
                         int32_t *out_ids, float *out_dist, int64_t cap) {
    HG_TRY(check_range_args(idx, Q, nq, radius, flags, lims, out_ids, out_dist, cap));
    if (nq == 0) {
        if (lims) lims[0] = 0;
        return 0;
    }
    if (idx->n == 0) {
        memset(lims, 0, sizeof(int64_t) * (static_cast<size_t>(nq) + 1));
        return 0;
    }
    hipStream_t st = idx->stream;
    Call call;
    HG_TRY(call.open(idx, st));
    HG_TRY(upload_queries(idx, Q, nq, st));
    // s_rmeta: [running total][lims: nq + 1][radii: nq]
    const size_t lims_bytes = sizeof(int64_t) * (static_cast<size_t>(nq) + 1);
    HG_TRY(idx->s_rmeta.ensure(sizeof(unsigned long long) + lims_bytes + sizeof(float) * static_cast<size_t>(nq)));
    unsigned long long *d_run = idx->s_rmeta.as<unsigned long long>();
    int64_t *d_lims = reinterpret_cast<int64_t *>(d_run + 1);
    float *d_radius = reinterpret_cast<float *>(d_lims + nq + 1);
    HG_HIP(hipMemcpyAsync(d_radius, radius, sizeof(float) * static_cast<size_t>(nq), hipMemcpyHostToDevice, st));
    if (out_ids) {
        HG_TRY(idx->s_ids.ensure(sizeof(int32_t) * static_cast<size_t>(cap)));
        HG_TRY(idx->s_outd.ensure(sizeof(float) * static_cast<size_t>(cap)));
    }
    HG_TRY(range_enqueue(idx, idx->s_q.as<float>(), nq, d_radius, flags, d_lims, out_ids ? idx->s_ids.as<int32_t>() : nullptr,
                         out_ids ? idx->s_outd.as<float>() : nullptr, cap, d_run, st));
    HG_HIP(hipMemcpyAsync(lims, d_lims, lims_bytes, hipMemcpyDeviceToHost, st));
    HG_TRY(call.sync());
    const int64_t total = lims[nq];
    if (out_ids && total > cap) {
        (void)call.close();
        set_error("the result holds %lld entries, the arrays %lld: lims is complete, size the arrays by lims[nq]", (long long)total, (long long)cap);
        return HNSWGPU_ELIMIT;
    }
    if (out_ids && total > 0) HG_TRY(call.stage_out(out_ids, out_dist, total));
    return call.close();
}

int hnswgpu_range_search_filtered_dev(hnswgpu_index *idx, const float *d_Q, int32_t nq, const float *d_radius, int32_t flags,
                                      const uint32_t *d_allow, int64_t *d_lims, int32_t *d_out_ids, float *d_out_dist, int64_t cap,
                                      void *stream) {
    return range_filtered_dev(idx, MaskForm::Single, d_Q, nq, d_radius, flags, d_allow, d_lims, d_out_ids, d_out_dist, cap, stream);
}
int hnswgpu_range_search_filtered(hnswgpu_index *idx, const float *Q, int32_t nq, const float *radius, int32_t flags,
                                  const uint32_t *allow, int64_t *lims, int32_t *out_ids, float *out_dist, int64_t cap) {
    return range_filtered_host(idx, MaskForm::Single, Q, nq, radius, flags, allow, lims, out_ids, out_dist, cap);
}
int hnswgpu_range_search_filtered_each_dev(hnswgpu_index *idx, const float *d_Q, int32_t nq, const float *d_radius, int32_t flags,
                                           const uint32_t *d_allow_each, int64_t *d_lims, int32_t *d_out_ids, float *d_out_dist,
                                           int64_t cap, void *stream) {
    return range_filtered_dev(idx, MaskForm::Each, d_Q, nq, d_radius, flags, d_allow_each, d_lims, d_out_ids, d_out_dist, cap, stream);
}
int hnswgpu_range_search_filtered_each(hnswgpu_index *idx, const float *Q, int32_t nq, const float *radius, int32_t flags,
                                       const uint32_t *allow_each, int64_t *lims, int32_t *out_ids, float *out_dist, int64_t cap) {
    return range_filtered_host(idx, MaskForm::Each, Q, nq, radius, flags, allow_each, lims, out_ids, out_dist, cap);
}

int hnswgpu_ivf_range_search_dev(hnswgpu_index *idx, const float *d_Q, int32_t nq, const float *d_radius, int32_t nprobe,
                                 const int32_t *d_probes, int32_t flags, int64_t *d_lims, int32_t *d_out_ids, float *d_out_dist,
                                 int64_t cap, int32_t *d_out_probes, void *stream) {
    HG_TRY(check_ivf_range_args(idx, d_Q, nq, d_radius, nprobe, flags, d_lims, d_out_ids, d_out_dist, cap));
    if (nq == 0) return 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    Call call;
    HG_TRY(call.open(idx, st));
    HG_TRY(check_ivf_range_handle(idx));
    if (idx->n == 0) {  // lists without rows: no list is scanned; a routed call reports none
        hipLaunchKernelGGL(range_zero_lims_kernel, dim3((nq + 1 + 255) / 256), dim3(256), 0, st, d_lims, static_cast<int64_t>(nq) + 1);
        HG_HIP(hipGetLastError());
        if (d_out_probes) HG_TRY(launch_ivf_range_probes(d_probes, d_probes ? nprobe : 0, d_out_probes, nprobe, nq, idx->nlist, st));
        return call.close();
    }
    HG_TRY(idx->s_rmeta.ensure(sizeof(unsigned long long)));
    HG_TRY(ivf_range_chain(idx, d_Q, nq, d_radius, nprobe, d_probes, flags, d_lims, d_out_ids, d_out_dist, cap, d_out_probes,
                           idx->s_rmeta.as<unsigned long long>(), st));
    return call.close();
}

int hnswgpu_ivf_range_search(hnswgpu_index *idx, const float *Q, int32_t nq, const float *radius, int32_t nprobe, const int32_t *probes,
                             int32_t flags, int64_t *lims, int32_t *out_ids, float *out_dist, int64_t cap, int32_t *out_probes) {
    HG_TRY(check_ivf_range_args(idx, Q, nq, radius, nprobe, flags, lims, out_ids, out_dist, cap));
    if (nq == 0) {
        if (lims) lims[0] = 0;
        return 0;
    }
    hipStream_t st = idx->stream;
    Call call;
    HG_TRY(call.open(idx, st));
    HG_TRY(check_ivf_range_handle(idx));
    const size_t tab = static_cast<size_t>(nq) * nprobe;
    if (probes)
        for (size_t i = 0; i < tab; i++) HG_REQUIRE(probes[i] >= -1 && probes[i] < idx->nlist, HNSWGPU_EINVAL, "probe list id out of range");
    if (idx->n == 0) {  // lists without rows: no list is scanned; a routed call reports none (as hnswgpu_ivf_search)
        memset(lims, 0, sizeof(int64_t) * (static_cast<size_t>(nq) + 1));
        if (out_probes)
            for (size_t i = 0; i < tab; i++) out_probes[i] = probes ? probes[i] : -1;
        return call.close();
    }
    HG_TRY(upload_queries(idx, Q, nq, st));
    // s_rmeta: [running total][lims: nq + 1][radii: nq]
    const size_t lims_bytes = sizeof(int64_t) * (static_cast<size_t>(nq) + 1);
    HG_TRY(idx->s_rmeta.ensure(sizeof(unsigned long long) + lims_bytes + sizeof(float) * static_cast<size_t>(nq)));
    unsigned long long *d_run = idx->s_rmeta.as<unsigned long long>();
    int64_t *d_lims = reinterpret_cast<int64_t *>(d_run + 1);
    float *d_radius = reinterpret_cast<float *>(d_lims + nq + 1);
    HG_HIP(hipMemcpyAsync(d_radius, radius, sizeof(float) * static_cast<size_t>(nq), hipMemcpyHostToDevice, st));
    // s_probes: the caller's table on its way in, the table used on its way out
    if (probes || out_probes) HG_TRY(idx->s_probes.ensure(sizeof(int32_t) * tab));
    if (probes) HG_HIP(hipMemcpyAsync(idx->s_probes.p, probes, sizeof(int32_t) * tab, hipMemcpyHostToDevice, st));
    if (out_ids) {
        HG_TRY(idx->s_ids.ensure(sizeof(int32_t) * static_cast<size_t>(cap)));
        HG_TRY(idx->s_outd.ensure(sizeof(float) * static_cast<size_t>(cap)));
    }
    HG_TRY(ivf_range_chain(idx, idx->s_q.as<float>(), nq, d_radius, nprobe, probes ? idx->s_probes.as<int32_t>() : nullptr, flags, d_lims,
                           out_ids ? idx->s_ids.as<int32_t>() : nullptr, out_ids ? idx->s_outd.as<float>() : nullptr, cap,
                           out_probes ? idx->s_probes.as<int32_t>() : nullptr, d_run, st));
    if (out_probes) HG_HIP(hipMemcpyAsync(out_probes, idx->s_probes.p, sizeof(int32_t) * tab, hipMemcpyDeviceToHost, st));
    HG_HIP(hipMemcpyAsync(lims, d_lims, lims_bytes, hipMemcpyDeviceToHost, st));
    HG_TRY(call.sync());
    const int64_t total = lims[nq];
    if (out_ids && total > cap) {
        (void)call.close();
        set_error("the result holds %lld entries, the arrays %lld: lims is complete, size the arrays by lims[nq]", (long long)total, (long long)cap);
        return HNSWGPU_ELIMIT;
    }
    if (out_ids && total > 0) HG_TRY(call.stage_out(out_ids, out_dist, total));
    return call.close();
}
