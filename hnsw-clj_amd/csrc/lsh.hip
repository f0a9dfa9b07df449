// lsh.hip -- the hybrid LSH index (src/hnsw/ann/hash/hybrid_lsh.clj): hyperplanes, hash, buckets, multi-probe search
// (C ABI: include/hnswgpu.h, "Hybrid LSH"; kernels: lsh_kernels.hpp, lsh_add_kernels.hpp for rows that join live tables,
// lsh_remove_kernels.hpp for rows that leave them and lsh_update_kernels.hpp for rows that take new values).
#include <string.h>

#include <new>
#include <vector>

#include "engine.hpp"
#include "ivf_update_ids.hpp"
#include "javarandom.hpp"
#include "lsh_add_kernels.hpp"
#include "lsh_kernels.hpp"
#include "lsh_remove_ids.hpp"
#include "lsh_remove_kernels.hpp"
#include "lsh_update_kernels.hpp"

namespace hg {

static int launch_lsh_hash(int nch, const LshHashArgs &a, hipStream_t st) {
    if (a.n <= 0) return 0;
#define CALL(N, R, L)                                                                                                          \
    hipLaunchKernelGGL((lsh_hash_kernel<N, R>), dim3(static_cast<unsigned>((a.n + kNWave * R - 1) / (kNWave * R))), dim3(kWG), 0, st, a)
    HG_DISPATCH(nch, false, CALL);
#undef CALL
    HG_HIP(hipGetLastError());
    return 0;
}

static int launch_lsh_scan(int nch, const LshScanArgs &a, hipStream_t st) {
    const size_t lds = a.take_max > kWave ? sizeof(uint64_t) * kNWave * a.take_max : 0;
    const unsigned grid = static_cast<unsigned>((a.npairs + kNWave - 1) / kNWave);
#define CALL(N, R, L) hipLaunchKernelGGL((lsh_bucket_scan_kernel<N, R, L>), dim3(grid), dim3(kWG), lds, st, a)
    HG_DISPATCH(nch, a.metric == METRIC_L2, CALL);
#undef CALL
    HG_HIP(hipGetLastError());
    return 0;
}

// (a.allow set) the same grid over lsh_filtered_scan_kernel: its queues come first in LDS
static int launch_lsh_filtered_scan(int nch, const LshScanArgs &a, hipStream_t st) {
    const size_t keys = a.take_max > kWave ? sizeof(uint64_t) * kNWave * a.take_max : 0;
    const unsigned grid = static_cast<unsigned>((a.npairs + kNWave - 1) / kNWave);
#define CALL(N, R, L) hipLaunchKernelGGL((lsh_filtered_scan_kernel<N, R, L>), dim3(grid), dim3(kWG), lsh_queue_bytes(R) + keys, st, a)
    HG_DISPATCH(nch, a.metric == METRIC_L2, CALL);
#undef CALL
    HG_HIP(hipGetLastError());
    return 0;
}

// The tables a build or an install stages: the handle takes them over only when every step has succeeded.
struct LshStaged {
    float *planes = nullptr;
    uint16_t *codes = nullptr;
    int64_t *off = nullptr;
    int32_t *ids = nullptr;
    ~LshStaged() {
        void *ptrs[] = {planes, codes, off, ids};
        for (void *p : ptrs)
            if (p) (void)hipFree(p);
    }
};

// The rows of a handle and their tables as hnswgpu_lsh_add / hnswgpu_lsh_remove stage them: what is left in it when it goes out
// of scope is freed -- the staged arrays on an early return, the handle's old ones behind the swap.
struct LshStagedRows {
    float *base = nullptr, *norms = nullptr;
    uint32_t *qrows = nullptr;
    float4 *qmeta = nullptr;
    LshStaged lsh;  // (the planes stay the handle's)
    ~LshStagedRows() {
        void *ptrs[] = {base, norms, qrows, qmeta};
        for (void *p : ptrs)
            if (p) (void)hipFree(p);
    }
    void swap_into(hnswgpu_index *idx, int64_t n) {
        std::swap(idx->d_base, base);  // (what the handle had goes with this object)
        std::swap(idx->d_norms, norms);
        std::swap(idx->d_qrows, qrows);
        std::swap(idx->d_qmeta, qmeta);
        std::swap(idx->d_lsh_codes, lsh.codes);
        std::swap(idx->d_lsh_off, lsh.off);
        std::swap(idx->d_lsh_ids, lsh.ids);
        idx->n = n;
    }
};

// planes: [tables][bits][dim] on the host.  Hash on the device; the buckets by a stable counting sort of the codes on the host
// (one pass per table over n codes read back: rows ascending inside a bucket by construction, never by the order of atomics).
static int lsh_install(hnswgpu_index *idx, Call &call, const float *planes, int32_t tables, int32_t bits, hipStream_t st) {
    const int64_t n = idx->n, ld = idx->ld, np = static_cast<int64_t>(tables) * bits, nb = static_cast<int64_t>(1) << bits;
    LshStaged s;
    HG_HIP(hipMalloc(reinterpret_cast<void **>(&s.planes), sizeof(float) * np * ld));
    if (ld != idx->dim) HG_HIP(hipMemsetAsync(s.planes, 0, sizeof(float) * np * ld, st));
    HG_HIP(hipMemcpy2DAsync(s.planes, sizeof(float) * ld, planes, sizeof(float) * idx->dim, sizeof(float) * idx->dim, np,
                            hipMemcpyHostToDevice, st));
    HG_HIP(hipMalloc(reinterpret_cast<void **>(&s.off), sizeof(int64_t) * tables * (nb + 1)));
    std::vector<int64_t> off(static_cast<size_t>(tables) * (nb + 1), 0);
    std::vector<int32_t> ids(static_cast<size_t>(tables) * n);
    if (n > 0) {
        HG_HIP(hipMalloc(reinterpret_cast<void **>(&s.codes), sizeof(uint16_t) * n * tables));
        HG_HIP(hipMalloc(reinterpret_cast<void **>(&s.ids), sizeof(int32_t) * n * tables));
        LshHashArgs h;
        h.planes = s.planes;
        h.rows = idx->d_base;
        h.ld = ld;
        h.n = n;
        h.tables = tables;
        h.bits = bits;
        h.codes = s.codes;
        HG_TRY(launch_lsh_hash(idx->nch, h, st));
        std::vector<uint16_t> codes(static_cast<size_t>(n) * tables);
        HG_HIP(hipMemcpyAsync(codes.data(), s.codes, sizeof(uint16_t) * codes.size(), hipMemcpyDeviceToHost, st));
        HG_HIP(hipStreamSynchronize(st));
        for (int32_t t = 0; t < tables; t++) {
            int64_t *o = off.data() + static_cast<size_t>(t) * (nb + 1);
            for (int64_t r = 0; r < n; r++) o[codes[r * tables + t] + 1]++;
            for (int64_t b = 0; b < nb; b++) o[b + 1] += o[b];
            std::vector<int64_t> at(o, o + nb);
            int32_t *dst = ids.data() + static_cast<size_t>(t) * n;
            for (int64_t r = 0; r < n; r++) dst[at[codes[r * tables + t]]++] = static_cast<int32_t>(r);
        }
        HG_HIP(hipMemcpyAsync(s.ids, ids.data(), sizeof(int32_t) * ids.size(), hipMemcpyHostToDevice, st));
    }
    HG_HIP(hipMemcpyAsync(s.off, off.data(), sizeof(int64_t) * off.size(), hipMemcpyHostToDevice, st));
    std::vector<float> keep(planes, planes + np * idx->dim);
    HG_TRY(call.quiesce());  // the uploads are done (the host vectors go away), and no search reads the old tables any more
    std::swap(idx->d_lsh_planes, s.planes);  // (what the handle had goes with `s`)
    std::swap(idx->d_lsh_codes, s.codes);
    std::swap(idx->d_lsh_off, s.off);
    std::swap(idx->d_lsh_ids, s.ids);
    idx->h_lsh_planes.swap(keep);
    idx->lsh_tables = tables;
    idx->lsh_bits = bits;
    return 0;
}

static int check_lsh_shape(const hnswgpu_index *idx, int32_t tables, int32_t bits) {
    HG_REQUIRE(idx, HNSWGPU_EINVAL, "idx is null");
    HG_REQUIRE(tables >= 1, HNSWGPU_EINVAL, "tables must be >= 1");
    HG_REQUIRE(tables <= kLshMaxTables, HNSWGPU_ELIMIT, "more than %d hash tables are not supported", kLshMaxTables);
    HG_REQUIRE(bits >= 1 && bits <= kLshMaxBits, HNSWGPU_ELIMIT, "need 1 <= bits <= %d", kLshMaxBits);
    return 0;
}

// Everything hnswgpu_lsh_search* checks and clamps, before the lock
static int check_lsh_search(const hnswgpu_index *idx, const void *Q, int32_t nq, int32_t k, int32_t num_probes, int32_t probe_radius,
                            int32_t take_main, int32_t take_flip, const void *ids, const void *dist) {
    HG_REQUIRE(idx, HNSWGPU_EINVAL, "idx is null");
    HG_REQUIRE(nq >= 0, HNSWGPU_EINVAL, "nq < 0");
    HG_REQUIRE(k >= 1, HNSWGPU_EINVAL, "k must be >= 1");
    HG_REQUIRE(take_main >= 1 && take_flip >= 1, HNSWGPU_EINVAL, "take_main and take_flip must be >= 1");
    HG_REQUIRE(num_probes >= 1 && probe_radius >= 0, HNSWGPU_EINVAL, "need num_probes >= 1 and probe_radius >= 0");
    HG_REQUIRE(nq == 0 || (Q && ids && dist), HNSWGPU_EINVAL, "null argument");
    HG_REQUIRE(k <= kLshMaxK, HNSWGPU_ELIMIT, "k > %d is not supported by the LSH search", kLshMaxK);
    HG_REQUIRE(take_main <= kLshMaxTake && take_flip <= kLshMaxTake, HNSWGPU_ELIMIT, "take_main / take_flip > %d is not supported",
               kLshMaxTake);
    return 0;
}

// d_Q [nq][dim] -> d_ids / d_dist [nq][k] on `st`; only enqueues.  The caller holds the handle's Call and has checked the arguments.
// d_allow: null -- the unfiltered search; else the mask of query q is d_allow + q * allow_stride ((n + 31) / 32 words; stride 0:
// one mask for the call), and the bucket scan is the filtered one.  Hash, probe table, keys and merge are the same either way.
static int lsh_search_enqueue(hnswgpu_index *idx, const float *d_Q, int32_t nq, int32_t k, int32_t num_probes, int32_t probe_radius,
                              int32_t take_main, int32_t take_flip, const uint32_t *d_allow, int64_t allow_stride, int32_t *d_ids,
                              float *d_dist, hipStream_t st) {
    HG_REQUIRE(idx->lsh_tables > 0, HNSWGPU_ESTATE, "index has no LSH tables (call hnswgpu_lsh_build / hnswgpu_set_lsh first)");
    const int32_t probes = std::min(num_probes, idx->lsh_tables), radius = std::min(probe_radius, idx->lsh_bits);
    const int32_t pp = probes * (1 + radius), take_max = std::max(take_main, take_flip);
    HG_REQUIRE(static_cast<int64_t>(pp) * idx->n < (static_cast<int64_t>(1) << 32), HNSWGPU_ELIMIT,
               "the probe stream of one query (probes x (1 + radius) x n rows) must stay below 2^32");
    if (idx->n == 0) return fill_empty_dev(d_ids, d_dist, static_cast<int64_t>(nq) * k, st);
    // slices of queries: 12 bytes per key slot of a query's pairs, a GiB of them at a time
    const int64_t per_query = static_cast<int64_t>(pp) * take_max;
    const int32_t slice = static_cast<int32_t>(std::min<int64_t>(nq, std::max<int64_t>(1, (static_cast<int64_t>(1) << 30) / (12 * per_query))));
    HG_TRY(idx->s_misc.ensure(sizeof(uint16_t) * static_cast<size_t>(slice) * idx->lsh_tables));
    HG_TRY(idx->s_pairs.ensure(sizeof(LshPair) * static_cast<size_t>(slice) * pp));
    HG_TRY(idx->s_partial.ensure(sizeof(uint64_t) * static_cast<size_t>(slice) * per_query));
    HG_TRY(idx->s_ord.ensure(sizeof(int32_t) * static_cast<size_t>(slice) * per_query));
    for (int32_t q0 = 0; q0 < nq; q0 += slice) {
        const int32_t m = std::min(slice, nq - q0);
        const float *Qs = d_Q + static_cast<int64_t>(q0) * idx->dim;
        HG_TRY(pad_queries(idx, Qs, idx->dim, m, st));  // the hash kernel reads whole float4s of zero-padded rows
        LshHashArgs h;
        h.planes = idx->d_lsh_planes;
        h.rows = idx->s_qp.as<float>();
        h.ld = idx->ld;
        h.n = m;
        h.tables = idx->lsh_tables;
        h.bits = idx->lsh_bits;
        h.codes = idx->s_misc.as<uint16_t>();
        HG_TRY(launch_lsh_hash(idx->nch, h, st));
        LshProbeArgs p;
        p.qcodes = h.codes;
        p.off = idx->d_lsh_off;
        p.n = idx->n;
        p.nq = m;
        p.tables = idx->lsh_tables;
        p.bits = idx->lsh_bits;
        p.probes = probes;
        p.radius = radius;
        p.take_main = take_main;
        p.take_flip = take_flip;
        p.pairs = idx->s_pairs.as<LshPair>();
        hipLaunchKernelGGL(lsh_probe_kernel, dim3((m + 255) / 256), dim3(256), 0, st, p);
        HG_HIP(hipGetLastError());
        LshScanArgs a;
        a.rows = idx->d_base;
        a.row_norms = idx->d_norms;
        a.ld = idx->ld;
        a.Q = Qs;
        a.qld = idx->dim;
        a.dim = idx->dim;
        a.metric = idx->metric;
        a.pairs = p.pairs;
        a.npairs = static_cast<int64_t>(m) * pp;
        a.ids = idx->d_lsh_ids;
        a.take_max = take_max;
        a.keys = idx->s_partial.as<uint64_t>();
        a.key_rows = idx->s_ord.as<int32_t>();
        a.allow = d_allow ? d_allow + static_cast<int64_t>(q0) * allow_stride : nullptr;  // (LshPair::q counts from the slice's first query)
        a.allow_stride = allow_stride;
        a.n = idx->n;
        HG_TRY(d_allow ? launch_lsh_filtered_scan(idx->nch, a, st) : launch_lsh_scan(idx->nch, a, st));
        LshMergeArgs g;
        g.keys = a.keys;
        g.key_rows = a.key_rows;
        g.nq = m;
        g.pp = pp;
        g.take_max = take_max;
        g.k = k;
        g.out_ids = d_ids + static_cast<int64_t>(q0) * k;
        g.out_dist = d_dist + static_cast<int64_t>(q0) * k;
        hipLaunchKernelGGL(lsh_merge_kernel, dim3(m), dim3(kWave), 0, st, g);
        HG_HIP(hipGetLastError());
    }
    return 0;
}

}  // namespace hg

using namespace hg;

extern "C" {

int hnswgpu_lsh_build(hnswgpu_index *idx, int32_t tables, int32_t bits, int32_t proj_dim, int64_t seed) {
    HG_TRY(check_lsh_shape(idx, tables, bits));
    HG_REQUIRE(proj_dim >= bits, HNSWGPU_EINVAL, "proj_dim must be >= bits");
    // (generate-random-matrix, :24-31: table by table, row by row, tables x proj_dim x dim draws; a table keeps its first `bits` rows)
    std::vector<float> planes(static_cast<size_t>(tables) * bits * idx->dim);
    JavaRandom rng(seed);
    for (int32_t t = 0; t < tables; t++)
        for (int32_t i = 0; i < proj_dim; i++)
            for (int32_t d = 0; d < idx->dim; d++) {
                const double g = rng.next_gaussian();
                if (i < bits) planes[(static_cast<size_t>(t) * bits + i) * idx->dim + d] = static_cast<float>(g);
            }
    hipStream_t st = idx->stream;
    Call call;
    HG_TRY(call.open(idx, st));
    HG_TRY(lsh_install(idx, call, planes.data(), tables, bits, st));
    HG_TRY(call.sync());
    return call.close();
}

int hnswgpu_set_lsh(hnswgpu_index *idx, const float *planes, int32_t tables, int32_t bits) {
    HG_REQUIRE(idx && planes, HNSWGPU_EINVAL, "null argument");
    HG_TRY(check_lsh_shape(idx, tables, bits));
    hipStream_t st = idx->stream;
    Call call;
    HG_TRY(call.open(idx, st));
    HG_TRY(lsh_install(idx, call, planes, tables, bits, st));
    HG_TRY(call.sync());
    return call.close();
}

int hnswgpu_lsh_sizes(hnswgpu_index *idx, int32_t *tables, int32_t *bits) {
    HG_REQUIRE(idx, HNSWGPU_EINVAL, "idx is null");
    std::lock_guard<std::mutex> lk(idx->mu);
    if (tables) *tables = idx->lsh_tables;
    if (bits) *bits = idx->lsh_bits;
    return 0;
}

int hnswgpu_lsh_get(hnswgpu_index *idx, float *planes, uint16_t *codes, int64_t *off, int32_t *ids) {
    HG_REQUIRE(idx, HNSWGPU_EINVAL, "idx is null");
    hipStream_t st = idx->stream;
    Call call;
    HG_TRY(call.open(idx, st));
    HG_REQUIRE(idx->lsh_tables > 0, HNSWGPU_ESTATE, "index has no LSH tables (call hnswgpu_lsh_build / hnswgpu_set_lsh first)");
    const size_t T = idx->lsh_tables, n = idx->n, nb1 = (static_cast<size_t>(1) << idx->lsh_bits) + 1;
    if (planes) memcpy(planes, idx->h_lsh_planes.data(), sizeof(float) * idx->h_lsh_planes.size());
    if (codes && n) HG_HIP(hipMemcpyAsync(codes, idx->d_lsh_codes, sizeof(uint16_t) * n * T, hipMemcpyDeviceToHost, st));
    if (off) HG_HIP(hipMemcpyAsync(off, idx->d_lsh_off, sizeof(int64_t) * T * nb1, hipMemcpyDeviceToHost, st));
    if (ids && n) HG_HIP(hipMemcpyAsync(ids, idx->d_lsh_ids, sizeof(int32_t) * n * T, hipMemcpyDeviceToHost, st));
    HG_TRY(call.sync());
    return call.close();
}

int hnswgpu_lsh_hash(hnswgpu_index *idx, const float *Q, int32_t nq, uint16_t *codes) {
    HG_REQUIRE(idx, HNSWGPU_EINVAL, "idx is null");
    HG_REQUIRE(nq >= 0, HNSWGPU_EINVAL, "nq < 0");
    HG_REQUIRE(nq == 0 || (Q && codes), HNSWGPU_EINVAL, "null argument");
    if (nq == 0) return 0;
    hipStream_t st = idx->stream;
    Call call;
    HG_TRY(call.open(idx, st));
    HG_REQUIRE(idx->lsh_tables > 0, HNSWGPU_ESTATE, "index has no LSH tables (call hnswgpu_lsh_build / hnswgpu_set_lsh first)");
    HG_TRY(upload_queries(idx, Q, nq, st));
    HG_TRY(pad_queries(idx, idx->s_q.as<float>(), idx->dim, nq, st));
    HG_TRY(idx->s_misc.ensure(sizeof(uint16_t) * static_cast<size_t>(nq) * idx->lsh_tables));
    LshHashArgs h;
    h.planes = idx->d_lsh_planes;
    h.rows = idx->s_qp.as<float>();
    h.ld = idx->ld;
    h.n = nq;
    h.tables = idx->lsh_tables;
    h.bits = idx->lsh_bits;
    h.codes = idx->s_misc.as<uint16_t>();
    HG_TRY(launch_lsh_hash(idx->nch, h, st));
    HG_HIP(hipMemcpyAsync(codes, h.codes, sizeof(uint16_t) * static_cast<size_t>(nq) * idx->lsh_tables, hipMemcpyDeviceToHost, st));
    HG_TRY(call.sync());
    return call.close();
}

// Rows join the tables of a live handle (include/hnswgpu.h).  The reference's HybridIndex has no add; what is restated is its
// bucket order (hybrid_lsh.clj:105-129: insertion order, which is row order): the grown handle holds what hnswgpu_create(all
// rows) + hnswgpu_set_lsh(the same planes) holds.  One chain on the handle's stream: base / norms / int8 rows grow as in
// hnswgpu_ivf_add, lsh_hash_kernel hashes the new rows behind a device copy of the old codes, four integer kernels
// (lsh_add_kernels.hpp) count, scan, place the new rows and move the old members; ONE readback of a word per table says that
// every table's grown buckets hold all rows.
int hnswgpu_lsh_add(hnswgpu_index *idx, const float *rows, int64_t m) {
    HG_REQUIRE(idx, HNSWGPU_EINVAL, "idx is null");
    HG_REQUIRE(m >= 0, HNSWGPU_EINVAL, "m must be >= 0");
    if (m == 0) return 0;
    HG_REQUIRE(rows, HNSWGPU_EINVAL, "rows is null");
    hipStream_t st = idx->stream;
    Call call;
    HG_TRY(call.open(idx, st));
    HG_REQUIRE(idx->lsh_tables > 0, HNSWGPU_ESTATE, "index has no LSH tables (call hnswgpu_lsh_build / hnswgpu_set_lsh first)");
    HG_REQUIRE(!idx->has_graph || idx->nparts > 0, HNSWGPU_ESTATE,
               "the index holds an HNSW graph: rows added to the LSH tables would be missing from the graph");
    HG_REQUIRE(idx->nparts == 0, HNSWGPU_ESTATE,
               "the index holds a forest of HNSW sub-graphs: rows added to the LSH tables would be missing from its parts");
    HG_REQUIRE(idx->nlist == 0 || idx->d_glistoff != nullptr, HNSWGPU_ESTATE,
               "the index holds IVF lists: rows added to the LSH tables would be missing from the lists");
    HG_REQUIRE(idx->d_glistoff == nullptr, HNSWGPU_ESTATE,
               "a shard of a larger IVF index (hnswgpu_set_ivf_shard) cannot grow alone: its lists would miss the rows");
    const int64_t n0 = idx->n, n1 = n0 + m;
    HG_REQUIRE(n1 < 2147483647LL, HNSWGPU_ELIMIT, "the index must hold fewer than 2^31 rows");
    HG_TRY(call.quiesce());
    const int64_t ld = idx->ld, nb = static_cast<int64_t>(1) << idx->lsh_bits;
    const int32_t tables = idx->lsh_tables;
    // Failure-atomic, as hnswgpu_ivf_add: every array the call makes is STAGED and goes with `nw` on an early return; the handle's
    // fields change only behind the last step (idx->mu is held and the streams are quiesced: no caller sees a state in between).
    LshStagedRows nw;
    auto grow = [&]() -> int {
        // ---- 1. the base matrix, its norms and base-order int8 rows grow
        HG_HIP(hipMalloc(reinterpret_cast<void **>(&nw.base), sizeof(float) * static_cast<size_t>(n1) * ld));
        HG_HIP(hipMalloc(reinterpret_cast<void **>(&nw.norms), sizeof(float) * static_cast<size_t>(n1)));
        if (n0 > 0) {
            HG_HIP(hipMemcpyAsync(nw.base, idx->d_base, sizeof(float) * static_cast<size_t>(n0) * ld, hipMemcpyDeviceToDevice, st));
            HG_HIP(hipMemcpyAsync(nw.norms, idx->d_norms, sizeof(float) * static_cast<size_t>(n0), hipMemcpyDeviceToDevice, st));
        }
        if (ld != idx->dim) HG_HIP(hipMemsetAsync(nw.base + n0 * ld, 0, sizeof(float) * static_cast<size_t>(m) * ld, st));
        HG_HIP(hipMemcpy2DAsync(nw.base + n0 * ld, sizeof(float) * ld, rows, sizeof(float) * idx->dim, sizeof(float) * idx->dim,
                                static_cast<size_t>(m), hipMemcpyHostToDevice, st));
        HG_TRY(launch_norms(idx->nch, nw.base + n0 * ld, ld, m, nw.norms + n0, st));
        if (idx->d_qrows) HG_TRY(quantize_rows(idx, nw.base, n1, &nw.qrows, &nw.qmeta, st));  // (all rows again: one pass over the base)
        // ---- 2. the new rows' codes, by the kernel and under the planes that made the old ones, behind a copy of those
        HG_HIP(hipMalloc(reinterpret_cast<void **>(&nw.lsh.codes), sizeof(uint16_t) * static_cast<size_t>(n1) * tables));
        HG_HIP(hipMalloc(reinterpret_cast<void **>(&nw.lsh.off), sizeof(int64_t) * tables * (nb + 1)));
        HG_HIP(hipMalloc(reinterpret_cast<void **>(&nw.lsh.ids), sizeof(int32_t) * static_cast<size_t>(n1) * tables));
        if (n0 > 0)
            HG_HIP(hipMemcpyAsync(nw.lsh.codes, idx->d_lsh_codes, sizeof(uint16_t) * static_cast<size_t>(n0) * tables,
                                  hipMemcpyDeviceToDevice, st));
        LshHashArgs h;
        h.planes = idx->d_lsh_planes;
        h.rows = nw.base + n0 * ld;
        h.ld = ld;
        h.n = m;
        h.tables = tables;
        h.bits = idx->lsh_bits;
        h.codes = nw.lsh.codes + n0 * tables;
        HG_TRY(launch_lsh_hash(idx->nch, h, st));
        // ---- 3. - 6. count, offsets, place, splice: launch boundaries are the only dependences
        const size_t cbytes = sizeof(uint32_t) * static_cast<size_t>(tables) * nb;
        HG_TRY(idx->s_misc.ensure(cbytes));
        HG_HIP(hipMemsetAsync(idx->s_misc.p, 0, cbytes, st));
        LshAddArgs a;
        a.codes = nw.lsh.codes;
        a.n0 = n0;
        a.m = m;
        a.tables = tables;
        a.bits = idx->lsh_bits;
        a.old_off = idx->d_lsh_off;
        a.new_off = nw.lsh.off;
        a.cursor = idx->s_misc.as<uint32_t>();
        a.old_ids = idx->d_lsh_ids;
        a.new_ids = nw.lsh.ids;
        const unsigned count_wgs = static_cast<unsigned>(std::min<int64_t>((m + kWG - 1) / kWG, 256));
        hipLaunchKernelGGL(lsh_add_count_kernel, dim3(count_wgs, static_cast<unsigned>(tables)), dim3(kWG), 0, st, a);
        hipLaunchKernelGGL(lsh_add_offsets_kernel, dim3(static_cast<unsigned>(tables)), dim3(kWG), 0, st, a);
        if (nb <= kLshAddLdsBuckets)
            hipLaunchKernelGGL(lsh_add_place_kernel<true>, dim3(static_cast<unsigned>(tables)), dim3(kWave), 0, st, a);
        else
            hipLaunchKernelGGL(lsh_add_place_kernel<false>, dim3(static_cast<unsigned>(tables)), dim3(kWave), 0, st, a);
        if (n0 > 0)
            hipLaunchKernelGGL(lsh_add_splice_kernel, dim3(static_cast<unsigned>((n0 * tables + kWG - 1) / kWG)), dim3(kWG), 0, st, a);
        HG_HIP(hipGetLastError());
        // ---- the one readback: every table's last offset (the tables have no host mirrors besides the planes)
        int64_t total[kLshMaxTables];
        HG_HIP(hipMemcpy2DAsync(total, sizeof(int64_t), nw.lsh.off + nb, sizeof(int64_t) * (nb + 1), sizeof(int64_t),
                                static_cast<size_t>(tables), hipMemcpyDeviceToHost, st));
        HG_HIP(hipStreamSynchronize(st));
        for (int32_t t = 0; t < tables; t++)
            HG_REQUIRE(total[t] == n1, HNSWGPU_EHIP, "the grown buckets of table %d hold %lld rows, not %lld", t, (long long)total[t],
                       (long long)n1);
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

// Rows leave the tables of a live handle (include/hnswgpu.h).  The reference's HybridIndex has no remove either; what is restated
// is again its bucket order: the shrunken handle holds what hnswgpu_create(the kept rows in their old order) + hnswgpu_set_lsh(the
// same planes) holds.  One chain on the handle's stream (lsh_remove_kernels.hpp): mark, rank, the kept rows / norms / codes to
// their ranks, removed rows per bucket, offsets, and the bucket ids compacted and renumbered (chunk counts, their scan, the
// scatter); ONE readback of 2 x tables + 1 words says that the rank scan, every table's last offset and every table's compacted
// ids all hold n1 rows.  Norms and codes are copied, not computed again; the int8 rows are made over the new base as add does.
int hnswgpu_lsh_remove(hnswgpu_index *idx, const int32_t *rows, int64_t m, int64_t *n_after) {
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
    HG_REQUIRE(idx->lsh_tables > 0, HNSWGPU_ESTATE, "index has no LSH tables (call hnswgpu_lsh_build / hnswgpu_set_lsh first)");
    HG_REQUIRE(!idx->has_graph || idx->nparts > 0, HNSWGPU_ESTATE,
               "the index holds an HNSW graph: it would keep the old numbering of the rows");
    HG_REQUIRE(idx->nparts == 0, HNSWGPU_ESTATE,
               "the index holds a forest of HNSW sub-graphs: its parts would keep the old numbering of the rows");
    HG_REQUIRE(idx->nlist == 0 || idx->d_glistoff != nullptr, HNSWGPU_ESTATE,
               "the index holds IVF lists: they would keep the old numbering of the rows");
    HG_REQUIRE(idx->d_glistoff == nullptr, HNSWGPU_ESTATE,
               "a shard of a larger IVF index (hnswgpu_set_ivf_shard) cannot shrink alone: its lists would keep the old numbering");
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
    const int64_t ld = idx->ld, nb = static_cast<int64_t>(1) << idx->lsh_bits;
    const int32_t tables = idx->lsh_tables;
    LshStagedRows nw;  // failure-atomic, as hnswgpu_lsh_add: the handle's fields change only behind the last step
    auto shrink = [&]() -> int {
        if (n1 > 0) {
            HG_HIP(hipMalloc(reinterpret_cast<void **>(&nw.base), sizeof(float) * static_cast<size_t>(n1) * ld));
            HG_HIP(hipMalloc(reinterpret_cast<void **>(&nw.norms), sizeof(float) * static_cast<size_t>(n1)));
            HG_HIP(hipMalloc(reinterpret_cast<void **>(&nw.lsh.codes), sizeof(uint16_t) * static_cast<size_t>(n1) * tables));
            HG_HIP(hipMalloc(reinterpret_cast<void **>(&nw.lsh.ids), sizeof(int32_t) * static_cast<size_t>(n1) * tables));
        }
        HG_HIP(hipMalloc(reinterpret_cast<void **>(&nw.lsh.off), sizeof(int64_t) * tables * (nb + 1)));
        // scratch, 16-byte sections: [gate | keep | removed] zeroed, then word_rank, chunk_base, the call's ids
        LshRemoveArgs a;
        a.n0 = n0;
        a.n1 = n1;
        a.m = m;
        a.W = (n0 + 31) / 32;
        a.ld = ld;
        a.tables = tables;
        a.bits = idx->lsh_bits;
        a.nchunks = (n0 + kWG - 1) / kWG;
        auto sect = [](size_t bytes) { return (bytes + 15) / 16 * 16; };
        const size_t o_keep = sect(sizeof(int64_t) * kLshRemoveGate), o_removed = o_keep + sect(sizeof(uint32_t) * a.W),
                     o_rank = o_removed + sect(sizeof(uint32_t) * tables * nb), o_chunk = o_rank + sect(sizeof(uint32_t) * a.W),
                     o_ids = o_chunk + sect(sizeof(uint32_t) * tables * a.nchunks), bytes = o_ids + sect(sizeof(int32_t) * m);
        HG_TRY(idx->s_misc.ensure(bytes));
        char *s = idx->s_misc.as<char>();
        HG_HIP(hipMemsetAsync(s, 0, o_rank, st));
        HG_HIP(hipMemcpyAsync(s + o_ids, rows, sizeof(int32_t) * static_cast<size_t>(m), hipMemcpyHostToDevice, st));
        a.gate = reinterpret_cast<int64_t *>(s);
        a.keep = reinterpret_cast<uint32_t *>(s + o_keep);
        a.removed = reinterpret_cast<uint32_t *>(s + o_removed);
        a.word_rank = reinterpret_cast<uint32_t *>(s + o_rank);
        a.chunk_base = reinterpret_cast<uint32_t *>(s + o_chunk);
        a.rows = reinterpret_cast<const int32_t *>(s + o_ids);
        a.old_base = idx->d_base;
        a.old_norms = idx->d_norms;
        a.old_codes = idx->d_lsh_codes;
        a.new_base = nw.base;
        a.new_norms = nw.norms;
        a.new_codes = nw.lsh.codes;
        a.old_off = idx->d_lsh_off;
        a.new_off = nw.lsh.off;
        a.old_ids = idx->d_lsh_ids;
        a.new_ids = nw.lsh.ids;
        const unsigned T = static_cast<unsigned>(tables), chunks = static_cast<unsigned>(a.nchunks);
        hipLaunchKernelGGL(lsh_remove_mark_kernel, dim3(static_cast<unsigned>((m + kWG - 1) / kWG)), dim3(kWG), 0, st, a);
        hipLaunchKernelGGL(lsh_remove_rank_kernel, dim3(1), dim3(kWG), 0, st, a);
        if (n1 > 0) hipLaunchKernelGGL(lsh_remove_rows_kernel, dim3(static_cast<unsigned>((n0 + kNWave - 1) / kNWave)), dim3(kWG), 0, st, a);
        const unsigned count_wgs = static_cast<unsigned>(std::min<int64_t>((a.W + kWG - 1) / kWG, 256));
        hipLaunchKernelGGL(lsh_remove_count_kernel, dim3(count_wgs, T), dim3(kWG), 0, st, a);
        hipLaunchKernelGGL(lsh_remove_offsets_kernel, dim3(T), dim3(kWG), 0, st, a);
        hipLaunchKernelGGL(lsh_remove_chunk_count_kernel, dim3(chunks, T), dim3(kWG), 0, st, a);
        hipLaunchKernelGGL(lsh_remove_chunk_scan_kernel, dim3(T), dim3(kWG), 0, st, a);
        if (n1 > 0) hipLaunchKernelGGL(lsh_remove_ids_kernel, dim3(chunks, T), dim3(kWG), 0, st, a);
        HG_HIP(hipGetLastError());
        if (idx->d_qrows && n1 > 0) HG_TRY(quantize_rows(idx, nw.base, n1, &nw.qrows, &nw.qmeta, st));  // (as add: one pass over the new base)
        // ---- the one readback
        int64_t gate[kLshRemoveGate];
        HG_HIP(hipMemcpyAsync(gate, a.gate, sizeof(gate), hipMemcpyDeviceToHost, st));
        HG_HIP(hipStreamSynchronize(st));
        HG_REQUIRE(gate[2 * kLshMaxTables] == n1, HNSWGPU_EHIP, "the mask keeps %lld rows, not %lld", (long long)gate[2 * kLshMaxTables],
                   (long long)n1);
        for (int32_t t = 0; t < tables; t++) {
            HG_REQUIRE(gate[t] == n1, HNSWGPU_EHIP, "the shrunken buckets of table %d hold %lld rows, not %lld", t, (long long)gate[t],
                       (long long)n1);
            HG_REQUIRE(gate[kLshMaxTables + t] == n1, HNSWGPU_EHIP, "the compacted ids of table %d hold %lld rows, not %lld", t,
                       (long long)gate[kLshMaxTables + t], (long long)n1);
        }
        return 0;
    };
    const int rc = shrink();
    if (rc != 0) {
        (void)hipStreamSynchronize(st);  // (nothing of the chain is in flight when `nw` frees what it staged)
        return rc;
    }
    nw.swap_into(idx, n1);  // (n1 == 0: no base, norms, codes or ids -- an empty handle with planes and all-zero offsets)
    if (n_after) *n_after = n1;
    return call.close();
}

// Rows of a live handle with tables take new values under their ids (include/hnswgpu.h).  The reference's HybridIndex is an
// immutable record and "Update existing vectors" an open item of its to-do list; what is restated is again its bucket order: the
// updated handle holds what hnswgpu_create(the base with the new values) + hnswgpu_set_lsh(the same planes) holds.  One chain on
// the handle's stream (lsh_update_kernels.hpp): the call's rows into a staging matrix in slot order (slot s = the s-th smallest
// id, ivf_update_ids.hpp), their norms (launch_norms) and codes (lsh_hash_kernel), device copies of base / norms / codes with the
// m rows scattered in, per table the entries that leave and join every bucket, the new offsets, the movers grouped by the bucket
// they leave and by the bucket they join, and the placement of the entries that stay and of those that join; the int8 rows are
// made over the new base as add does; ONE readback of four words per table.
int hnswgpu_lsh_update(hnswgpu_index *idx, const int32_t *ids, const float *rows, int64_t m) {
    HG_REQUIRE(idx, HNSWGPU_EINVAL, "idx is null");
    HG_REQUIRE(m >= 0, HNSWGPU_EINVAL, "m must be >= 0");
    HG_REQUIRE(ids || m == 0, HNSWGPU_EINVAL, "ids is null");
    HG_REQUIRE(rows || m == 0, HNSWGPU_EINVAL, "rows is null");
    if (m == 0) return 0;  // nothing to update: nothing happens, whatever the handle holds
    hipStream_t st = idx->stream;
    Call call;
    HG_TRY(call.open(idx, st));
    HG_REQUIRE(idx->lsh_tables > 0, HNSWGPU_ESTATE, "index has no LSH tables (call hnswgpu_lsh_build / hnswgpu_set_lsh first)");
    HG_REQUIRE(!idx->has_graph || idx->nparts > 0, HNSWGPU_ESTATE,
               "the index holds an HNSW graph: its edges would stand for the old values of the rows");
    HG_REQUIRE(idx->nparts == 0, HNSWGPU_ESTATE,
               "the index holds a forest of HNSW sub-graphs: its edges would stand for the old values of the rows");
    HG_REQUIRE(idx->nlist == 0 || idx->d_glistoff != nullptr, HNSWGPU_ESTATE,
               "the index holds IVF lists: they would keep the old values of the rows");
    HG_REQUIRE(idx->d_glistoff == nullptr, HNSWGPU_ESTATE,
               "a shard of a larger IVF index (hnswgpu_set_ivf_shard) cannot be updated alone: its lists would keep the old values");
    const int64_t n = idx->n;
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
    const int64_t ld = idx->ld, nb = static_cast<int64_t>(1) << idx->lsh_bits;
    const int32_t tables = idx->lsh_tables;
    LshStagedRows nw;  // failure-atomic, as hnswgpu_lsh_add: the handle's fields change only behind the last step
    auto update = [&]() -> int {
        const size_t nn = static_cast<size_t>(n), mm = static_cast<size_t>(m), T = static_cast<size_t>(tables);
        HG_HIP(hipMalloc(reinterpret_cast<void **>(&nw.base), sizeof(float) * nn * ld));
        HG_HIP(hipMalloc(reinterpret_cast<void **>(&nw.norms), sizeof(float) * nn));
        HG_HIP(hipMalloc(reinterpret_cast<void **>(&nw.lsh.codes), sizeof(uint16_t) * nn * T));
        HG_HIP(hipMalloc(reinterpret_cast<void **>(&nw.lsh.off), sizeof(int64_t) * T * (nb + 1)));
        HG_HIP(hipMalloc(reinterpret_cast<void **>(&nw.lsh.ids), sizeof(int32_t) * nn * T));
        // scratch.  s_tile: the caller's rows as they came.  s_misc2: the staging matrix and its norms.  s_misc, 16-byte sections:
        // [gate | count] zeroed, then seg, grouped, the slots' row ids and call positions, their new and their old codes
        LshUpdateArgs a;
        memset(&a, 0, sizeof(a));
        a.n = n;
        a.m = m;
        a.ld = ld;
        a.dim = idx->dim;
        a.tables = tables;
        a.bits = idx->lsh_bits;
        auto sect = [](size_t bytes) { return (bytes + 15) / 16 * 16; };
        const size_t o_count = sect(sizeof(unsigned long long) * kLshUpdateGate), o_seg = o_count + sect(sizeof(uint32_t) * 2 * T * nb),
                     o_grouped = o_seg + sect(sizeof(uint32_t) * 2 * T * (nb + 1)), o_uid = o_grouped + sect(sizeof(int32_t) * 2 * T * mm),
                     o_from = o_uid + sect(sizeof(int32_t) * mm), o_scodes = o_from + sect(sizeof(int32_t) * mm),
                     o_ocodes = o_scodes + sect(sizeof(uint16_t) * mm * T), bytes = o_ocodes + sect(sizeof(uint16_t) * mm * T);
        HG_TRY(idx->s_misc.ensure(bytes));
        HG_TRY(idx->s_misc2.ensure(sect(sizeof(float) * mm * ld) + sizeof(float) * mm));
        HG_TRY(idx->s_tile.ensure(sizeof(float) * mm * idx->dim));
        char *s = idx->s_misc.as<char>();
        HG_HIP(hipMemsetAsync(s, 0, o_seg, st));
        HG_HIP(hipMemcpyAsync(s + o_uid, uid.data(), sizeof(int32_t) * mm, hipMemcpyHostToDevice, st));
        HG_HIP(hipMemcpyAsync(s + o_from, from.data(), sizeof(int32_t) * mm, hipMemcpyHostToDevice, st));
        HG_HIP(hipMemcpyAsync(idx->s_tile.p, rows, sizeof(float) * mm * idx->dim, hipMemcpyHostToDevice, st));
        a.gate = reinterpret_cast<unsigned long long *>(s);
        a.count = reinterpret_cast<uint32_t *>(s + o_count);
        a.seg = reinterpret_cast<uint32_t *>(s + o_seg);
        a.grouped = reinterpret_cast<int32_t *>(s + o_grouped);
        a.uid = reinterpret_cast<const int32_t *>(s + o_uid);
        a.from = reinterpret_cast<const int32_t *>(s + o_from);
        uint16_t *scodes = reinterpret_cast<uint16_t *>(s + o_scodes);
        a.scodes = scodes;
        a.ocodes = reinterpret_cast<uint16_t *>(s + o_ocodes);
        a.raw = idx->s_tile.as<float>();
        a.stage = idx->s_misc2.as<float>();
        float *snorms = reinterpret_cast<float *>(idx->s_misc2.as<char>() + sect(sizeof(float) * mm * ld));
        a.snorms = snorms;
        a.old_codes = idx->d_lsh_codes;
        a.new_base = nw.base;
        a.new_norms = nw.norms;
        a.new_codes = nw.lsh.codes;
        a.old_off = idx->d_lsh_off;
        a.new_off = nw.lsh.off;
        a.old_ids = idx->d_lsh_ids;
        a.new_ids = nw.lsh.ids;
        const unsigned slot_wgs = static_cast<unsigned>((m + kNWave - 1) / kNWave), Tu = static_cast<unsigned>(tables);
        // ---- 1. the staging matrix in slot order, its norms (the kernel hnswgpu_create uses: the same bits) and its codes (the
        // kernel and the planes that made the old ones)
        hipLaunchKernelGGL(lsh_update_stage_kernel, dim3(slot_wgs), dim3(kWG), 0, st, a);
        HG_HIP(hipGetLastError());
        HG_TRY(launch_norms(idx->nch, a.stage, ld, m, snorms, st));
        LshHashArgs h;
        h.planes = idx->d_lsh_planes;
        h.rows = a.stage;
        h.ld = ld;
        h.n = m;
        h.tables = tables;
        h.bits = idx->lsh_bits;
        h.codes = scodes;
        HG_TRY(launch_lsh_hash(idx->nch, h, st));
        // ---- 2. the staged base, norms and codes: device copies of the old ones with the m rows scattered in
        HG_HIP(hipMemcpyAsync(nw.base, idx->d_base, sizeof(float) * nn * ld, hipMemcpyDeviceToDevice, st));
        HG_HIP(hipMemcpyAsync(nw.norms, idx->d_norms, sizeof(float) * nn, hipMemcpyDeviceToDevice, st));
        HG_HIP(hipMemcpyAsync(nw.lsh.codes, idx->d_lsh_codes, sizeof(uint16_t) * nn * T, hipMemcpyDeviceToDevice, st));
        hipLaunchKernelGGL(lsh_update_scatter_kernel, dim3(slot_wgs), dim3(kWG), 0, st, a);
        if (idx->d_qrows) HG_TRY(quantize_rows(idx, nw.base, n, &nw.qrows, &nw.qmeta, st));  // (as add: one pass over the new base)
        // ---- 3. - 6. count, offsets, group, place: launch boundaries are the only dependences
        const unsigned count_wgs = static_cast<unsigned>(std::min<int64_t>((m + kWG - 1) / kWG, 256));
        hipLaunchKernelGGL(lsh_update_count_kernel, dim3(count_wgs, Tu, 2), dim3(kWG), 0, st, a);
        hipLaunchKernelGGL(lsh_update_offsets_kernel, dim3(Tu), dim3(kWG), 0, st, a);
        if (nb <= kLshAddLdsBuckets)
            hipLaunchKernelGGL(lsh_update_group_kernel<true>, dim3(Tu, 2), dim3(kWave), 0, st, a);
        else
            hipLaunchKernelGGL(lsh_update_group_kernel<false>, dim3(Tu, 2), dim3(kWave), 0, st, a);
        hipLaunchKernelGGL(lsh_update_keep_kernel, dim3(static_cast<unsigned>((n + kWG - 1) / kWG), Tu), dim3(kWG), 0, st, a);
        hipLaunchKernelGGL(lsh_update_join_kernel, dim3(static_cast<unsigned>((m + kWG - 1) / kWG), Tu), dim3(kWG), 0, st, a);
        HG_HIP(hipGetLastError());
        // ---- the one readback
        unsigned long long gate[kLshUpdateGate];
        HG_HIP(hipMemcpyAsync(gate, a.gate, sizeof(gate), hipMemcpyDeviceToHost, st));
        HG_HIP(hipStreamSynchronize(st));
        for (int32_t t = 0; t < tables; t++) {
            const long long total = static_cast<long long>(gate[LSH_UPD_TOTAL * kLshMaxTables + t]),
                            left = static_cast<long long>(gate[LSH_UPD_LEFT * kLshMaxTables + t]),
                            joined = static_cast<long long>(gate[LSH_UPD_JOINED * kLshMaxTables + t]),
                            placed = static_cast<long long>(gate[LSH_UPD_PLACED * kLshMaxTables + t]);
            HG_REQUIRE(total == n, HNSWGPU_EHIP, "the new buckets of table %d hold %lld rows, not %lld", t, total, (long long)n);
            HG_REQUIRE(left == joined, HNSWGPU_EHIP, "%lld entries left the buckets of table %d and %lld joined them", left, t, joined);
            HG_REQUIRE(placed == n, HNSWGPU_EHIP, "%lld entries of table %d were placed, not %lld", placed, t, (long long)n);
        }
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

int hnswgpu_lsh_search_dev(hnswgpu_index *idx, const float *d_Q, int32_t nq, int32_t k, int32_t num_probes, int32_t probe_radius,
                           int32_t take_main, int32_t take_flip, int32_t *d_out_ids, float *d_out_dist, void *stream) {
    HG_TRY(check_lsh_search(idx, d_Q, nq, k, num_probes, probe_radius, take_main, take_flip, d_out_ids, d_out_dist));
    if (nq == 0) return 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    Call call;
    HG_TRY(call.open(idx, st));
    HG_TRY(lsh_search_enqueue(idx, d_Q, nq, k, num_probes, probe_radius, take_main, take_flip, nullptr, 0, d_out_ids, d_out_dist, st));
    return call.close();
}

int hnswgpu_lsh_search(hnswgpu_index *idx, const float *Q, int32_t nq, int32_t k, int32_t num_probes, int32_t probe_radius,
                       int32_t take_main, int32_t take_flip, int32_t *out_ids, float *out_dist) {
    HG_TRY(check_lsh_search(idx, Q, nq, k, num_probes, probe_radius, take_main, take_flip, out_ids, out_dist));
    if (nq == 0) return 0;
    hipStream_t st = idx->stream;
    Call call;
    HG_TRY(call.open(idx, st));
    HG_TRY(call.stage_in(Q, nq, k));
    HG_TRY(lsh_search_enqueue(idx, idx->s_q.as<float>(), nq, k, num_probes, probe_radius, take_main, take_flip, nullptr, 0,
                              idx->s_ids.as<int32_t>(), idx->s_outd.as<float>(), st));
    HG_TRY(call.stage_out(out_ids, out_dist, static_cast<int64_t>(nq) * k));
    return call.close();
}

// ---- filtered search: the allow-mask through the bucket scan (lsh_filtered_scan_kernel; the contract: include/hnswgpu.h) ----
// One body for both forms of the mask: Single is stride 0, Each stride (n + 31) / 32.  Device arrays: enqueues only, reads
// nothing back -- nothing needs a count, the wave that reads a bucket filters it.
static int lsh_filtered_dev(hnswgpu_index *idx, MaskForm form, const float *d_Q, int32_t nq, int32_t k, int32_t num_probes,
                            int32_t probe_radius, int32_t take_main, int32_t take_flip, const uint32_t *d_allow, int32_t *d_out_ids,
                            float *d_out_dist, void *stream) {
    HG_TRY(check_lsh_search(idx, d_Q, nq, k, num_probes, probe_radius, take_main, take_flip, d_out_ids, d_out_dist));
    if (nq == 0) return 0;
    HG_REQUIRE(d_allow, HNSWGPU_EINVAL, "allow is null");
    hipStream_t st = static_cast<hipStream_t>(stream);
    Call call;
    HG_TRY(call.open(idx, st));
    const int64_t stride = form == MaskForm::Each ? (idx->n + 31) / 32 : 0;
    HG_TRY(lsh_search_enqueue(idx, d_Q, nq, k, num_probes, probe_radius, take_main, take_flip, d_allow, stride, d_out_ids, d_out_dist, st));
    return call.close();
}

// Host arrays.  One caller's batch, its mask -- Each: its [nq][W] masks -- staged whole as hnswgpu_ivf_search_filtered_each
// stages its own: masks differ between callers, so the call takes no part in the call combiner.
static int lsh_filtered_host(hnswgpu_index *idx, MaskForm form, const float *Q, int32_t nq, int32_t k, int32_t num_probes,
                             int32_t probe_radius, int32_t take_main, int32_t take_flip, const uint32_t *allow, int32_t *out_ids,
                             float *out_dist) {
    HG_TRY(check_lsh_search(idx, Q, nq, k, num_probes, probe_radius, take_main, take_flip, out_ids, out_dist));
    if (nq == 0) return 0;
    HG_REQUIRE(allow, HNSWGPU_EINVAL, "allow is null");
    hipStream_t st = idx->stream;
    Call call;
    HG_TRY(call.open(idx, st));
    HG_TRY(call.stage_in(Q, nq, k));
    if (idx->n > 0) HG_TRY(call.stage_mask(allow, form, nq));  // (an empty index has no mask words, and its search reads none)
    const int64_t stride = form == MaskForm::Each ? (idx->n + 31) / 32 : 0;
    HG_TRY(lsh_search_enqueue(idx, idx->s_q.as<float>(), nq, k, num_probes, probe_radius, take_main, take_flip,
                              idx->s_fmask.as<uint32_t>(), stride, idx->s_ids.as<int32_t>(), idx->s_outd.as<float>(), st));
    HG_TRY(call.stage_out(out_ids, out_dist, static_cast<int64_t>(nq) * k));
    return call.close();
}

int hnswgpu_lsh_search_filtered_dev(hnswgpu_index *idx, const float *d_Q, int32_t nq, int32_t k, int32_t num_probes, int32_t probe_radius,
                                    int32_t take_main, int32_t take_flip, const uint32_t *d_allow, int32_t *d_out_ids, float *d_out_dist,
                                    void *stream) {
    return lsh_filtered_dev(idx, MaskForm::Single, d_Q, nq, k, num_probes, probe_radius, take_main, take_flip, d_allow, d_out_ids,
                            d_out_dist, stream);
}
int hnswgpu_lsh_search_filtered(hnswgpu_index *idx, const float *Q, int32_t nq, int32_t k, int32_t num_probes, int32_t probe_radius,
                                int32_t take_main, int32_t take_flip, const uint32_t *allow, int32_t *out_ids, float *out_dist) {
    return lsh_filtered_host(idx, MaskForm::Single, Q, nq, k, num_probes, probe_radius, take_main, take_flip, allow, out_ids, out_dist);
}
int hnswgpu_lsh_search_filtered_each_dev(hnswgpu_index *idx, const float *d_Q, int32_t nq, int32_t k, int32_t num_probes,
                                         int32_t probe_radius, int32_t take_main, int32_t take_flip, const uint32_t *d_allow_each,
                                         int32_t *d_out_ids, float *d_out_dist, void *stream) {
    return lsh_filtered_dev(idx, MaskForm::Each, d_Q, nq, k, num_probes, probe_radius, take_main, take_flip, d_allow_each, d_out_ids,
                            d_out_dist, stream);
}
int hnswgpu_lsh_search_filtered_each(hnswgpu_index *idx, const float *Q, int32_t nq, int32_t k, int32_t num_probes, int32_t probe_radius,
                                     int32_t take_main, int32_t take_flip, const uint32_t *allow_each, int32_t *out_ids, float *out_dist) {
    return lsh_filtered_host(idx, MaskForm::Each, Q, nq, k, num_probes, probe_radius, take_main, take_flip, allow_each, out_ids, out_dist);
}

}  // extern "C"
