// engine.hpp -- host-side state of one index handle + helpers shared by the translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <string>
#include <string>
#include <utility>
#include <vector>

#include "tuning.hpp"

#include "../../include/hnswgpu.h"
#include "kernels.hpp"
#include "tile_args.hpp"

namespace hg {

void set_error(const char *fmt, ...);
extern std::atomic<int64_t> g_launch_count[HNSWGPU_COUNT_N];  // hnswgpu_launch_count
inline void count_launch(int which) { g_launch_count[which].fetch_add(1, std::memory_order_relaxed); }

#define HG_HIP(expr)                                                                             \
    do {                                                                                         \
        hipError_t _e = (expr);                                                                  \
        if (_e != hipSuccess) {                                                                  \
            hg::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
            return _e == hipErrorOutOfMemory ? HNSWGPU_ENOMEM : HNSWGPU_EHIP;                    \
        }                                                                                        \
    } while (0)

#define HG_TRY(expr)             \
    do {                         \
        int _rc = (expr);        \
        if (_rc != 0) return _rc; \
    } while (0)

#define HG_REQUIRE(cond, code, ...)  \
    do {                             \
        if (!(cond)) {               \
            hg::set_error(__VA_ARGS__); \
            return (code);           \
        }                            \
    } while (0)

struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    int ensure(size_t bytes) {
        if (bytes <= cap) return 0;
        if (p) {
            HG_HIP(hipFree(p));
            p = nullptr;
            cap = 0;
        }
        size_t want = bytes + bytes / 4 + 256;
        HG_HIP(hipMalloc(&p, want));
        cap = want;
        return 0;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
    template <class T>
    T *as() const {
        return static_cast<T *>(p);
    }
};

// Scratch of one launch with the dense bounds table (dense_kernels.hpp): the query codes + scalars, and the table.  One per
// place a launch can be enqueued from without waiting for the launch before it: the handle's (every call inside an hg::Call
// scope -- those are ordered one behind the other, whatever their streams) and one per Slot.  Grown on demand.
struct DenseScratch {
    DevBuf codes, lb;
};

enum { PROF_IVF_SCAN = 0, PROF_HNSW = 1, PROF_ASSIGN = 2, PROF_UPDATE = 3, PROF_N = 4 };  // (PROF_UPDATE: the device chain of hnswgpu_ivf_update)

// The form of a filtered call's allow-mask (include/hnswgpu.h), W = (n + 31) / 32 words: one mask shared by the call's queries,
// or [nq][W], one per query
enum class MaskForm { Single, Each };

}  // namespace hg

struct hnswgpu_index {
    int device = 0;
    int metric = 0;
    int64_t n = 0;
    int dim = 0;
    int64_t ld = 0;  // row stride in floats (multiple of 4)
    int nch = 0;     // 256-float chunks per row (template parameter NCH)
    float *d_base = nullptr;
    float *d_norms = nullptr;
    // int8 copy of the rows + per-row (scale, error bound) for the HNSW traversal's rejection test (kernels.hpp:
    // quantize_rows_kernel); made when a graph is installed or built, null while rejection_mode is 0
    uint32_t *d_qrows = nullptr;
    float4 *d_qmeta = nullptr;
    // int8 copy of the IVF list rows (list order) in the MFMA tile layout + per-row bound terms, for the bounds pass of
    // the list scan (stream_kernels.hpp); made with the lists, null while rejection_mode is 0
    uint32_t *d_lctile = nullptr;
    float4 *d_lcmeta = nullptr;
    uint2 *d_lhalf = nullptr;    // list rows in fp16, row-major (four halves per element), + per-row (scale, E, 0, 1/|v|)
    float4 *d_lhmeta = nullptr;
    unsigned long long *d_rej_stats = nullptr;  // [2], counted by the traversal while profiling is on
    int rejection_mode = 1;  // 0 = off, 1 = batches that fill the chip (hnsw_launch_plan), 2 = every launch
    // HNSW, mode 1: the first large launch on a graph counts what the int8 test decides (f32 rows fetched / neighbours
    // evaluated, hnsw_launch_plan); where it rejects too little to pay for its own bytes -- rows whose neighbours all lie
    // within the bounds' width of the list's worst -- the later large launches evaluate every neighbour in f32.  0 = not
    // measured, 1 = measured (the counters are on their way to hnsw_cal_host), 2 = decided; reset with the graph.
    int hnsw_cal_state = 0;
    bool hnsw_rej_off = false;
    double hnsw_cal_frac = 0.0;  // f32 rows / neighbours of the measured launch
    unsigned long long *d_hnsw_cal = nullptr, *hnsw_cal_host = nullptr;  // [2] device counters, pinned host copy
    hipEvent_t ev_hnsw_cal = nullptr;
    // IVF, mode 1: the first search measures what the int8 bounds separate on THIS data (ivf_calibrate) and switches the
    // survivor stream off for the handle when they leave more than a quarter of the candidates
    bool ivf_calibrated = false, ivf_calibrating = false, ivf_stream_off = false;
    int cus = 256;
    hipStream_t stream = nullptr;
    std::mutex mu;
    // Combining of concurrent synchronous searches (hnswgpu_hnsw_search from many host threads, the reference's
    // parallel-search-futures pattern): callers queue their request; one of them -- the collector -- takes everything
    // that is queued with the same (k, ef) as ONE batch, launches it and hands the results back.  Twenty threads issuing
    // single queries then share a launch instead of queueing twenty of them one after the other.
    struct SearchReq {
        const float *Q;
        int32_t nq, k, ef;  // ef: layer-0 breadth of an HNSW request, nprobe of an IVF request
        int32_t *out_ids;
        float *out_dist;
        int64_t *stats;
        int rc = 0;
        std::string err;
        // 0 = queued, 1 = served (rc / err / outputs are final), 2 = "you collect the next batch".  Every caller sleeps on
        // ITS OWN word (futex): serving a batch of 200 wakes 200 threads one by one, none of which then fights the
        // other 199 for a shared mutex (the condition-variable broadcast of round 1 collapsed at 200 callers).
        std::atomic<uint32_t> state{0};
    };
    struct Combiner {
        std::mutex mu;
        std::vector<SearchReq *> pending;
        std::atomic<int> npending{0};  // pending.size(), readable without the lock (a lingering collector polls it)
        bool collector = false;        // a thread is forming the next batch (at most one at a time)
        int inflight = 0;              // batches launched and not yet answered
        int max_inflight = 1;          // batches that may overlap on the device (own stream + staging each)
        SearchReq *slot_waiter = nullptr;  // the collector, parked until a batch in flight completes
        // (atomics: a lingering collector reads both while a finishing batch of the other slot writes them)
        std::atomic<int> last{0};              // requests in the batch launched last
        std::atomic<double> last_run_us{0.0};  // how long that batch took from launch to results (its callers return after that)
    };
    Combiner cmb_hnsw, cmb_ivf;
    // One batch in flight of the small synchronous searches: its own stream, one block of MAPPED pinned host memory
    // that the kernels read the queries from and write the results to (no copy calls at all), and a flag in that
    // block the last workgroup sets and the host thread spins on (no interrupt, no hipStreamSynchronize).
    struct Slot {
        std::mutex mu;
        hipStream_t st = nullptr;
        void *h = nullptr;      // host address of the block
        void *d = nullptr;      // device address of the same bytes
        size_t cap = 0;
        int32_t *d_again = nullptr;    // [1 + kZcMaxQueries]: queries that ran out of ghost slots (see hnsw.hip)
        uint32_t *d_done = nullptr;    // workgroups that have finished the current launch
        int32_t *d_order = nullptr;    // [2 x kZcMaxQueries]: order and keys of an ordered launch (order_kernels.hpp)
        uint32_t seq = 0;              // value the flag takes when the current launch has finished
        hg::DenseScratch dense;        // a slot launch's own bounds table (two slot launches may be in flight)
    };
    Slot slots[2];
    void *h_pin = nullptr;    // pinned host staging of a large combined batch (queries in, results out)
    size_t h_pin_cap = 0;
    // cross-stream ordering of the shared scratch buffers: the last call's completion event
    hipEvent_t ev_last = nullptr;
    hipStream_t ev_stream = nullptr;
    bool ev_valid = false;

    // HNSW graph (device + host mirror for export)
    bool has_graph = false;
    uint64_t graph_gen = 0;  // bumped whenever the graph is replaced: a search in flight on a slot stream notices

    int M = 0, M0 = 0, entry = -1, max_level = 0;
    int build_flags = 0;  // HNSWGPU_BUILD_* the graph was built with (hnswgpu_hnsw_add inserts the same way); 0 for an installed graph
    int64_t up_blocks = 0;
    int32_t *d_levels = nullptr, *d_l0 = nullptr, *d_upadj = nullptr;
    int64_t *d_upoff = nullptr;
    std::vector<int32_t> h_levels, h_l0, h_upadj;
    std::vector<int64_t> h_upoff;
    // A FOREST (hnswgpu_set_graph_parts / hnswgpu_hnsw_build_parts): nparts > 0, the rows grouped by part -- part p is rows
    // [h_part_off[p], h_part_off[p + 1]) with a sub-graph of its own (entry row or -1 for an empty part, top level); no edge leaves
    // its part.  entry is -1 then and max_level the largest part's.  Searched by hnswgpu_hnsw_search_parts alone (hnsw.hip).
    int nparts = 0;
    int64_t max_part = 0;  // rows of the largest part: what the visited set of a forest launch is sized and placed by
    std::vector<int64_t> h_part_off;
    std::vector<int32_t> h_part_entry, h_part_level;
    int4 *d_parts = nullptr;  // [nparts] (first row, entry, top level, rows): parts_kernels.hpp
    // scratch of a forest search: the item table, the per-item result lists and counters, the host entry's probe table
    hg::DevBuf s_pt_items, s_pt_ids, s_pt_dist, s_pt_stats, s_pt_probes;

    // IVF-FLAT (device: centroids + rows re-ordered so every list is contiguous)
    int nlist = 0;
    int64_t max_list_len = 0;
    int64_t min_list_len = 0;  // (of this handle's lists; a shard: of the lists it holds -- the wave-per-query routing tail needs k rows in every list)
    float *d_cent = nullptr, *d_cnorms = nullptr, *d_lrows = nullptr, *d_lnorms = nullptr;
    int64_t *d_listoff = nullptr;
    int32_t *d_listids = nullptr;
    // a SHARD of a larger IVF index (hnswgpu_set_ivf_shard): prefix sums of the list lengths of the WHOLE index, so
    // that every shard numbers its candidates as the unsharded search would; nullptr on an ordinary index
    int64_t *d_glistoff = nullptr;
    // rows of the WHOLE index the lists belong to (= n on an ordinary index; the sum of the global list lengths on a shard):
    // everything that chooses a kernel path or sizes a sample by the MEAN LIST LENGTH uses this, so that a shard decides
    // what the unsharded index decides (a shard holds n / ndev rows over the same nlist)
    int64_t ivf_n_global = 0;
    bool lrows_alias = false;  // lists are the base rows in place (list_ids = 0..n-1): d_lrows / d_lnorms alias d_base / d_norms
    std::vector<float> h_cent;
    std::vector<int64_t> h_listoff, h_glistlen;
    std::vector<int32_t> h_listids;

    // Hybrid LSH (lsh.hip, lsh_kernels.hpp): lsh_tables sign-projection hash tables of lsh_bits bits over the base rows, or none
    // (lsh_tables == 0).  Planes [tables * bits][ld] zero padded, codes [n][tables], and per table the buckets as
    // off[2^bits + 1] into ids[n] (rows ascending inside a bucket); the caller's planes [tables][bits][dim] for export.
    int lsh_tables = 0, lsh_bits = 0;
    float *d_lsh_planes = nullptr;
    uint16_t *d_lsh_codes = nullptr;
    int64_t *d_lsh_off = nullptr;
    int32_t *d_lsh_ids = nullptr;
    std::vector<float> h_lsh_planes;

    // scratch (grown on demand, reused across calls; calls are serialised by `mu`)
    hg::DevBuf s_q, s_partial, s_ord, s_dist, s_pairs, s_ids, s_outd, s_probes, s_stats, s_misc, s_misc2, s_vis, s_qp, s_qn, s_tile, s_grp, s_done, s_pf, s_solo, s_bk, s_heavy, s_home, s_dh, s_hord;
    // s_hord: order[nq] | keys[nq] of an ordered HNSW launch (order_kernels.hpp); the last such launch's, for hnswgpu_hnsw_last_order
    const int32_t *hnsw_order_last = nullptr;
    int32_t hnsw_order_nq = 0;
    // The dense bounds table in front of large wave-kernel launches (hnswgpu_set_hnsw_dense_bounds; hnsw_launch_plan holds the
    // rule): mode 1 = the rule, 0 = never, 2 = every eligible launch; the table of one launch stays within dense_budget bytes.
    int dense_mode = 1;
    size_t dense_budget = static_cast<size_t>(2) << 30;
    int64_t dense_launches = 0;  // launches that used the table
    int dense_rows_mode = 0;     // hnswgpu_hnsw_dense_rows: f32 rows in flight of such launches on 768-float rows, 0 = the rule, 2 / 4
    int64_t dense_rows4_launches = 0;  // ... and those that kept four
    hg::DenseScratch s_dense;
    // s_bk: the per-list pair counters of the IVF survivor stream -- zero between searches (the work-list kernel clears
    // them behind its last read); bk_dirty = a search was enqueued past the point that fills them but not past the
    // work-list kernel (an error in between): the next search clears them itself
    bool bk_dirty = false;
    // filtered search (filter_kernels.hpp): the call's mask on the device, the passing row ids, the compaction's block counts
    // (+ the 8-byte total behind them), and the traversal's unfiltered result lists
    hg::DevBuf s_fmask, s_fpass, s_fblk, s_fids, s_fdist;
    // ... and for the IVF list scan: the mask in list order, the passing positions below every list's first
    hg::DevBuf s_flmask, s_ffoff;
    // ... and for one mask per query: the groups' union masks, the word per union row (who of the group allows it), the
    // selection's per-query candidate counts.  (The lists live in s_fpass, the block counts and totals in s_fblk.)
    hg::DevBuf s_feum, s_feuw, s_feqc;
    uint32_t pf_seq = 0;  // number of the last small launch, helper or several-CU kernel (hnsw.hip: hnsw_number_launch is its one owner)
    size_t s_done_n = 0;  // counters per half of s_done (scan tails | route tails)
    uint32_t vis_gen = 0;  // last generation number handed to an HBM visited slab

    // profiling
    bool prof = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> prof_ev[hg::PROF_N];
    double prof_ms[hg::PROF_N] = {0, 0, 0, 0};
    int64_t prof_cnt[hg::PROF_N] = {0, 0, 0, 0};
};

namespace hg {

inline int64_t ivf_mean_len(const hnswgpu_index *idx) {
    return std::max<int64_t>(1, (idx->ivf_n_global > 0 ? idx->ivf_n_global : idx->n) / std::max(idx->nlist, 1));
}

int pick_nch(int64_t ld);  // 0 if unsupported
// hipFuncSetAttribute is per device: true the first time a call site asks on the current device
bool attr_needed(bool (&done)[64]);

// launch wrappers (engine.hip / hnsw.hip)
// CALL(NCH, RB, L2) for the row-loader width `nch` (pick_nch) -- every kernel template's dispatch
#define HG_DISPATCH(nch, l2, CALL)                                        \
    do {                                                                  \
        if (l2) {                                                         \
            switch (nch) {                                                \
                case 1: CALL(1, 8, true); break;                          \
                case 2: CALL(2, 8, true); break;                          \
                case 3: CALL(3, 8, true); break;                          \
                case 4: CALL(4, 4, true); break;                          \
                case 6: CALL(6, 4, true); break;                          \
                case 8: CALL(8, 2, true); break;                          \
                case 12: CALL(12, 2, true); break;                        \
                default: set_error("unsupported row length"); return HNSWGPU_ELIMIT; \
            }                                                             \
        } else {                                                          \
            switch (nch) {                                                \
                case 1: CALL(1, 8, false); break;                         \
                case 2: CALL(2, 8, false); break;                         \
                case 3: CALL(3, 8, false); break;                         \
                case 4: CALL(4, 4, false); break;                         \
                case 6: CALL(6, 4, false); break;                         \
                case 8: CALL(8, 2, false); break;                         \
                case 12: CALL(12, 2, false); break;                       \
                default: set_error("unsupported row length"); return HNSWGPU_ELIMIT; \
            }                                                             \
        }                                                                 \
    } while (0)

// Everything one HNSW traversal launch decides, computed once before anything is allocated, numbered, synchronised or enqueued
// (hnsw.hip: hnsw_launch_plan, where every rule and its measured reason live) from the handle's state, the launch's shape and ONE
// reading of the tuning table.  The stages behind it (hnsw_launch_resources, hnsw_dispatch) fill arguments from it and decide nothing.
enum class HnswKernel {
    Search,         // hnsw_search_kernel (kernels.hpp): a workgroup of nw waves per query
    SearchHelpers,  // ... with helper workgroups that evaluate ahead of it: a handful of queries, short lists
    Solo,           // hnsw_solo_kernel (solo_kernels.hpp): a handful of queries, each over several CUs
    Wave            // hnsw_wave_kernel (wave_kernels.hpp): one wave per query, main list + admission buffer
};
using HnswKernelFn = void (*)(HnswArgs);
struct HnswLaunchPlan {
    HnswKernel kernel;
    HnswKernelFn fn;      // its instantiation for (nch, metric, rejection, nw, vis_global)
    int nch;              // 256-float chunks per row
    bool rejection;       // the int8 rejection test is on
    bool calibrate;       // rejection mode 1: this launch counts what the test decides (hnswgpu_index::hnsw_cal_state 0 -> 1)
    bool vis_global;      // the visited set as generation stamps in HBM: a slab of n stamps per workgroup of `grid`,
    int64_t gens;         // `gens` generation numbers per launch;
    int32_t nwords;       // otherwise a bitset of nwords words in LDS
    int nw;               // Search: waves per query
    int grid, block;
    size_t lds;
    // SearchHelpers / Solo: helper workgroups per query, list entries looked at ahead, and the parts of one of the four regions
    // of s_pf / s_solo: [mailboxes: mail_bytes][pf_res / solo_claim: table_bytes][solo_rec: rec_bytes]
    int32_t pf_groups, pf_hints;
    bool pf_eval;         // SearchHelpers: the helpers publish distances (false: they only warm the L2)
    int32_t solo_chase, solo_log2s;
    size_t mail_bytes, table_bytes, rec_bytes, region;
    int32_t repeat_cap;   // list capacity of the repeat pass behind this launch, beside the SAME visited set (0: no repeat pass)
    bool ordered;         // Wave: the queries dealt to the XCDs in the order of their nearest pivot row (order_kernels.hpp)
    bool dense;           // Wave: the int8 bounds of the whole batch from a table computed in front of the launch (dense_kernels.hpp),
    int64_t lb_ld;        // its row stride (floats)
    int dense_rows;       // ... and the f32 rows in flight of its nch 3 instances, 2 or 4 (0: every other launch, HG_HNSW_ROWS decides)
};
// Row width -> CALL(NCH, R, RF): f32 rows in flight per wave without / with the int8 rejection test -- the one table of the three
// traversal kernels.  With the test a hop fetches f32 rows for a handful of neighbours only, half or a quarter of them in flight
// are plenty, and the kernel then holds more waves per SIMD (dim 768, one wave per query: 159 -> 99 VGPRs, five waves instead of
// three: 10,000 queries 2.24M -> 2.43M QPS, 4,096 queries 1.89M -> 2.39M, 1,024 queries 0.75 -> 0.68 ms).  Longer rows keep their
// count: at dim 1536 (HBM-resident, 1.25M rows) two rows in flight instead of four cost 7 % although a third wave fits per SIMD.
// RF3, the cell of nch 3: 2 for hnsw_search_kernel and hnsw_wave_kernel (the measurement above); hnsw_solo_kernel, whose third
// argument is the rows in flight of a HELPER wave (it never runs the test), takes 4 there -- kept as found, the history names no
// measurement for it, and each cell is an instantiation, hence a register count.
#define HG_HNSW_ROWS(nch, RF3, CALL)       \
    switch (nch) {                         \
        case 1: CALL(1, 8, 4);             \
        case 2: CALL(2, 8, 4);             \
        case 3: CALL(3, 8, RF3);           \
        case 4: CALL(4, 4, 4);             \
        case 6: CALL(6, 4, 4);             \
        case 8: CALL(8, 2, 2);             \
        case 12: CALL(12, 2, 2);           \
        default: return nullptr;           \
    }
// CALL for a kernel family F<NCH, rows in flight, L2>(plan) that runs the test: returns its instance for (p.rejection, l2)
#define HG_HNSW_ROWS_IN_FLIGHT(F, N, R, RF) \
    return p.rejection ? (l2 ? F<N, RF, true>(p) : F<N, RF, false>(p)) : (l2 ? F<N, R, true>(p) : F<N, R, false>(p))
// the instantiation a plan names, or null for an unsupported row length (solo.hip / wave.hip: the three kernel families are
// translation units of their own so that they compile side by side)
HnswKernelFn hnsw_solo_kernel_for(const HnswLaunchPlan &p, const HnswArgs &a);
HnswKernelFn hnsw_wave_kernel_for(const HnswLaunchPlan &p, const HnswArgs &a);
HnswKernelFn hnsw_parts_kernel_for(const HnswLaunchPlan &p, const HnswArgs &a);  // parts.hip: either family with the item table
// dense.hip: the wave kernel's instantiations that read the bounds table; the table's row stride for n rows; the bytes of a
// batch's query codes (its QueryScal block follows them); query codes + table, two launches
HnswKernelFn hnsw_wave_dense_kernel_for(const HnswLaunchPlan &p, const HnswArgs &a);
int64_t hnsw_dense_ld(int64_t n);
size_t hnsw_dense_code_bytes(int nch, int32_t nq);
int launch_hnsw_dense(const hnswgpu_index *idx, const float *d_Q, int64_t qld, int32_t nq, void *codes, float *lb, int64_t lb_ld,
                      hipStream_t st);
struct OrderArgs;
int launch_hnsw_order(int nch, const OrderArgs &a, hipStream_t st);  // wave.hip: key pass + counting sort
int launch_norms(int nch, const float *rows, int64_t ld, int64_t n, float *out, hipStream_t st);
int ensure_qrows(hnswgpu_index *idx, hipStream_t st);
// int8 codes + per-row bound terms of `n` rows into freshly allocated *crows / *cmeta (the caller owns them)
int quantize_rows(hnswgpu_index *idx, const float *rows, int64_t n, uint32_t **crows, float4 **cmeta, hipStream_t st);
int ensure_list_codes(hnswgpu_index *idx, hipStream_t st);
int ensure_list_half(hnswgpu_index *idx, hipStream_t st);
int launch_scan(int nch, const ScanArgs &a, hipStream_t st);
int launch_merge(const MergeArgs &a, hipStream_t st);
// Serve `me` through combiner `c`: queue it, lead one batch at a time while it is not done.  `take(first, r, total)`
// says whether request r may join a batch that starts with `first` and already holds `total` queries; `run` launches
// a batch and returns its error code.
constexpr int kZcMaxQueries = 256;  // largest combined batch served through a Slot (one workgroup per query and CU)
// stream, counters, mapped block of at least `bytes` (sets the device only where it has to allocate)
int slot_prepare(hnswgpu_index::Slot &s, size_t bytes, int device);
// Spin on the completion flag of a slot launch (value `seq`); falls back to hipStreamSynchronize if it does not show.
int slot_wait(hnswgpu_index::Slot &s, volatile uint32_t *flag, uint32_t seq);
int combine_search(hnswgpu_index::Combiner &c, hnswgpu_index::SearchReq &me,
                   const std::function<bool(const hnswgpu_index::SearchReq *, const hnswgpu_index::SearchReq *, int64_t)> &take,
                   const std::function<int(const std::vector<hnswgpu_index::SearchReq *> &, int32_t)> &run);
// pinned staging block of a combined batch (grown on demand)
int ensure_pinned(hnswgpu_index *idx, size_t bytes);
int scan_dense_topk(hnswgpu_index *idx, ScanArgs a, int32_t nq, int64_t nrows, hipStream_t st);
// Everything one IVF search decides, computed once before its first launch (ivf.hip: ivf_search_plan, where every rule and its
// measured reason live) from the handle's state, the call's shape (whether a host flag is wanted among it) and ONE reading of the
// tuning table.  The stages of ivf_search_enqueue and launch_ivf_route fill their arguments from it and decide nothing themselves.
enum class IvfScan {
    Tile,    // MFMA tile scan (cosine / dot: the k-ordered summation; Euclidean: l2_group_kernel)
    Group,   // register-row group kernel: the GEMV order, a list fetched once per group of queries
    Stream,  // survivor stream: int8 bounds -> survivors -> f32 distances in the GEMV order
    Fused,   // one GEMV per pair, merge / decode / copy in the scan's last workgroups
    Gemv     // one GEMV per pair, merge and decode launches behind it
};
enum class IvfRoute {
    Given,      // the caller's lists
    OneLaunch,  // ivf_route_kernel: distances, choice, probe table (and the stream's query set-up) in one launch
    DistTail,   // a distance pass that shares centroid rows among queries, then the tail as a launch of its own
    TileTopk,   // the centroid table through the tile kernel
    GroupTopk,  // ... through the register-row group kernel (GEMV order)
    Dense,      // dense [nq][nlist] distances + select
    Scan        // partial lists + merge
};
struct IvfSearchPlan {
    int32_t nq, k, nprobe;  // nprobe: clamped to the number of lists unless the caller chose them
    int64_t npairs;         // nq * nprobe
    int64_t cand_stride;    // candidates per query, upper bound (a multiple of 4)
    IvfScan scan;
    bool list_order;        // Fused / Gemv: the pairs in list order (pair_order_kernel), in runs of order_run
    int32_t order_run;
    int64_t tile_wgs, tile_ptiles;  // Tile / Group: workgroups the items are sized for; tiles per item of the persistent kernel (0: an item per workgroup)
    IvfRoute route;
    bool query_prep;        // Stream behind a routing without the stream's set-up: ivf_query_prep_kernel
    int32_t seed_rows;      // OneLaunch / DistTail / query_prep: rows of the nearest list the first threshold is taken from ...
    bool seed_half;         // ... in half precision
    size_t route_lds;       // OneLaunch / DistTail: the tail's selection lists
    bool route_tail_wave;   // DistTail: the tail with a wave per query (+ ivf_bucket_fill_kernel)
    bool route_mfma;        // DistTail: the distances on the f32 matrix cores, route_mfma_slices (0: automatic) slices per query group;
    int64_t route_mfma_slices, route_wgs;  // otherwise on the VALU, cut for route_wgs workgroups
    // Stream only, in the order of its stages
    bool grouped;           // the pairs filed by list (buckets of bk_cap members), a work list of up to wbound items
    bool ordered;           // the queries served in the order of their nearest list
    bool folded;            // the work list by extra workgroups of the routing tail's launch
    bool home;              // the home-list pass (implies grouped and ordered): items of home_chunk rows, up to home_bound of them
    bool mid;               // the half-precision pass
    bool heavy;             // the heavy list (queries one workgroup cannot serve)
    bool narrow;            // the bounds pass: the lane = row epilogue;
    int qblocks;            // 32-query column blocks per group;
    int64_t chunk_rows;     // rows per work item (whole tiles);
    int32_t nchunks;        // items per list at most
    int64_t wbound;
    int32_t bk_cap;
    int64_t surv_cap;       // survivors per query that fit
    int64_t home_chunk, home_bound, home_stride, home_strays;  // home_stride: floats per query of the home list's bounds
    bool home_select_wave;  // a wave per query selects the home list's survivors
    uint32_t heavy_times_mean, heavy_thr;
    int32_t mid_slices_auto;  // workgroups per query of the half-precision pass by the rule (what `heavy` goes by) ...
    int32_t mid_slices;       // ... and as launched (HNSWGPU_TUNE_MID_SLICES overrides)
    int32_t mid_compact;      // entries up to which the pass compacts a survivor list (0: it does not)
    int32_t finish_slices, finish_span, finish_adapt, finish_bisect, finish_direct;
    int64_t finish_pstride;   // keys per query handed to its last workgroup
    bool flag_in_finish;      // a flagged synchronous call: the finish kernel's last workgroup tells the caller
};
// The flag word a small synchronous IVF call spins on (ivf.hip: ivf_search_batch_slot): its device address and the value it takes.
// taken: the search went through the finish kernel, whose last workgroup sets it; otherwise a one-thread launch behind the search does.
struct IvfHostFlag {
    uint32_t *flag;
    uint32_t val;
    bool taken;
};
// the survivor stream's buffers that the routing step prepares (stream_kernels.hpp), or null
struct RouteStream {
    uint32_t *qcodes;
    QueryScal *qscal;
    uint32_t *tau, *surv_cnt;
    uint32_t *bk_cnt;  // per-list buckets of (query, list) pairs, or null (ungrouped bounds pass)
    uint2 *bk_mem;
    const struct WorklistArgs *wl;  // the plan's `folded`: the bounds pass's work list by extra workgroups of the tail's launch (filed: set by the launch)
};
// small IVF batches: routing in one launch (IvfRoute::OneLaunch); larger stream batches: distance pass + tail (DistTail)
int launch_ivf_route(hnswgpu_index *idx, const IvfSearchPlan &p, const float *d_Q, Pair *pairs, int32_t *probes, int32_t *qcnt,
                     hipStream_t st, const RouteStream *rs);
// the survivor stream of the IVF list scan (stream_kernels.hpp)
struct StreamArgs;
struct FinishArgs;
struct PrepArgs;
int launch_query_prep(const PrepArgs &a, int nch, hipStream_t st);
// narrow: the epilogue for few queries per probed list (lane = row); otherwise lane = query
struct MidArgs;
struct HeavyArgs;
struct HomeArgs;
int launch_mid(const MidArgs &a, int nch, hipStream_t st);
int launch_heavy(const HeavyArgs &a, hipStream_t st);
int launch_home(const HomeArgs &a, int64_t blocks, int nch, hipStream_t st);
int launch_stream_bounds(const StreamArgs &a, int64_t blocks, int nch, bool narrow, hipStream_t st, int qblocks = 1);
int launch_finish(const FinishArgs &a, int nch, hipStream_t st);
// zero-initialised per-query counters of the fused tails (s_done: [n] scan / finish tails | [n] route tails)
int ensure_counters(hnswgpu_index *idx, size_t n, hipStream_t st);
int scan_fused(hnswgpu_index *idx, ScanArgs a, int32_t nq, int32_t pairs_per_query, int64_t max_rows, int64_t mean_rows,
               hipStream_t st, int prof_slot);
extern unsigned long long *g_tile_dbg_buf;
#ifdef HG_DIAG
extern int g_stream_dbg, g_tile_dbg;
#endif
int launch_gather(int nch, GatherArgs a, int32_t nq, hipStream_t st);
int scan_rows_per_iter(int nch);  // kNWave * RB

// pick chunking for a scan: returns nchunks, sets chunk_rows
int plan_chunks(int nch, int64_t max_rows, int64_t mean_rows, int64_t npairs, int32_t *chunk_rows,
                bool list_pairs = false);

// scan + merge: per-query ascending top-k of (ord, dist) into s_ord / s_dist ([nq][k])
int scan_topk(hnswgpu_index *idx, ScanArgs a, int32_t nq, int32_t pairs_per_query, int64_t max_rows,
              hipStream_t st, int prof_slot, int64_t mean_rows = 0);

void prof_begin(hnswgpu_index *idx, int slot, hipStream_t st, hipEvent_t *e0);
void prof_end(hnswgpu_index *idx, int slot, hipStream_t st, hipEvent_t e0);

int upload_queries(hnswgpu_index *idx, const float *Q, int32_t nq, hipStream_t st);

// --- tiled (MFMA) scan path -------------------------------------------------------------------------
bool tile_path_ok(const hnswgpu_index *idx);  // metric != L2 and dim fits the LDS-resident query group
int tile_mode();                               // HNSWGPU_TUNE_TILE: -1 auto, 0 never, 1 whenever possible
int launch_tile(const TileArgs &a, int64_t ngroups_bound, int dim, hipStream_t st);
int launch_select(const SelectArgs &a, hipStream_t st);
// queries (nq x dim, row stride qld) -> s_qp (nq x ld, zero padded) + s_qn (device-order norms)
int pad_queries(hnswgpu_index *idx, const float *d_Q, int64_t qld, int32_t nq, hipStream_t st);
// every query against rows [0, nrows): per-query ascending top-k into s_ord / s_dist
int tile_topk_all(hnswgpu_index *idx, const float *Qp, const float *q_norms, int32_t nq, const float *rows,
                  const float *row_norms, int64_t nrows, int32_t k, hipStream_t st, int prof_slot, bool gemv_order = false);

// One call on a handle: the owner of idx->mu, the current device and the ordering of the handle's shared scratch buffers across
// streams.  open() takes the lock, sets the device and makes `st` wait for the event of the call before (ev_last) when that one ran
// on another stream.  However the scope is left -- close() on the success path, the destructor behind an early error return --
// ev_last / ev_stream / ev_valid describe everything the call may have enqueued on `st`: an event recorded behind it, or, once
// sync() has waited for `st` behind the call's last enqueue, nothing (`st` had waited for the event before: no work of this handle
// is in flight).  The scope may be narrower than its function and may be opened on a slot stream (ivf.hip: ivf_search_batch_slot).
// hnsw_search_batch_slot alone takes no part: it enqueues under a plain lock of idx->mu, works in its slot's own memory and in
// tagged regions of s_pf / s_solo (hnsw.hip: hnsw_number_launch), and is waited for by quiesce().
class Call {
public:
    Call() = default;
    Call(const Call &) = delete;
    Call &operator=(const Call &) = delete;
    ~Call() {
        if (idx_) (void)leave();  // an early return: raw HIP calls, the thread's error message stays the caller's
    }
    int open(hnswgpu_index *idx, hipStream_t st);
    // Before device memory that searches read is freed (graph, lists): wait for `st` AND for the two slot streams -- the small
    // synchronous HNSW searches launch on those outside the event ordering and release idx->mu before their kernel has finished.
    int quiesce();
    int sync();   // hipStreamSynchronize(st), behind the call's last enqueue
    int close();  // reports a failing hipEventRecord; the lock is held to the end of the scope
    // Host staging of a search through s_q / s_ids / s_outd: the queries up and room for nq * k results; the enqueue goes between
    // the two; then ids and distances down and sync()
    int stage_in(const float *Q, int32_t nq, int32_t k);
    int stage_out(int32_t *out_ids, float *out_dist, int64_t cnt);
    // ... and of a filtered one: the caller's mask words (W, or nq * W: one mask per query) up into s_fmask
    int stage_mask(const uint32_t *allow, MaskForm form, int32_t nq);
private:
    hipError_t leave();
    hnswgpu_index *idx_ = nullptr;
    hipStream_t st_ = nullptr;
    bool idle_ = false;
    std::unique_lock<std::mutex> lk_;
};

void fill_empty(int32_t *ids, float *dist, int64_t cnt);  // no rows: id -1 at distance +inf

// --- filtered search (filter_kernels.hpp; the allow-mask: include/hnswgpu.h) ---------------------------------------------
int64_t mask_popcount(const uint32_t *allow, int64_t n);  // passing rows among the first n bits, on the host
// the first k passing entries of every query's list ids_in / dist_in [nq][kk] (-1 padded), -1 / +inf padded (filter_take_kernel);
// allow_stride: words between the masks of two queries, 0 = one mask shared by all
int launch_filter_take(const int32_t *ids_in, const float *dist_in, int32_t nq, int32_t kk, int32_t k, const uint32_t *d_allow,
                       int64_t n, int32_t *d_out_ids, float *d_out_dist, hipStream_t st, int64_t allow_stride);

// The set bits of a `len`-bit device mask as an ascending list in s_fpass (engine.hip).  p_host: the caller's count, or
constexpr int64_t kMaskCountRead = -1;    // ... read the total back once (the calling thread waits for `st`)
constexpr int64_t kMaskCountDevice = -2;  // ... no readback: the list holds `len` entries, the total stays at *d_total
int mask_compact(hnswgpu_index *idx, const uint32_t *d_allow, int64_t len, int64_t p_host, int64_t *p, hipStream_t st,
                 const unsigned long long **d_total = nullptr);
int fill_empty_dev(int32_t *d_ids, float *d_dist, int64_t cnt, hipStream_t st);
// IVF-FLAT filtered search (filter_kernels.hpp; driven by ivf.hip: ivf_filtered_chain)
int launch_list_mask(hnswgpu_index *idx, const uint32_t *d_allow, uint32_t *d_lmask, hipStream_t st);
int launch_list_foff(hnswgpu_index *idx, const int32_t *d_pass_pos, const unsigned long long *d_total, int64_t cap, int32_t *d_foff,
                     hipStream_t st);
int launch_ivf_filtered_scan(int nch, const IvfFilteredArgs &a, hipStream_t st);
// ... with one mask per query
int launch_ivf_each_scan(int nch, const IvfEachArgs &a, hipStream_t st);

// The block of host memory of one combined batch -- a Slot's mapped block and the pinned staging block alike:
// [64-byte header: flag word, repeat count][queries][stats, 2 x int64 per query, or absent][ids][distances], every section on a
// 64-byte boundary.  The accessors take the block's host or device address.
struct BatchBlock {
    int32_t k, dim;
    size_t o_q, o_s, o_i, o_d, bytes;  // o_s == 0: no stats
    BatchBlock(int32_t dim, int32_t total, int32_t k, bool stats);
    uint32_t *flag(void *b) const { return static_cast<uint32_t *>(b); }
    int32_t *again(void *b) const { return static_cast<int32_t *>(b) + 1; }
    float *queries(void *b) const { return reinterpret_cast<float *>(static_cast<char *>(b) + o_q); }
    int64_t *stats(void *b) const { return o_s ? reinterpret_cast<int64_t *>(static_cast<char *>(b) + o_s) : nullptr; }
    int32_t *ids(void *b) const { return reinterpret_cast<int32_t *>(static_cast<char *>(b) + o_i); }
    float *dist(void *b) const { return reinterpret_cast<float *>(static_cast<char *>(b) + o_d); }
    void pack(void *host, const std::vector<hnswgpu_index::SearchReq *> &batch) const;     // the callers' queries, one behind the other
    void scatter(void *host, const std::vector<hnswgpu_index::SearchReq *> &batch) const;  // ids, distances and stats back to each caller
    // a free Slot and its lock (both busy: more callers than the combiner's batches in flight -- cannot happen, but wait for the first)
    static hnswgpu_index::Slot *acquire_slot(hnswgpu_index *idx, std::unique_lock<std::mutex> &lk);
};

}  // namespace hg
