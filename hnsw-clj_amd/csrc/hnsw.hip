// hnsw.hip -- HNSW graph import/export, batched GPU search and batched GPU-assisted build.
// Reference: src/hnsw/ultra_fast.clj (file:line cited per function).
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

#include "build_kernels.hpp"
#include "engine.hpp"
#include "hnsw_remove_kernels.hpp"  // the graph side of hnswgpu_hnsw_remove
#include "hnsw_update_kernels.hpp"  // the unlink of hnswgpu_hnsw_update: the same repair, nothing renumbered
#include "ivf_update_ids.hpp"       // the id check every update shares
#include "lsh_remove_ids.hpp"       // the id check every removal shares
#include "javarandom.hpp"
#include "order_kernels.hpp"  // OrderArgs, for hnsw_launch_resources
#include "parts_kernels.hpp"  // the item table and the counters of a forest launch (hnsw_parts_enqueue)
#include "solo_kernels.hpp"  // solo_lds_bytes and the sizes of the several-CU kernel's mailboxes, for hnsw_launch_plan

namespace hg {

constexpr size_t kMaxLds = 160 * 1024;  // the LDS of a CU

// The dynamic LDS of the three traversal kernels (solo_lds_bytes: solo_kernels.hpp, beside the layout it sizes)
static size_t hnsw_lds_bytes(int cap, int nwords, int nw) {
    // kernels.hpp: hnsw_search_kernel's layout -- ONE list of 8-byte entries + a 16-bit merged position per slot
    return sizeof(uint2) * cap + sizeof(int32_t) * 3 * kMaxDeg + sizeof(int32_t) * 16 + sizeof(int32_t) * nw * kWave +
           sizeof(uint2) * kPfRing + sizeof(uint32_t) * nwords + sizeof(uint16_t) * cap + 16;
}

static size_t wave_lds_bytes(int cap, int nwords) {
    // wave_kernels.hpp: hnsw_wave_kernel's layout -- the main list, the buffer's image, the expansion's candidates, the visited set
    return sizeof(uint2) * cap + sizeof(uint2) * kWave + 2 * sizeof(int32_t) * kMaxDeg + sizeof(uint32_t) * nwords + 16;
}

// Visited-set placement: an LDS bitset while it leaves room for several workgroups per CU, otherwise
// generation stamps in HBM (4 B per row per resident workgroup; 288 GB makes that cheap).
constexpr int64_t kLdsVisitedMaxRows = 262144;  // 32 KiB bitset
// (the several-CU kernel serves launches with the LDS bitset only, and its tags keep 18 bits of a node: solo_kernels.hpp, solo_tag)
static_assert(kLdsVisitedMaxRows <= (1 << 18), "solo_tag holds 18 bits of a node id");
// The one predicate of hnsw_launch_plan and of the call combiner (hnsw_search_batch); vis_global_env: HNSWGPU_TUNE_VIS_GLOBAL, the
// testing override (the HBM stamps at every size)
static bool hnsw_vis_global(int64_t n, int64_t vis_global_env) { return vis_global_env != 0 || n > kLdsVisitedMaxRows; }

constexpr int kPfMaxQueries = 128;  // up to half a CU count of queries: every traversal and at least one helper per query get a CU
static_assert(kPfMaxQueries == kSoloMaxQueries, "one bound for both kinds of small launch");
constexpr int kSoloMinEf = 96;      // (hnsw_launch_plan: the several-CU kernel by default from this ef -- 96, not 200)
constexpr int kOrderMinQueries = 10000;  // (hnsw_launch_plan: the wave kernel's queries in the order of their nearest pivot from this batch size)

// Stage 1 of a launch.  Rejection mode 1 MEASURES (once per graph, on its first large launch: HnswLaunchPlan::calibrate): the
// counters travel to pinned host memory behind an event, and the first launch that finds the event complete turns them into the
// verdict hnsw_launch_plan reads as plain state.  Nothing here blocks.
static void hnsw_calibration_absorb(hnswgpu_index *idx) {
    if (idx->hnsw_cal_state != 1 || !idx->ev_hnsw_cal || hipEventQuery(idx->ev_hnsw_cal) != hipSuccess) return;
    const double f32_rows = static_cast<double>(idx->hnsw_cal_host[0]), nb = static_cast<double>(idx->hnsw_cal_host[1]);
    idx->hnsw_cal_frac = nb > 0 ? f32_rows / nb : 0.0;
    const double keep = static_cast<double>(tune(HNSWGPU_TUNE_HNSW_CALIBRATE_PCT, 65)) / 100.0;
    idx->hnsw_rej_off = nb > 0 && idx->hnsw_cal_frac > keep;  // the test leaves more than that of the rows to fetch
    idx->hnsw_cal_state = 2;
}

// The instantiation of hnsw_search_kernel a plan names (wave.hip and solo.hip hold the other two families' tables: the three
// compile side by side)
template <int N, int R, bool L>
static HnswKernelFn search_kernel(const HnswLaunchPlan &p) {
    if (p.kernel == HnswKernel::SearchHelpers) return &hnsw_search_kernel<N, R, L, 4, false, true>;
    if (p.vis_global) return p.nw == 1 ? &hnsw_search_kernel<N, R, L, 1, true> : (p.nw == 2 ? &hnsw_search_kernel<N, R, L, 2, true> : &hnsw_search_kernel<N, R, L, 4, true>);
    return p.nw == 1 ? &hnsw_search_kernel<N, R, L, 1, false> : (p.nw == 2 ? &hnsw_search_kernel<N, R, L, 2, false> : &hnsw_search_kernel<N, R, L, 4, false>);
}

static HnswKernelFn hnsw_search_kernel_for(const HnswLaunchPlan &p, const HnswArgs &a) {
    const bool l2 = a.metric == METRIC_L2;
#define PICK(N, R, RF) HG_HNSW_ROWS_IN_FLIGHT(search_kernel, N, R, RF)
    HG_HNSW_ROWS(p.nch, 2, PICK);
#undef PICK
}

// Stage 2: everything ONE launch decides (HnswLaunchPlan, engine.hpp) -- a pure function of the handle's state, of the launch's
// shape (a: nq, ef, cap, n, M0, max_level, metric; build mode = q_rows, repeat pass = q_index) and of one reading of the tuning
// table: every key at most once, every rule evaluated once, here.  The table is process-wide and another thread may change it
// while a search is being enqueued: a repeat pass is planned from its first pass's plan (`first`) and reads no key at all, so that
// its list is sized for the visited set it then runs with.  Nothing is allocated, numbered, synchronised or enqueued before this
// has returned 0: the limits a launch can exceed are found here.
// plain_search: the first pass of an unfiltered search call (search_enqueue) -- the launches the dense bounds table may serve.
static int hnsw_launch_plan(const hnswgpu_index *idx, const HnswArgs &a, const HnswLaunchPlan *first, HnswLaunchPlan &p,
                            bool plain_search = false) {
    memset(&p, 0, sizeof(p));
    const bool build = a.q_rows != nullptr, repeat = a.q_index != nullptr;
    // A forest launch (HnswArgs::items: a.nq counts items, a.nwords covers the largest part): a traversal never leaves its part,
    // so the visited set is placed and sized by the LARGEST PART -- a 1M-row index of 24 parts keeps the LDS bitset its 24 handles
    // had.  Such launches stay on hnsw_search_kernel and hnsw_wave_kernel, the two that read the item table: no helpers, no
    // several-CU kernel, no ordered dealing (the pivot keys are per query, the slots per item).
    const bool parts = a.items != nullptr;
    const int64_t vis_rows = parts ? idx->max_part : a.n;
    p.nch = idx->nch;
    // The rejection test on int8 rows (kernels.hpp: quantize_rows_kernel) turns one memory round trip per hop into two
    // shorter ones: 2.2x the throughput once the chip is bandwidth-bound, ~5 % slower while a launch is latency-bound.
    // 31k x 768, ef 100, ms per launch without / with: 256 queries 0.537 / 0.571, 512: 0.607 / 0.590, 768: 0.817 /
    // 0.611, 1024: 1.05 / 0.74, 10000: 9.9 / 4.4 (tools/hnsw_batch_sweep.py) -- on from two queries per CU.
    p.rejection = a.qrows && (idx->rejection_mode == 2 || (idx->rejection_mode == 1 && a.nq >= 2 * idx->cus && idx->dim >= 128));
    // Mode 1 also MEASURES (once per graph, on its first large launch): the int8 stage pays while it keeps enough f32 rows
    // from being fetched -- 31k x 768 clustered, ef 640: half of them; 1.25M x 1536 clustered, ef 256: a tenth, and the
    // launch then requests 1.15x the bytes of the plain traversal (profiles/r04_config5_hnsw_shard.txt).  Results never
    // depend on it.  (A launch that counts for the profile does not measure: the kernel has one pair of counters.)
    if (p.rejection && idx->rejection_mode == 1 && !build && !repeat && tune(HNSWGPU_TUNE_HNSW_CALIBRATE, 1) != 0) {
        if (idx->hnsw_cal_state == 2 && idx->hnsw_rej_off) p.rejection = false;
        p.calibrate = idx->hnsw_cal_state == 0 && !(idx->prof && idx->d_rej_stats);
    }
    if (repeat) {  // repeat pass: few (usually no) work items, one large-list workgroup per CU at most
        p.kernel = HnswKernel::Search;
        p.vis_global = first->vis_global;
        p.nw = 4;
        p.grid = std::min(a.nq, 256);
    } else {
        // tuning override (HNSWGPU_TUNE_HNSW_NW = 1 | 2 | 4); 0 = choose by batch size
        const int64_t nw_raw = tune(HNSWGPU_TUNE_HNSW_NW, 0);
        const int nw_env = (nw_raw == 1 || nw_raw == 2 || nw_raw == 4) ? static_cast<int>(nw_raw) : 0;
        p.vis_global = hnsw_vis_global(vis_rows, tune(HNSWGPU_TUNE_VIS_GLOBAL, 0));
        // helper workgroups per query that prefetch neighbour rows into the query's XCD L2 (kernels.hpp, HnswArgs::pf_mail):
        // HNSWGPU_TUNE_PREFETCH = <G> overrides (0 = off, and the several-CU path with it).  ONE key, two intended defaults and
        // clamps: 4 (at most 16) helpers for the round-2 helper kernel, 8 (at most 31) for the several-CU kernel.
        const int64_t pf_env = tune(HNSWGPU_TUNE_PREFETCH, kTuneUnset);
        const int helper_groups = pf_env == kTuneUnset ? 4 : static_cast<int>(std::max<int64_t>(0, std::min<int64_t>(16, pf_env)));
        const int solo_groups = pf_env == kTuneUnset ? 8 : static_cast<int>(std::max<int64_t>(0, std::min<int64_t>(31, pf_env)));
        const bool small = helper_groups > 0 && !p.vis_global && !build && !parts && a.nq <= kPfMaxQueries && nw_env == 0 &&
                           a.n < (1LL << 31) && a.M0 <= kMaxDeg;
        // HNSWGPU_TUNE_SOLO: 1 (default) = launches whose list is long enough for the split to pay (ef >= kSoloMinEf = 96: a search of
        // a few dozen expansions is a descent whose every step waits for the step before it, and the round-2 helpers serve it as well --
        // 31k x 768 clustered, one query, round-2 helpers / this kernel: ef 50 249 / 255 us, ef 100 378 / 350, ef 200 612 / 524, ef 640
        // 1,900 / 1,210), 2 = every small launch, 0 = never
        const int64_t solo_mode = tune(HNSWGPU_TUNE_SOLO, 1);
        const bool solo = small && solo_groups > 0 && (solo_mode >= 2 || (solo_mode == 1 && a.ef >= kSoloMinEf));
        const int64_t hints_env = tune(HNSWGPU_TUNE_PF_HINTS, kTuneUnset);
        const auto hints = [hints_env](int dflt) {
            return static_cast<int32_t>(std::max<int64_t>(1, std::min<int64_t>(32, hints_env == kTuneUnset ? dflt : hints_env)));
        };
        // waves per query.  Measured on 31k x 768, ef 128 (tools/tune_hnsw.py): a query takes 1.1 / 1.4 / 2.0 ms
        // with 4 / 2 / 1 waves, and a CU holds 3 / 6 / 12 such workgroups (VGPR-limited), so once a batch
        // exceeds one residency round fewer waves per query win: 10,000 queries run at 601k / 776k / 802k QPS.
        int nw = nw_env > 0 ? nw_env : (a.nq > 1536 ? 1 : (a.nq > 768 ? 2 : 4));
        // with the rejection test (fewer f32 rows in flight: HG_HNSW_ROWS) a CU holds 4 / 8 / 20 such workgroups up to dim 768:
        // 1,024 queries 0.60 / 0.68 / 0.96 ms with 4 / 2 / 1 waves, 2,048: 1.15 / 0.93 / 1.06, 3,072: 1.68 / 1.51 / 1.36
        if (nw_env == 0 && p.rejection && p.nch <= 3) nw = a.nq > 2048 ? 1 : (a.nq > 1024 ? 2 : 4);
        // Launches that fill the chip with one wave per query, and every launch with a long list, take the kernel whose list is a
        // main list + a register-resident admission buffer (wave_kernels.hpp: no positional merge per expansion, the next
        // candidate out of register windows; 8 bytes of LDS per list slot).  31k x 768 clustered, QPS single-workgroup kernel /
        // this one (tools/wave_sweep.py): 10,000 queries ef 50 4.55M / 4.80M, ef 640 516k / 778k, ef 1600 151k / 263k, ef 3200 51k /
        // 91k; 2,048 queries ef 640 467k / 554k; 256 queries ef 50 459k / 418k (four waves per query are the better shape for a
        // short list on a chip that is not full), ef 640 82k / 92k, ef 3200 13.9k / 22.7k.  HNSWGPU_TUNE_HNSW_WAVE = 0: never (A/B).
        const int nwords = p.vis_global ? 0 : a.nwords;
        const int64_t wave_mode = tune(HNSWGPU_TUNE_HNSW_WAVE, 1);  // 2 = every launch it can serve (tests)
        const bool wave = wave_mode != 0 && !small && nw_env == 0 && wave_lds_bytes(a.cap, nwords) <= kMaxLds && a.M0 <= kMaxDeg &&
                          (wave_mode >= 2 || nw == 1 || a.ef >= 640);
        // a long candidate list (large ef) bounds the queries a CU holds by its LDS, not by registers: fewer than ~13 waves per
        // CU cannot hide the hop's dependent round trips, so the queries that fit get more waves each (the int8 and f32 steps
        // of a hop then run side by side).  31k x 768 clustered, 10,000 queries, QPS with 1 / 2 / 4 waves: ef 400 729k / 784k /
        // 513k, ef 800 250k / 343k / 258k, ef 1600 60k / 89k / 116k, ef 3200 10.8k / 17.7k / 25.6k (tools/large_ef_nw.py).
        if (nw_env == 0 && !wave)
            while (nw < 4 && static_cast<int64_t>(kMaxLds / hnsw_lds_bytes(a.cap, nwords, nw)) * nw < 13) nw *= 2;
        p.grid = a.nq;
        if (solo) {  // one query over several CUs (solo_kernels.hpp)
            p.kernel = HnswKernel::Solo;
            p.rejection = false;  // the owner's own int8 pass stays off: for a handful of queries it costs what it saves
            p.pf_groups = std::max(1, std::min(solo_groups, idx->cus / std::max(a.nq, 1) - 1));
            // the window the fetchers keep evaluated ahead of the sequencer: 8 entries for short searches (ef 100: 350 us against 382
            // with 16), 16 from ef 256 (ef 640: 1.21 ms against 1.25 with 8, 1.28 with 32)
            p.pf_hints = hints(a.ef < 256 ? 8 : 16);
            p.solo_chase = tune(HNSWGPU_TUNE_SOLO_CHASE, 1) != 0 ? 1 : 0;
            p.grid = 8 * ((a.nq + 7) / 8) * (1 + p.pf_groups);
            // slots per query of the node-keyed tables: one per row while that stays small (no collisions), else ~32 per list
            // entry (a search claims ~1.5 ef nodes; a record overwritten before the owner has used it costs the owner a gather),
            // and the whole region within 512 MB
            int log2s = static_cast<int>(tune(HNSWGPU_TUNE_SOLO_SLOTS, 0));
            if (log2s <= 0) {
                const int64_t want = std::min<int64_t>(a.n, 32LL * a.ef);
                log2s = 11;
                while ((1LL << log2s) < want && log2s < 18) log2s++;
                while (log2s > 11 && (static_cast<int64_t>(a.nq) << log2s) * a.M0 * 8 > (512LL << 20)) log2s--;
            }
            p.solo_log2s = std::max(8, std::min(log2s, 18));
            const size_t S = static_cast<size_t>(1) << p.solo_log2s;
            // (the mailboxes at a fixed place whatever the batch: a word there never holds an older launch's table entry)
            p.mail_bytes = (sizeof(uint32_t) * kSoloMailWords * kSoloMaxQueries + 255) & ~static_cast<size_t>(255);
            p.table_bytes = (sizeof(uint32_t) * S * a.nq + 255) & ~static_cast<size_t>(255);
            p.rec_bytes = sizeof(unsigned long long) * S * a.M0 * a.nq;
        } else if (small) {  // the round-2 helper kernel
            p.kernel = HnswKernel::SearchHelpers;
            nw = 4;
            // as many helper workgroups per query as find a CU of their own beside the traversals (at most the configured number)
            p.pf_groups = std::max(1, std::min(helper_groups, idx->cus / std::max(a.nq, 1) - 1));
            p.pf_hints = hints(4);
            p.grid = 8 * ((a.nq + 7) / 8) * (1 + p.pf_groups);
            // per region: the mailboxes, then the helpers' published bounds [query][ring slot][neighbour slot]
            p.mail_bytes = sizeof(uint32_t) * kPfMailWords * kPfMaxQueries;
            p.table_bytes = sizeof(unsigned long long) * kPfMaxQueries * kPfRing * kMaxDeg;
            // the helpers evaluate the neighbours of the hinted nodes and publish the distances (kernels.hpp: pf_res); the
            // traversal's own int8 bounds pass stays off: for a handful of queries it costs what it saves
            p.pf_eval = tune(HNSWGPU_TUNE_PF_EVAL, 1) != 0;  // 0 = the helpers only warm the L2 (A/B)
            if (p.pf_eval) p.rejection = false;
        } else {
            p.kernel = wave ? HnswKernel::Wave : HnswKernel::Search;
        }
        p.region = p.mail_bytes + p.table_bytes + p.rec_bytes;
        p.nw = nw;
        // The wave kernel's time follows the bytes that leave the XCD L2s, and queries near each other read largely the same
        // rows: its search launches deal their queries to the XCDs in the order of their nearest pivot row (order_kernels.hpp:
        // a key pass over the int8 rows + a counting sort in front of the traversal; results never depend on it).
        // 31k x 768 clustered (the bench's index), ms per launch plain / ordered, medians of three rounds of ten launches, the
        // two alternating (tools/hnsw_batch_sweep.py --order): ef 640: 2,048 queries 3.503 / 3.588, 4,096: 6.903 / 6.918, 10,000:
        // 12.180 / 11.984; ef 100: 2,048: 1.193 / 1.194, 4,096: 1.486 / 1.628, 10,000: 3.060 / 3.066 (the rounds overlap).  Up to
        // 4,096 queries the chip holds the whole batch at once (16 waves x 256 CUs): no query waits for a slot, so there is no
        // "one XCD at one time" to arrange, and the order costs instead (why 4,096 at ef 100 loses 9.6 % was not looked into).
        // On from 10,000 queries: the smallest measured batch at which ordered is faster at ef 640 and not apart from plain at
        // ef 100.
        // HNSWGPU_TUNE_HNSW_ORDER: 1 (default) = from kOrderMinQueries queries, 0 = never (A/B), 2 = every such launch (tests).
        // (The int8 ROWS decide, not the rejection test: a handle whose test is calibrated off still has them.)
        const int64_t order_mode = tune(HNSWGPU_TUNE_HNSW_ORDER, 1);
        p.ordered = p.kernel == HnswKernel::Wave && !build && !parts && idx->d_qrows && idx->d_qmeta &&
                    (order_mode >= 2 || (order_mode == 1 && a.nq >= kOrderMinQueries));
        if (p.ordered) p.grid = 8 * ((a.nq + 7) / 8);  // slots: eight eighths of order[], the ragged end's surplus slots serve nobody
        // The int8 bounds of the WHOLE batch against ALL rows from the matrix cores, in front of the launch (dense_kernels.hpp): the
        // traversal then reads 4 bytes per fresh neighbour instead of an int8 row -- the same floats, by the same code_lower_bound.
        // Eligible: a plain search launch of the wave kernel with the test on whose table (nq x lb_ld floats) is within the handle's
        // budget (hnswgpu_set_hnsw_dense_bounds: 2 GiB by default -- the 1.25M-row shards are outside it by design).  It pays only
        // while a query tests a sizeable share of the rows (a query tests about 6.5 ef neighbours) and the chip is full.
        // 31k x 768 clustered (the bench's index), ms per launch without / with the table, medians of three rounds of ten launches,
        // the two alternating (tools/hnsw_batch_sweep.py --dense; the rounds of a setting lie within 0.6 % of each other):
        // ef 640: 2,048 queries 3.502 / 2.682, 4,096: 6.884 / 5.250, 10,000: 11.912 / 9.300; ef 1600: 10,000: 37.316 / 28.140;
        // ef 320: 4,096: 3.276 / 2.602, 10,000: 7.033 / 5.587; ef 200: 4,096: 2.326 / 1.906, 10,000: 5.025 / 4.042;
        // ef 100: 4,096: 1.482 / 1.298, 10,000: 3.004 / 2.687.  At the headline the table costs 0.63 ms (hnsw_dense_bounds_kernel)
        // + 0.013 ms (the query codes): profiles/hnsw_dense_gemm_ab.txt (with the first kernel, 0.96 ms, ef 100 was 3.8 % faster at
        // 4,096 queries and 1.0 % slower at 10,000, and the rule stood at 6 % of n: profiles/hnsw_dense_bounds_ab.txt).
        // On where 6.5 ef is at least 2 % of n (2.1 % at ef 100, 4.2 % at ef 200, 6.7 % at ef 320, 13 % at ef 640, 33 % at ef 1600:
        // 11 - 25 % faster at every measured batch) from 8 queries per CU, the smallest batch measured.  Nothing was measured below
        // 2.1 %, nor below 8 queries per CU.
        p.lb_ld = hnsw_dense_ld(a.n);
        const bool dense_rule = a.nq >= 8 * idx->cus && 6.5 * a.ef >= 0.02 * static_cast<double>(a.n);
        p.dense = plain_search && p.kernel == HnswKernel::Wave && p.rejection && !build && !parts && idx->dense_mode != 0 &&
                  static_cast<double>(a.nq) * static_cast<double>(p.lb_ld) * sizeof(float) <= static_cast<double>(idx->dense_budget) &&
                  (idx->dense_mode >= 2 || dense_rule);
        // f32 rows a wave of such a launch keeps in flight, on 768-float rows (nch 3; every other width: HG_HNSW_ROWS).  Without the
        // query code and the eight-row int8 loop the instance with FOUR rows holds 102-103 VGPRs (four waves per SIMD, 16 per CU; two
        // rows: 74-75, six per SIMD), and a hop fetches its rows in half the dependent round trips.  The rule this started from --
        // four where the LDS admits 16 workgroups per CU at most (10,240 B each), so that they cost no resident wave -- left 2-4 %
        // behind between ef 320 and 512.  31k x 768 clustered (the bench's index), ms per launch two / four rows, medians of three
        // rounds of ten launches, the two alternating (tools/hnsw_batch_sweep.py --rows; the rounds of a setting lie within 0.8 %
        // of each other; LDS per workgroup in brackets):
        // 10,000 queries: ef 256 (7,244 B) 5.062 / 5.145, ef 288 (7,500) 5.435 / 5.525, ef 304 (7,628) 5.617 / 5.714, ef 320 (7,756)
        // 6.127 / 5.900, ef 384 (8,268) 6.933 / 6.656, ef 448 (8,780) 7.825 / 7.490, ef 512 (9,292) 8.473 / 8.279, ef 640 (10,316)
        // 10.028 / 9.657, ef 1600 (17,996) 30.376 / 28.443; ef 640: 2,048 queries 2.991 / 2.819, 4,096: 5.565 / 5.357; 4,096 queries:
        // ef 320 2.805 / 2.778, ef 448 3.318 / 3.305.
        // Two rows are 1.7 % faster up to 7,628 B and four 2-6 % from 7,756 B: the TWO-row launch is what changes there (+ 9 % from
        // ef 304 to 320 for 5 % more list; supposed: a CU hands out LDS in steps, 6 x 1,280 = 7,680, and holds 18 such workgroups
        // instead of 21), the four-row one holds 16 by its registers on both sides.  Four rows from kDenseRows4Lds; launches whose
        // visited set is in HBM (less LDS per workgroup) were not measured and follow the same bytes.
        // hnswgpu_hnsw_dense_rows (per handle, like the table's mode): 0 = this rule, 2 / 4 = forced (A/B, tests).
        constexpr size_t kDenseRows4Lds = 7680;
        if (p.dense && p.nch == 3)
            p.dense_rows = idx->dense_rows_mode != 0 ? idx->dense_rows_mode : (wave_lds_bytes(a.cap, nwords) > kDenseRows4Lds ? 4 : 2);
    }
    p.nwords = p.vis_global ? 0 : a.nwords;
    if (p.vis_global) {
        // one slab of n stamps per workgroup; a persistent grid bounds the slab count
        const int64_t budget = 16LL << 30;
        int64_t max_wg = budget / (4 * std::max<int64_t>(a.n, 1));
        max_wg = std::min<int64_t>(std::max<int64_t>(max_wg, 256), 256 * 12);
        const int64_t slots = p.ordered ? 8 * ((static_cast<int64_t>(a.nq) + 7) / 8) : a.nq;
        p.grid = static_cast<int>(std::min<int64_t>(slots, max_wg));
        if (p.ordered) p.grid = std::max(8, p.grid & ~7);  // a multiple of 8: workgroup b's slots b, b + grid, ... stay on its XCD
        p.gens = (slots + p.grid - 1) / p.grid * (a.max_level + 1);
    }
    p.block = p.kernel == HnswKernel::Solo ? kWG : (p.kernel == HnswKernel::Wave ? kWave : p.nw * kWave);
    p.lds = p.kernel == HnswKernel::Solo   ? solo_lds_bytes(a.cap, p.nwords)
            : p.kernel == HnswKernel::Wave ? wave_lds_bytes(a.cap, p.nwords)
                                           : hnsw_lds_bytes(a.cap, p.nwords, p.nw);
    // No public call reaches this limit today: check_hnsw_args and both builders cap ef at 4096, so cap <= 4128, and the visited
    // bits take 32 KiB at most (kLdsVisitedMaxRows).  The three size functions then give at most 10 B x 4128 + 2,384 + 32,768 =
    // 76,432 B (hnsw_search_kernel, four waves), 8 B x 4128 + 1,040 + 32,768 = 66,832 B (hnsw_wave_kernel) and 8 B x 4128 +
    // 36,248 + 32,768 = 102,040 B (hnsw_solo_kernel) of the 163,840; a repeat pass's list (repeat_cap, below) is cut to fit.
    HG_REQUIRE(p.lds <= kMaxLds, HNSWGPU_ELIMIT, "HNSW search state (%zu B: ef=%d, n=%lld) exceeds the 160 KiB LDS of a CU", p.lds,
               a.ef, (long long)a.n);
    p.calibrate = p.calibrate && p.rejection;
    if (!build && !repeat) {
        // Queries that run out of ghost slots are repeated with the largest candidate list the LDS holds (search_enqueue) -- beside
        // the visited set THIS plan chose
        const size_t fixed = hnsw_lds_bytes(0, p.nwords, 4);
        const int64_t cap_max = std::min<int64_t>(65000, static_cast<int64_t>((kMaxLds - fixed) / (sizeof(uint2) + sizeof(uint16_t))));
        const int64_t big = std::min<int64_t>(cap_max - a.ef, vis_rows);
        p.repeat_cap = big > kGhost ? static_cast<int32_t>(a.ef + big) : 0;
    }
    p.fn = parts                          ? hnsw_parts_kernel_for(p, a)
           : p.kernel == HnswKernel::Solo ? hnsw_solo_kernel_for(p, a)
           : p.dense                      ? hnsw_wave_dense_kernel_for(p, a)
           : p.kernel == HnswKernel::Wave ? hnsw_wave_kernel_for(p, a)
                                          : hnsw_search_kernel_for(p, a);
    HG_REQUIRE(p.fn, HNSWGPU_ELIMIT, "unsupported row length");
    return 0;
}

// every stream that may still run a launch that reads or writes s_pf / s_solo (the slot launches take no part in hg::Call's event ordering)
static int hnsw_tables_idle(hnswgpu_index *idx, hipStream_t st) {
    for (auto &sl : idx->slots)
        if (sl.st) HG_HIP(hipStreamSynchronize(sl.st));
    if (idx->stream) HG_HIP(hipStreamSynchronize(idx->stream));
    HG_HIP(hipStreamSynchronize(st));
    return 0;
}

// The launch number of the small launches, the ONE owner of hnswgpu_index::pf_seq for the round-2 helper kernel and the several-CU
// kernel alike.  Contract: a word written into s_pf or s_solo under launch number s can never be read by a launch whose tag
// compares equal to s's (all 24 bits in the helper tables: (number << 8 | lap); the low 14 bits in solo_tag) unless it is that
// launch -- whichever path took the launches in between.  One counter of 24 bits serves both tables: whenever it reaches a multiple
// of 0x4000 (2^24 among them) the streams are waited for, every allocated table is cleared and the counter moves on, so two
// launches whose numbers agree in the low 14 bits always have a clearing of both tables between them.  The number is never 0, in
// either width (tag 0 is what fresh memory holds: nothing).  Four regions in rotation (number & 3), so that launches in flight
// (two Slots) never share one.  Cost: one synchronise-and-clear per 16383 small launches.
static int hnsw_number_launch(hnswgpu_index *idx, hipStream_t st) {
    idx->pf_seq = (idx->pf_seq + 1) & 0xffffff;
    if ((idx->pf_seq & 0x3fff) != 0) return 0;
    HG_TRY(hnsw_tables_idle(idx, st));
    for (DevBuf *t : {&idx->s_pf, &idx->s_solo})
        if (t->p) HG_HIP(hipMemsetAsync(t->p, 0, t->cap, st));
    HG_HIP(hipStreamSynchronize(st));
    idx->pf_seq++;
    return 0;
}

// Stage 3: everything that touches the handle or a stream before the kernel, and the plan's part of HnswArgs.  Decides nothing.
static int hnsw_launch_resources(hnswgpu_index *idx, const HnswLaunchPlan &p, HnswArgs &a, hipStream_t st, int32_t *order_mem,
                                 DenseScratch *dense_mem) {
    a.dbg = g_tile_dbg_buf;  // null outside diagnostic sessions
    if (p.dense) {  // dense_mem: a slot launch's own scratch (two may be in flight); otherwise the handle's, ordered by the call scope
        DenseScratch &ds = dense_mem ? *dense_mem : idx->s_dense;
        HG_TRY(ds.codes.ensure(hnsw_dense_code_bytes(p.nch, a.nq) + sizeof(QueryScal) * static_cast<size_t>(a.nq)));
        HG_TRY(ds.lb.ensure(sizeof(float) * static_cast<size_t>(a.nq) * static_cast<size_t>(p.lb_ld)));
        HG_TRY(launch_hnsw_dense(idx, a.Q, a.qld, a.nq, ds.codes.p, ds.lb.as<float>(), p.lb_ld, st));
        a.lb = ds.lb.as<float>();
        a.lb_ld = p.lb_ld;
        idx->dense_launches++;
        if (p.dense_rows == 4) idx->dense_rows4_launches++;
    }
    if (p.ordered) {  // order_mem: a slot launch's own [order | keys] (two may be in flight); otherwise the handle's scratch
        if (!order_mem) {
            HG_TRY(idx->s_hord.ensure(sizeof(int32_t) * 2 * static_cast<size_t>(a.nq)));
            order_mem = idx->s_hord.as<int32_t>();
        }
        OrderArgs o;
        o.Q = a.Q;
        o.qld = a.qld;
        o.dim = a.dim;
        o.metric = a.metric;
        o.nq = a.nq;
        o.n = a.n;
        o.qrows = idx->d_qrows;
        o.qmeta = idx->d_qmeta;
        o.order = order_mem;
        o.keys = order_mem + a.nq;
        HG_TRY(launch_hnsw_order(p.nch, o, st));
        a.q_order = o.order;
        idx->hnsw_order_last = o.order;
        idx->hnsw_order_nq = a.nq;
    }
    a.rej_stats = idx->prof ? idx->d_rej_stats : nullptr;
    if (!p.rejection) a.qrows = nullptr;
    a.nwords = p.nwords;
    if (p.kernel == HnswKernel::SearchHelpers || p.kernel == HnswKernel::Solo) {
        const bool solo = p.kernel == HnswKernel::Solo;
        DevBuf &tab = solo ? idx->s_solo : idx->s_pf;
        // Growing the buffer frees the old one: every stream that may still run a launch on it is waited for first (s_pf has one
        // size: it grows once, from nothing).  Fresh memory is zeroed (tag 0 = nothing), and the zero fill is waited for: the other
        // slot's launch runs on ITS stream and would otherwise see the old bytes -- harmless for results, the words are tagged,
        // but its helpers would poll until their timeout.
        if (tab.cap < 4 * p.region) {
            if (solo) HG_TRY(hnsw_tables_idle(idx, st));
            HG_TRY(tab.ensure(4 * p.region));
            HG_HIP(hipMemsetAsync(tab.p, 0, tab.cap, st));
            HG_HIP(hipStreamSynchronize(st));
        }
        HG_TRY(hnsw_number_launch(idx, st));
        a.pf_seq = idx->pf_seq;
        a.pf_groups = p.pf_groups;
        a.pf_hints = p.pf_hints;
        // one mailbox per query at the head of the launch's region (the several-CU kernel's regions: a quarter of the buffer each)
        char *reg = static_cast<char *>(tab.p) + (idx->pf_seq & 3) * (solo ? (tab.cap / 4 & ~static_cast<size_t>(255)) : p.region);
        a.pf_mail = reinterpret_cast<uint32_t *>(reg);
        if (solo) {
            a.solo_chase = p.solo_chase;
            a.solo_log2s = p.solo_log2s;
            a.solo_claim = reinterpret_cast<uint32_t *>(reg + p.mail_bytes);
            a.solo_rec = reinterpret_cast<unsigned long long *>(reg + p.mail_bytes + p.table_bytes);
        } else if (p.pf_eval) {
            a.pf_res = reinterpret_cast<unsigned long long *>(reg + p.mail_bytes);
        }
    }
    if (p.vis_global) {
        const size_t need = sizeof(uint32_t) * static_cast<size_t>(a.n) * p.grid;
        if (need > idx->s_vis.cap) {
            HG_TRY(idx->s_vis.ensure(need));
            HG_HIP(hipMemsetAsync(idx->s_vis.p, 0, idx->s_vis.cap, st));
            idx->vis_gen = 0;
        }
        if (static_cast<int64_t>(idx->vis_gen) + p.gens >= 0xfffffff0LL) {
            HG_HIP(hipMemsetAsync(idx->s_vis.p, 0, idx->s_vis.cap, st));
            idx->vis_gen = 0;
        }
        a.vis = idx->s_vis.as<uint32_t>();
        a.vis_stride = a.n;
        a.gen_base = idx->vis_gen;
        idx->vis_gen += static_cast<uint32_t>(p.gens);
    }
    if (p.calibrate) {
        if (!idx->d_hnsw_cal) {
            HG_HIP(hipMalloc(reinterpret_cast<void **>(&idx->d_hnsw_cal), 2 * sizeof(unsigned long long)));
            HG_HIP(hipHostMalloc(reinterpret_cast<void **>(&idx->hnsw_cal_host), 2 * sizeof(unsigned long long), hipHostMallocDefault));
            HG_HIP(hipEventCreateWithFlags(&idx->ev_hnsw_cal, hipEventDisableTiming));
        }
        HG_HIP(hipMemsetAsync(idx->d_hnsw_cal, 0, 2 * sizeof(unsigned long long), st));
        a.rej_stats = idx->d_hnsw_cal;
    }
    return 0;
}

// Stage 4: the one launch block of the three kernel families (the limit of dynamic LDS is raised on every launch beyond 48 KiB)
static int hnsw_dispatch(const HnswLaunchPlan &p, const HnswArgs &a, hipStream_t st) {
    if (p.lds > 48 * 1024)
        HG_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(p.fn), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(p.lds)));
    hipLaunchKernelGGL(p.fn, dim3(p.grid), dim3(p.block), p.lds, st, a);
    HG_HIP(hipGetLastError());
    return 0;
}

// Stages 3 to 5 of a planned launch; the tail: the launch counters, and a measuring launch sends its counters on their way
static int hnsw_launch_planned(hnswgpu_index *idx, const HnswLaunchPlan &p, HnswArgs a, hipStream_t st, int32_t *order_mem = nullptr,
                               DenseScratch *dense_mem = nullptr) {
    HG_TRY(hnsw_launch_resources(idx, p, a, st, order_mem, dense_mem));
    HG_TRY(hnsw_dispatch(p, a, st));
    if (p.kernel == HnswKernel::Solo) count_launch(HNSWGPU_COUNT_HNSW_SOLO);
    else if (p.kernel == HnswKernel::SearchHelpers) count_launch(HNSWGPU_COUNT_HNSW_HELPERS);
    else count_launch(p.rejection ? HNSWGPU_COUNT_HNSW_REJECTION : HNSWGPU_COUNT_HNSW_PLAIN);
    if (p.kernel == HnswKernel::Wave) count_launch(HNSWGPU_COUNT_HNSW_WAVE);
    if (p.ordered) count_launch(HNSWGPU_COUNT_HNSW_ORDERED);
    if (p.calibrate) {
        HG_HIP(hipMemcpyAsync(idx->hnsw_cal_host, idx->d_hnsw_cal, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
        HG_HIP(hipEventRecord(idx->ev_hnsw_cal, st));
        idx->hnsw_cal_state = 1;
    }
    return 0;
}

// One HNSW traversal launch, stages 1 to 5 (the builder's; search_enqueue keeps its plan for the repeat pass)
static int launch_hnsw_idx(hnswgpu_index *idx, const HnswArgs &a, hipStream_t st) {
    if (a.nq <= 0) return 0;
    HnswLaunchPlan p;
    hnsw_calibration_absorb(idx);
    HG_TRY(hnsw_launch_plan(idx, a, nullptr, p));
    return hnsw_launch_planned(idx, p, a, st);
}

static void free_graph(hnswgpu_index *idx) {
    idx->graph_gen++;  // searches in flight on a slot stream compare it before their repeat pass
    idx->build_flags = 0;  // (an installed graph has none: engine.hpp; hnswgpu_hnsw_build_ex sets them once its graph stands)
    idx->hnsw_cal_state = 0;  // the next graph is measured afresh
    idx->hnsw_rej_off = false;
    void *ptrs[] = {idx->d_levels, idx->d_l0, idx->d_upadj, idx->d_upoff};
    for (void *p : ptrs)
        if (p) (void)hipFree(p);
    idx->d_levels = idx->d_l0 = idx->d_upadj = nullptr;
    idx->d_upoff = nullptr;
    idx->has_graph = false;
    if (idx->d_parts) (void)hipFree(idx->d_parts);  // a forest's part tables go with its graph
    idx->d_parts = nullptr;
    idx->nparts = 0;
    idx->max_part = 0;
    idx->h_part_off.clear();
    idx->h_part_entry.clear();
    idx->h_part_level.clear();
}

static int alloc_graph(hnswgpu_index *idx, int M, int M0, int64_t up_blocks) {
    int64_t n = std::max<int64_t>(idx->n, 1);
    HG_HIP(hipMalloc(reinterpret_cast<void **>(&idx->d_levels), sizeof(int32_t) * n));
    HG_HIP(hipMalloc(reinterpret_cast<void **>(&idx->d_l0), sizeof(int32_t) * n * M0));
    HG_HIP(hipMalloc(reinterpret_cast<void **>(&idx->d_upoff), sizeof(int64_t) * (n + 1)));
    HG_HIP(hipMalloc(reinterpret_cast<void **>(&idx->d_upadj), sizeof(int32_t) * std::max<int64_t>(up_blocks, 1) * M));
    idx->M = M;
    idx->M0 = M0;
    idx->up_blocks = up_blocks;
    return 0;
}

static void fill_args(const hnswgpu_index *idx, HnswArgs &a) {
    memset(&a, 0, sizeof(a));
    a.rows = idx->d_base;
    a.row_norms = idx->d_norms;
    a.qrows = idx->d_qrows;
    a.qmeta = idx->d_qmeta;
    a.ld = idx->ld;
    a.n = idx->n;
    a.dim = idx->dim;
    a.metric = idx->metric;
    a.l0_adj = idx->d_l0;
    a.M0 = idx->M0;
    a.up_off = idx->d_upoff;
    a.up_adj = idx->d_upadj;
    a.M = idx->M;
    a.entry = idx->entry;
    a.max_level = idx->max_level;
    a.nwords = static_cast<int32_t>((idx->n + 31) / 32);
}

// A slot launch (see hnswgpu_index::Slot): the kernel publishes its completion to the host itself, the repeat pass is
// left to the caller (it knows from host_again whether any query needs one -- on ordinary data none does).
struct SlotSignal {
    int32_t *again;        // device: [0] = count, [1..] = queries to repeat; zero between calls
    uint32_t *done_cnt;    // device: zero between calls
    uint32_t *host_flag;   // device address of the flag word in the mapped block
    int32_t *host_again;   // device address of the repeat count in the mapped block
    uint32_t flag_val;
    int32_t *order;        // device: [2 x kZcMaxQueries], order and keys of an ordered launch
    DenseScratch *dense;   // the slot's scratch of a launch with the dense bounds table
};

static int search_enqueue(hnswgpu_index *idx, const float *d_Q, int32_t nq, int32_t k, int32_t ef,
                          int32_t *d_ids, float *d_dist, int64_t *d_stats, hipStream_t st,
                          const SlotSignal *sig = nullptr, bool repeat_only = false, bool filtered = false) {
    // under the handle's lock: a forest has no entry point of its own (the one check behind every plain and filtered search)
    HG_REQUIRE(idx->nparts == 0, HNSWGPU_ESTATE,
               "the index holds a forest (hnswgpu_set_graph_parts / hnswgpu_hnsw_build_parts): search it with hnswgpu_hnsw_search_parts");
    HnswArgs a;
    fill_args(idx, a);
    a.Q = d_Q;
    a.qld = idx->dim;
    a.nq = nq;
    a.ef = ef;
    a.k = k;
    a.cap = ef + kGhost;
    a.out_ids = d_ids;
    a.out_dist = d_dist;
    a.stats = d_stats;
    if (nq <= 0) return 0;
    // one plan -- one reading of the tuning table -- per call: the first pass's, which also sizes the repeat pass
    HnswLaunchPlan p;
    if (!repeat_only) hnsw_calibration_absorb(idx);
    HG_TRY(hnsw_launch_plan(idx, a, nullptr, p, !filtered));
    int32_t *again_cnt, *again;
    if (sig) {
        again_cnt = sig->again;
        again = again_cnt + 1;
    } else {
        // queries that run out of ghost slots (hundreds of duplicated rows) list themselves in s_probes[1 ..]
        HG_TRY(idx->s_probes.ensure(sizeof(int32_t) * (static_cast<size_t>(nq) + 1)));
        again_cnt = idx->s_probes.as<int32_t>();
        again = again_cnt + 1;
        HG_HIP(hipMemsetAsync(again_cnt, 0, sizeof(int32_t), st));
    }
    int rc = 0;
    if (!repeat_only) {
        a.again = again;
        a.again_cnt = again_cnt;
        if (sig) {
            a.done_cnt = sig->done_cnt;
            a.host_flag = sig->host_flag;
            a.host_again = sig->host_again;
            a.flag_val = sig->flag_val;
        }
        hipEvent_t e0;
        prof_begin(idx, PROF_HNSW, st, &e0);
        rc = hnsw_launch_planned(idx, p, a, st, sig ? sig->order : nullptr, sig ? sig->dense : nullptr);
        prof_end(idx, PROF_HNSW, st, e0);
        if (rc || sig) return rc;
        a.done_cnt = nullptr;
        a.host_flag = nullptr;
    }
    // ... and are repeated, on the device and without a host round trip, with the largest candidate list the LDS
    // holds, so that every tie the reference would still expand (ultra_fast.clj:175-178, `<=`) is kept.  The pass
    // finds no work item on ordinary data (a few microseconds).
    if (p.repeat_cap) {
        a.cap = p.repeat_cap;
        a.again = nullptr;
        a.again_cnt = nullptr;
        a.q_index = again;
        a.nq_dev = again_cnt;
        HnswLaunchPlan r;
        HG_TRY(hnsw_launch_plan(idx, a, &p, r));
        rc = hnsw_launch_planned(idx, r, a, st);
    }
    if (repeat_only && rc == 0) HG_HIP(hipMemsetAsync(again_cnt, 0, sizeof(int32_t), st));  // zero between calls
    return rc;
}

struct HostGraph {
    int64_t n;
    int M, M0;
    std::vector<int32_t> levels, l0, l0_cnt, up, up_cnt;
    std::vector<float> l0_d, up_d;
    std::vector<int64_t> up_off;
    int entry = -1, top = -1;

    int32_t *adj(int32_t node, int lc, float **d, int32_t **cnt, int *m) {
        if (lc == 0) {
            *d = &l0_d[static_cast<size_t>(node) * (M0 + 1)];
            *cnt = &l0_cnt[node];
            *m = M0;
            return &l0[static_cast<size_t>(node) * (M0 + 1)];
        }
        int64_t blk = up_off[node] + (lc - 1);
        *d = &up_d[static_cast<size_t>(blk) * (M + 1)];
        *cnt = &up_cnt[blk];
        *m = M;
        return &up[static_cast<size_t>(blk) * (M + 1)];
    }

    // rows whose adjacency changed since the last upload (device copy is patched incrementally)
    std::vector<int32_t> dirty0;
    std::vector<int64_t> dirtyu;
    std::vector<uint8_t> flag0, flagu;
    // 1 once a list has been pruned: it is then sorted by (distance, insertion order) and stays so
    std::vector<uint8_t> sorted0, sortedu;

    // the dirty lists a linking thread appends to (its own: a node's flags are only touched by the thread that owns
    // the node, the lists are concatenated after the batch)
    struct Dirty {
        std::vector<int32_t> d0;
        std::vector<int64_t> du;
    };

    void mark(int32_t node, int lc, Dirty &out) {
        if (lc == 0) {
            if (!flag0[node]) {
                flag0[node] = 1;
                out.d0.push_back(node);
            }
        } else {
            int64_t blk = up_off[node] + (lc - 1);
            if (!flagu[blk]) {
                flagu[blk] = 1;
                out.du.push_back(blk);
            }
        }
    }

    // one direction of "Connect bidirectionally" (ultra_fast.clj:255-266) + prune-connections-ultra
    // (:279-299): an over-full list keeps its m closest by (distance, insertion order) -- (take max-conns
    // (sort-by dist connections)), a stable sort.  Edge distances are stored with the edges, so pruning needs no
    // distance evaluation.  After its first pruning a list IS that sorted order, and appending one edge and
    // stable-sorting again equals inserting it behind the last edge with distance <= its own and dropping the
    // last: a shift instead of a sort (the sort was most of the 0.25 s of host time in a 0.33 s 31k x 768 build).
    void add_edge(int32_t from, int32_t to, int lc, float dist, Dirty &out) {
        float *d;
        int32_t *cnt;
        int m;
        int32_t *a = adj(from, lc, &d, &cnt, &m);
        for (int i = 0; i < *cnt; i++)
            if (a[i] == to) return;
        uint8_t &srt = lc == 0 ? sorted0[from] : sortedu[up_off[from] + (lc - 1)];
        if (*cnt == m && srt) {
            if (!(dist < d[m - 1])) return;  // sorts last (ties go behind the older edges) and is dropped again
            int pos = m - 1;
            while (pos > 0 && dist < d[pos - 1]) pos--;
            for (int i = m - 1; i > pos; i--) {
                a[i] = a[i - 1];
                d[i] = d[i - 1];
            }
            a[pos] = to;
            d[pos] = dist;
            mark(from, lc, out);
            return;
        }
        a[*cnt] = to;
        d[*cnt] = dist;
        (*cnt)++;
        mark(from, lc, out);
        if (*cnt > m) {  // first overflow of this list: the stable sort itself
            int ord[kMaxDeg + 1];
            const int c = *cnt;
            for (int i = 0; i < c; i++) ord[i] = i;
            std::stable_sort(ord, ord + c, [&](int x, int y) { return d[x] < d[y]; });
            int32_t na[kMaxDeg + 1];
            float nd[kMaxDeg + 1];
            for (int i = 0; i < m; i++) {
                na[i] = a[ord[i]];
                nd[i] = d[ord[i]];
            }
            for (int i = 0; i < m; i++) {
                a[i] = na[i];
                d[i] = nd[i];
            }
            a[m] = -1;
            *cnt = m;
            srt = 1;
        }
    }

    // graph.clj's builder: an edge is appended while the list has room; into a full list it is PENDING until the list is
    // re-selected by the heuristic (prune-connections, graph.clj:208-232) -- returns false then
    bool append_edge(int32_t from, int32_t to, int lc, float dist, Dirty &out) {
        float *d;
        int32_t *cnt;
        int m;
        int32_t *a = adj(from, lc, &d, &cnt, &m);
        for (int i = 0; i < *cnt; i++)
            if (a[i] == to) return true;
        if (*cnt >= m) return false;
        a[*cnt] = to;
        d[*cnt] = dist;
        (*cnt)++;
        mark(from, lc, out);
        return true;
    }
    void set_list(int32_t node, int lc, const int32_t *ids, const float *ds, int n, Dirty &out) {
        float *d;
        int32_t *cnt;
        int m;
        int32_t *a = adj(node, lc, &d, &cnt, &m);
        for (int i = 0; i < n; i++) {
            a[i] = ids[i];
            d[i] = ds[i];
        }
        for (int i = n; i <= m; i++) a[i] = -1;
        *cnt = n;
        mark(node, lc, out);
    }
    // one side of a symmetric removal (graph.clj:226-231); true if the edge was there
    bool remove_edge(int32_t from, int32_t to, int lc, Dirty &out) {
        float *d;
        int32_t *cnt;
        int m;
        int32_t *a = adj(from, lc, &d, &cnt, &m);
        for (int i = 0; i < *cnt; i++)
            if (a[i] == to) {
                for (int t = i; t + 1 < *cnt; t++) {
                    a[t] = a[t + 1];
                    d[t] = d[t + 1];
                }
                a[--(*cnt)] = -1;
                mark(from, lc, out);
                return true;
            }
        return false;
    }
};

// Host threads of the linker.  A batch's edges are applied in two sweeps that give every adjacency list exactly the
// sequence of updates the sequential loop gives it: (A) every new node's OWN lists (disjoint between nodes),
// (B) the reverse edges, each thread walking the whole batch in order and applying the edges whose TARGET node it
// owns (node mod T).  No locks, and the graph does not depend on the thread count.
class LinkPool {
public:
    explicit LinkPool(int n) {
        for (int i = 1; i < n; i++) th_.emplace_back([this, i] { worker(i); });
    }
    ~LinkPool() {
        {
            std::lock_guard<std::mutex> lk(mu_);
            stop_ = true;
        }
        cv_.notify_all();
        for (auto &t : th_) t.join();
    }
    int size() const { return static_cast<int>(th_.size()) + 1; }
    void run(const std::function<void(int)> &f) {
        {
            std::lock_guard<std::mutex> lk(mu_);
            job_ = &f;
            pending_ = static_cast<int>(th_.size());
            gen_++;
        }
        cv_.notify_all();
        f(0);
        std::unique_lock<std::mutex> lk(mu_);
        done_.wait(lk, [this] { return pending_ == 0; });
    }

private:
    void worker(int id) {
        int seen = 0;
        for (;;) {
            const std::function<void(int)> *f;
            {
                std::unique_lock<std::mutex> lk(mu_);
                cv_.wait(lk, [&] { return stop_ || gen_ != seen; });
                if (stop_) return;
                seen = gen_;
                f = job_;
            }
            (*f)(id);
            {
                std::lock_guard<std::mutex> lk(mu_);
                if (--pending_ == 0) done_.notify_one();
            }
        }
    }
    std::vector<std::thread> th_;
    std::mutex mu_;
    std::condition_variable cv_, done_;
    const std::function<void(int)> *job_ = nullptr;
    int gen_ = 0, pending_ = 0;
    bool stop_ = false;
};

// dst[ids[i] * width + j] = packed[i * width + j]
__global__ void scatter_rows_kernel(int32_t *dst, int width, const int64_t *ids, const int32_t *packed, int64_t count) {
    int64_t t = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (t >= count * width) return;
    int64_t i = t / width;
    int j = static_cast<int>(t % width);
    dst[ids[i] * width + j] = packed[t];
}

// pinned host staging buffer (grown on demand): pageable vectors made the adjacency patches of a 1.25M-row build
// 2.6 s of its 13 s
struct PinnedBuf {
    void *p = nullptr;
    size_t cap = 0;
    ~PinnedBuf() {
        if (p) (void)hipHostFree(p);
    }
    int ensure(size_t bytes) {
        if (bytes <= cap) return 0;
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
        size_t want = bytes + bytes / 2 + 4096;
        HG_HIP(hipHostMalloc(&p, want, hipHostMallocDefault));
        cap = want;
        return 0;
    }
};

// patch the device adjacency with the rows that changed (full arrays are never re-sent)
static int upload_dirty(hnswgpu_index *idx, HostGraph &g, hipStream_t st, PinnedBuf &pin, LinkPool &pool) {
    for (int pass = 0; pass < 2; pass++) {
        const int width = pass == 0 ? g.M0 : g.M;
        const int64_t cnt = pass == 0 ? static_cast<int64_t>(g.dirty0.size()) : static_cast<int64_t>(g.dirtyu.size());
        if (cnt == 0) continue;
        const size_t ids_bytes = sizeof(int64_t) * static_cast<size_t>(cnt);
        const size_t pack_bytes = sizeof(int32_t) * static_cast<size_t>(cnt) * width;
        HG_TRY(pin.ensure(ids_bytes + pack_bytes));
        int64_t *ids = static_cast<int64_t *>(pin.p);
        int32_t *pack = reinterpret_cast<int32_t *>(ids + cnt);
        auto pack_range = [&](int64_t lo, int64_t hi) {
            for (int64_t i = lo; i < hi; i++) {
                int64_t row = pass == 0 ? g.dirty0[i] : g.dirtyu[i];
                ids[i] = row;
                const int32_t *src = pass == 0 ? &g.l0[row * (g.M0 + 1)] : &g.up[row * (g.M + 1)];
                const int have = pass == 0 ? g.l0_cnt[row] : g.up_cnt[row];
                for (int j = 0; j < width; j++) pack[i * width + j] = j < have ? src[j] : -1;
                if (pass == 0) g.flag0[row] = 0;
                else g.flagu[row] = 0;
            }
        };
        const int nt = cnt >= 4096 ? pool.size() : 1;
        if (nt == 1) pack_range(0, cnt);
        else pool.run([&](int me) { pack_range(cnt * me / nt, cnt * (me + 1) / nt); });
        HG_TRY(idx->s_partial.ensure(ids_bytes + pack_bytes + 64));
        int64_t *d_ids = idx->s_partial.as<int64_t>();
        int32_t *d_pack = reinterpret_cast<int32_t *>(d_ids + cnt);
        HG_HIP(hipMemcpyAsync(d_ids, ids, ids_bytes + pack_bytes, hipMemcpyHostToDevice, st));  // ids | pack, one copy
        int64_t total = cnt * width;
        hipLaunchKernelGGL(scatter_rows_kernel, dim3(static_cast<unsigned>((total + 255) / 256)), dim3(256), 0, st,
                           pass == 0 ? idx->d_l0 : idx->d_upadj, width, d_ids, d_pack, cnt);
        HG_HIP(hipGetLastError());
        HG_HIP(hipStreamSynchronize(st));  // the staging buffers are reused by the next pass
        if (pass == 0) g.dirty0.clear();
        else g.dirtyu.clear();
    }
    return 0;
}

static int upload_graph(hnswgpu_index *idx, const HostGraph &g, hipStream_t st, std::vector<int32_t> &tmp0,
                        std::vector<int32_t> &tmpu) {
    const int64_t n = g.n;
    tmp0.assign(static_cast<size_t>(n) * g.M0, -1);
    for (int64_t i = 0; i < n; i++)
        for (int j = 0; j < g.l0_cnt[i] && j < g.M0; j++) tmp0[i * g.M0 + j] = g.l0[i * (g.M0 + 1) + j];
    const int64_t blocks = g.up_off[n];
    tmpu.assign(static_cast<size_t>(std::max<int64_t>(blocks, 1)) * g.M, -1);
    for (int64_t b = 0; b < blocks; b++)
        for (int j = 0; j < g.up_cnt[b] && j < g.M; j++) tmpu[b * g.M + j] = g.up[b * (g.M + 1) + j];
    HG_HIP(hipMemcpyAsync(idx->d_l0, tmp0.data(), sizeof(int32_t) * tmp0.size(), hipMemcpyHostToDevice, st));
    HG_HIP(hipMemcpyAsync(idx->d_upadj, tmpu.data(), sizeof(int32_t) * tmpu.size(), hipMemcpyHostToDevice, st));
    HG_HIP(hipStreamSynchronize(st));
    return 0;
}

// The part tables of a forest as the caller hands them over (hnswgpu_set_graph_parts); null = a plain graph
struct PartTables {
    int32_t nparts;
    const int64_t *off;     // [nparts + 1]
    const int32_t *entry;   // [nparts], -1 for an empty part
    const int32_t *level;   // [nparts], the entry's level
};

// Everything hnswgpu_set_graph and hnswgpu_set_graph_parts require of their arrays, before anything on the handle changes.  The
// kernels trust it: every edge points at a node that exists on that layer -- and, in a forest, inside the edge's own part (the
// LDS visited set of a forest launch covers one part).
static int check_graph(const hnswgpu_index *idx, const int32_t *levels, const int32_t *l0_adj, int32_t M0, const int64_t *up_off,
                       const int32_t *up_adj, int32_t M, int32_t entry, int32_t max_level, const PartTables *pt) {
    HG_REQUIRE(idx, HNSWGPU_EINVAL, "idx is null");
    const int64_t n = idx->n;
    HG_REQUIRE(n == 0 || (levels && l0_adj && up_off), HNSWGPU_EINVAL, "null argument");
    HG_REQUIRE(M >= 1 && M0 >= 1 && M0 <= kMaxDeg && M <= kMaxDeg, HNSWGPU_ELIMIT, "need 1 <= M, M0 <= %d", kMaxDeg);
    if (pt) {
        HG_REQUIRE(pt->nparts >= 1 && pt->off && pt->entry && pt->level, HNSWGPU_EINVAL, "need nparts >= 1 and the three part tables");
        HG_REQUIRE(pt->off[0] == 0 && pt->off[pt->nparts] == n, HNSWGPU_EINVAL, "part_off must run from 0 to n");
        for (int32_t p = 0; p < pt->nparts; p++) {
            const int64_t lo = pt->off[p], hi = pt->off[p + 1];
            HG_REQUIRE(lo <= hi && hi <= n, HNSWGPU_EINVAL, "part_off is not monotone at part %d", p);
            if (lo == hi) {
                HG_REQUIRE(pt->entry[p] == -1, HNSWGPU_EINVAL, "part %d is empty: its entry must be -1", p);
                continue;
            }
            HG_REQUIRE(pt->entry[p] >= lo && pt->entry[p] < hi, HNSWGPU_EINVAL, "the entry of part %d lies outside the part", p);
            HG_REQUIRE(pt->level[p] >= 0 && levels[pt->entry[p]] >= pt->level[p], HNSWGPU_EINVAL, "part %d: entry level < max_level", p);
        }
    } else if (n > 0) {
        HG_REQUIRE(entry >= 0 && entry < n, HNSWGPU_EINVAL, "entry out of range");
        HG_REQUIRE(max_level >= 0 && levels[entry] >= max_level, HNSWGPU_EINVAL, "entry level < max_level");
    }
    if (n == 0) return 0;
    HG_REQUIRE(up_off[0] == 0, HNSWGPU_EINVAL, "up_off[0] != 0");
    const int64_t whole[2] = {0, n};
    const int32_t np = pt ? pt->nparts : 1;
    for (int32_t p = 0; p < np; p++) {
        const int64_t lo = pt ? pt->off[p] : whole[0], hi = pt ? pt->off[p + 1] : whole[1];
        const int32_t top = pt ? pt->level[p] : max_level;
        for (int64_t i = lo; i < hi; i++) {
            HG_REQUIRE(levels[i] >= 0, HNSWGPU_EINVAL, "node %lld has a negative level", (long long)i);
            HG_REQUIRE(up_off[i + 1] - up_off[i] == levels[i], HNSWGPU_EINVAL,
                       "up_off is not the prefix sum of levels at node %lld", (long long)i);
            HG_REQUIRE(levels[i] <= top, HNSWGPU_EINVAL, "node %lld level > max_level", (long long)i);
        }
    }
    HG_REQUIRE(up_off[n] == 0 || up_adj, HNSWGPU_EINVAL, "up_adj is null");
    for (int32_t p = 0; p < np; p++) {
        const int64_t lo = pt ? pt->off[p] : whole[0], hi = pt ? pt->off[p + 1] : whole[1];
        for (int64_t i = lo * M0; i < hi * M0; i++)
            HG_REQUIRE(l0_adj[i] == -1 || (l0_adj[i] >= lo && l0_adj[i] < hi), HNSWGPU_EINVAL,
                       pt ? "l0_adj entry leaves its part" : "l0_adj entry out of range");
        for (int64_t i = lo; i < hi; i++)
            for (int lv = 1; lv <= levels[i]; lv++)
                for (int j = 0; j < M; j++) {
                    int32_t nb = up_adj[(up_off[i] + lv - 1) * M + j];
                    HG_REQUIRE(nb == -1 || (nb >= lo && nb < hi), HNSWGPU_EINVAL,
                               pt ? "up_adj entry leaves its part" : "up_adj entry out of range");
                    HG_REQUIRE(nb < 0 || levels[nb] >= lv, HNSWGPU_EINVAL,
                               "edge %lld->%d on layer %d: target has no such layer", (long long)i, nb, lv);
                }
    }
    return 0;
}

// Checked arrays -> the handle, inside the caller's call scope.  The device copies are made and filled BESIDE what the handle
// holds; only when they stand is the old graph freed and the handle switched over, so a failing call leaves the handle as it was.
static int install_graph(hnswgpu_index *idx, Call &call, hipStream_t st, const int32_t *levels, const int32_t *l0_adj, int32_t M0,
                         const int64_t *up_off, const int32_t *up_adj, int32_t M, int32_t entry, int32_t max_level,
                         const PartTables *pt) {
    const int64_t n = idx->n, n1 = std::max<int64_t>(n, 1);
    const int64_t blocks = n > 0 ? up_off[n] : 0;
    std::vector<int4> parts;
    int64_t max_part = 0;
    int32_t top = n > 0 ? max_level : 0;
    if (pt) {
        parts.resize(pt->nparts);
        top = 0;
        for (int32_t p = 0; p < pt->nparts; p++) {
            const int64_t rows = pt->off[p + 1] - pt->off[p];
            parts[p] = make_int4(static_cast<int32_t>(pt->off[p]), rows > 0 ? pt->entry[p] : -1, rows > 0 ? pt->level[p] : 0,
                                 static_cast<int32_t>(rows));
            max_part = std::max(max_part, rows);
            if (rows > 0) top = std::max(top, pt->level[p]);
        }
    }
    struct Staged {
        int32_t *levels = nullptr, *l0 = nullptr, *upadj = nullptr;
        int64_t *upoff = nullptr;
        int4 *parts = nullptr;
        ~Staged() {
            void *ptrs[] = {levels, l0, upadj, upoff, parts};
            for (void *p : ptrs)
                if (p) (void)hipFree(p);
        }
    } sg;
    HG_HIP(hipMalloc(reinterpret_cast<void **>(&sg.levels), sizeof(int32_t) * n1));
    HG_HIP(hipMalloc(reinterpret_cast<void **>(&sg.l0), sizeof(int32_t) * n1 * M0));
    HG_HIP(hipMalloc(reinterpret_cast<void **>(&sg.upoff), sizeof(int64_t) * (n1 + 1)));
    HG_HIP(hipMalloc(reinterpret_cast<void **>(&sg.upadj), sizeof(int32_t) * std::max<int64_t>(blocks, 1) * M));
    if (pt) {
        HG_HIP(hipMalloc(reinterpret_cast<void **>(&sg.parts), sizeof(int4) * parts.size()));
        HG_HIP(hipMemcpyAsync(sg.parts, parts.data(), sizeof(int4) * parts.size(), hipMemcpyHostToDevice, st));
    }
    if (n > 0) {
        HG_HIP(hipMemcpyAsync(sg.levels, levels, sizeof(int32_t) * n, hipMemcpyHostToDevice, st));
        HG_HIP(hipMemcpyAsync(sg.l0, l0_adj, sizeof(int32_t) * n * M0, hipMemcpyHostToDevice, st));
        HG_HIP(hipMemcpyAsync(sg.upoff, up_off, sizeof(int64_t) * (n + 1), hipMemcpyHostToDevice, st));
        if (blocks > 0) HG_HIP(hipMemcpyAsync(sg.upadj, up_adj, sizeof(int32_t) * blocks * M, hipMemcpyHostToDevice, st));
    }
    HG_TRY(ensure_qrows(idx, st));  // (of the ROWS: nothing of the graph)
    // host mirrors: built aside as well (an allocation failure throws nothing past here)
    std::vector<int32_t> h_levels, h_l0, h_upadj;
    std::vector<int64_t> h_upoff(1, 0), h_part_off;
    std::vector<int32_t> h_part_entry, h_part_level;
    if (n > 0) {
        h_levels.assign(levels, levels + n);
        h_l0.assign(l0_adj, l0_adj + n * M0);
        h_upoff.assign(up_off, up_off + n + 1);
        if (blocks > 0) h_upadj.assign(up_adj, up_adj + blocks * M);
    }
    if (pt) {
        h_part_off.assign(pt->off, pt->off + pt->nparts + 1);
        for (const int4 &q : parts) {
            h_part_entry.push_back(q.y);
            h_part_level.push_back(q.z);
        }
    }
    // every earlier call on this handle is ordered before `st` by the scope, except the small synchronous searches on
    // the slot streams: once `st` and both slot streams are idle nothing can still be traversing the graph that is about
    // to be freed (and no other handle on this GPU is stalled) -- and the copies above have arrived
    HG_TRY(call.quiesce());
    free_graph(idx);
    idx->d_levels = sg.levels;
    idx->d_l0 = sg.l0;
    idx->d_upoff = sg.upoff;
    idx->d_upadj = sg.upadj;
    idx->d_parts = sg.parts;
    sg = Staged();
    idx->M = M;
    idx->M0 = M0;
    idx->up_blocks = blocks;
    idx->h_levels.swap(h_levels);
    idx->h_l0.swap(h_l0);
    idx->h_upoff.swap(h_upoff);
    idx->h_upadj.swap(h_upadj);
    idx->nparts = pt ? pt->nparts : 0;
    idx->max_part = max_part;
    idx->h_part_off.swap(h_part_off);
    idx->h_part_entry.swap(h_part_entry);
    idx->h_part_level.swap(h_part_level);
    idx->entry = (n > 0 && !pt) ? entry : -1;
    idx->max_level = top;
    idx->has_graph = true;
    return 0;
}

// One forest search of at most kPartsMaxItems items, enqueued on `st` inside the caller's call scope: the item table from the
// probe table, ONE traversal launch over all (query, probe) items + its repeat pass (per item), the counters into the caller's
// layout, the merge in probe order.
constexpr int64_t kPartsMaxItems = 1 << 20;
static int hnsw_parts_enqueue(hnswgpu_index *idx, const float *d_Q, int32_t nq, int32_t k_part, int32_t ef, const int32_t *d_probes,
                              int32_t nprobe, int32_t k, int32_t *d_ids, float *d_dist, int64_t *d_stats, hipStream_t st) {
    const int64_t items = static_cast<int64_t>(nq) * nprobe;
    if (items <= 0) return 0;
    HG_REQUIRE(idx->nparts > 0 && idx->d_parts, HNSWGPU_ESTATE, "the index holds no forest (call hnswgpu_hnsw_build_parts / hnswgpu_set_graph_parts)");
    HnswArgs a;
    fill_args(idx, a);
    a.Q = d_Q;
    a.qld = idx->dim;
    a.nq = static_cast<int32_t>(items);
    a.ef = ef;
    a.k = k_part;
    a.cap = ef + kGhost;
    a.nwords = static_cast<int32_t>((idx->max_part + 31) / 32);
    HG_TRY(idx->s_pt_items.ensure(sizeof(int4) * items));
    HG_TRY(idx->s_pt_ids.ensure(sizeof(int32_t) * items * k_part));
    HG_TRY(idx->s_pt_dist.ensure(sizeof(float) * items * k_part));
    if (d_stats) HG_TRY(idx->s_pt_stats.ensure(sizeof(int64_t) * 2 * items));
    HG_TRY(idx->s_probes.ensure(sizeof(int32_t) * (static_cast<size_t>(items) + 1)));  // again[]: the items to repeat
    a.items = idx->s_pt_items.as<int4>();
    a.out_ids = idx->s_pt_ids.as<int32_t>();
    a.out_dist = idx->s_pt_dist.as<float>();
    a.stats = d_stats ? idx->s_pt_stats.as<int64_t>() : nullptr;
    HnswLaunchPlan p;
    hnsw_calibration_absorb(idx);
    HG_TRY(hnsw_launch_plan(idx, a, nullptr, p));
    const unsigned blocks = static_cast<unsigned>((items + 255) / 256);
    hipLaunchKernelGGL(parts_items_kernel, dim3(blocks), dim3(256), 0, st, d_probes, nq, nprobe, idx->d_parts, idx->nparts,
                       idx->s_pt_items.as<int4>());
    HG_HIP(hipGetLastError());
    int32_t *again_cnt = idx->s_probes.as<int32_t>(), *again = again_cnt + 1;
    HG_HIP(hipMemsetAsync(again_cnt, 0, sizeof(int32_t), st));
    a.again = again;
    a.again_cnt = again_cnt;
    hipEvent_t e0;
    prof_begin(idx, PROF_HNSW, st, &e0);
    int rc = hnsw_launch_planned(idx, p, a, st);
    prof_end(idx, PROF_HNSW, st, e0);
    HG_TRY(rc);
    if (p.repeat_cap) {  // as search_enqueue's: the items that ran out of ghost slots, with the largest list the LDS holds
        a.cap = p.repeat_cap;
        a.again = nullptr;
        a.again_cnt = nullptr;
        a.q_index = again;
        a.nq_dev = again_cnt;
        HnswLaunchPlan r;
        HG_TRY(hnsw_launch_plan(idx, a, &p, r));
        HG_TRY(hnsw_launch_planned(idx, r, a, st));
    }
    if (d_stats) {
        hipLaunchKernelGGL(parts_stats_kernel, dim3(blocks), dim3(256), 0, st, idx->s_pt_stats.as<int64_t>(), nq, nprobe, d_stats);
        HG_HIP(hipGetLastError());
    }
    return hnswgpu_merge_lists_dev(idx->device, idx->s_pt_ids.as<int32_t>(), idx->s_pt_dist.as<float>(), nprobe, nq, k_part, k, d_ids,
                                   d_dist, st);
}

}  // namespace hg

using namespace hg;

extern "C" {

int hnswgpu_set_graph(hnswgpu_index *idx, const int32_t *levels, const int32_t *l0_adj, int32_t M0,
                      const int64_t *up_off, const int32_t *up_adj, int32_t M, int32_t entry, int32_t max_level) {
    HG_TRY(check_graph(idx, levels, l0_adj, M0, up_off, up_adj, M, entry, max_level, nullptr));
    hipStream_t st = idx->stream;
    Call call;
    HG_TRY(call.open(idx, st));
    HG_TRY(install_graph(idx, call, st, levels, l0_adj, M0, up_off, up_adj, M, entry, max_level, nullptr));
    return call.close();
}

int hnswgpu_set_graph_parts(hnswgpu_index *idx, const int32_t *levels, const int32_t *l0_adj, int32_t M0, const int64_t *up_off,
                            const int32_t *up_adj, int32_t M, int32_t nparts, const int64_t *part_off, const int32_t *part_entry,
                            const int32_t *part_max_level) {
    const PartTables pt = {nparts, part_off, part_entry, part_max_level};
    HG_TRY(check_graph(idx, levels, l0_adj, M0, up_off, up_adj, M, -1, 0, &pt));
    hipStream_t st = idx->stream;
    Call call;
    HG_TRY(call.open(idx, st));
    HG_TRY(install_graph(idx, call, st, levels, l0_adj, M0, up_off, up_adj, M, -1, 0, &pt));
    return call.close();
}

int hnswgpu_graph_parts(const hnswgpu_index *idx, int32_t *nparts, int64_t *part_off, int32_t *part_entry, int32_t *part_max_level) {
    HG_REQUIRE(idx, HNSWGPU_EINVAL, "idx is null");
    HG_REQUIRE(idx->has_graph && idx->nparts > 0, HNSWGPU_ESTATE, "the index holds no forest (call hnswgpu_hnsw_build_parts / hnswgpu_set_graph_parts)");
    if (nparts) *nparts = idx->nparts;
    if (part_off) memcpy(part_off, idx->h_part_off.data(), sizeof(int64_t) * idx->h_part_off.size());
    if (part_entry) memcpy(part_entry, idx->h_part_entry.data(), sizeof(int32_t) * idx->h_part_entry.size());
    if (part_max_level) memcpy(part_max_level, idx->h_part_level.data(), sizeof(int32_t) * idx->h_part_level.size());
    return 0;
}

int hnswgpu_graph_sizes(const hnswgpu_index *idx, int32_t *M, int32_t *M0, int64_t *up_blocks, int32_t *entry,
                        int32_t *max_level) {
    HG_REQUIRE(idx, HNSWGPU_EINVAL, "idx is null");
    HG_REQUIRE(idx->has_graph, HNSWGPU_ESTATE, "index has no graph");
    if (M) *M = idx->M;
    if (M0) *M0 = idx->M0;
    if (up_blocks) *up_blocks = idx->up_blocks;
    if (entry) *entry = idx->entry;
    if (max_level) *max_level = idx->max_level;
    return 0;
}

int hnswgpu_get_graph(const hnswgpu_index *idx, int32_t *levels, int32_t *l0_adj, int64_t *up_off,
                      int32_t *up_adj) {
    HG_REQUIRE(idx, HNSWGPU_EINVAL, "idx is null");
    HG_REQUIRE(idx->has_graph, HNSWGPU_ESTATE, "index has no graph");
    if (levels && !idx->h_levels.empty()) memcpy(levels, idx->h_levels.data(), sizeof(int32_t) * idx->h_levels.size());
    if (l0_adj && !idx->h_l0.empty()) memcpy(l0_adj, idx->h_l0.data(), sizeof(int32_t) * idx->h_l0.size());
    if (up_off) memcpy(up_off, idx->h_upoff.data(), sizeof(int64_t) * idx->h_upoff.size());
    if (up_adj && !idx->h_upadj.empty()) memcpy(up_adj, idx->h_upadj.data(), sizeof(int32_t) * idx->h_upadj.size());
    return 0;
}

static int check_hnsw_args(const hnswgpu_index *idx, const void *Q, int32_t nq, int32_t k, int32_t *ef,
                           const void *ids, const void *dist, bool parts = false) {
    HG_REQUIRE(idx, HNSWGPU_EINVAL, "idx is null");
    HG_REQUIRE(nq >= 0 && k >= 1, HNSWGPU_EINVAL, "need nq >= 0 and k >= 1");
    HG_REQUIRE(nq == 0 || (Q && ids && dist), HNSWGPU_EINVAL, "null argument");
    HG_REQUIRE(idx->has_graph, HNSWGPU_ESTATE, "index has no graph (call hnswgpu_hnsw_build / hnswgpu_set_graph)");
    HG_REQUIRE(idx->nparts == 0 || parts, HNSWGPU_ESTATE,
               "the index holds a forest (hnswgpu_set_graph_parts / hnswgpu_hnsw_build_parts): search it with hnswgpu_hnsw_search_parts");
    HG_REQUIRE(idx->nparts > 0 || !parts, HNSWGPU_ESTATE,
               "the index holds no forest (call hnswgpu_hnsw_build_parts / hnswgpu_set_graph_parts)");
    if (*ef <= 0) *ef = k > 50 ? k : 50;  // ef = (max k 50), ultra_fast.clj:355
    if (*ef < k) *ef = k;
    HG_REQUIRE(*ef <= 4096, HNSWGPU_ELIMIT, "ef > 4096 is not supported");
    return 0;
}

static bool zero_copy() { return tune(HNSWGPU_TUNE_ZEROCOPY, 1) != 0; }  // 0 = always stage through copies (A/B measurements)

// Small combined batches (at most one workgroup per CU): the queries are written into a block of mapped pinned host
// memory, the traversal kernel reads them from there and writes ids / distances / counters back into the same block,
// and its last workgroup sets a flag the calling thread spins on.  One kernel launch is the only runtime call on the
// path: no copy, no counter reset, no second launch, no hipStreamSynchronize (measured before: 0.49 ms per
// single-query call for a 0.35 ms kernel).  Two such batches may be in flight (own stream, block and counters each).
static int hnsw_search_batch_slot(hnswgpu_index *idx, const std::vector<hnswgpu_index::SearchReq *> &batch, int32_t total) {
    const int32_t k = batch[0]->k, ef = batch[0]->ef;
    const BatchBlock b(idx->dim, total, k, true);
    std::unique_lock<std::mutex> sl;
    hnswgpu_index::Slot *slot = BatchBlock::acquire_slot(idx, sl);
    HG_TRY(slot_prepare(*slot, b.bytes, idx->device));
    void *hp = slot->h, *dp = slot->d;
    b.pack(hp, batch);
    SlotSignal sig;
    sig.again = slot->d_again;
    sig.done_cnt = slot->d_done;
    sig.host_flag = b.flag(dp);
    sig.host_again = b.again(dp);
    sig.flag_val = ++slot->seq;
    sig.order = slot->d_order;
    sig.dense = &slot->dense;
    uint64_t gen;
    HG_HIP(hipSetDevice(idx->device));
    {
        // the index state is read (and the launch enqueued) under its lock -- a plain one: this path takes no part in hg::Call's
        // event ordering (engine.hpp)
        std::lock_guard<std::mutex> lk(idx->mu);
        HG_REQUIRE(idx->has_graph && idx->n > 0, HNSWGPU_ESTATE, "index has no graph (call hnswgpu_hnsw_build / hnswgpu_set_graph)");
        gen = idx->graph_gen;
        HG_TRY(search_enqueue(idx, b.queries(dp), total, k, ef, b.ids(dp), b.dist(dp), b.stats(dp), slot->st, &sig));
    }
    HG_TRY(slot_wait(*slot, b.flag(hp), sig.flag_val));
    if (*static_cast<volatile int32_t *>(b.again(hp)) != 0) {
        // some query met more tied candidates than the ghost slots hold (hundreds of duplicated rows): the repeat pass --
        // against the graph the first pass ran on, or not at all (set_graph / hnsw_build wait for this slot's stream
        // before they free the old graph, but may have installed a new one since the first pass finished)
        std::lock_guard<std::mutex> lk(idx->mu);
        HG_REQUIRE(idx->has_graph && idx->graph_gen == gen, HNSWGPU_ESTATE,
                   "the graph was replaced while a search on it was in flight");
        HG_TRY(search_enqueue(idx, b.queries(dp), total, k, ef, b.ids(dp), b.dist(dp), b.stats(dp), slot->st, &sig, true));
        HG_HIP(hipStreamSynchronize(slot->st));
    }
    b.scatter(hp, batch);
    return 0;
}

// One launch for a set of queued synchronous requests with the same (k, ef): queries concatenated on the host,
// results scattered back (see hnswgpu_index::SearchReq).
static int hnsw_search_batch(hnswgpu_index *idx, const std::vector<hnswgpu_index::SearchReq *> &batch, int32_t total) {
    // (the mapped-memory slot serves the LDS visited set: the plan's own predicate)
    if (zero_copy() && total <= kZcMaxQueries && !hnsw_vis_global(idx->n, tune(HNSWGPU_TUNE_VIS_GLOBAL, 0)))
        return hnsw_search_batch_slot(idx, batch, total);
    const int32_t k = batch[0]->k, ef = batch[0]->ef;
    hipStream_t st = idx->stream;
    Call call;
    HG_TRY(call.open(idx, st));
    // under the lock: a concurrent set_graph / hnsw_build may have replaced the graph since the caller's argument check
    HG_REQUIRE(idx->has_graph && idx->n > 0, HNSWGPU_ESTATE, "index has no graph (call hnswgpu_hnsw_build / hnswgpu_set_graph)");
    // one pinned staging block, four transfers per batch whatever the number of callers in it.  (Replaying the single-query
    // sequence -- upload, counter reset, two launches, downloads -- as one captured hipGraph was tried and changed nothing:
    // 0.483 ms per call either way, the time is on the device.)
    const BatchBlock b(idx->dim, total, k, true);
    HG_TRY(ensure_pinned(idx, b.bytes));
    void *hp = idx->h_pin;
    b.pack(hp, batch);
    HG_TRY(call.stage_in(b.queries(hp), total, k));
    HG_TRY(idx->s_stats.ensure(sizeof(int64_t) * 2 * total));
    HG_TRY(search_enqueue(idx, idx->s_q.as<float>(), total, k, ef, idx->s_ids.as<int32_t>(), idx->s_outd.as<float>(),
                          idx->s_stats.as<int64_t>(), st));
    HG_HIP(hipMemcpyAsync(b.stats(hp), idx->s_stats.p, sizeof(int64_t) * 2 * total, hipMemcpyDeviceToHost, st));
    HG_TRY(call.stage_out(b.ids(hp), b.dist(hp), static_cast<int64_t>(total) * k));
    b.scatter(hp, batch);
    return call.close();
}

int hnswgpu_hnsw_search_dev(hnswgpu_index *idx, const float *d_Q, int32_t nq, int32_t k, int32_t ef,
                            int32_t *d_out_ids, float *d_out_dist, int64_t *d_stats, void *stream) {
    HG_TRY(check_hnsw_args(idx, d_Q, nq, k, &ef, d_out_ids, d_out_dist));
    if (nq == 0) return 0;
    HG_REQUIRE(idx->n > 0, HNSWGPU_ESTATE, "empty index: use the host entry point");
    hipStream_t st = static_cast<hipStream_t>(stream);
    Call call;
    HG_TRY(call.open(idx, st));
    HG_TRY(search_enqueue(idx, d_Q, nq, k, ef, d_out_ids, d_out_dist, d_stats, st));
    return call.close();
}

int hnswgpu_hnsw_search(hnswgpu_index *idx, const float *Q, int32_t nq, int32_t k, int32_t ef, int32_t *out_ids,
                        float *out_dist, int64_t *stats) {
    HG_TRY(check_hnsw_args(idx, Q, nq, k, &ef, out_ids, out_dist));
    if (nq == 0) return 0;
    int64_t cnt = static_cast<int64_t>(nq) * k;
    if (idx->n == 0) {  // (if (or (nil? entry-point) (zero? size)) [] ...), ultra_fast.clj:349-351
        fill_empty(out_ids, out_dist, cnt);
        if (stats) memset(stats, 0, sizeof(int64_t) * 2 * nq);
        return 0;
    }
    // queue the request; whoever finds no leader becomes one and serves the queue, batch by batch
    hnswgpu_index::SearchReq me;
    me.Q = Q;
    me.nq = nq;
    me.k = k;
    me.ef = ef;
    me.out_ids = out_ids;
    me.out_dist = out_dist;
    me.stats = stats;
    return combine_search(
        idx->cmb_hnsw, me,
        [](const hnswgpu_index::SearchReq *first, const hnswgpu_index::SearchReq *r, int64_t total) {
            return r->k == first->k && r->ef == first->ef && total + r->nq <= 16384;  // one traversal arithmetic: any mix
        },
        [idx](const std::vector<hnswgpu_index::SearchReq *> &batch, int32_t total) {
            return hnsw_search_batch(idx, batch, total);
        });
}

// the argument check of both forest search entries; nprobe: the caller's, or the number of parts without a probe table
static int check_parts_args(const hnswgpu_index *idx, const void *Q, int32_t nq, int32_t k_part, int32_t *ef, const void *probes,
                            int32_t *nprobe, int32_t k, const void *ids, const void *dist) {
    HG_TRY(check_hnsw_args(idx, Q, nq, k_part, ef, ids, dist, true));
    HG_REQUIRE(k >= 1, HNSWGPU_EINVAL, "need k >= 1");
    HG_REQUIRE(k <= 1024, HNSWGPU_ELIMIT, "k > 1024 is not supported");
    if (!probes) *nprobe = idx->nparts;
    HG_REQUIRE(*nprobe >= 1, HNSWGPU_EINVAL, "need nprobe >= 1");
    HG_REQUIRE(static_cast<int64_t>(*nprobe) * k_part < 2147483647LL && *nprobe <= kPartsMaxItems, HNSWGPU_ELIMIT,
               "nprobe * k_part too large");
    return 0;
}

// The reference's two indexes of many small graphs (partitioned_hnsw.clj:149-196, ivf_hnsw.clj:286-325) on one handle and in one
// traversal launch: item (q, r) is hnswgpu_hnsw_search(k_part, ef) of query q on a handle over the rows of part probes[q][r] alone
// -- ids (handle rows), distance bits and counters --, the result hnswgpu_merge_lists_dev of a query's items in probe order.
int hnswgpu_hnsw_search_parts_dev(hnswgpu_index *idx, const float *d_Q, int32_t nq, int32_t k_part, int32_t ef, const int32_t *d_probes,
                                  int32_t nprobe, int32_t k, int32_t *d_out_ids, float *d_out_dist, int64_t *d_stats, void *stream) {
    HG_TRY(check_parts_args(idx, d_Q, nq, k_part, &ef, d_probes, &nprobe, k, d_out_ids, d_out_dist));
    if (nq == 0) return 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    Call call;
    HG_TRY(call.open(idx, st));
    HG_REQUIRE(idx->nparts > 0 && (d_probes || nprobe == idx->nparts), HNSWGPU_ESTATE, "the forest was replaced while the call was on its way");
    const int32_t step = static_cast<int32_t>(std::max<int64_t>(1, kPartsMaxItems / nprobe));
    for (int32_t q0 = 0; q0 < nq; q0 += step) {
        const int32_t m = std::min(step, nq - q0);
        HG_TRY(hnsw_parts_enqueue(idx, d_Q + static_cast<int64_t>(q0) * idx->dim, m, k_part, ef,
                                  d_probes ? d_probes + static_cast<int64_t>(q0) * nprobe : nullptr, nprobe, k,
                                  d_out_ids + static_cast<int64_t>(q0) * k, d_out_dist + static_cast<int64_t>(q0) * k,
                                  d_stats ? d_stats + 2 * static_cast<int64_t>(q0) * nprobe : nullptr, st));
    }
    return call.close();
}

// One caller's staged batch (probe tables differ between callers: no part in the call combiner or the mapped-memory slots), in
// slices of at most kPartsMaxItems items.
int hnswgpu_hnsw_search_parts(hnswgpu_index *idx, const float *Q, int32_t nq, int32_t k_part, int32_t ef, const int32_t *probes,
                              int32_t nprobe, int32_t k, int32_t *out_ids, float *out_dist, int64_t *stats) {
    HG_TRY(check_parts_args(idx, Q, nq, k_part, &ef, probes, &nprobe, k, out_ids, out_dist));
    if (nq == 0) return 0;
    hipStream_t st = idx->stream;
    Call call;
    HG_TRY(call.open(idx, st));
    HG_REQUIRE(idx->nparts > 0 && (probes || nprobe == idx->nparts), HNSWGPU_ESTATE, "the forest was replaced while the call was on its way");
    const int32_t step = static_cast<int32_t>(std::max<int64_t>(1, kPartsMaxItems / nprobe));
    for (int32_t q0 = 0; q0 < nq; q0 += step) {
        const int32_t m = std::min(step, nq - q0);
        const int64_t items = static_cast<int64_t>(m) * nprobe;
        HG_TRY(call.stage_in(Q + static_cast<int64_t>(q0) * idx->dim, m, k));
        int32_t *d_probes = nullptr;
        if (probes) {
            HG_TRY(idx->s_pt_probes.ensure(sizeof(int32_t) * items));
            d_probes = idx->s_pt_probes.as<int32_t>();
            HG_HIP(hipMemcpyAsync(d_probes, probes + static_cast<int64_t>(q0) * nprobe, sizeof(int32_t) * items, hipMemcpyHostToDevice, st));
        }
        int64_t *d_stats = nullptr;
        if (stats) {
            HG_TRY(idx->s_stats.ensure(sizeof(int64_t) * 2 * items));
            d_stats = idx->s_stats.as<int64_t>();
        }
        HG_TRY(hnsw_parts_enqueue(idx, idx->s_q.as<float>(), m, k_part, ef, d_probes, nprobe, k, idx->s_ids.as<int32_t>(),
                                  idx->s_outd.as<float>(), d_stats, st));
        if (stats)
            HG_HIP(hipMemcpyAsync(stats + 2 * static_cast<int64_t>(q0) * nprobe, d_stats, sizeof(int64_t) * 2 * items, hipMemcpyDeviceToHost, st));
        HG_TRY(call.stage_out(out_ids + static_cast<int64_t>(q0) * k, out_dist + static_cast<int64_t>(q0) * k, static_cast<int64_t>(m) * k));
    }
    return call.close();
}

int hnswgpu_hnsw_last_order(hnswgpu_index *idx, int32_t *order, int32_t *keys, int32_t cap, int32_t *nq) {
    HG_REQUIRE(idx && nq && cap >= 0, HNSWGPU_EINVAL, "need idx, nq and cap >= 0");
    std::lock_guard<std::mutex> lk(idx->mu);
    *nq = idx->hnsw_order_last ? idx->hnsw_order_nq : 0;
    const size_t m = static_cast<size_t>(std::min(cap, *nq));
    if (m == 0 || (!order && !keys)) return 0;
    HG_HIP(hipSetDevice(idx->device));
    HG_HIP(hipDeviceSynchronize());  // whichever stream the launch ran on
    if (order) HG_HIP(hipMemcpy(order, idx->hnsw_order_last, sizeof(int32_t) * m, hipMemcpyDeviceToHost));
    if (keys) HG_HIP(hipMemcpy(keys, idx->hnsw_order_last + *nq, sizeof(int32_t) * m, hipMemcpyDeviceToHost));
    return 0;
}

// The dense bounds table (dense_kernels.hpp) per handle: the rule's switch and budget, what it has done, and the table itself
int hnswgpu_set_hnsw_dense_bounds(hnswgpu_index *idx, int32_t mode, int64_t budget_mb) {
    HG_REQUIRE(idx, HNSWGPU_EINVAL, "idx is null");
    HG_REQUIRE(mode >= 0 && mode <= 2, HNSWGPU_EINVAL, "mode must be 0 (never), 1 (the rule) or 2 (every eligible launch)");
    HG_REQUIRE(budget_mb < (1LL << 40), HNSWGPU_EINVAL, "budget_mb out of range");
    std::lock_guard<std::mutex> lk(idx->mu);
    idx->dense_mode = mode;
    if (budget_mb >= 0) idx->dense_budget = static_cast<size_t>(budget_mb) << 20;
    return 0;
}

int hnswgpu_hnsw_dense_bounds_state(hnswgpu_index *idx, int32_t *mode, int64_t *budget_mb, int64_t *launches, int64_t *bytes) {
    HG_REQUIRE(idx, HNSWGPU_EINVAL, "idx is null");
    std::lock_guard<std::mutex> lk(idx->mu);
    if (mode) *mode = idx->dense_mode;
    if (budget_mb) *budget_mb = static_cast<int64_t>(idx->dense_budget >> 20);
    if (launches) *launches = idx->dense_launches;
    if (bytes) {
        size_t b = idx->s_dense.codes.cap + idx->s_dense.lb.cap;
        for (auto &sl : idx->slots) b += sl.dense.codes.cap + sl.dense.lb.cap;
        *bytes = static_cast<int64_t>(b);
    }
    return 0;
}

int hnswgpu_hnsw_dense_rows(hnswgpu_index *idx, int32_t rows, int32_t *rows_set, int64_t *launches_four) {
    HG_REQUIRE(idx, HNSWGPU_EINVAL, "idx is null");
    HG_REQUIRE(rows < 0 || rows == 0 || rows == 2 || rows == 4, HNSWGPU_EINVAL, "rows must be 0 (the rule), 2 or 4 (negative: unchanged)");
    std::lock_guard<std::mutex> lk(idx->mu);
    if (rows >= 0) idx->dense_rows_mode = rows;
    if (rows_set) *rows_set = idx->dense_rows_mode;
    if (launches_four) *launches_four = idx->dense_rows4_launches;
    return 0;
}

int hnswgpu_hnsw_dense_bounds(hnswgpu_index *idx, const float *Q, int32_t nq, int64_t qld, float *out) {
    HG_REQUIRE(idx && Q && out && nq >= 1, HNSWGPU_EINVAL, "null argument");
    HG_REQUIRE(qld >= idx->dim, HNSWGPU_EINVAL, "qld is smaller than the dimension");
    hipStream_t st = idx->stream;
    Call call;
    HG_TRY(call.open(idx, st));
    HG_REQUIRE(idx->n > 0, HNSWGPU_ESTATE, "empty index");
    HG_TRY(ensure_qrows(idx, st));
    HG_REQUIRE(idx->d_qrows, HNSWGPU_EINVAL,
               "this handle has no int8 rows (hnswgpu_set_rejection_test: mode 0, or mode 1 with dim < 128)");
    const size_t qfloats = static_cast<size_t>(nq - 1) * static_cast<size_t>(qld) + idx->dim;
    HG_TRY(idx->s_q.ensure(sizeof(float) * qfloats));
    HG_HIP(hipMemcpyAsync(idx->s_q.p, Q, sizeof(float) * qfloats, hipMemcpyHostToDevice, st));
    const int64_t lb_ld = hnsw_dense_ld(idx->n);
    DenseScratch &ds = idx->s_dense;
    HG_TRY(ds.codes.ensure(hnsw_dense_code_bytes(idx->nch, nq) + sizeof(QueryScal) * static_cast<size_t>(nq)));
    HG_TRY(ds.lb.ensure(sizeof(float) * static_cast<size_t>(nq) * static_cast<size_t>(lb_ld)));
    HG_TRY(launch_hnsw_dense(idx, idx->s_q.as<float>(), qld, nq, ds.codes.p, ds.lb.as<float>(), lb_ld, st));
    HG_HIP(hipMemcpy2DAsync(out, sizeof(float) * idx->n, ds.lb.p, sizeof(float) * lb_ld, sizeof(float) * idx->n, nq, hipMemcpyDeviceToHost, st));
    HG_TRY(call.sync());
    return call.close();
}

// Filtered search (api/protocol.clj:34-41,97-102): the unfiltered traversal at ef for kk = min(ef, 1024) results per query
// into s_fids / s_fdist, then the first k passing entries of every list (filter_kernels.hpp: filter_take_kernel).
// The take reads query q's mask at d_allow + q * W (Each), or the call's one mask (Single).
static int hnsw_filtered_enqueue(hnswgpu_index *idx, MaskForm form, const float *d_Q, int32_t nq, int32_t k, int32_t ef,
                                 const uint32_t *d_allow, int32_t *d_ids, float *d_dist, int64_t *d_stats, hipStream_t st) {
    const int32_t kk = ef < 1024 ? ef : 1024;
    const size_t cnt = static_cast<size_t>(nq) * kk;
    HG_TRY(idx->s_fids.ensure(sizeof(int32_t) * cnt));
    HG_TRY(idx->s_fdist.ensure(sizeof(float) * cnt));
    HG_TRY(search_enqueue(idx, d_Q, nq, kk, ef, idx->s_fids.as<int32_t>(), idx->s_fdist.as<float>(), d_stats, st, nullptr, false, true));
    return launch_filter_take(idx->s_fids.as<int32_t>(), idx->s_fdist.as<float>(), nq, kk, k, d_allow, idx->n, d_ids, d_dist, st,
                              form == MaskForm::Each ? (idx->n + 31) / 32 : 0);
}

// The two entry points of the filtered traversal, one body each for both forms of the mask.
static int hnsw_filtered_dev(hnswgpu_index *idx, MaskForm form, const float *d_Q, int32_t nq, int32_t k, int32_t ef,
                             const uint32_t *d_allow, int32_t *d_out_ids, float *d_out_dist, int64_t *d_stats, void *stream) {
    HG_TRY(check_hnsw_args(idx, d_Q, nq, k, &ef, d_out_ids, d_out_dist));
    HG_REQUIRE(d_allow, HNSWGPU_EINVAL, "allow is null");
    if (nq == 0) return 0;
    HG_REQUIRE(idx->n > 0, HNSWGPU_ESTATE, "empty index: use the host entry point");
    hipStream_t st = static_cast<hipStream_t>(stream);
    Call call;
    HG_TRY(call.open(idx, st));
    HG_TRY(hnsw_filtered_enqueue(idx, form, d_Q, nq, k, ef, d_allow, d_out_ids, d_out_dist, d_stats, st));
    return call.close();
}

// One caller's staged batch: masks differ between callers, so this entry takes no part in the call combiner.
static int hnsw_filtered_host(hnswgpu_index *idx, MaskForm form, const float *Q, int32_t nq, int32_t k, int32_t ef,
                              const uint32_t *allow, int32_t *out_ids, float *out_dist, int64_t *stats) {
    HG_TRY(check_hnsw_args(idx, Q, nq, k, &ef, out_ids, out_dist));
    HG_REQUIRE(allow, HNSWGPU_EINVAL, "allow is null");
    if (nq == 0) return 0;
    const int64_t cnt = static_cast<int64_t>(nq) * k;
    if (idx->n == 0) {
        fill_empty(out_ids, out_dist, cnt);
        if (stats) memset(stats, 0, sizeof(int64_t) * 2 * nq);
        return 0;
    }
    hipStream_t st = idx->stream;
    Call call;
    HG_TRY(call.open(idx, st));
    // under the lock: a concurrent set_graph / hnsw_build may have replaced the graph since the argument check
    HG_REQUIRE(idx->has_graph && idx->n > 0, HNSWGPU_ESTATE, "index has no graph (call hnswgpu_hnsw_build / hnswgpu_set_graph)");
    HG_TRY(call.stage_in(Q, nq, k));
    HG_TRY(call.stage_mask(allow, form, nq));
    int64_t *d_stats = nullptr;
    if (stats) {
        HG_TRY(idx->s_stats.ensure(sizeof(int64_t) * 2 * nq));
        d_stats = idx->s_stats.as<int64_t>();
    }
    HG_TRY(hnsw_filtered_enqueue(idx, form, idx->s_q.as<float>(), nq, k, ef, idx->s_fmask.as<uint32_t>(), idx->s_ids.as<int32_t>(),
                                 idx->s_outd.as<float>(), d_stats, st));
    if (stats) HG_HIP(hipMemcpyAsync(stats, d_stats, sizeof(int64_t) * 2 * nq, hipMemcpyDeviceToHost, st));
    HG_TRY(call.stage_out(out_ids, out_dist, cnt));
    return call.close();
}

int hnswgpu_hnsw_search_filtered_dev(hnswgpu_index *idx, const float *d_Q, int32_t nq, int32_t k, int32_t ef,
                                     const uint32_t *d_allow, int32_t *d_out_ids, float *d_out_dist, int64_t *d_stats,
                                     void *stream) {
    return hnsw_filtered_dev(idx, MaskForm::Single, d_Q, nq, k, ef, d_allow, d_out_ids, d_out_dist, d_stats, stream);
}
int hnswgpu_hnsw_search_filtered(hnswgpu_index *idx, const float *Q, int32_t nq, int32_t k, int32_t ef, const uint32_t *allow,
                                 int32_t *out_ids, float *out_dist, int64_t *stats) {
    return hnsw_filtered_host(idx, MaskForm::Single, Q, nq, k, ef, allow, out_ids, out_dist, stats);
}
// One mask per query (include/hnswgpu.h): the same traversal and take; the take reads allow_each + q * W.
int hnswgpu_hnsw_search_filtered_each_dev(hnswgpu_index *idx, const float *d_Q, int32_t nq, int32_t k, int32_t ef,
                                          const uint32_t *d_allow_each, int32_t *d_out_ids, float *d_out_dist,
                                          int64_t *d_stats, void *stream) {
    return hnsw_filtered_dev(idx, MaskForm::Each, d_Q, nq, k, ef, d_allow_each, d_out_ids, d_out_dist, d_stats, stream);
}
int hnswgpu_hnsw_search_filtered_each(hnswgpu_index *idx, const float *Q, int32_t nq, int32_t k, int32_t ef,
                                      const uint32_t *allow_each, int32_t *out_ids, float *out_dist, int64_t *stats) {
    return hnsw_filtered_host(idx, MaskForm::Each, Q, nq, k, ef, allow_each, out_ids, out_dist, stats);
}

}  // extern "C"

namespace hg {

// Distances of the edges of `nlists` adjacency lists (list t belongs to node owner[t], `width` slots, -1 padded), by the
// traversal's own arithmetic: d(node, neighbour) carries the bits the build-mode search reported for that edge (the lane
// sums are symmetric in their two operands).  One wave per list.  insert-single prunes an over-full list by the stored
// edge distances (ultra_fast.clj:279-299); a graph that arrives through hnswgpu_set_graph / hnswgpu_load has none.
template <int NCH, int RB, bool L2>
__global__ __launch_bounds__(kWG) void edge_dist_kernel(const float *rows, const float *norms, int64_t ld, int dim, int metric,
                                                        const int32_t *owner, const int32_t *adj, int width, int64_t nlists,
                                                        float *out) {
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t t = static_cast<int64_t>(blockIdx.x) * kNWave + (threadIdx.x >> 6);
    if (t >= nlists) return;
    const int64_t node = owner ? owner[t] : t;
    const int nvec = static_cast<int>(ld / 4);
    float4 q[NCH];
    load_row<NCH>(q, rows + node * ld, nvec, lane, true);
    const float qn = metric == METRIC_COS ? norms[node] : 0.0f;
    for (int j0 = 0; j0 < width; j0 += RB) {
        float4 r[RB][NCH];
        int32_t nb[RB];
#pragma unroll
        for (int b = 0; b < RB; b++) {
            nb[b] = j0 + b < width ? adj[t * width + j0 + b] : -1;
            load_row<NCH>(r[b], rows + static_cast<int64_t>(nb[b] >= 0 ? nb[b] : 0) * ld, nvec, lane, nb[b] >= 0);
        }
#pragma unroll
        for (int b = 0; b < RB; b++) {
            const float sum = wave_sum(lane_partial<NCH, L2>(q, r[b]));
            if (lane == 0 && j0 + b < width)
                out[t * width + j0 + b] = nb[b] >= 0 ? finish_dist(metric, sum, qn, metric == METRIC_COS ? norms[nb[b]] : 0.0f) : 0.0f;
        }
    }
}

static int launch_edge_dist(hnswgpu_index *idx, const int32_t *d_owner, const int32_t *d_adj, int width, int64_t nlists,
                            float *d_out, hipStream_t st) {
    if (nlists <= 0) return 0;
    const unsigned grid = static_cast<unsigned>((nlists + kNWave - 1) / kNWave);
    const bool l2 = idx->metric == METRIC_L2;
#define CALL(N, R, L)                                                                                                  \
    hipLaunchKernelGGL((edge_dist_kernel<N, R, L>), dim3(grid), dim3(kWG), 0, st, idx->d_base, idx->d_norms, idx->ld, idx->dim, \
                       idx->metric, d_owner, d_adj, width, nlists, d_out)
    HG_DISPATCH(idx->nch, l2, CALL);
#undef CALL
    HG_HIP(hipGetLastError());
    return 0;
}

// RAII for the builder's own device buffers
struct OwnedBuf : DevBuf {
    ~OwnedBuf() { release(); }
};

static int launch_heur(hnswgpu_index *idx, HeurArgs a, hipStream_t st) {
    if (a.ntasks <= 0) return 0;
    a.rows = idx->d_base;
    a.row_norms = idx->d_norms;
    a.ld = idx->ld;
    a.dim = idx->dim;
    a.metric = idx->metric;
    a.keep_rows = tune(HNSWGPU_TUNE_BUILD_KEEP_ROWS, 1) != 0 ? 1 : 0;
    const bool l2 = idx->metric == METRIC_L2;
#define CALL(N, R, L) hipLaunchKernelGGL((heuristic_select_kernel<N, R, L>), dim3(a.ntasks), dim3(kWG), 0, st, a)
    HG_DISPATCH(idx->nch, l2, CALL);
#undef CALL
    HG_HIP(hipGetLastError());
    return 0;
}

// d(u, c) over the tasks' candidate ranges (hnsw_remove_kernels.hpp): edge_dist_kernel's arithmetic and dispatch
static int launch_remove_dist(hnswgpu_index *idx, const HnswRemoveArgs &a, hipStream_t st) {
    if (a.ntasks <= 0) return 0;
    const unsigned grid = static_cast<unsigned>((a.ntasks + kNWave - 1) / kNWave);
    const bool l2 = idx->metric == METRIC_L2;
#define CALL(N, R, L) \
    hipLaunchKernelGGL((hnsw_remove_dist_kernel<N, R, L>), dim3(grid), dim3(kWG), 0, st, a, idx->d_base, idx->d_norms, idx->dim, idx->metric)
    HG_DISPATCH(idx->nch, l2, CALL);
#undef CALL
    HG_HIP(hipGetLastError());
    return 0;
}

// The scratch of a list repair (hnswgpu_hnsw_remove, hnswgpu_hnsw_update) in s_misc, 16-byte sections: [gate | keep | cnt] zeroed,
// [owner] -1, then word_rank, the call's ids (uploaded from `rows`), the task tables.  a.r.n0 / m / W, a.blocks0 and a.nlists are set.
static int hnsw_repair_scratch(hnswgpu_index *idx, HnswRemoveArgs &a, const int32_t *rows, hipStream_t st) {
    auto sect = [](size_t bytes) { return (bytes + 15) / 16 * 16; };
    const size_t o_keep = sect(sizeof(int64_t) * kLshRemoveGate), o_cnt = o_keep + sect(sizeof(uint32_t) * a.r.W),
                 o_owner = o_cnt + sect(sizeof(uint32_t) * a.nlists), o_rank = o_owner + sect(sizeof(int32_t) * a.blocks0),
                 o_ids = o_rank + sect(sizeof(uint32_t) * a.r.W), o_tlist = o_ids + sect(sizeof(int32_t) * a.r.m),
                 o_tm = o_tlist + sect(sizeof(int32_t) * a.nlists), o_toff = o_tm + sect(sizeof(int32_t) * a.nlists),
                 bytes = o_toff + sect(sizeof(int64_t) * (a.nlists + 1));
    HG_TRY(idx->s_misc.ensure(bytes));
    char *s = idx->s_misc.as<char>();
    HG_HIP(hipMemsetAsync(s, 0, o_owner, st));
    if (a.blocks0 > 0) HG_HIP(hipMemsetAsync(s + o_owner, 0xff, sizeof(int32_t) * a.blocks0, st));
    HG_HIP(hipMemcpyAsync(s + o_ids, rows, sizeof(int32_t) * static_cast<size_t>(a.r.m), hipMemcpyHostToDevice, st));
    a.r.gate = reinterpret_cast<int64_t *>(s);
    a.r.keep = reinterpret_cast<uint32_t *>(s + o_keep);
    a.cnt = reinterpret_cast<uint32_t *>(s + o_cnt);
    a.owner = reinterpret_cast<int32_t *>(s + o_owner);
    a.r.word_rank = reinterpret_cast<uint32_t *>(s + o_rank);
    a.r.rows = reinterpret_cast<const int32_t *>(s + o_ids);
    a.task_list = reinterpret_cast<int32_t *>(s + o_tlist);
    a.task_m = reinterpret_cast<int32_t *>(s + o_tm);
    a.task_off = reinterpret_cast<int64_t *>(s + o_toff);
    return 0;
}

// The graph side of a list repair behind the mask and its rank scan: the owners of the upper blocks, the list pass, the scan of
// the candidate counts -- its two totals are read back to size the candidate arrays (no cap to overflow) -- then gather,
// distances over the handle's present rows (the candidates are old ids), the per-task sort, the selection of the handle's
// builder and the scatter.  RENUM: hnsw_remove_kernels.hpp.  a.ntasks / a.ncand are set on return.
template <bool RENUM>
static int hnsw_repair_chain(hnswgpu_index *idx, HnswRemoveArgs &a, hipStream_t st) {
    auto sect = [](size_t bytes) { return (bytes + 15) / 16 * 16; };
    const int M0 = a.M0;
    const unsigned list_wgs = static_cast<unsigned>((a.nlists + kNWave - 1) / kNWave);
    hipLaunchKernelGGL(hnsw_remove_owner_kernel, dim3(static_cast<unsigned>((a.r.n0 + kWG - 1) / kWG)), dim3(kWG), 0, st, a);
    hipLaunchKernelGGL(hnsw_remove_lists_kernel<RENUM>, dim3(list_wgs), dim3(kWG), 0, st, a);
    hipLaunchKernelGGL(hnsw_remove_scan_kernel, dim3(1), dim3(kWG), 0, st, a);
    HG_HIP(hipGetLastError());
    int64_t totals[2] = {0, 0};
    HG_HIP(hipMemcpyAsync(totals, a.r.gate + kHnswRemoveGateCand, sizeof(totals), hipMemcpyDeviceToHost, st));
    HG_HIP(hipStreamSynchronize(st));
    a.ncand = totals[0];
    a.ntasks = totals[1];
    HG_REQUIRE(a.ntasks >= 0 && a.ntasks <= a.nlists && a.ncand >= a.ntasks &&
                   a.ncand <= a.ntasks * static_cast<int64_t>(kSelMaxCand) && a.ntasks < 2147483647LL,
               HNSWGPU_EHIP, "the candidate scan counts %lld candidates of %lld lists", (long long)a.ncand, (long long)a.ntasks);
    if (a.ntasks == 0) return 0;
    const bool heuristic = (idx->build_flags & HNSWGPU_BUILD_HEURISTIC) != 0;
    HG_TRY(idx->s_ids.ensure(sizeof(int32_t) * static_cast<size_t>(a.ncand)));
    HG_TRY(idx->s_outd.ensure(sizeof(float) * static_cast<size_t>(a.ncand)));
    a.cand_id = idx->s_ids.as<int32_t>();
    a.cand_d = idx->s_outd.as<float>();
    const unsigned task_wgs = static_cast<unsigned>((a.ntasks + kNWave - 1) / kNWave);
    hipLaunchKernelGGL(hnsw_remove_gather_kernel, dim3(task_wgs), dim3(kWG), 0, st, a);
    HG_HIP(hipGetLastError());
    HG_TRY(launch_remove_dist(idx, a, st));  // (the handle still holds the old rows: the candidates are old ids)
    hipLaunchKernelGGL(hnsw_remove_sort_kernel, dim3(static_cast<unsigned>(a.ntasks)), dim3(kWG), 0, st, a);
    HG_HIP(hipGetLastError());
    if (heuristic) {
        const size_t slots = static_cast<size_t>(a.ntasks) * M0;
        const size_t o_d = sect(sizeof(int32_t) * slots), o_c = o_d + sect(sizeof(float) * slots);
        HG_TRY(idx->s_misc2.ensure(o_c + sect(sizeof(int32_t) * static_cast<size_t>(a.ntasks))));
        char *h = idx->s_misc2.as<char>();
        HeurArgs ha;
        memset(&ha, 0, sizeof(ha));
        ha.ntasks = static_cast<int32_t>(a.ntasks);
        ha.off = a.task_off;
        ha.cand_id = a.cand_id;
        ha.cand_d = a.cand_d;
        ha.m = a.task_m;
        ha.extend = 0;
        ha.out_stride = M0;
        ha.out_id = reinterpret_cast<int32_t *>(h);
        ha.out_d = reinterpret_cast<float *>(h + o_d);
        ha.out_cnt = reinterpret_cast<int32_t *>(h + o_c);
        HG_TRY(launch_heur(idx, ha, st));
        a.sel = ha.out_id;
    }
    hipLaunchKernelGGL(hnsw_remove_scatter_kernel<RENUM>, dim3(task_wgs), dim3(kWG), 0, st, a);
    HG_HIP(hipGetLastError());
    return 0;
}

// A pending reverse edge of graph.clj's builder: `id` wants into the FULL list of `target` on layer `lc`.
struct PendingEdge {
    int32_t target, lc, id;
    float dist;
    int64_t seq;  // position in the batch's sequential order of reverse edges
};

// The re-selection of the over-full lists of one batch (prune-connections, graph.clj:208-232): per (target, layer) the
// candidates are its m present edges plus the pending ones, ascending by (distance, id); heuristic_select_kernel keeps
// at most m of them (extend-candidates? false); with `sym` every dropped edge leaves the other node's list as well
// (:226-231).  Batched: every task sees the lists as they stood when the batch's appends were done (the batched build's
// own semantics); `seq_exact` (one insert per batch, the reference's order): a task whose list an earlier task of the
// same insert has shortened is selected again from the list as it then stands -- the sequential loop's result.
struct Pruner {
    hnswgpu_index *idx;
    HostGraph &g;
    hipStream_t st;
    bool sym, seq_exact;
    OwnedBuf d_task, d_out;
    std::vector<int64_t> off;
    std::vector<int32_t> cid, tm, oid, ocnt;
    std::vector<float> cd, od;
    struct Task {
        int32_t target, lc;
        int64_t first;  // its pending edges: pend[first, first + npend)
        int32_t npend;
    };
    std::vector<Task> tasks;
    int64_t n_tasks = 0, n_removed = 0;

    Pruner(hnswgpu_index *i, HostGraph &gr, hipStream_t s, bool sy, bool sq) : idx(i), g(gr), st(s), sym(sy), seq_exact(sq) {}

    // candidates of task t from the CURRENT list + its pending edges, ascending by (distance, id)
    void gather(const Task &t, const std::vector<PendingEdge> &pend, std::vector<std::pair<float, int32_t>> &c) {
        float *d;
        int32_t *cnt;
        int m;
        int32_t *a = g.adj(t.target, t.lc, &d, &cnt, &m);
        c.clear();
        for (int i = 0; i < *cnt; i++) c.emplace_back(d[i], a[i]);
        for (int i = 0; i < t.npend; i++) c.emplace_back(pend[t.first + i].dist, pend[t.first + i].id);
        std::sort(c.begin(), c.end());
        if (c.size() > static_cast<size_t>(kSelMaxCand)) c.resize(kSelMaxCand);
    }

    int select(const std::vector<std::vector<std::pair<float, int32_t>>> &cands, const std::vector<int32_t> &ms) {
        const int nt = static_cast<int>(cands.size());
        off.assign(nt + 1, 0);
        for (int i = 0; i < nt; i++) off[i + 1] = off[i] + static_cast<int64_t>(cands[i].size());
        const int64_t tot = off[nt];
        cid.resize(std::max<int64_t>(tot, 1));
        cd.resize(std::max<int64_t>(tot, 1));
        for (int i = 0; i < nt; i++)
            for (size_t j = 0; j < cands[i].size(); j++) {
                cid[off[i] + j] = cands[i][j].second;
                cd[off[i] + j] = cands[i][j].first;
            }
        return select_flat(nt, ms);
    }

    // off / cid / cd hold `nt` tasks; ms their m.  Results in oid / od / ocnt (stride M0).
    int select_flat(int nt, const std::vector<int32_t> &ms) {
        const int64_t tot = off[nt];
        const int stride = g.M0;
        const size_t b_off = sizeof(int64_t) * (nt + 1), b_id = sizeof(int32_t) * tot, b_d = sizeof(float) * tot, b_m = sizeof(int32_t) * nt;
        HG_TRY(d_task.ensure(b_off + b_id + b_d + b_m + 64));
        char *dp = static_cast<char *>(d_task.p);
        HG_HIP(hipMemcpyAsync(dp, off.data(), b_off, hipMemcpyHostToDevice, st));
        HG_HIP(hipMemcpyAsync(dp + b_off, cid.data(), b_id, hipMemcpyHostToDevice, st));
        HG_HIP(hipMemcpyAsync(dp + b_off + b_id, cd.data(), b_d, hipMemcpyHostToDevice, st));
        HG_HIP(hipMemcpyAsync(dp + b_off + b_id + b_d, ms.data(), b_m, hipMemcpyHostToDevice, st));
        const size_t o_id = sizeof(int32_t) * static_cast<size_t>(nt) * stride, o_d = sizeof(float) * static_cast<size_t>(nt) * stride,
                     o_c = sizeof(int32_t) * nt;
        HG_TRY(d_out.ensure(o_id + o_d + o_c + 64));
        char *op = static_cast<char *>(d_out.p);
        HeurArgs a;
        memset(&a, 0, sizeof(a));
        a.ntasks = nt;
        a.off = reinterpret_cast<const int64_t *>(dp);
        a.cand_id = reinterpret_cast<const int32_t *>(dp + b_off);
        a.cand_d = reinterpret_cast<const float *>(dp + b_off + b_id);
        a.m = reinterpret_cast<const int32_t *>(dp + b_off + b_id + b_d);
        a.extend = 0;  // prune-connections passes extend-candidates? false (graph.clj:222)
        a.out_stride = stride;
        a.out_id = reinterpret_cast<int32_t *>(op);
        a.out_d = reinterpret_cast<float *>(op + o_id);
        a.out_cnt = reinterpret_cast<int32_t *>(op + o_id + o_d);
        HG_TRY(launch_heur(idx, a, st));
        oid.resize(static_cast<size_t>(nt) * stride);
        od.resize(static_cast<size_t>(nt) * stride);
        ocnt.resize(nt);
        HG_HIP(hipMemcpyAsync(oid.data(), a.out_id, o_id, hipMemcpyDeviceToHost, st));
        HG_HIP(hipMemcpyAsync(od.data(), a.out_d, o_d, hipMemcpyDeviceToHost, st));
        HG_HIP(hipMemcpyAsync(ocnt.data(), a.out_cnt, o_c, hipMemcpyDeviceToHost, st));
        HG_HIP(hipStreamSynchronize(st));
        return 0;
    }

    // The batched build's form of run(): every task sees the lists as they stood when the batch's appends were done, so
    // the tasks are independent -- candidates gathered and sorted, lists replaced and (SYMMETRIC) removals collected by the
    // linker's threads, flat arrays throughout (a 1.25M-row build has millions of tasks of ~33 candidates).
    int run_batched(std::vector<PendingEdge> &pend, LinkPool &pool, std::vector<HostGraph::Dirty> &dirties) {
        if (pend.empty()) return 0;
        std::sort(pend.begin(), pend.end(), [](const PendingEdge &x, const PendingEdge &y) {
            return x.target != y.target ? x.target < y.target : (x.lc != y.lc ? x.lc < y.lc : x.seq < y.seq);
        });
        tasks.clear();
        for (size_t i = 0; i < pend.size();) {
            size_t j = i;
            while (j < pend.size() && pend[j].target == pend[i].target && pend[j].lc == pend[i].lc) j++;
            tasks.push_back({pend[i].target, pend[i].lc, static_cast<int64_t>(i), static_cast<int32_t>(j - i)});
            i = j;
        }
        const int nt = static_cast<int>(tasks.size());
        off.assign(nt + 1, 0);
        std::vector<int32_t> ms(nt);
        for (int i = 0; i < nt; i++) {
            const Task &t = tasks[i];
            const int have = t.lc == 0 ? g.l0_cnt[t.target] : g.up_cnt[g.up_off[t.target] + (t.lc - 1)];
            off[i + 1] = off[i] + std::min<int64_t>(kSelMaxCand, static_cast<int64_t>(have) + t.npend);
            ms[i] = t.lc == 0 ? g.M0 : g.M;
        }
        cid.resize(std::max<int64_t>(off[nt], 1));
        cd.resize(std::max<int64_t>(off[nt], 1));
        const int nth = nt >= 1024 ? pool.size() : 1;
        auto fill = [&](int me) {
            std::vector<std::pair<float, int32_t>> c;
            for (int i = static_cast<int>(static_cast<int64_t>(nt) * me / nth); i < static_cast<int>(static_cast<int64_t>(nt) * (me + 1) / nth); i++) {
                gather(tasks[i], pend, c);
                for (size_t j = 0; j < c.size(); j++) {
                    cid[off[i] + j] = c[j].second;
                    cd[off[i] + j] = c[j].first;
                }
            }
        };
        if (nth == 1) fill(0);
        else pool.run(fill);
        HG_TRY(select_flat(nt, ms));
        n_tasks += nt;
        const int stride = g.M0;
        std::vector<std::vector<std::pair<int32_t, std::pair<int32_t, int32_t>>>> removals(nth);
        auto apply = [&](int me) {
            for (int i = static_cast<int>(static_cast<int64_t>(nt) * me / nth); i < static_cast<int>(static_cast<int64_t>(nt) * (me + 1) / nth); i++) {
                const Task &t = tasks[i];
                const int32_t *keep = &oid[static_cast<size_t>(i) * stride];
                const int nk = ocnt[i];
                if (sym)  // (before the list is replaced: the candidates are the present edges + the parked ones)
                    for (int64_t j = off[i]; j < off[i + 1]; j++) {
                        bool kept = false;
                        for (int r = 0; r < nk; r++) kept |= keep[r] == cid[j];
                        if (!kept) removals[me].push_back({cid[j], {t.target, t.lc}});
                    }
                g.set_list(t.target, t.lc, keep, &od[static_cast<size_t>(i) * stride], nk, dirties[me]);
            }
        };
        if (nth == 1) apply(0);
        else pool.run(apply);
        for (auto &rv : removals)  // (a removal touches another node's list: serial, and commutative -- the order does not matter)
            for (auto &r : rv)
                if (g.remove_edge(r.first, r.second.first, r.second.second, dirties[0])) n_removed++;
        return 0;
    }

    // pend: the batch's pending edges in sequential order (seq ascending)
    int run(std::vector<PendingEdge> &pend, HostGraph::Dirty &dirty) {
        if (pend.empty()) return 0;
        // group by (target, lc), a group's edges in sequential order; the groups in the order of their first edge
        std::stable_sort(pend.begin(), pend.end(), [](const PendingEdge &x, const PendingEdge &y) {
            return x.target != y.target ? x.target < y.target : x.lc < y.lc;
        });
        tasks.clear();
        for (size_t i = 0; i < pend.size();) {
            size_t j = i;
            while (j < pend.size() && pend[j].target == pend[i].target && pend[j].lc == pend[i].lc) j++;
            tasks.push_back({pend[i].target, pend[i].lc, static_cast<int64_t>(i), static_cast<int32_t>(j - i)});
            i = j;
        }
        std::sort(tasks.begin(), tasks.end(), [&](const Task &x, const Task &y) { return pend[x.first].seq < pend[y.first].seq; });
        const int nt = static_cast<int>(tasks.size());
        std::vector<std::vector<std::pair<float, int32_t>>> cands(nt);
        std::vector<int32_t> ms(nt);
        for (int i = 0; i < nt; i++) {
            gather(tasks[i], pend, cands[i]);
            ms[i] = tasks[i].lc == 0 ? g.M0 : g.M;
        }
        HG_TRY(select(cands, ms));
        n_tasks += nt;
        const int stride = g.M0;
        // keep-lists of the launch above (select() is reused for the re-selections of the sequential mode)
        std::vector<int32_t> kid(oid), kcnt(ocnt);
        std::vector<float> kd(od);
        std::vector<std::pair<int32_t, int32_t>> touched;  // (node, layer) lists shortened by a removal of this run
        auto is_touched = [&](int32_t node, int32_t lc) {
            for (auto &tl : touched)
                if (tl.first == node && tl.second == lc) return true;
            return false;
        };
        std::vector<std::pair<int32_t, std::pair<int32_t, int32_t>>> removals;  // batched: applied after every list is set
        for (int i = 0; i < nt; i++) {
            const Task &t = tasks[i];
            const int32_t *keep = &kid[static_cast<size_t>(i) * stride];
            const float *keepd = &kd[static_cast<size_t>(i) * stride];
            int nk = kcnt[i];
            std::vector<std::pair<float, int32_t>> *cv = &cands[i];
            std::vector<std::vector<std::pair<float, int32_t>>> one(1);
            if (seq_exact && is_touched(t.target, t.lc)) {
                // an earlier pruning of this insert took an edge out of this list: the sequential loop meets it shorter
                float *d;
                int32_t *cnt;
                int m;
                (void)g.adj(t.target, t.lc, &d, &cnt, &m);
                int used = 0;
                while (used < t.npend && *cnt < m) {  // room again: plain appends
                    g.append_edge(t.target, pend[t.first + used].id, t.lc, pend[t.first + used].dist, dirty);
                    used++;
                }
                if (used == t.npend) continue;
                Task rest = {t.target, t.lc, t.first + used, t.npend - used};
                gather(rest, pend, one[0]);
                std::vector<int32_t> m1(1, t.lc == 0 ? g.M0 : g.M);
                HG_TRY(select(one, m1));
                n_tasks++;
                keep = oid.data();
                keepd = od.data();
                nk = ocnt[0];
                cv = &one[0];
            }
            g.set_list(t.target, t.lc, keep, keepd, nk, dirty);
            if (sym)
                for (auto &c : *cv) {
                    bool kept = false;
                    for (int r = 0; r < nk; r++) kept |= keep[r] == c.second;
                    if (kept) continue;
                    if (seq_exact) {
                        if (g.remove_edge(c.second, t.target, t.lc, dirty)) {
                            n_removed++;
                            touched.emplace_back(c.second, t.lc);
                        }
                    } else {
                        removals.push_back({c.second, {t.target, t.lc}});
                    }
                }
        }
        for (auto &r : removals)
            if (g.remove_edge(r.first, r.second.first, r.second.second, dirty)) n_removed++;
        return 0;
    }
};

// insert-batch (ultra_fast.clj:303-344) over rows [done, g.n): every node of a batch runs the reference's per-level
// search (search-layer-ultra with ef-construction at layer 0 and 1 above, :250-251) on the GPU against the graph as it
// stood when the batch started, then the host links the batch in row order (:255-266) and prunes over-full lists
// (:279-299).  The device adjacency (idx->d_l0 / d_upadj, sized for g.n) holds the graph of rows [0, done) on entry and
// of all rows on return; g.entry / g.top are updated (:271-273).
// `flags` (include/hnswgpu.h, HNSWGPU_BUILD_*): SEQUENTIAL = one insert per batch, the walk starting at
// min(level, entry-level) with the entry point (:247-248) -- insert-single itself; HEURISTIC = links chosen by
// get-neighbors-heuristic (graph.clj:162-198) on the device (heuristic_select_kernel) instead of the m closest, over-full
// lists re-selected the same way (prune-connections, graph.clj:208-232); SYMMETRIC = a dropped edge leaves both lists
// (:226-231); EXTEND = extend-candidates? for the new node's own selection (:191-195).
// `ids` (hnswgpu_hnsw_update): the rows to insert are ids[0, count) in that order instead of the range [done, g.n) -- rows of
// g that no list names and whose own lists are empty; `done` then is the number of rows the graph links when the call begins
// (the batch size rule reads it) and grows by a batch's rows as before.  Null: the range.
static int insert_batches(hnswgpu_index *idx, HostGraph &g, int64_t done, int ef, hipStream_t st, int flags, const int32_t *ids = nullptr,
                          int64_t count = 0) {
    const bool seq = flags & HNSWGPU_BUILD_SEQUENTIAL, heur = flags & HNSWGPU_BUILD_HEURISTIC;
    const bool sym = heur && (flags & HNSWGPU_BUILD_SYMMETRIC), extend = flags & HNSWGPU_BUILD_EXTEND;
    const int64_t first = done, n = ids ? done + count : g.n;  // positions [done, n) of the insertion order
    auto row_of = [ids, first](int64_t pos) { return ids ? ids[pos - first] : static_cast<int32_t>(pos); };
    const int M0 = g.M0;
    const int64_t blocks = g.up_off[g.n];
    int maxlv = 1;
    for (int64_t i = done; i < n; i++) maxlv = std::max(maxlv, g.levels[row_of(i)]);
    // scratch sizing; the batch actually used grows with the graph (see below)
    const int64_t maxB = seq ? 1 : std::max<int64_t>(1, std::min<int64_t>(16384, tune(HNSWGPU_TUNE_BUILD_BATCH, 16384)));
    const int kk = heur ? ef : M0;         // layer-0 candidates a search hands back: all of them for the heuristic
    HG_TRY(idx->s_ids.ensure(sizeof(int32_t) * maxB * kk));
    HG_TRY(idx->s_outd.ensure(sizeof(float) * maxB * kk));
    HG_TRY(idx->s_misc.ensure(sizeof(int32_t) * maxB * (2 + maxlv)));   // q_rows, q_levels, up_out_ids
    HG_TRY(idx->s_misc2.ensure(sizeof(float) * maxB * maxlv));           // up_out_dist
    int32_t *d_qrows = idx->s_misc.as<int32_t>();
    int32_t *d_qlev = d_qrows + maxB;
    int32_t *d_upids = d_qlev + maxB;
    // the new nodes' own selections (heuristic mode): [maxB][M0] ids, distances, [maxB] counts, [maxB + 1] offsets
    OwnedBuf d_sel;
    int32_t *d_selid = nullptr, *d_selcnt = nullptr;
    float *d_seld = nullptr;
    int64_t *d_seloff = nullptr;
    if (heur) {
        HG_TRY(d_sel.ensure((sizeof(int32_t) + sizeof(float)) * maxB * M0 + sizeof(int32_t) * maxB + sizeof(int64_t) * (maxB + 1) + 64));
        d_seloff = d_sel.as<int64_t>();
        d_selid = reinterpret_cast<int32_t *>(d_seloff + maxB + 1);
        d_seld = reinterpret_cast<float *>(d_selid + maxB * M0);
        d_selcnt = reinterpret_cast<int32_t *>(d_seld + maxB * M0);
        std::vector<int64_t> h_off(maxB + 1);
        for (int64_t b = 0; b <= maxB; b++) h_off[b] = b * kk;
        HG_HIP(hipMemcpyAsync(d_seloff, h_off.data(), sizeof(int64_t) * (maxB + 1), hipMemcpyHostToDevice, st));
        HG_HIP(hipStreamSynchronize(st));
    }
    std::vector<int32_t> h_ids(maxB * M0), h_up(maxB * maxlv), h_qrows(maxB), h_qlev(maxB);
    std::vector<float> h_d(maxB * M0), h_upd(maxB * maxlv);
    g.flag0.assign(g.n, 0);
    g.flagu.assign(std::max<int64_t>(blocks, 1), 0);
    // linker threads: at most 16 (a GPU box's CPU share per GPU), HNSWGPU_BUILD_THREADS overrides (1 = sequential)
    int nthreads = static_cast<int>(std::min<unsigned>(16u, std::max(1u, std::thread::hardware_concurrency())));
    if (const int64_t e = tune(HNSWGPU_TUNE_BUILD_THREADS, 0)) nthreads = static_cast<int>(std::max<int64_t>(1, std::min<int64_t>(64, e)));
    if (n - done < 256 || seq) nthreads = 1;  // a handful of rows: no pool to start
    LinkPool pool(nthreads);
    std::vector<HostGraph::Dirty> dirties(pool.size());
    std::vector<std::vector<PendingEdge>> pendings(pool.size());
    std::vector<PendingEdge> pend;
    Pruner pruner(idx, g, st, sym, seq);
    PinnedBuf pin;
    const bool timing = tune(HNSWGPU_TUNE_BUILD_TIMING, 0) != 0;  // developer switch: where a build spends its time
    double t_gpu = 0.0, t_link = 0.0, t_up = 0.0, t_prune = 0.0;
    int64_t nbatch = 0;
    auto now = []() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    while (done < n) {
        const double tb0 = timing ? now() : 0.0;
        // a batch never exceeds 1/8 of the graph it is searched against; beyond 2048 it grows slowly (1/64)
        // so that big indexes amortise the per-batch round trip without starving early quality
        int64_t B = std::min<int64_t>({maxB, std::max<int64_t>(1, done / 8), 2048 + done / 64, n - done});
        HG_TRY(upload_dirty(idx, g, st, pin, pool));
        if (timing) t_up += now() - tb0;
        for (int64_t b = 0; b < B; b++) {
            h_qrows[b] = row_of(done + b);
            h_qlev[b] = g.levels[h_qrows[b]];
        }
        HG_HIP(hipMemcpyAsync(d_qrows, h_qrows.data(), sizeof(int32_t) * B, hipMemcpyHostToDevice, st));
        HG_HIP(hipMemcpyAsync(d_qlev, h_qlev.data(), sizeof(int32_t) * B, hipMemcpyHostToDevice, st));
        HnswArgs a;
        fill_args(idx, a);
        a.entry = g.entry;
        a.max_level = g.top;
        a.Q = idx->d_base;
        a.qld = idx->ld;
        a.q_rows = d_qrows;
        a.q_levels = d_qlev;
        a.ref_start = seq ? 1 : 0;
        a.nq = static_cast<int32_t>(B);
        a.ef = ef;
        a.k = kk;
        a.cap = ef + kGhost;
        a.out_ids = idx->s_ids.as<int32_t>();
        a.out_dist = idx->s_outd.as<float>();
        a.stats = nullptr;
        a.up_out_ids = d_upids;
        a.up_out_dist = idx->s_misc2.as<float>();
        a.up_stride = maxlv;
        HG_TRY(launch_hnsw_idx(idx, a, st));
        int32_t *h_cnt = nullptr;
        std::vector<int32_t> h_selcnt;
        if (heur) {  // the new nodes' own links: get-neighbors-heuristic over the search's ef candidates
            HeurArgs ha;
            memset(&ha, 0, sizeof(ha));
            ha.ntasks = static_cast<int32_t>(B);
            ha.off = d_seloff;
            ha.cand_id = a.out_ids;
            ha.cand_d = a.out_dist;
            ha.m = nullptr;
            ha.m_all = M0;
            ha.extend = extend ? 1 : 0;
            ha.out_stride = M0;
            ha.out_id = d_selid;
            ha.out_d = d_seld;
            ha.out_cnt = d_selcnt;
            HG_TRY(launch_heur(idx, ha, st));
            h_selcnt.resize(B);
            HG_HIP(hipMemcpyAsync(h_ids.data(), d_selid, sizeof(int32_t) * B * M0, hipMemcpyDeviceToHost, st));
            HG_HIP(hipMemcpyAsync(h_d.data(), d_seld, sizeof(float) * B * M0, hipMemcpyDeviceToHost, st));
            HG_HIP(hipMemcpyAsync(h_selcnt.data(), d_selcnt, sizeof(int32_t) * B, hipMemcpyDeviceToHost, st));
            h_cnt = h_selcnt.data();
        } else {
            HG_HIP(hipMemcpyAsync(h_ids.data(), a.out_ids, sizeof(int32_t) * B * M0, hipMemcpyDeviceToHost, st));
            HG_HIP(hipMemcpyAsync(h_d.data(), a.out_dist, sizeof(float) * B * M0, hipMemcpyDeviceToHost, st));
        }
        HG_HIP(hipMemcpyAsync(h_up.data(), a.up_out_ids, sizeof(int32_t) * B * maxlv, hipMemcpyDeviceToHost, st));
        HG_HIP(hipMemcpyAsync(h_upd.data(), a.up_out_dist, sizeof(float) * B * maxlv, hipMemcpyDeviceToHost, st));
        HG_HIP(hipStreamSynchronize(st));
        const double tb1 = timing ? now() : 0.0;
        const int top_at_start = g.top;
        const int take = std::min(M0, ef);
        // (A) own lists of node done + b; (B) reverse edges into the lists of nodes owned by thread `me` (of `nt`)
        auto link_own = [&](int64_t b, HostGraph::Dirty &dirty) {
            const int32_t id = row_of(done + b);
            const int L = g.levels[id];
            for (int lc = std::min(L, top_at_start); lc >= 1; lc--) {
                const int32_t nb = h_up[b * maxlv + (lc - 1)];
                if (nb < 0 || nb == id) continue;
                g.add_edge(id, nb, lc, h_upd[b * maxlv + (lc - 1)], dirty);
            }
            const int mine = h_cnt ? h_cnt[b] : take;
            for (int t = 0; t < mine; t++) {
                const int32_t nb = h_ids[b * M0 + t];
                if (nb < 0) break;
                if (nb == id) continue;
                g.add_edge(id, nb, 0, h_d[b * M0 + t], dirty);
            }
        };
        // the batch's reverse edges are numbered in the sequential loop's order: node by node, layers top down,
        // a layer's links in selection order
        auto link_reverse = [&](int64_t b, int me, int nt, HostGraph::Dirty &dirty, std::vector<PendingEdge> &pq) {
            const int32_t id = row_of(done + b);
            const int L = g.levels[id];
            int64_t sq = b * (maxlv + M0);
            auto rev = [&](int32_t nb, int lc, float dist) {
                if (heur) {
                    if (!g.append_edge(nb, id, lc, dist, dirty)) pq.push_back({nb, lc, id, dist, sq});
                } else {
                    g.add_edge(nb, id, lc, dist, dirty);
                }
            };
            for (int lc = std::min(L, top_at_start); lc >= 1; lc--, sq++) {
                const int32_t nb = h_up[b * maxlv + (lc - 1)];
                if (nb < 0 || nb == id || nb % nt != me) continue;
                rev(nb, lc, h_upd[b * maxlv + (lc - 1)]);
            }
            sq = b * (maxlv + M0) + maxlv;
            const int mine = h_cnt ? h_cnt[b] : take;
            for (int t = 0; t < mine; t++, sq++) {
                const int32_t nb = h_ids[b * M0 + t];
                if (nb < 0) break;
                if (nb == id || nb % nt != me) continue;
                rev(nb, 0, h_d[b * M0 + t]);
            }
        };
        const int nt = B >= 256 ? pool.size() : 1;  // small batches: the hand-over costs more than it saves
        if (nt == 1) {
            for (int64_t b = 0; b < B; b++) link_own(b, dirties[0]);
            for (int64_t b = 0; b < B; b++) link_reverse(b, 0, 1, dirties[0], pendings[0]);
        } else {
            pool.run([&](int me) {
                const int64_t lo = B * me / nt, hi = B * (me + 1) / nt;
                for (int64_t b = lo; b < hi; b++) link_own(b, dirties[me]);
            });
            pool.run([&](int me) {
                for (int64_t b = 0; b < B; b++) link_reverse(b, me, nt, dirties[me], pendings[me]);
            });
        }
        const double tb2 = timing ? now() : 0.0;
        if (heur) {  // the over-full lists of this batch: prune-connections (graph.clj:208-232) on the device
            pend.clear();
            for (auto &pq : pendings) {
                pend.insert(pend.end(), pq.begin(), pq.end());
                pq.clear();
            }
            std::sort(pend.begin(), pend.end(), [](const PendingEdge &x, const PendingEdge &y) { return x.seq < y.seq; });
            if (seq) HG_TRY(pruner.run(pend, dirties[0]));
            else HG_TRY(pruner.run_batched(pend, pool, dirties));
        }
        for (auto &dd : dirties) {
            g.dirty0.insert(g.dirty0.end(), dd.d0.begin(), dd.d0.end());
            g.dirtyu.insert(g.dirtyu.end(), dd.du.begin(), dd.du.end());
            dd.d0.clear();
            dd.du.clear();
        }
        for (int64_t b = 0; b < B; b++) {  // :271-273
            const int32_t id = row_of(done + b);
            if (g.levels[id] > g.top) {
                g.entry = id;
                g.top = g.levels[id];
            }
        }
        done += B;
        if (timing) {
            t_gpu += tb1 - tb0;
            t_link += tb2 - tb1;
            t_prune += now() - tb2;
            nbatch++;
        }
    }
    if (timing)
        fprintf(stderr, "hnsw build: %lld batches, %.2f s upload + search + download (%.2f s of it packing and uploading "
                        "changed adjacency rows), %.2f s host linking, %.2f s re-selection of %lld over-full lists (%lld edges "
                        "removed from the other side)\n",
                static_cast<long long>(nbatch), t_gpu, t_up, t_link, t_prune, static_cast<long long>(pruner.n_tasks),
                static_cast<long long>(pruner.n_removed));
    return 0;
}

// A graph that stands on the device -- the handle's d_l0 / d_upadj over rows [0, n0), mirrored by h_l0 / h_upadj / h_upoff --
// becomes the lists of a HostGraph `g` that is sized already (g.n >= n0, the same up_off below n0): the edges, and their
// distances, which the reference's pruning sorts by (ultra_fast.clj:279-299), recomputed on the device by the traversal's own
// arithmetic over the handle's base rows.  Step 2 of hnswgpu_hnsw_add and of hnswgpu_hnsw_update.
static int adopt_graph(hnswgpu_index *idx, HostGraph &g, int64_t n0, const int32_t *h_l0, const int32_t *h_upadj, const int64_t *h_upoff,
                       hipStream_t st) {
    const int M = g.M, M0 = g.M0;
    const int64_t blocks0 = h_upoff[n0];
    std::vector<float> d0(static_cast<size_t>(n0) * M0), du(static_cast<size_t>(std::max<int64_t>(blocks0, 1)) * M);
    std::vector<int32_t> owner(static_cast<size_t>(std::max<int64_t>(blocks0, 1)));
    for (int64_t i = 0; i < n0; i++)
        for (int64_t b = h_upoff[i]; b < h_upoff[i + 1]; b++) owner[b] = static_cast<int32_t>(i);
    HG_TRY(idx->s_outd.ensure(sizeof(float) * (d0.size() + du.size())));
    HG_TRY(idx->s_ids.ensure(sizeof(int32_t) * owner.size()));
    float *dd0 = idx->s_outd.as<float>(), *ddu = dd0 + d0.size();
    HG_HIP(hipMemcpyAsync(idx->s_ids.p, owner.data(), sizeof(int32_t) * owner.size(), hipMemcpyHostToDevice, st));
    HG_TRY(launch_edge_dist(idx, nullptr, idx->d_l0, M0, n0, dd0, st));
    HG_TRY(launch_edge_dist(idx, idx->s_ids.as<int32_t>(), idx->d_upadj, M, blocks0, ddu, st));
    if (n0 > 0) HG_HIP(hipMemcpyAsync(d0.data(), dd0, sizeof(float) * d0.size(), hipMemcpyDeviceToHost, st));
    if (blocks0 > 0) HG_HIP(hipMemcpyAsync(du.data(), ddu, sizeof(float) * static_cast<size_t>(blocks0) * M, hipMemcpyDeviceToHost, st));
    HG_HIP(hipStreamSynchronize(st));
    // a full list whose distances ascend IS the pruned order (prune-connections-ultra's stable sort is the identity on
    // it); any other list is still in insertion order and gets its first sort when it overflows
    auto adopt = [](const int32_t *src, const float *dsrc, int width, int32_t *dst, float *ddst, int32_t &cnt, uint8_t &srt) {
        int c = 0;
        while (c < width && src[c] >= 0) c++;
        bool asc = true;
        for (int j = 0; j < c; j++) {
            dst[j] = src[j];
            ddst[j] = dsrc[j];
            if (j > 0 && dsrc[j] < dsrc[j - 1]) asc = false;
        }
        cnt = c;
        srt = (c == width && asc) ? 1 : 0;
    };
    for (int64_t i = 0; i < n0; i++)
        adopt(&h_l0[static_cast<size_t>(i) * M0], &d0[static_cast<size_t>(i) * M0], M0, &g.l0[static_cast<size_t>(i) * (M0 + 1)],
              &g.l0_d[static_cast<size_t>(i) * (M0 + 1)], g.l0_cnt[i], g.sorted0[i]);
    for (int64_t b = 0; b < blocks0; b++)
        adopt(&h_upadj[static_cast<size_t>(b) * M], &du[static_cast<size_t>(b) * M], M, &g.up[static_cast<size_t>(b) * (M + 1)],
              &g.up_d[static_cast<size_t>(b) * (M + 1)], g.up_cnt[b], g.sortedu[b]);
    return 0;
}

// the finished host graph -> device adjacency + the host mirrors of the handle
static int publish_graph(hnswgpu_index *idx, HostGraph &g, hipStream_t st) {
    std::vector<int32_t> tmp0, tmpu;
    const int64_t blocks = g.up_off[g.n];
    HG_TRY(upload_graph(idx, g, st, tmp0, tmpu));
    idx->h_levels = g.levels;
    idx->h_upoff = g.up_off;
    idx->h_l0.swap(tmp0);
    tmpu.resize(static_cast<size_t>(blocks) * g.M);
    idx->h_upadj.swap(tmpu);
    idx->entry = g.entry;
    idx->max_level = std::max(g.top, 0);
    idx->has_graph = true;
    return 0;
}

// levels of rows [from, to): floor(ml * -ln U), ml = 1/ln 2 (ultra_fast.clj:133,143-147), U the row's draw of
// java.util.Random(seed) -- row i takes the i-th nextDouble, so rows added later continue the build's sequence
static void draw_levels(int64_t seed, int64_t from, int64_t to, std::vector<int32_t> &levels, std::vector<int64_t> &up_off) {
    JavaRandom rng(seed);
    const double ml = 1.0 / log(2.0);
    for (int64_t i = 0; i < to; i++) {
        const double u = rng.next_double();
        if (i < from) continue;
        const int lv = u > 0.0 ? static_cast<int>(ml * (-log(u))) : 30;
        levels[i] = std::min(lv, 30);
        up_off[i + 1] = up_off[i] + levels[i];
    }
}

}  // namespace hg

extern "C" {

// build-index / insert-batch (ultra_fast.clj:303-344) as batched insertion (insert_batches above).
// Level draw: floor(ml * -ln U), ml = 1/ln 2 (:133,:143-147), U from java.util.Random(seed).
// flags = 0, the fast default -- differences from the reference's sequential insert-single, stated in DESIGN.md: nodes
// of one batch do not see each other (batches grow from 1 to at most 1/8 of the graph, capped); the walk starts at the
// top layer with ef = 1 instead of at min(level, entry-level) (:247-248); each node links to its m CLOSEST candidates
// (the reference's `(take m candidates)` takes PriorityQueue array order, which is unspecified).
// HNSWGPU_BUILD_SEQUENTIAL removes the first two (insert-single itself: the graph equals oracle.c's orc_hnsw_build_ex
// edge for edge); HNSWGPU_BUILD_HEURISTIC / _SYMMETRIC / _EXTEND select links as src/hnsw/graph.clj:162-232 does.
int hnswgpu_hnsw_build(hnswgpu_index *idx, int32_t M, int32_t ef_construction, int64_t seed) {
    return hnswgpu_hnsw_build_ex(idx, M, ef_construction, seed, 0);
}

int hnswgpu_hnsw_build_ex(hnswgpu_index *idx, int32_t M, int32_t ef_construction, int64_t seed, int32_t flags) {
    HG_REQUIRE(idx, HNSWGPU_EINVAL, "idx is null");
    HG_REQUIRE((flags & ~(HNSWGPU_BUILD_SEQUENTIAL | HNSWGPU_BUILD_HEURISTIC | HNSWGPU_BUILD_SYMMETRIC | HNSWGPU_BUILD_EXTEND)) == 0,
               HNSWGPU_EINVAL, "unknown build flags 0x%x", flags);
    HG_REQUIRE(!(flags & (HNSWGPU_BUILD_SYMMETRIC | HNSWGPU_BUILD_EXTEND)) || (flags & HNSWGPU_BUILD_HEURISTIC), HNSWGPU_EINVAL,
               "HNSWGPU_BUILD_SYMMETRIC / _EXTEND qualify HNSWGPU_BUILD_HEURISTIC");
    HG_REQUIRE(M >= 1 && 2 * M <= kMaxDeg, HNSWGPU_ELIMIT, "need 1 <= M <= %d", kMaxDeg / 2);
    HG_REQUIRE(ef_construction >= 1 && ef_construction <= 4096, HNSWGPU_ELIMIT, "need 1 <= ef_construction <= 4096");
    hipStream_t st = idx->stream;
    Call call;
    HG_TRY(call.open(idx, st));
    const int64_t n = idx->n;
    const int M0 = 2 * M;
    HostGraph g;
    g.n = n;
    g.M = M;
    g.M0 = M0;
    g.levels.resize(n);
    g.up_off.assign(n + 1, 0);
    draw_levels(seed, 0, n, g.levels, g.up_off);
    const int64_t blocks = n > 0 ? g.up_off[n] : 0;
    HG_TRY(call.quiesce());  // as in hnswgpu_set_graph
    free_graph(idx);
    HG_TRY(alloc_graph(idx, M, M0, blocks));
    HG_TRY(ensure_qrows(idx, st));
    if (n == 0) {
        idx->h_levels.clear();
        idx->h_l0.clear();
        idx->h_upoff.assign(1, 0);
        idx->h_upadj.clear();
        idx->entry = -1;
        idx->max_level = 0;
        idx->has_graph = true;
        idx->build_flags = flags;  // (rows added to the empty graph are linked by the builder that was asked for)
        return call.close();
    }
    g.l0.assign(static_cast<size_t>(n) * (M0 + 1), -1);
    g.l0_d.assign(static_cast<size_t>(n) * (M0 + 1), 0.f);
    g.l0_cnt.assign(n, 0);
    g.up.assign(static_cast<size_t>(std::max<int64_t>(blocks, 1)) * (M + 1), -1);
    g.up_d.assign(static_cast<size_t>(std::max<int64_t>(blocks, 1)) * (M + 1), 0.f);
    g.up_cnt.assign(std::max<int64_t>(blocks, 1), 0);
    g.sorted0.assign(n, 0);
    g.sortedu.assign(std::max<int64_t>(blocks, 1), 0);
    HG_HIP(hipMemcpyAsync(idx->d_levels, g.levels.data(), sizeof(int32_t) * n, hipMemcpyHostToDevice, st));
    HG_HIP(hipMemcpyAsync(idx->d_upoff, g.up_off.data(), sizeof(int64_t) * (n + 1), hipMemcpyHostToDevice, st));
    HG_HIP(hipMemsetAsync(idx->d_l0, 0xff, sizeof(int32_t) * n * M0, st));
    HG_HIP(hipMemsetAsync(idx->d_upadj, 0xff, sizeof(int32_t) * std::max<int64_t>(blocks, 1) * M, st));
    g.entry = 0;  // first element becomes the entry point (:229-231)
    g.top = g.levels[0];
    HG_TRY(insert_batches(idx, g, 1, ef_construction, st, flags));
    HG_TRY(publish_graph(idx, g, st));
    idx->build_flags = flags;  // (only a graph that stands carries its builder: hnswgpu_hnsw_add inserts the same way)
    return call.close();
}

// A forest built part by part: every non-empty part's rows -- contiguous in the handle's base matrix -- become a temporary handle
// that hnswgpu_hnsw_build_ex builds exactly as a caller's handle over those rows alone (same seed: the part's rows draw levels as
// rows 0, 1, ... of their own handle; same flags), its graph is exported and its ids shifted by the part's first row.  The forest
// is installed once, when every part stands: on any error the handle keeps what it had.
int hnswgpu_hnsw_build_parts(hnswgpu_index *idx, int32_t nparts, const int64_t *part_off, int32_t M, int32_t ef_construction,
                             int64_t seed, int32_t flags) {
    HG_REQUIRE(idx, HNSWGPU_EINVAL, "idx is null");
    HG_REQUIRE(nparts >= 1 && part_off, HNSWGPU_EINVAL, "need nparts >= 1 and part_off");
    HG_REQUIRE((flags & ~(HNSWGPU_BUILD_SEQUENTIAL | HNSWGPU_BUILD_HEURISTIC | HNSWGPU_BUILD_SYMMETRIC | HNSWGPU_BUILD_EXTEND)) == 0,
               HNSWGPU_EINVAL, "unknown build flags 0x%x", flags);
    HG_REQUIRE(!(flags & (HNSWGPU_BUILD_SYMMETRIC | HNSWGPU_BUILD_EXTEND)) || (flags & HNSWGPU_BUILD_HEURISTIC), HNSWGPU_EINVAL,
               "HNSWGPU_BUILD_SYMMETRIC / _EXTEND qualify HNSWGPU_BUILD_HEURISTIC");
    HG_REQUIRE(M >= 1 && 2 * M <= kMaxDeg, HNSWGPU_ELIMIT, "need 1 <= M <= %d", kMaxDeg / 2);
    HG_REQUIRE(ef_construction >= 1 && ef_construction <= 4096, HNSWGPU_ELIMIT, "need 1 <= ef_construction <= 4096");
    hipStream_t st = idx->stream;
    Call call;
    HG_TRY(call.open(idx, st));
    const int64_t n = idx->n;
    HG_REQUIRE(part_off[0] == 0 && part_off[nparts] == n, HNSWGPU_EINVAL, "part_off must run from 0 to n");
    for (int32_t p = 0; p < nparts; p++)
        HG_REQUIRE(part_off[p] <= part_off[p + 1] && part_off[p + 1] <= n, HNSWGPU_EINVAL, "part_off is not monotone at part %d", p);
    const int M0 = 2 * M;
    std::vector<int32_t> levels(n), l0(static_cast<size_t>(n) * M0, -1), up, entry(nparts, -1), top(nparts, 0);
    std::vector<int64_t> up_off(n + 1, 0);
    for (int32_t p = 0; p < nparts; p++) {
        const int64_t lo = part_off[p], rows = part_off[p + 1] - lo;
        if (rows == 0) continue;
        hnswgpu_index *tmp = nullptr;
        HG_TRY(hnswgpu_create_dev(idx->d_base + lo * idx->ld, rows, idx->dim, idx->ld, idx->metric, idx->device, st, &tmp));
        const int rc = [&]() -> int {
            tmp->rejection_mode = idx->rejection_mode;  // (the builder's searches decide as the caller's handle would: never a result)
            HG_TRY(hnswgpu_hnsw_build_ex(tmp, M, ef_construction, seed, flags));
            const int64_t blocks0 = up_off[lo], blocks = tmp->up_blocks;
            up.resize(static_cast<size_t>(blocks0 + blocks) * M, -1);
            std::vector<int64_t> off_p(rows + 1);
            HG_TRY(hnswgpu_get_graph(tmp, levels.data() + lo, l0.data() + lo * M0, off_p.data(), up.data() + blocks0 * M));
            for (int64_t i = 0; i <= rows; i++) up_off[lo + i] = blocks0 + off_p[i];
            for (int64_t i = lo * M0; i < (lo + rows) * M0; i++)
                if (l0[i] >= 0) l0[i] += static_cast<int32_t>(lo);
            for (int64_t i = blocks0 * M; i < (blocks0 + blocks) * M; i++)
                if (up[i] >= 0) up[i] += static_cast<int32_t>(lo);
            entry[p] = tmp->entry + static_cast<int32_t>(lo);
            top[p] = tmp->max_level;
            return 0;
        }();
        (void)hnswgpu_destroy(tmp);
        HG_HIP(hipSetDevice(idx->device));
        HG_TRY(rc);
    }
    const PartTables pt = {nparts, part_off, entry.data(), top.data()};
    HG_TRY(check_graph(idx, levels.data(), l0.data(), M0, up_off.data(), up.data(), M, -1, 0, &pt));
    HG_TRY(install_graph(idx, call, st, levels.data(), l0.data(), M0, up_off.data(), up.data(), M, -1, 0, &pt));
    return call.close();
}

// insert-single on a LIVE index (ultra_fast.clj:216-275, reached by add-vector! src/hnsw/api.clj:30-33 and add!
// src/hnsw/api/simple.clj:31-42): `m` more rows join the base matrix and the graph that is installed.  The new rows'
// levels continue the seeded java.util.Random sequence (row i takes its i-th draw), they are inserted in batches by the
// kernels and the linker of hnswgpu_hnsw_build against the CURRENT graph -- whose edge distances, which the reference's
// pruning sorts by (:279-299), are recomputed on the device by the traversal's own arithmetic -- and the device
// adjacency, the int8 rows and the host mirrors grow with them.  Row ids of the new rows: n, n + 1, ...
int hnswgpu_hnsw_add(hnswgpu_index *idx, const float *rows, int64_t m, int32_t ef_construction, int64_t seed) {
    HG_REQUIRE(idx, HNSWGPU_EINVAL, "idx is null");
    HG_REQUIRE(m >= 0, HNSWGPU_EINVAL, "m must be >= 0");
    if (m == 0) return 0;
    HG_REQUIRE(rows, HNSWGPU_EINVAL, "rows is null");
    HG_REQUIRE(ef_construction >= 1 && ef_construction <= 4096, HNSWGPU_ELIMIT, "need 1 <= ef_construction <= 4096");
    hipStream_t st = idx->stream;
    Call call;
    HG_TRY(call.open(idx, st));
    HG_REQUIRE(idx->has_graph, HNSWGPU_ESTATE, "index has no graph (call hnswgpu_hnsw_build / hnswgpu_set_graph first)");
    HG_REQUIRE(idx->nparts == 0, HNSWGPU_ESTATE,
               "the index holds a forest: a new row has no part (rebuild with hnswgpu_hnsw_build_parts / hnswgpu_set_graph_parts)");
    HG_REQUIRE(idx->nlist == 0, HNSWGPU_ESTATE,
               "the index holds IVF lists over its present rows: add rows first, then build / install the lists");
    HG_REQUIRE(idx->lsh_tables == 0, HNSWGPU_ESTATE,
               "the index holds LSH tables over its present rows: add rows first, then build / install the tables");
    HG_REQUIRE(idx->M0 == 2 * idx->M, HNSWGPU_ESTATE, "hnswgpu_hnsw_add needs a graph with M0 = 2 M (as hnswgpu_hnsw_build makes)");
    const int64_t n0 = idx->n, n1 = n0 + m;
    HG_REQUIRE(n1 < 2147483647LL, HNSWGPU_ELIMIT, "the index must hold fewer than 2^31 rows");
    HG_TRY(call.quiesce());
    const int M = idx->M, M0 = idx->M0;
    const int64_t ld = idx->ld;
    // Failure-atomic: everything the call makes -- the grown base, norms, int8 rows, device graph -- is STAGED; the handle's
    // fields point at the staged arrays while the insertion searches run against them (idx->mu is held and the streams are
    // quiesced: no caller can see the intermediate state) and are restored, the staged arrays freed, if any step fails: the
    // index then is exactly what it was (n, graph, host mirrors).  On success the old arrays are freed.
    // Cost: O(n) per call, not per row (the base is copied, every row re-quantised, the installed edges' distances
    // recomputed: ~1 ms per million 768-d rows each) -- add rows in batches.
    struct Staged {
        float *base = nullptr, *norms = nullptr;
        uint32_t *qrows = nullptr;
        float4 *qmeta = nullptr;
        int32_t *levels = nullptr, *l0 = nullptr, *upadj = nullptr;
        int64_t *upoff = nullptr;
    } nw, old;
    old.base = idx->d_base;
    old.norms = idx->d_norms;
    old.qrows = idx->d_qrows;
    old.qmeta = idx->d_qmeta;
    old.levels = idx->d_levels;
    old.l0 = idx->d_l0;
    old.upadj = idx->d_upadj;
    old.upoff = idx->d_upoff;
    const int64_t old_blocks = idx->up_blocks;
    bool installed = false;
    auto free_staged = [](Staged &sg) {
        void *ptrs[] = {sg.base, sg.norms, sg.qrows, sg.qmeta, sg.levels, sg.l0, sg.upadj, sg.upoff};
        for (void *p : ptrs)
            if (p) (void)hipFree(p);
        sg = Staged();
    };
    HostGraph g;
    const int rc = [&]() -> int {
        // ---- 1. the base matrix, its norms and int8 rows grow (staged)
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
        if (old.qrows) HG_TRY(quantize_rows(idx, nw.base, n1, &nw.qrows, &nw.qmeta, st));  // (all rows again: one pass over the base)
        // ---- 2. the host graph: the installed adjacency + its edge distances, then room for the new rows
        g.n = n1;
        g.M = M;
        g.M0 = M0;
        g.levels = idx->h_levels;
        g.levels.resize(n1, 0);
        g.up_off = idx->h_upoff;
        g.up_off.resize(n1 + 1, 0);
        draw_levels(seed, n0, n1, g.levels, g.up_off);
        const int64_t blocks0 = idx->h_upoff[n0], blocks1 = g.up_off[n1];
        g.l0.assign(static_cast<size_t>(n1) * (M0 + 1), -1);
        g.l0_d.assign(static_cast<size_t>(n1) * (M0 + 1), 0.f);
        g.l0_cnt.assign(n1, 0);
        g.up.assign(static_cast<size_t>(std::max<int64_t>(blocks1, 1)) * (M + 1), -1);
        g.up_d.assign(static_cast<size_t>(std::max<int64_t>(blocks1, 1)) * (M + 1), 0.f);
        g.up_cnt.assign(std::max<int64_t>(blocks1, 1), 0);
        g.sorted0.assign(n1, 0);
        g.sortedu.assign(std::max<int64_t>(blocks1, 1), 0);
        HG_TRY(adopt_graph(idx, g, n0, idx->h_l0.data(), idx->h_upadj.data(), idx->h_upoff.data(), st));  // (the old base: still in place)
        g.entry = idx->entry;
        g.top = idx->max_level;
        // ---- 3. the device graph grows: old rows copied, new rows empty (staged)
        HG_HIP(hipMalloc(reinterpret_cast<void **>(&nw.levels), sizeof(int32_t) * n1));
        HG_HIP(hipMalloc(reinterpret_cast<void **>(&nw.l0), sizeof(int32_t) * n1 * M0));
        HG_HIP(hipMalloc(reinterpret_cast<void **>(&nw.upoff), sizeof(int64_t) * (n1 + 1)));
        HG_HIP(hipMalloc(reinterpret_cast<void **>(&nw.upadj), sizeof(int32_t) * std::max<int64_t>(blocks1, 1) * M));
        HG_HIP(hipMemcpyAsync(nw.levels, g.levels.data(), sizeof(int32_t) * n1, hipMemcpyHostToDevice, st));
        HG_HIP(hipMemcpyAsync(nw.upoff, g.up_off.data(), sizeof(int64_t) * (n1 + 1), hipMemcpyHostToDevice, st));
        HG_HIP(hipMemsetAsync(nw.l0, 0xff, sizeof(int32_t) * n1 * M0, st));
        HG_HIP(hipMemsetAsync(nw.upadj, 0xff, sizeof(int32_t) * std::max<int64_t>(blocks1, 1) * M, st));
        if (n0 > 0) HG_HIP(hipMemcpyAsync(nw.l0, idx->d_l0, sizeof(int32_t) * n0 * M0, hipMemcpyDeviceToDevice, st));
        if (blocks0 > 0) HG_HIP(hipMemcpyAsync(nw.upadj, idx->d_upadj, sizeof(int32_t) * blocks0 * M, hipMemcpyDeviceToDevice, st));
        HG_HIP(hipStreamSynchronize(st));
        // ---- 4. the insertion searches run against the staged arrays
        idx->d_base = nw.base;
        idx->d_norms = nw.norms;
        idx->d_qrows = nw.qrows;
        idx->d_qmeta = nw.qmeta;
        idx->d_levels = nw.levels;
        idx->d_l0 = nw.l0;
        idx->d_upoff = nw.upoff;
        idx->d_upadj = nw.upadj;
        idx->up_blocks = blocks1;
        idx->n = n1;
        idx->graph_gen++;
        installed = true;
        if (n0 == 0) {  // an empty index with an (empty) graph: the first new row becomes the entry point (:229-231)
            g.entry = 0;
            g.top = g.levels[0];
            HG_TRY(insert_batches(idx, g, 1, ef_construction, st, idx->build_flags & ~HNSWGPU_BUILD_SEQUENTIAL));
        } else {
            HG_TRY(insert_batches(idx, g, n0, ef_construction, st, idx->build_flags & ~HNSWGPU_BUILD_SEQUENTIAL));
        }
        return publish_graph(idx, g, st);  // (host mirrors, entry, max_level: assigned only once the uploads succeeded)
    }();
    if (rc != 0) {
        (void)hipStreamSynchronize(st);
        if (installed) {
            idx->d_base = old.base;
            idx->d_norms = old.norms;
            idx->d_qrows = old.qrows;
            idx->d_qmeta = old.qmeta;
            idx->d_levels = old.levels;
            idx->d_l0 = old.l0;
            idx->d_upoff = old.upoff;
            idx->d_upadj = old.upadj;
            idx->up_blocks = old_blocks;
            idx->n = n0;
            idx->graph_gen++;
        }
        free_staged(nw);
        return rc;
    }
    free_staged(old);
    return call.close();
}

// Rows leave a live graph (include/hnswgpu.h).  The reference has no delete (pure_hnsw.clj:16 is a todo); what is restated is the
// list layout, the repair rule is this project's own: the kept rows are renumbered densely in their old order, a list that loses
// no member keeps its members in their order, a list that loses one is selected again -- as the handle's builder prunes an
// over-full list -- from its kept members and the kept members of the same-layer lists of the members that left, all read from
// the graph as it stood when the call began.  One chain on the handle's stream (remove_kernels.hpp, hnsw_remove_kernels.hpp):
// mark, rank, the kept base rows / norms to their ranks, levels and up_off, the list pass, the scan of the candidate counts (its
// two totals are read to size the candidate arrays), gather, distances, sort, selection, scatter; the int8 rows are made again
// over the moved rows.  Everything is staged; the handle takes the staged arrays over behind ONE readback: the gate's three
// counts and the new graph for the host mirrors.  The traversal's rejection-test verdict (hnsw_cal_state) is reset, as free_graph
// resets it wherever a graph is replaced: the next large launch measures the new graph.
int hnswgpu_hnsw_remove(hnswgpu_index *idx, const int32_t *rows, int64_t m, int64_t *n_after) {
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
    HG_REQUIRE(idx->has_graph, HNSWGPU_ESTATE, "index has no graph (call hnswgpu_hnsw_build / hnswgpu_set_graph first)");
    HG_REQUIRE(idx->nparts == 0, HNSWGPU_ESTATE,
               "the index holds a forest of HNSW sub-graphs: its part tables would keep the old numbering of the rows");
    HG_REQUIRE(idx->nlist == 0, HNSWGPU_ESTATE, "the index holds IVF lists: they would keep the old numbering of the rows");
    HG_REQUIRE(idx->lsh_tables == 0, HNSWGPU_ESTATE, "the index holds LSH tables: they would keep the old numbering of the rows");
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
    const int M = idx->M, M0 = idx->M0;
    const int64_t ld = idx->ld, blocks0 = idx->up_blocks;
    struct Staged {
        float *base = nullptr, *norms = nullptr;
        uint32_t *qrows = nullptr;
        float4 *qmeta = nullptr;
        int32_t *levels = nullptr, *l0 = nullptr, *upadj = nullptr;
        int64_t *upoff = nullptr;
        void release() {
            void *ptrs[] = {base, norms, qrows, qmeta, levels, l0, upadj, upoff};
            for (void *p : ptrs)
                if (p) (void)hipFree(p);
            *this = Staged();
        }
    } nw, old;
    old.base = idx->d_base, old.norms = idx->d_norms, old.qrows = idx->d_qrows, old.qmeta = idx->d_qmeta;
    old.levels = idx->d_levels, old.l0 = idx->d_l0, old.upadj = idx->d_upadj, old.upoff = idx->d_upoff;
    std::vector<int32_t> h_levels, h_l0, h_upadj;
    std::vector<int64_t> h_upoff;
    int64_t blocks1 = 0;
    int32_t entry1 = -1, top1 = 0;
    auto shrink = [&]() -> int {
        // what the host knows before the device does: the kept rows' levels summed (the staged upper layer's size and the
        // gate's second count) and where a kept entry point lands
        std::vector<uint8_t> gone(static_cast<size_t>(n0), 0);
        for (int64_t i = 0; i < m; i++) gone[rows[i]] = 1;
        int64_t below_entry = 0;
        for (int64_t r = 0; r < n0; r++) {
            if (gone[r]) continue;
            blocks1 += idx->h_levels[r];
            if (r < idx->entry) below_entry++;
        }
        const bool entry_kept = idx->entry >= 0 && idx->entry < n0 && !gone[idx->entry];
        const size_t rows1 = static_cast<size_t>(std::max<int64_t>(n1, 1)), ub1 = static_cast<size_t>(std::max<int64_t>(blocks1, 1));
        if (n1 > 0) {
            HG_HIP(hipMalloc(reinterpret_cast<void **>(&nw.base), sizeof(float) * rows1 * ld));
            HG_HIP(hipMalloc(reinterpret_cast<void **>(&nw.norms), sizeof(float) * rows1));
        }
        HG_HIP(hipMalloc(reinterpret_cast<void **>(&nw.levels), sizeof(int32_t) * rows1));
        HG_HIP(hipMalloc(reinterpret_cast<void **>(&nw.l0), sizeof(int32_t) * rows1 * M0));
        HG_HIP(hipMalloc(reinterpret_cast<void **>(&nw.upoff), sizeof(int64_t) * (rows1 + 1)));
        HG_HIP(hipMalloc(reinterpret_cast<void **>(&nw.upadj), sizeof(int32_t) * ub1 * M));
        HG_HIP(hipMemsetAsync(nw.l0, 0xff, sizeof(int32_t) * rows1 * M0, st));
        HG_HIP(hipMemsetAsync(nw.upadj, 0xff, sizeof(int32_t) * ub1 * M, st));
        HnswRemoveArgs a;
        memset(&a, 0, sizeof(a));
        a.r.n0 = n0;
        a.r.n1 = n1;
        a.r.m = m;
        a.r.W = (n0 + 31) / 32;
        a.r.ld = ld;
        a.M = M;
        a.M0 = M0;
        a.blocks0 = blocks0;
        a.blocks1 = blocks1;
        a.nlists = n0 + blocks0;
        HG_TRY(hnsw_repair_scratch(idx, a, rows, st));
        a.r.old_base = old.base;
        a.r.old_norms = old.norms;
        a.r.new_base = nw.base;
        a.r.new_norms = nw.norms;
        a.old_levels = old.levels;
        a.old_l0 = old.l0;
        a.old_upadj = old.upadj;
        a.old_upoff = old.upoff;
        a.new_levels = nw.levels;
        a.new_l0 = nw.l0;
        a.new_upadj = nw.upadj;
        a.new_upoff = nw.upoff;
        const unsigned row_wgs = static_cast<unsigned>((n0 + kNWave - 1) / kNWave);
        hipLaunchKernelGGL(lsh_remove_mark_kernel, dim3(static_cast<unsigned>((m + kWG - 1) / kWG)), dim3(kWG), 0, st, a.r);
        hipLaunchKernelGGL(lsh_remove_rank_kernel, dim3(1), dim3(kWG), 0, st, a.r);
        if (n1 > 0) hipLaunchKernelGGL(lsh_remove_rows_kernel, dim3(row_wgs), dim3(kWG), 0, st, a.r);
        hipLaunchKernelGGL(hnsw_remove_levels_kernel, dim3(1), dim3(kWG), 0, st, a);
        HG_HIP(hipGetLastError());
        if (old.qrows && n1 > 0) HG_TRY(quantize_rows(idx, nw.base, n1, &nw.qrows, &nw.qmeta, st));  // (as add: one pass over the new base)
        HG_TRY(hnsw_repair_chain<true>(idx, a, st));  // owner, list pass, scan, gather, distances, sort, selection, scatter
        // ---- the one readback: gate, levels, up_off, both adjacency arrays
        int64_t gate[kLshRemoveGate];
        h_levels.resize(static_cast<size_t>(n1));
        h_l0.resize(static_cast<size_t>(n1) * M0);
        h_upoff.assign(static_cast<size_t>(n1) + 1, 0);
        h_upadj.resize(static_cast<size_t>(blocks1) * M);
        HG_HIP(hipMemcpyAsync(gate, a.r.gate, sizeof(gate), hipMemcpyDeviceToHost, st));
        HG_HIP(hipMemcpyAsync(h_upoff.data(), nw.upoff, sizeof(int64_t) * (n1 + 1), hipMemcpyDeviceToHost, st));
        if (n1 > 0) {
            HG_HIP(hipMemcpyAsync(h_levels.data(), nw.levels, sizeof(int32_t) * n1, hipMemcpyDeviceToHost, st));
            HG_HIP(hipMemcpyAsync(h_l0.data(), nw.l0, sizeof(int32_t) * n1 * M0, hipMemcpyDeviceToHost, st));
        }
        if (blocks1 > 0) HG_HIP(hipMemcpyAsync(h_upadj.data(), nw.upadj, sizeof(int32_t) * blocks1 * M, hipMemcpyDeviceToHost, st));
        HG_HIP(hipStreamSynchronize(st));
        HG_REQUIRE(gate[2 * kRemoveMaxTables] == n1, HNSWGPU_EHIP, "the mask keeps %lld rows, not %lld", (long long)gate[2 * kRemoveMaxTables],
                   (long long)n1);
        HG_REQUIRE(gate[kHnswRemoveGateOff] == blocks1 && h_upoff[n1] == blocks1, HNSWGPU_EHIP,
                   "the shrunken graph holds %lld upper-layer lists, not %lld", (long long)gate[kHnswRemoveGateOff], (long long)blocks1);
        HG_REQUIRE(gate[kHnswRemoveGateRows] == n1, HNSWGPU_EHIP, "the list pass moved %lld layer-0 lists, not %lld",
                   (long long)gate[kHnswRemoveGateRows], (long long)n1);
        // the entry point, from the mirrors: kept -> its new id; gone -> the kept row of the highest level, the lowest id among equals
        if (n1 == 0) {
            entry1 = -1, top1 = 0;
        } else if (entry_kept) {
            entry1 = static_cast<int32_t>(below_entry), top1 = idx->max_level;
        } else {
            entry1 = 0;
            for (int64_t r = 1; r < n1; r++)
                if (h_levels[r] > h_levels[entry1]) entry1 = static_cast<int32_t>(r);
            top1 = h_levels[entry1];
        }
        return 0;
    };
    int rc;
    try {
        rc = shrink();
    } catch (const std::bad_alloc &) {
        set_error("host allocation failed in hnswgpu_hnsw_remove");
        rc = HNSWGPU_ENOMEM;
    }
    if (rc != 0) {
        (void)hipStreamSynchronize(st);  // (nothing of the chain is in flight when the staged arrays are freed)
        nw.release();
        return rc;
    }
    idx->d_base = nw.base, idx->d_norms = nw.norms, idx->d_qrows = nw.qrows, idx->d_qmeta = nw.qmeta;
    idx->d_levels = nw.levels, idx->d_l0 = nw.l0, idx->d_upadj = nw.upadj, idx->d_upoff = nw.upoff;
    idx->n = n1;
    idx->up_blocks = blocks1;
    idx->h_levels.swap(h_levels);
    idx->h_l0.swap(h_l0);
    idx->h_upoff.swap(h_upoff);
    idx->h_upadj.swap(h_upadj);
    idx->entry = entry1;
    idx->max_level = top1;
    idx->graph_gen++;
    idx->hnsw_cal_state = 0;  // as free_graph: the shrunken graph is measured afresh
    idx->hnsw_rej_off = false;
    old.release();
    if (n_after) *n_after = n1;
    return call.close();
}

// Rows of a live graph take new values (include/hnswgpu.h).  The reference has no update (its to-do list names it); the rule is
// this project's own and is its two mutation rules composed under stable ids.  UNLINK: hnswgpu_hnsw_remove's one-hop repair with
// the call's ids U as the rows that left and nothing renumbered -- one chain on the handle's stream (hnsw_update_kernels.hpp: the
// mask, the rows and norms scattered into copies, the list pass, the scan, gather, distances, sort, selection, scatter), the
// int8 rows made again over the new base.  ONE readback brings the gate's three counts and the unlinked graph.  RE-INSERT: the
// rows of U, ascending, with the levels they have, by hnswgpu_hnsw_add's insertion (insert_batches over an id list) against the
// staged arrays.  Everything is staged and the handle restored on any failure, as hnswgpu_hnsw_add does.
int hnswgpu_hnsw_update(hnswgpu_index *idx, const int32_t *ids, const float *rows, int64_t m, int32_t ef_construction) {
    HG_REQUIRE(idx, HNSWGPU_EINVAL, "idx is null");
    HG_REQUIRE(m >= 0, HNSWGPU_EINVAL, "m must be >= 0");
    HG_REQUIRE(m == 0 || ids, HNSWGPU_EINVAL, "ids is null");
    HG_REQUIRE(m == 0 || rows, HNSWGPU_EINVAL, "rows is null");
    HG_REQUIRE(ef_construction >= 1 && ef_construction <= 4096, HNSWGPU_ELIMIT, "need 1 <= ef_construction <= 4096");
    if (m == 0) return 0;
    hipStream_t st = idx->stream;
    Call call;
    HG_TRY(call.open(idx, st));
    HG_REQUIRE(idx->has_graph, HNSWGPU_ESTATE, "index has no graph (call hnswgpu_hnsw_build / hnswgpu_set_graph first)");
    HG_REQUIRE(idx->nparts == 0, HNSWGPU_ESTATE,
               "the index holds a forest of HNSW sub-graphs: an update would link a row across its part (rebuild the part's graph)");
    HG_REQUIRE(idx->nlist == 0, HNSWGPU_ESTATE, "the index holds IVF lists: they would keep the rows' old values (hnswgpu_ivf_update)");
    HG_REQUIRE(idx->lsh_tables == 0, HNSWGPU_ESTATE, "the index holds LSH tables: they would keep the rows' old values (hnswgpu_lsh_update)");
    HG_REQUIRE(idx->M0 == 2 * idx->M, HNSWGPU_ESTATE, "hnswgpu_hnsw_update needs a graph with M0 = 2 M (as hnswgpu_hnsw_build makes)");
    const int64_t n = idx->n;
    std::vector<int32_t> uid, from;  // uid: U ascending, the insertion order
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
    const int M = idx->M, M0 = idx->M0;
    const int64_t ld = idx->ld, blocks = idx->up_blocks;
    // Failure-atomic, as hnswgpu_hnsw_add: what the call makes is STAGED (levels and up_off are not: no level changes), the
    // handle's fields point at the staged arrays while the insertion searches run and are put back if any step fails.
    struct Staged {
        float *base = nullptr, *norms = nullptr;
        uint32_t *qrows = nullptr;
        float4 *qmeta = nullptr;
        int32_t *l0 = nullptr, *upadj = nullptr;
        void release() {
            void *ptrs[] = {base, norms, qrows, qmeta, l0, upadj};
            for (void *p : ptrs)
                if (p) (void)hipFree(p);
            *this = Staged();
        }
    } nw, old;
    old.base = idx->d_base, old.norms = idx->d_norms, old.qrows = idx->d_qrows, old.qmeta = idx->d_qmeta;
    old.l0 = idx->d_l0, old.upadj = idx->d_upadj;
    const int old_cal = idx->hnsw_cal_state;
    const bool old_rej_off = idx->hnsw_rej_off;
    bool installed = false;
    HostGraph g;
    auto update = [&]() -> int {
        const size_t nn = static_cast<size_t>(n), mm = static_cast<size_t>(m), ub = static_cast<size_t>(std::max<int64_t>(blocks, 1));
        // what the host knows before the device does: the lists of U (the gate's second count) and the entry the insertion starts at
        std::vector<uint8_t> in_u(nn, 0);
        int64_t u_lists = m;
        for (int64_t s = 0; s < m; s++) {
            in_u[uid[s]] = 1;
            u_lists += idx->h_levels[uid[s]];
        }
        int32_t entry1 = idx->entry, top1 = idx->max_level;
        int64_t skip = 0;  // rows of U that stand in the graph before the insertion begins
        if (m == n) {      // an empty graph: the lowest id is its first row, as hnswgpu_hnsw_add's
            entry1 = uid[0], top1 = idx->h_levels[uid[0]], skip = 1;
        } else if (entry1 < 0 || entry1 >= n || in_u[entry1]) {  // hnswgpu_hnsw_remove's rule: the highest level, the lowest id among equals
            entry1 = -1;
            for (int64_t r = 0; r < n; r++)
                if (!in_u[r] && (entry1 < 0 || idx->h_levels[r] > idx->h_levels[entry1])) entry1 = static_cast<int32_t>(r);
            top1 = idx->h_levels[entry1];
        }
        // ---- 1. copies of the base and the norms take the call's rows; the int8 rows are made again
        OwnedBuf d_stage;
        HG_TRY(d_stage.ensure(sizeof(float) * mm * (ld + 1)));
        float *stage = d_stage.as<float>(), *snorms = stage + mm * ld;
        HG_HIP(hipMalloc(reinterpret_cast<void **>(&nw.base), sizeof(float) * nn * ld));
        HG_HIP(hipMalloc(reinterpret_cast<void **>(&nw.norms), sizeof(float) * nn));
        HG_HIP(hipMalloc(reinterpret_cast<void **>(&nw.l0), sizeof(int32_t) * nn * M0));
        HG_HIP(hipMalloc(reinterpret_cast<void **>(&nw.upadj), sizeof(int32_t) * ub * M));
        HG_HIP(hipMemcpyAsync(nw.base, old.base, sizeof(float) * nn * ld, hipMemcpyDeviceToDevice, st));
        HG_HIP(hipMemcpyAsync(nw.norms, old.norms, sizeof(float) * nn, hipMemcpyDeviceToDevice, st));
        HG_HIP(hipMemsetAsync(nw.l0, 0xff, sizeof(int32_t) * nn * M0, st));
        HG_HIP(hipMemsetAsync(nw.upadj, 0xff, sizeof(int32_t) * ub * M, st));
        if (ld != idx->dim) HG_HIP(hipMemsetAsync(stage, 0, sizeof(float) * mm * ld, st));
        HG_HIP(hipMemcpy2DAsync(stage, sizeof(float) * ld, rows, sizeof(float) * idx->dim, sizeof(float) * idx->dim, mm, hipMemcpyHostToDevice, st));
        HG_TRY(launch_norms(idx->nch, stage, ld, m, snorms, st));
        // ---- 2. the unlink: the mask of U, then hnswgpu_hnsw_remove's repair at the lists' own places under the old ids
        HnswRemoveArgs a;
        memset(&a, 0, sizeof(a));
        a.r.n0 = a.r.n1 = n;
        a.r.m = m;
        a.r.W = (n + 31) / 32;
        a.r.ld = ld;
        a.M = M;
        a.M0 = M0;
        a.blocks0 = a.blocks1 = blocks;
        a.nlists = n + blocks;
        HG_TRY(hnsw_repair_scratch(idx, a, ids, st));
        a.old_levels = idx->d_levels;
        a.old_l0 = old.l0;
        a.old_upadj = old.upadj;
        a.old_upoff = idx->d_upoff;
        a.new_levels = idx->d_levels;  // (never written: the levels kernel is hnswgpu_hnsw_remove's alone)
        a.new_upoff = idx->d_upoff;
        a.new_l0 = nw.l0;
        a.new_upadj = nw.upadj;
        const HnswUpdateRows ur = {n, m, ld, a.r.rows, stage, snorms, nw.base, nw.norms};
        hipLaunchKernelGGL(lsh_remove_mark_kernel, dim3(static_cast<unsigned>((m + kWG - 1) / kWG)), dim3(kWG), 0, st, a.r);
        hipLaunchKernelGGL(lsh_remove_rank_kernel, dim3(1), dim3(kWG), 0, st, a.r);
        hipLaunchKernelGGL(hnsw_update_rows_kernel, dim3(static_cast<unsigned>((m + kNWave - 1) / kNWave)), dim3(kWG), 0, st, ur);
        HG_HIP(hipGetLastError());
        if (old.qrows) HG_TRY(quantize_rows(idx, nw.base, n, &nw.qrows, &nw.qmeta, st));  // (as add: one pass over the new base)
        HG_TRY(hnsw_repair_chain<false>(idx, a, st));  // (distances over the handle's old rows: no row of U takes part in any)
        // ---- the one readback: the gate and the unlinked graph, for the linker and the host mirrors
        int64_t gate[kLshRemoveGate];
        std::vector<int32_t> h_l0(nn * M0), h_upadj(static_cast<size_t>(blocks) * M);
        HG_HIP(hipMemcpyAsync(gate, a.r.gate, sizeof(gate), hipMemcpyDeviceToHost, st));
        HG_HIP(hipMemcpyAsync(h_l0.data(), nw.l0, sizeof(int32_t) * nn * M0, hipMemcpyDeviceToHost, st));
        if (blocks > 0) HG_HIP(hipMemcpyAsync(h_upadj.data(), nw.upadj, sizeof(int32_t) * blocks * M, hipMemcpyDeviceToHost, st));
        HG_HIP(hipStreamSynchronize(st));
        HG_REQUIRE(gate[kHnswUpdateGateKept] == n - m, HNSWGPU_EHIP, "the mask marks %lld rows, not %lld", (long long)(n - gate[kHnswUpdateGateKept]),
                   (long long)m);
        HG_REQUIRE(gate[kHnswUpdateGateCleared] == u_lists, HNSWGPU_EHIP, "the list pass cleared %lld lists, not %lld",
                   (long long)gate[kHnswUpdateGateCleared], (long long)u_lists);
        HG_REQUIRE(gate[kHnswUpdateGateSeen] == n - m, HNSWGPU_EHIP, "the list pass saw %lld rows outside the call, not %lld",
                   (long long)gate[kHnswUpdateGateSeen], (long long)(n - m));
        // ---- 3. the insertion searches run against the staged arrays
        idx->d_base = nw.base, idx->d_norms = nw.norms, idx->d_qrows = nw.qrows, idx->d_qmeta = nw.qmeta;
        idx->d_l0 = nw.l0, idx->d_upadj = nw.upadj;
        idx->graph_gen++;
        idx->hnsw_cal_state = 0;  // as hnswgpu_hnsw_remove: the new graph is measured afresh
        idx->hnsw_rej_off = false;
        installed = true;
        g.n = n;
        g.M = M;
        g.M0 = M0;
        g.levels = idx->h_levels;
        g.up_off = idx->h_upoff;
        g.l0.assign(nn * (M0 + 1), -1);
        g.l0_d.assign(nn * (M0 + 1), 0.f);
        g.l0_cnt.assign(nn, 0);
        g.up.assign(ub * (M + 1), -1);
        g.up_d.assign(ub * (M + 1), 0.f);
        g.up_cnt.assign(ub, 0);
        g.sorted0.assign(nn, 0);
        g.sortedu.assign(ub, 0);
        HG_TRY(adopt_graph(idx, g, n, h_l0.data(), h_upadj.data(), idx->h_upoff.data(), st));
        g.entry = entry1;
        g.top = top1;
        HG_TRY(insert_batches(idx, g, n - m + skip, ef_construction, st, idx->build_flags & ~HNSWGPU_BUILD_SEQUENTIAL, uid.data() + skip, m - skip));
        HG_TRY(publish_graph(idx, g, st));  // (host mirrors, entry, max_level: assigned only once the uploads succeeded)
        idx->hnsw_cal_state = 0;  // (the insertion's own launches are not the measurement of the graph that now stands)
        idx->hnsw_rej_off = false;
        return 0;
    };
    int rc;
    try {
        rc = update();
    } catch (const std::bad_alloc &) {
        set_error("host allocation failed in hnswgpu_hnsw_update");
        rc = HNSWGPU_ENOMEM;
    }
    if (rc != 0) {
        (void)hipStreamSynchronize(st);  // (nothing of the call is in flight when the staged arrays are freed)
        if (installed) {
            idx->d_base = old.base, idx->d_norms = old.norms, idx->d_qrows = old.qrows, idx->d_qmeta = old.qmeta;
            idx->d_l0 = old.l0, idx->d_upadj = old.upadj;
            idx->graph_gen++;
            idx->hnsw_cal_state = old_cal;
            idx->hnsw_rej_off = old_rej_off;
        }
        nw.release();
        return rc;
    }
    old.release();
    return call.close();
}

}  // extern "C"
