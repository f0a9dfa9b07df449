// hnsw_remove_kernels.hpp -- rows leave a live HNSW graph (hnsw.hip: hnswgpu_hnsw_remove).  The mask of the rows that go, the rank
// scan and the row mover are remove_kernels.hpp's (tables = 0); what is here is the graph side: the kept rows' levels and the
// shrunken up_off, every kept list renumbered and closed up, and the RE-SELECTION of every list that lost a member from the OLD
// graph alone: its kept members joined with the kept members of the same-layer lists of the members that left (one hop through
// what left), their distances to the list's node by the traversal's arithmetic, sorted ascending by (distance, id) with repeats
// dropped -- the cand_id / cand_d / off of heuristic_select_kernel (build_kernels.hpp) -- and the selection written over the
// list under the new ids.  Every kernel reads the old arrays and writes the staged ones: no list ever sees another list's repair.
// A wave per adjacency list (kMaxDeg <= kWave: a lane per slot), ballot / popcount for the in-wave compaction, LDS for the sort.
// No kernel waits for another workgroup; every loop is bounded by n0, w or w * w; every index is checked before its store; the
// one atomicAdd counts (a commutative sum) and decides no destination.  Included by hnsw.hip only.
// The list pass and the scatter carry a template parameter RENUM: true is the removal described above; false is the UNLINK of
// hnswgpu_hnsw_update (hnsw_update_kernels.hpp), the same repair with nothing renumbered -- every list stays at its place (the
// staged arrays have the old shape: new_upoff = old_upoff, blocks1 = blocks0, n1 = n0), ids are written as they are, and the
// lists of the marked rows themselves are cleared instead of dropped.
#pragma once
#include "build_kernels.hpp"
#include "remove_kernels.hpp"

namespace hg {

static_assert(kMaxDeg <= kWave, "a lane per slot of an adjacency list");
static_assert(kMaxDeg * kMaxDeg <= kSelMaxCand, "w kept members of each of w members that left fit one selection task");

// words of LshRemoveArgs::gate the graph side writes (the rank scan's total stays at 2 * kRemoveMaxTables)
constexpr int kHnswRemoveGateOff = 0;    // the new up_off[n1]
constexpr int kHnswRemoveGateRows = 1;   // kept layer-0 lists the list pass saw
constexpr int kHnswRemoveGateCand = 2;   // candidates of all tasks
constexpr int kHnswRemoveGateTasks = 3;  // lists to select again
constexpr int kHnswRemoveGateCleared = 4;  // RENUM = false: lists of marked rows the list pass cleared

struct HnswRemoveArgs {
    LshRemoveArgs r;     // n0, n1, m, W, ld, rows, keep, word_rank, old / new base and norms, gate; tables = 0
    int32_t M, M0;
    int64_t blocks0, blocks1;  // upper-layer lists before / after (blocks1: the kept rows' levels summed on the host)
    int64_t nlists;            // n0 + blocks0: list t < n0 is node t's layer 0, list n0 + b is upper block b
    const int32_t *old_levels, *old_l0, *old_upadj;
    const int64_t *old_upoff;
    int32_t *new_levels, *new_l0, *new_upadj;
    int64_t *new_upoff;
    int32_t *owner;      // [blocks0] the node of an old upper block
    uint32_t *cnt;       // [nlists] candidates of a list that lost a member (u excluded, repeats included); 0: nothing to select
    int32_t *task_list;  // [nlists] the lists with cnt > 0, ascending
    int64_t *task_off;   // [nlists + 1] a task's range of cand_id / cand_d
    int32_t *task_m;     // [nlists] links wanted: M0 at layer 0, M above
    int64_t ntasks, ncand;  // read back behind the scan: what cand_id / cand_d are sized by
    int32_t *cand_id;    // OLD ids
    float *cand_d;
    const int32_t *sel;  // [ntasks][M0] heuristic_select_kernel's out_id, or null: the first w of a task's sorted range
};

// list t of the old graph: its node, layer, width and slots.  false: no such list (or an owner out of range: never)
__device__ __forceinline__ bool hnsw_remove_list(const HnswRemoveArgs &a, int64_t t, int64_t &u, int &lc, int &w, const int32_t *&old) {
    if (t < 0 || t >= a.nlists) return false;
    if (t < a.r.n0) {
        u = t, lc = 0, w = a.M0;
        old = a.old_l0 + t * a.M0;
        return true;
    }
    const int64_t b = t - a.r.n0;
    u = a.owner[b];
    if (u < 0 || u >= a.r.n0) return false;
    lc = static_cast<int>(b - a.old_upoff[u]) + 1;
    w = a.M;
    old = a.old_upadj + b * a.M;
    return lc >= 1 && lc <= a.old_levels[u];
}

// node v's list on layer lc of the old graph, or null where v does not reach that layer
__device__ __forceinline__ const int32_t *hnsw_remove_list_of(const HnswRemoveArgs &a, int64_t v, int lc) {
    if (lc == 0) return a.old_l0 + v * a.M0;
    if (a.old_levels[v] < lc) return nullptr;
    const int64_t b = a.old_upoff[v] + lc - 1;
    if (b < 0 || b >= a.blocks0) return nullptr;
    return a.old_upadj + b * a.M;
}

// the id a kept row carries in the staged graph: its rank among the kept rows, or (RENUM = false) the id it has
template <bool RENUM>
__device__ __forceinline__ int64_t hnsw_remove_id(const HnswRemoveArgs &a, int64_t r) {
    return RENUM ? lsh_remove_rank(a.r, r) : r;
}

// where list (u, lc) of a KEPT node stands in the staged graph (RENUM = false: of any node), or null (never: the gate would say so)
template <bool RENUM>
__device__ __forceinline__ int32_t *hnsw_remove_dest(const HnswRemoveArgs &a, int64_t u, int lc) {
    const int64_t to = hnsw_remove_id<RENUM>(a, u);
    if (to < 0 || to >= a.r.n1) return nullptr;
    if (lc == 0) return a.new_l0 + to * a.M0;
    const int64_t b = a.new_upoff[to] + lc - 1;
    if (b < 0 || b >= a.blocks1) return nullptr;
    return a.new_upadj + b * a.M;
}

// 1. ONE workgroup: the kept rows' levels to their ranks, the new up_off as the exclusive sum of the kept levels (block scan with
// a carry, as lsh_remove_rank_kernel)
static __global__ __launch_bounds__(kWG) void hnsw_remove_levels_kernel(HnswRemoveArgs a) {
    __shared__ uint32_t wsum[kNWave];
    int64_t carry = 0;
    for (int64_t r0 = 0; r0 < a.r.n0; r0 += kWG) {
        const int64_t r = r0 + threadIdx.x;
        const bool kept = lsh_remove_kept(a.r, r);
        const int32_t lv = kept ? a.old_levels[r] : 0;
        uint32_t total;
        const int64_t before = carry + wg_exclusive_sum(static_cast<uint32_t>(lv > 0 ? lv : 0), wsum, &total);
        if (kept) {
            const int64_t to = lsh_remove_rank(a.r, r);
            if (to < a.r.n1) {
                a.new_levels[to] = lv;
                a.new_upoff[to] = before;
            }
        }
        carry += total;
    }
    if (threadIdx.x == 0) {
        a.new_upoff[a.r.n1] = carry;
        a.r.gate[kHnswRemoveGateOff] = carry;
    }
}

// 1b. A thread per old node: the owner of each of its upper blocks (as many as its level)
static __global__ __launch_bounds__(kWG) void hnsw_remove_owner_kernel(HnswRemoveArgs a) {
    const int64_t r = static_cast<int64_t>(blockIdx.x) * kWG + threadIdx.x;
    if (r >= a.r.n0) return;
    const int64_t b0 = a.old_upoff[r];
    const int32_t lv = a.old_levels[r];
    for (int32_t i = 0; i < lv; i++)
        if (b0 + i >= 0 && b0 + i < a.blocks0) a.owner[b0 + i] = static_cast<int32_t>(r);
}

// 2. One wave per old list of a kept node: its kept members in their order under their new ids, -1 padded, to the list's new
// place; and, if a member left, the number of its candidates.  RENUM = false: a list of a marked node is cleared at its place
template <bool RENUM>
__global__ __launch_bounds__(kWG) void hnsw_remove_lists_kernel(HnswRemoveArgs a) {
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t t = static_cast<int64_t>(blockIdx.x) * kNWave + (threadIdx.x >> 6);
    int64_t u;
    int lc, w;
    const int32_t *old;
    if (!hnsw_remove_list(a, t, u, lc, w, old)) return;  // (wave-uniform, as every branch on t, u, lc below)
    const bool u_kept = lsh_remove_kept(a.r, u);
    if (RENUM && !u_kept) return;
    int32_t *dst = hnsw_remove_dest<RENUM>(a, u, lc);
    if (!dst) return;
    if (!RENUM && !u_kept) {
        if (lane < w) dst[lane] = -1;
        if (lane == 0) atomicAdd(reinterpret_cast<unsigned long long *>(a.r.gate + kHnswRemoveGateCleared), 1ull);
        return;
    }
    const int32_t nb = lane < w ? old[lane] : -1;
    const bool valid = nb >= 0 && nb < a.r.n0;
    const bool kept = valid && lsh_remove_kept(a.r, nb);
    const uint64_t mk = __ballot(kept), ml = __ballot(valid && !kept);
    const uint64_t below = (1ull << lane) - 1ull;
    const int nk = __popcll(mk);
    if (kept) dst[__popcll(mk & below)] = static_cast<int32_t>(hnsw_remove_id<RENUM>(a, nb));
    if (lane >= nk && lane < w) dst[lane] = -1;
    if (lane == 0 && lc == 0) atomicAdd(reinterpret_cast<unsigned long long *>(a.r.gate + kHnswRemoveGateRows), 1ull);
    if (ml == 0) return;
    int c = __popcll(__ballot(kept && nb != u));
    for (uint64_t rest = ml; rest != 0; rest &= rest - 1) {  // at most w members that left
        const int j = __ffsll(static_cast<unsigned long long>(rest)) - 1;
        const int64_t v = __shfl(nb, j, kWave);
        const int32_t *lst = hnsw_remove_list_of(a, v, lc);
        if (!lst) continue;
        const int32_t x = lane < w ? lst[lane] : -1;
        c += __popcll(__ballot(x >= 0 && x < a.r.n0 && x != u && lsh_remove_kept(a.r, x)));
    }
    if (lane == 0) a.cnt[t] = static_cast<uint32_t>(c);
}

// 3. ONE workgroup: the exact scan of the candidate counts and of the lists that have any -- every task's list, width and range
static __global__ __launch_bounds__(kWG) void hnsw_remove_scan_kernel(HnswRemoveArgs a) {
    __shared__ uint32_t wsum[kNWave];
    int64_t carry_c = 0, carry_t = 0;
    for (int64_t t0 = 0; t0 < a.nlists; t0 += kWG) {
        const int64_t t = t0 + threadIdx.x;
        const uint32_t c = t < a.nlists ? a.cnt[t] : 0u;
        uint32_t total_c, total_t;
        const int64_t before_c = carry_c + wg_exclusive_sum(c, wsum, &total_c);
        const int64_t k = carry_t + wg_exclusive_sum(c > 0 ? 1u : 0u, wsum, &total_t);
        if (c > 0 && k < a.nlists) {
            a.task_list[k] = static_cast<int32_t>(t);
            a.task_off[k] = before_c;
            a.task_m[k] = t < a.r.n0 ? a.M0 : a.M;
        }
        carry_c += total_c;
        carry_t += total_t;
    }
    if (threadIdx.x == 0) {
        if (carry_t <= a.nlists) a.task_off[carry_t] = carry_c;
        a.r.gate[kHnswRemoveGateCand] = carry_c;
        a.r.gate[kHnswRemoveGateTasks] = carry_t;
    }
}

// 4. One wave per task: the candidates' OLD ids into the task's range, in the order the list pass counted them
static __global__ __launch_bounds__(kWG) void hnsw_remove_gather_kernel(HnswRemoveArgs a) {
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t k = static_cast<int64_t>(blockIdx.x) * kNWave + (threadIdx.x >> 6);
    if (k >= a.ntasks) return;
    int64_t u;
    int lc, w;
    const int32_t *old;
    if (!hnsw_remove_list(a, a.task_list[k], u, lc, w, old)) return;
    const int64_t base = a.task_off[k], end = a.task_off[k + 1];
    if (base < 0 || end > a.ncand) return;
    const uint64_t below = (1ull << lane) - 1ull;
    const int32_t nb = lane < w ? old[lane] : -1;
    const bool valid = nb >= 0 && nb < a.r.n0;
    const bool kept = valid && lsh_remove_kept(a.r, nb);
    const uint64_t ml = __ballot(valid && !kept);
    const bool mine = kept && nb != u;
    uint64_t mk = __ballot(mine);
    int64_t pos = base + __popcll(mk & below);
    if (mine && pos < end) a.cand_id[pos] = nb;
    int64_t filled = base + __popcll(mk);
    for (uint64_t rest = ml; rest != 0; rest &= rest - 1) {
        const int j = __ffsll(static_cast<unsigned long long>(rest)) - 1;
        const int64_t v = __shfl(nb, j, kWave);
        const int32_t *lst = hnsw_remove_list_of(a, v, lc);
        if (!lst) continue;
        const int32_t x = lane < w ? lst[lane] : -1;
        const bool ok = x >= 0 && x < a.r.n0 && x != u && lsh_remove_kept(a.r, x);
        mk = __ballot(ok);
        pos = filled + __popcll(mk & below);
        if (ok && pos < end) a.cand_id[pos] = x;
        filled += __popcll(mk);
    }
}

// 5. One wave per task: d(u, c) of its candidates -- edge_dist_kernel (hnsw.hip) over ranges of an offset table: the same loads,
// the same lane sums, the same finish on the stored norms
template <int NCH, int RB, bool L2>
__global__ __launch_bounds__(kWG) void hnsw_remove_dist_kernel(HnswRemoveArgs a, const float *rows, const float *norms, int dim, int metric) {
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t k = static_cast<int64_t>(blockIdx.x) * kNWave + (threadIdx.x >> 6);
    if (k >= a.ntasks) return;
    int64_t u;
    int lc, w;
    const int32_t *old;
    if (!hnsw_remove_list(a, a.task_list[k], u, lc, w, old)) return;
    const int64_t base = a.task_off[k];
    int64_t end = a.task_off[k + 1];
    if (base < 0 || end > a.ncand) return;
    if (end - base > kSelMaxCand) end = base + kSelMaxCand;
    const int64_t ld = a.r.ld;
    const int nvec = static_cast<int>(ld / 4);
    float4 q[NCH];
    load_row<NCH>(q, rows + u * ld, nvec, lane, true);
    const float qn = metric == METRIC_COS ? norms[u] : 0.0f;
    for (int64_t j0 = base; j0 < end; j0 += RB) {
        float4 r[RB][NCH];
        int32_t nb[RB];
#pragma unroll
        for (int b = 0; b < RB; b++) {
            nb[b] = j0 + b < end ? a.cand_id[j0 + b] : -1;
            if (nb[b] >= a.r.n0) nb[b] = -1;
            load_row<NCH>(r[b], rows + static_cast<int64_t>(nb[b] >= 0 ? nb[b] : 0) * ld, nvec, lane, nb[b] >= 0);
        }
#pragma unroll
        for (int b = 0; b < RB; b++) {
            const float sum = wave_sum(lane_partial<NCH, L2>(q, r[b]));
            if (lane == 0 && j0 + b < end)
                a.cand_d[j0 + b] = nb[b] >= 0 ? finish_dist(metric, sum, qn, metric == METRIC_COS ? norms[nb[b]] : 0.0f) : 0.0f;
        }
    }
}

// a float as a word that ascends with it (-0 with +0: equal distances are told apart by the id alone) and back
__device__ __forceinline__ uint32_t hnsw_remove_key(float d) {
    const uint32_t b = d == 0.0f ? 0u : __float_as_uint(d);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float hnsw_remove_unkey(uint32_t s) { return __uint_as_float((s & 0x80000000u) ? (s & 0x7fffffffu) : ~s); }

// 6. One workgroup per task: its range sorted ascending by (distance, id) in LDS (a bitonic network over the next power of two,
// all-ones beyond the range) and written back without the repeats -- an id twice carries the same distance bits twice, so its
// copies are neighbours -- the rest of the range -1: what heuristic_select_kernel reads as padding
static __global__ __launch_bounds__(kWG) void hnsw_remove_sort_kernel(HnswRemoveArgs a) {
    __shared__ uint64_t key[kSelMaxCand];
    __shared__ uint32_t wsum[kNWave];
    const int64_t k = blockIdx.x;
    if (k >= a.ntasks) return;
    const int64_t base = a.task_off[k], end = a.task_off[k + 1];
    if (base < 0 || end > a.ncand || end <= base) return;  // (uniform over the workgroup)
    const int tid = threadIdx.x;
    int C = static_cast<int>(end - base > kSelMaxCand ? kSelMaxCand : end - base);
    int P = 2;
    while (P < C) P <<= 1;
    for (int i = tid; i < P; i += kWG)
        key[i] = i < C ? (static_cast<uint64_t>(hnsw_remove_key(a.cand_d[base + i])) << 32) | static_cast<uint32_t>(a.cand_id[base + i])
                       : ~0ull;
    __syncthreads();
    for (int kk = 2; kk <= P; kk <<= 1)
        for (int j = kk >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < P; i += kWG) {
                const int p = i ^ j;
                if (p > i) {
                    const uint64_t x = key[i], y = key[p];
                    if ((x > y) == ((i & kk) == 0)) {
                        key[i] = y;
                        key[p] = x;
                    }
                }
            }
            __syncthreads();
        }
    int64_t carry = 0;
    for (int i0 = 0; i0 < C; i0 += kWG) {
        const int i = i0 + tid;
        const bool first = i < C && (i == 0 || static_cast<uint32_t>(key[i]) != static_cast<uint32_t>(key[i - 1]));
        uint32_t total;
        const int64_t to = carry + wg_exclusive_sum(first ? 1u : 0u, wsum, &total);
        if (first && to < C) {
            a.cand_id[base + to] = static_cast<int32_t>(static_cast<uint32_t>(key[i]));
            a.cand_d[base + to] = hnsw_remove_unkey(static_cast<uint32_t>(key[i] >> 32));
        }
        carry += total;
    }
    for (int64_t i = carry + tid; i < end - base; i += kWG) {
        a.cand_id[base + i] = -1;
        a.cand_d[base + i] = 0.0f;
    }
}

// 7. One wave per task: the selection -- heuristic_select_kernel's, or the first w of the sorted range -- over the task's list in
// the staged graph, under the new ids (RENUM = false: the ids as they are), -1 padded
template <bool RENUM>
__global__ __launch_bounds__(kWG) void hnsw_remove_scatter_kernel(HnswRemoveArgs a) {
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t k = static_cast<int64_t>(blockIdx.x) * kNWave + (threadIdx.x >> 6);
    if (k >= a.ntasks) return;
    int64_t u;
    int lc, w;
    const int32_t *old;
    if (!hnsw_remove_list(a, a.task_list[k], u, lc, w, old)) return;
    if (!lsh_remove_kept(a.r, u)) return;
    int32_t *dst = hnsw_remove_dest<RENUM>(a, u, lc);
    if (!dst || lane >= w) return;
    const int64_t base = a.task_off[k], end = a.task_off[k + 1];
    int32_t id = -1;
    if (a.sel) id = a.sel[k * a.M0 + lane];
    else if (base >= 0 && base + lane < end && end <= a.ncand) id = a.cand_id[base + lane];
    dst[lane] = (id >= 0 && lsh_remove_kept(a.r, id)) ? static_cast<int32_t>(hnsw_remove_id<RENUM>(a, id)) : -1;
}

}  // namespace hg
