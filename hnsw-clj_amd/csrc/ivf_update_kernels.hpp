// ivf_update_kernels.hpp -- rows of a live handle with inverted lists take new values (ivf.hip: hnswgpu_ivf_update).  Slot s of a
// call is its s-th smallest row id (ivf_update_ids.hpp).  Here: the call's rows into a staging matrix in slot order, their scatter
// into the staged base, every slot's present list and whether it leaves it, the offsets of the new lists, the stable compaction
// of the positions that remain, the placement of the movers behind them, and the splice of the list-order rows.  Integer work
// and row copies only: the distances behind `assign` are the scan kernel's (kernels.hpp, GEMV order), the norms are
// row_norms_kernel's, the int8 / half copies are made by the kernels that make them for a fresh set of lists.  The mask of the
// rows that remain in their lists is the keep mask of remove_kernels.hpp, so its rank, chunk count and chunk scan kernels run
// unchanged over it.  Every destination is a function of the old arrays and the call alone -- prefix counts of the positions that
// remain, a mover's STABLE rank in slot order among the movers into its list -- never of the order atomics arrive in (the only
// atomics are integer sums and an OR).  No kernel waits for another workgroup, every loop is bounded by kWG, ld or log2(nlist),
// and every index is checked against n / m / nlist before its store.
#pragma once
#include "remove_kernels.hpp"

namespace hg {

constexpr uint32_t kUpdBadAssign = 1;    // IvfUpdateArgs::flags: a new row without a nearest list (assign >= nlist, a NaN distance or a NaN norm)
constexpr uint32_t kUpdNotIdentity = 2;  // a new list position that does not hold the row of the same number
constexpr uint32_t kUpdStaged = 0xffffffffu;  // IvfUpdateArgs::origin of a position whose row comes from the staging matrix
constexpr int kUpdLdsLists = 2048;       // lists up to which a workgroup searches the offsets in LDS
constexpr int kUpdCounts = 4;            // IvfUpdateArgs::counts: movers, stayers, positions joined, new_off[nlist]

struct IvfUpdateArgs {
    // the keep mask and the compaction's first two steps: n0 = n1 = n, W, nchunks, keep (the DROP bits of the movers until
    // lsh_remove_rank_kernel), word_rank, chunk_base, old_ids = the list ids.  Of its gate, [2 * kRemoveMaxTables] is the rows that
    // do not move (rank scan) and [kRemoveMaxTables] the list positions that remain (lsh_remove_chunk_scan_kernel)
    LshRemoveArgs r;
    int64_t m;
    int32_t nlist, dim;
    const int32_t *uid;      // [m] slot -> row id, ascending
    const int32_t *from;     // [m] slot -> position in the caller's arrays
    const float *raw;        // [m][dim] the caller's rows as they came
    float *stage;            // [m][ld] ... in slot order, padding zeroed
    const float *snorms;     // [m] their norms (row_norms_kernel)
    const uint32_t *assign;  // [m] their nearest lists
    const float *adist;      // [m] ... and the distances to them (NaN: the scan named a list all the same)
    int32_t *slot_of;        // [n] row -> slot, -1 = not updated (all ones before ivf_update_stage_kernel)
    int32_t *slot_list;      // [m] the list slot s sits in (all ones before ivf_update_mark_kernel)
    uint32_t *leave, *join;  // [nlist] positions that leave / join a list (zero before ivf_update_mark_kernel)
    unsigned long long *counts;  // [kUpdCounts] zero before ivf_update_mark_kernel
    uint32_t *flags;         // [1] kUpd*, zero before ivf_update_mark_kernel
    const int64_t *old_off;  // [nlist + 1]
    int64_t *new_off;        // [nlist + 1]
    int64_t *kept_off;       // [nlist + 1] the positions that remain below list l: old_off[l] - leaves below l
    uint32_t *src;           // [n] the old position of the k-th position that remains
    int32_t *new_ids;        // [n]
    uint32_t *origin;        // [n] the old position a new position's row comes from, or kUpdStaged
    const float *old_lrows, *old_lnorms;
    float *new_base, *new_norms, *new_lrows, *new_lnorms;
};

// the list of position p: the last l with off[l] <= p (empty lists share an offset with their successor).  At most 32 steps.
__device__ __forceinline__ int ivf_update_list_of(const int64_t *off, int nlist, int64_t p) {
    int lo = 0, hi = nlist;
    while (lo + 1 < hi) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] <= p) lo = mid;
        else hi = mid;
    }
    return lo;
}

// the offsets a workgroup searches: a copy in LDS when it fits (all threads call this), the global array otherwise
__device__ __forceinline__ const int64_t *ivf_update_offsets_in_lds(const int64_t *off, int nlist, int64_t *lds) {
    if (nlist > kUpdLdsLists) return off;
    for (int l = threadIdx.x; l <= nlist; l += kWG) lds[l] = off[l];
    __syncthreads();
    return lds;
}

// 1. One wave per slot: the caller's row `from[s]` becomes row s of the staging matrix (ld floats, the padding zero), and the
// row-to-slot map learns the slot.
__global__ __launch_bounds__(kWG) void ivf_update_stage_kernel(IvfUpdateArgs a) {
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t s = static_cast<int64_t>(blockIdx.x) * kNWave + (threadIdx.x >> 6);
    if (s >= a.m) return;  // (wave-uniform)
    const int64_t f = a.from[s], r = a.uid[s];
    if (f < 0 || f >= a.m || r < 0 || r >= a.r.n0) return;
    const float *sp = a.raw + f * a.dim;
    float *dp = a.stage + s * a.r.ld;
    for (int64_t j = lane; j < a.r.ld; j += kWave) dp[j] = j < a.dim ? sp[j] : 0.0f;
    if (lane == 0) a.slot_of[r] = static_cast<int32_t>(s);
}

// 2. One wave per slot: the staged row and its norm replace row uid[s] of the staged base (a device copy of the old one).
__global__ __launch_bounds__(kWG) void ivf_update_base_kernel(IvfUpdateArgs a) {
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t s = static_cast<int64_t>(blockIdx.x) * kNWave + (threadIdx.x >> 6);
    if (s >= a.m) return;  // (wave-uniform)
    const int64_t r = a.uid[s];
    if (r < 0 || r >= a.r.n0) return;
    const float4 *sp = reinterpret_cast<const float4 *>(a.stage + s * a.r.ld);
    float4 *dp = reinterpret_cast<float4 *>(a.new_base + r * a.r.ld);
    for (int64_t j = lane; j < a.r.ld / 4; j += kWave) dp[j] = sp[j];
    if (lane == 0) a.new_norms[r] = a.snorms[s];
}

// 3. One thread per OLD list position: a position that holds an updated row names the slot's present list; the slot is a mover when
// its new nearest list is another one -- its row's bit goes into the mask (DROP bits), its old list counts a leave, its new list
// a join -- and a stayer otherwise.  (A slot without a nearest list -- no list named, a NaN distance, which the scan's keys order like
// any other value, or a NaN norm, which the cosine distance answers with 1 for every centroid -- stays where it is; the call fails
// at the readback.)
__global__ __launch_bounds__(kWG) void ivf_update_mark_kernel(IvfUpdateArgs a) {
    __shared__ int64_t soff[kUpdLdsLists + 1];
    const int64_t *off = ivf_update_offsets_in_lds(a.old_off, a.nlist, soff);
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t p = static_cast<int64_t>(blockIdx.x) * kWG + threadIdx.x;
    const int64_t r = p < a.r.n0 ? a.r.old_ids[p] : -1;
    const int64_t s = r >= 0 && r < a.r.n0 ? a.slot_of[r] : -1;
    bool mover = false, stayer = false, bad = false;
    if (s >= 0 && s < a.m) {
        const int l = ivf_update_list_of(off, a.nlist, p);
        const uint32_t to = a.assign[s];
        const float d = a.adist[s], nrm = a.snorms[s];
        bad = to >= static_cast<uint32_t>(a.nlist) || d != d || nrm != nrm;
        a.slot_list[s] = bad ? static_cast<int32_t>(to) : l;  // (bad: never a mover for ivf_update_place_kernel either)
        mover = !bad && to != static_cast<uint32_t>(l);
        stayer = !mover;
        if (mover) {
            atomicOr(a.r.keep + (r >> 5), 1u << (r & 31));
            atomicAdd(a.leave + l, 1u);
            atomicAdd(a.join + to, 1u);
        }
    }
    const unsigned long long bm = __ballot(mover), bs = __ballot(stayer);
    const bool any_bad = __any(bad);
    if (lane == 0) {
        if (bm) atomicAdd(a.counts + 0, static_cast<unsigned long long>(__popcll(bm)));
        if (bs) atomicAdd(a.counts + 1, static_cast<unsigned long long>(__popcll(bs)));
        if (any_bad) atomicOr(a.flags, kUpdBadAssign);
    }
}

// 4. ONE workgroup: kept_off[l] = old_off[l] - the leaves below l, new_off[l] = kept_off[l] + the joins below l (two block scans
// with a carry, the scan of ivf_add_offsets_kernel).  A list every member of which leaves keeps its place with two equal offsets.
__global__ __launch_bounds__(kWG) void ivf_update_offsets_kernel(IvfUpdateArgs a) {
    __shared__ uint32_t wsum[kNWave];
    int64_t left = 0, joined = 0;
    for (int l0 = 0; l0 <= a.nlist; l0 += kWG) {
        const int l = l0 + threadIdx.x;
        uint32_t tl, tj;
        const uint32_t bl = wg_exclusive_sum(l < a.nlist ? a.leave[l] : 0u, wsum, &tl);
        const uint32_t bj = wg_exclusive_sum(l < a.nlist ? a.join[l] : 0u, wsum, &tj);
        if (l <= a.nlist) {
            const int64_t kept = a.old_off[l] - (left + bl);
            a.kept_off[l] = kept;
            a.new_off[l] = kept + joined + bj;
            if (l == a.nlist) a.counts[3] = static_cast<unsigned long long>(kept + joined + bj);
        }
        left += tl;
        joined += tj;
    }
}

// 5. The stable compaction of the positions that remain (the shape of ivf_remove_ids_kernel; chunk_base is the scanned output of
// lsh_remove_chunk_count_kernel / lsh_remove_chunk_scan_kernel over the same mask): the position p that remains as the k-th --
// its chunk's base plus those before it in the chunk -- is recorded as src[k].  Lists are contiguous and the order of positions is
// kept: the members of list l that remain are src[kept_off[l] .. kept_off[l + 1]), in their old order.
__global__ __launch_bounds__(kWG) void ivf_update_compact_kernel(IvfUpdateArgs a) {
    __shared__ uint32_t wsum[kNWave];
    const int64_t p = static_cast<int64_t>(blockIdx.x) * kWG + threadIdx.x;
    const int64_t r = p < a.r.n0 ? a.r.old_ids[p] : -1;
    const bool kept = lsh_remove_kept(a.r, r);
    uint32_t total;
    const uint32_t before = wg_exclusive_sum(kept ? 1u : 0u, wsum, &total);
    if (p >= a.r.n0 || !kept) return;
    const int64_t k = static_cast<int64_t>(a.r.chunk_base[blockIdx.x]) + before;
    if (k < a.r.n0) a.src[k] = static_cast<uint32_t>(p);
}

// 6. One workgroup per list (the shape of ivf_add_place_kernel): the call's movers INTO the list, in slot order -- ascending by row
// id --, take the positions behind the members that remain: new_ids[new_off[l] + remaining + rank] = uid[s], rank = the movers
// into l in the slots below s.  Per 256 slots: a ballot per wave, popcount below the lane, the waves' counts through LDS.
__global__ __launch_bounds__(kWG) void ivf_update_place_kernel(IvfUpdateArgs a) {
    __shared__ uint32_t wsum[kNWave];
    const uint32_t l = blockIdx.x;
    const uint32_t mine = a.join[l];
    if (mine == 0) return;
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    const int64_t first = a.new_off[l] + (a.kept_off[l + 1] - a.kept_off[l]);
    uint32_t placed = 0;
    for (int64_t i0 = 0; i0 < a.m && placed < mine; i0 += kWG) {
        const int64_t i = i0 + threadIdx.x;
        const bool in = i < a.m && a.assign[i] == l && a.slot_list[i] != static_cast<int32_t>(l);
        const unsigned long long b = __ballot(in);
        __syncthreads();
        if (lane == 0) wsum[wave] = static_cast<uint32_t>(__popcll(b));
        __syncthreads();
        uint32_t before = 0, all = 0;
        for (int w = 0; w < kNWave; w++) {
            if (w < wave) before += wsum[w];
            all += wsum[w];
        }
        if (in) {
            const uint32_t rank = placed + before + __popcll(b & ((1ull << lane) - 1ull));
            const int64_t pos = first + rank;
            if (rank < mine && pos >= 0 && pos < a.r.n0) a.new_ids[pos] = a.uid[i];
        }
        placed += all;
    }
    if (threadIdx.x == 0) atomicAdd(a.counts + 2, static_cast<unsigned long long>(placed));
}

// 7a. One thread per NEW list position: a position among the list's remaining members takes the id of the member that remains
// there and names its old position as the origin of its row -- the staging matrix for a stayer --; a position behind them holds
// the mover ivf_update_place_kernel named.  A position that does not hold the row of its own number clears the identity.
__global__ __launch_bounds__(kWG) void ivf_update_ids_kernel(IvfUpdateArgs a) {
    __shared__ int64_t soff[kUpdLdsLists + 1];
    const int64_t *off = ivf_update_offsets_in_lds(a.new_off, a.nlist, soff);
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t q = static_cast<int64_t>(blockIdx.x) * kWG + threadIdx.x;
    bool moved = false;
    if (q < a.r.n0) {
        const int l = ivf_update_list_of(off, a.nlist, q);
        const int64_t in_list = q - off[l], remain = a.kept_off[l + 1] - a.kept_off[l], k = a.kept_off[l] + in_list;
        int64_t id = -1;
        uint32_t origin = kUpdStaged;
        if (in_list >= 0 && in_list < remain && k >= 0 && k < a.r.n0) {
            const int64_t p = a.src[k];
            if (p < a.r.n0) {
                id = a.r.old_ids[p];
                if (id >= 0 && id < a.r.n0) {
                    a.new_ids[q] = static_cast<int32_t>(id);
                    if (a.slot_of[id] < 0) origin = static_cast<uint32_t>(p);
                }
            }
        } else {
            id = a.new_ids[q];
        }
        a.origin[q] = origin;
        moved = id != q;
    }
    if (__any(moved) && lane == 0) atomicOr(a.flags, kUpdNotIdentity);
}

// 7b. The splice, one wave per NEW list position: row and norm come from the old list-order arrays at the recorded origin, or from
// the staging matrix -- stayers at their old place, movers behind the members that remain.  Never in place.
__global__ __launch_bounds__(kWG) void ivf_update_splice_kernel(IvfUpdateArgs a) {
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t q = static_cast<int64_t>(blockIdx.x) * kNWave + (threadIdx.x >> 6);
    if (q >= a.r.n0) return;  // (wave-uniform)
    const uint32_t o = a.origin[q];
    const float *src;
    float norm;
    if (o == kUpdStaged) {
        const int64_t id = a.new_ids[q];
        if (id < 0 || id >= a.r.n0) return;
        const int64_t s = a.slot_of[id];
        if (s < 0 || s >= a.m) return;
        src = a.stage + s * a.r.ld;
        norm = a.snorms[s];
    } else {
        if (static_cast<int64_t>(o) >= a.r.n0) return;
        src = a.old_lrows + static_cast<int64_t>(o) * a.r.ld;
        norm = a.old_lnorms[o];
    }
    const float4 *sp = reinterpret_cast<const float4 *>(src);
    float4 *dp = reinterpret_cast<float4 *>(a.new_lrows + q * a.r.ld);
    for (int64_t j = lane; j < a.r.ld / 4; j += kWave) dp[j] = sp[j];
    if (lane == 0) a.new_lnorms[q] = norm;
}

}  // namespace hg
