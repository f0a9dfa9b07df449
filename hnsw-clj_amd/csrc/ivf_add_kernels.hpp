// ivf_add_kernels.hpp -- rows join the inverted lists of a live handle (ivf.hip: hnswgpu_ivf_add): where every new row
// goes, and the grown list-order arrays.  Integer work and row copies only: the distances behind `assign` are the scan
// kernel's (kernels.hpp, GEMV order), the int8 / half copies of the grown rows are made by the kernels that make them for
// a fresh set of lists.  Everything here is deterministic: counts are integer sums, a new row's place inside its list is
// its STABLE rank among the call's rows of that list (ballot / popcount, never the order atomics happen to arrive in).
#pragma once
#include "kernels.hpp"

namespace hg {

constexpr uint32_t kAddBadAssign = 1;   // flag bits of IvfAddArgs::flags: a new row without a nearest list (assign >= nlist)
constexpr uint32_t kAddNotIdentity = 2;  // a new row whose list position is not its row id
constexpr int kAddLdsLists = 4096;       // lists up to which ivf_add_count_kernel counts in LDS first

struct IvfAddArgs {
    const uint32_t *assign;  // [m] nearest list of new row i (row id n0 + i)
    int64_t m, n0;
    int32_t nlist;
    const int64_t *old_off;  // [nlist + 1] the lists as they stand
    int64_t *new_off;        // [nlist + 1] ... and grown
    uint32_t *counts;        // [nlist] new rows per list (zero before ivf_add_count_kernel)
    uint32_t *flags;         // [1] kAdd* (zero before ivf_add_count_kernel)
    int32_t *new_ids;        // [n0 + m] row ids in list order, grown
    // ivf_splice_kernel
    const int32_t *old_ids;  // [n0]
    const float *old_lrows, *old_lnorms;  // list order, as they stand
    const float *base, *norms;            // the grown base (rows [n0, n0 + m) are the new ones)
    int64_t ld;
    float *new_lrows, *new_lnorms;  // list order, grown
};

// counts[l] = new rows of list l.  Integer adds: the sums do not depend on their order.  With few enough lists a workgroup
// counts its rows in LDS and adds every list's count once.
__global__ __launch_bounds__(kWG) void ivf_add_count_kernel(IvfAddArgs a) {
    __shared__ uint32_t hist[kAddLdsLists];
    const bool in_lds = a.nlist <= kAddLdsLists;
    if (in_lds) {
        for (int l = threadIdx.x; l < a.nlist; l += kWG) hist[l] = 0;
        __syncthreads();
    }
    bool bad = false;
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * kWG + threadIdx.x; i < a.m; i += static_cast<int64_t>(gridDim.x) * kWG) {
        const uint32_t l = a.assign[i];
        if (l >= static_cast<uint32_t>(a.nlist)) bad = true;
        else if (in_lds) atomicAdd(&hist[l], 1u);
        else atomicAdd(a.counts + l, 1u);
    }
    if (__any(bad) && (threadIdx.x & (kWave - 1)) == 0) atomicOr(a.flags, kAddBadAssign);
    if (in_lds) {
        __syncthreads();
        for (int l = threadIdx.x; l < a.nlist; l += kWG)
            if (hist[l]) atomicAdd(a.counts + l, hist[l]);
    }
}

// new_off[l] = old_off[l] + new rows of the lists below l: a list's shift is new_off[l] - old_off[l].  One workgroup.
__global__ __launch_bounds__(kWG) void ivf_add_offsets_kernel(IvfAddArgs a) {
    __shared__ uint32_t wsum[kNWave];
    int64_t carry = 0;
    for (int l0 = 0; l0 <= a.nlist; l0 += kWG) {
        const int l = l0 + threadIdx.x;
        uint32_t total;
        const uint32_t before = wg_exclusive_sum(l < a.nlist ? a.counts[l] : 0u, wsum, &total);
        if (l <= a.nlist) a.new_off[l] = a.old_off[l] + carry + before;
        carry += total;
    }
}

// One workgroup per list: the call's rows of that list, in row order, take the positions behind the list's old members --
// new_ids[new_off[l] + old length + rank] = n0 + i, rank = earlier rows of the call in the same list.  Per 256 rows: a
// ballot per wave, popcount below the lane, the waves' counts through LDS.
__global__ __launch_bounds__(kWG) void ivf_add_place_kernel(IvfAddArgs a) {
    __shared__ uint32_t wsum[kNWave];
    const uint32_t l = blockIdx.x;
    const uint32_t mine = a.counts[l];
    if (mine == 0) return;
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    const int64_t first = a.new_off[l] + (a.old_off[l + 1] - a.old_off[l]);
    uint32_t placed = 0;
    bool moved = false;
    for (int64_t i0 = 0; i0 < a.m && placed < mine; i0 += kWG) {
        const int64_t i = i0 + threadIdx.x;
        const bool in = i < a.m && a.assign[i] == l;
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
            const int64_t pos = first + placed + before + __popcll(b & ((1ull << lane) - 1ull));
            a.new_ids[pos] = static_cast<int32_t>(a.n0 + i);
            moved |= pos != a.n0 + i;
        }
        placed += all;
    }
    if (__any(moved) && lane == 0) atomicOr(a.flags, kAddNotIdentity);
}

// One wave per position of the grown list order.  A position among a list's old members takes row, norm and id from the
// old list-order arrays, `shift` positions further down (a contiguous source, no gather over the base); a position
// behind them takes the row ivf_add_place_kernel named there from the grown base.
__global__ __launch_bounds__(kWG) void ivf_splice_kernel(IvfAddArgs a) {
    if (*a.flags & kAddBadAssign) return;  // (positions nobody named: the call fails once the flags are read back)
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t n1 = a.n0 + a.m;
    const int64_t pos = static_cast<int64_t>(blockIdx.x) * kNWave + __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
    if (pos >= n1) return;
    int lo = 0, hi = a.nlist;  // the list of pos: the last l with new_off[l] <= pos (empty lists share an offset with their successor)
    while (lo + 1 < hi) {
        const int mid = (lo + hi) >> 1;
        if (a.new_off[mid] <= pos) lo = mid;
        else hi = mid;
    }
    const int64_t in_list = pos - a.new_off[lo], old_len = a.old_off[lo + 1] - a.old_off[lo];
    const float *src;
    float norm;
    if (in_list < old_len) {
        const int64_t from = a.old_off[lo] + in_list;
        src = a.old_lrows + from * a.ld;
        norm = a.old_lnorms[from];
        if (lane == 0) a.new_ids[pos] = a.old_ids[from];
    } else {
        const int64_t id = a.new_ids[pos];
        if (id < a.n0 || id >= n1) return;
        src = a.base + id * a.ld;
        norm = a.norms[id];
    }
    const float4 *sp = reinterpret_cast<const float4 *>(src);
    float4 *dp = reinterpret_cast<float4 *>(a.new_lrows + pos * a.ld);
    for (int i = lane; i < a.ld / 4; i += kWave) dp[i] = sp[i];
    if (lane == 0) a.new_lnorms[pos] = norm;
}

}  // namespace hg
