// lsh_remove_kernels.hpp -- rows leave a live handle with hash tables (lsh.hip: hnswgpu_lsh_remove): the mask of the rows that go,
// every kept row's new id (its rank among the kept rows), the kept rows / norms / codes moved to their ranks, the shrunken
// offsets, and every table's bucket ids compacted and renumbered.  Integer work and copies only: nothing is hashed or summed in
// floating point again.  Everything here is deterministic: the mask is built with atomicOr (commutative: it does not depend on
// the order the ids arrive in, and an id named twice sets one bit), counts are integer sums, and a kept entry's destination is a
// function of the mask and the old arrays alone -- a prefix count of kept entries before it, never the order atomics arrive in.
// No kernel here waits for another workgroup: the steps depend on each other through launch boundaries only, every loop is
// bounded by n0, m, W or 2^bits, and every index is checked against n1 / 2^bits before its store.
#pragma once
#include "kernels.hpp"
#include "lsh_add_kernels.hpp"  // kLshAddLdsBuckets
#include "lsh_kernels.hpp"      // kLshMaxTables
#include "remove_kernels.hpp"   // LshRemoveArgs and steps 1, 2, 3, 6a, 6b: shared with hnswgpu_ivf_remove

namespace hg {

static_assert(kRemoveMaxTables == kLshMaxTables, "the gate of LshRemoveArgs has a word per table");

// 4. removed[t][b] = the MARKED rows with code b in table t: a thread per mask word walks the word's dropped rows (at most 32),
// so a row named twice counts once.  blockIdx.y is the table; counts in LDS first while 2^bits words fit (lsh_add_count_kernel).
__global__ __launch_bounds__(kWG) void lsh_remove_count_kernel(LshRemoveArgs a) {
    __shared__ uint32_t hist[kLshAddLdsBuckets];
    const int t = blockIdx.y;
    const uint32_t nb = 1u << a.bits;
    const bool in_lds = nb <= static_cast<uint32_t>(kLshAddLdsBuckets);
    uint32_t *counts = a.removed + static_cast<int64_t>(t) * nb;
    if (in_lds) {
        for (uint32_t b = threadIdx.x; b < nb; b += kWG) hist[b] = 0;
        __syncthreads();
    }
    for (int64_t w = static_cast<int64_t>(blockIdx.x) * kWG + threadIdx.x; w < a.W; w += static_cast<int64_t>(gridDim.x) * kWG) {
        const int64_t left = a.n0 - w * 32;
        uint32_t drop = ~a.keep[w] & (left >= 32 ? 0xffffffffu : (1u << left) - 1u);
        while (drop) {  // (at most 32 rounds: every round clears a bit)
            const int64_t r = w * 32 + (__ffs(drop) - 1);
            drop &= drop - 1u;
            const uint32_t b = a.old_codes[r * a.tables + t];
            if (b >= nb) continue;  // (a code has `bits` bits)
            if (in_lds) atomicAdd(&hist[b], 1u);
            else atomicAdd(counts + b, 1u);
        }
    }
    if (in_lds) {
        __syncthreads();
        for (uint32_t b = threadIdx.x; b < nb; b += kWG)
            if (hist[b]) atomicAdd(counts + b, hist[b]);
    }
}

// 5. One workgroup per table, the mirror of lsh_add_offsets_kernel: new_off[b] = old_off[b] - the removed rows of the buckets below b
__global__ __launch_bounds__(kWG) void lsh_remove_offsets_kernel(LshRemoveArgs a) {
    __shared__ uint32_t wsum[kNWave];
    const int t = blockIdx.x;
    const int64_t nb = static_cast<int64_t>(1) << a.bits;
    const int64_t *old_off = a.old_off + t * (nb + 1);
    int64_t *new_off = a.new_off + t * (nb + 1);
    const uint32_t *removed = a.removed + t * nb;
    int64_t carry = 0;
    for (int64_t b0 = 0; b0 <= nb; b0 += kWG) {
        const int64_t b = b0 + threadIdx.x;
        uint32_t total;
        const int64_t gone = carry + wg_exclusive_sum(b < nb ? removed[b] : 0u, wsum, &total);
        if (b <= nb) new_off[b] = old_off[b] - gone;
        if (b == nb) a.gate[t] = old_off[b] - gone;
        carry += total;
    }
}

// 6c. The stable compaction: a kept entry at position p goes to the kept entries before p -- its chunk's base plus the kept
// positions before it in the chunk -- under its row's new id.  Buckets are contiguous and the rank is monotone, so every bucket's
// kept members stay together, in their order, ascending, and start at new_off of the bucket.
__global__ __launch_bounds__(kWG) void lsh_remove_ids_kernel(LshRemoveArgs a) {
    __shared__ uint32_t wsum[kNWave];
    const int64_t t = blockIdx.y, p = static_cast<int64_t>(blockIdx.x) * kWG + threadIdx.x;
    const int64_t r = p < a.n0 ? a.old_ids[t * a.n0 + p] : -1;
    const bool kept = lsh_remove_kept(a, r);
    uint32_t total;
    const uint32_t before = wg_exclusive_sum(kept ? 1u : 0u, wsum, &total);
    if (!kept) return;
    const int64_t to = static_cast<int64_t>(a.chunk_base[t * a.nchunks + blockIdx.x]) + before, id = lsh_remove_rank(a, r);
    if (to < a.n1 && id < a.n1) a.new_ids[t * a.n1 + to] = static_cast<int32_t>(id);
}

}  // namespace hg
