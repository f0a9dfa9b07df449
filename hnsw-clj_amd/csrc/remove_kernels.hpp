// remove_kernels.hpp -- what every removal of rows from a live handle shares (hnswgpu_lsh_remove: lsh_remove_kernels.hpp, lsh.hip;
// hnswgpu_ivf_remove: ivf_remove_kernels.hpp, ivf.hip): the mask of the rows that go, every kept row's new id (its rank among the
// kept rows), the kept rows / norms (/ hash codes) moved to their ranks, and the first two steps of the stable compaction of an
// id array: the kept entries per chunk of kWG positions and their scan.  Integer work and copies only.  Everything here is
// deterministic: the mask is built with atomicOr (commutative: it does not depend on the order the ids arrive in, and an id named
// twice sets one bit), counts are integer sums.  No kernel here waits for another workgroup: the steps depend on each other
// through launch boundaries only, every loop is bounded by n0, m or W, and every index is checked against n1 before its store.
// Included by two translation units: the kernels are static.
#pragma once
#include "kernels.hpp"

namespace hg {

constexpr int kRemoveMaxTables = 16;  // (= kLshMaxTables: lsh_remove_kernels.hpp asserts it)

constexpr int kLshRemoveGate = 2 * kRemoveMaxTables + 1;  // words of the one readback (LshRemoveArgs::gate)

struct LshRemoveArgs {
    int64_t n0, n1, m, W;  // rows before / after, ids in the call, mask words (n0 + 31) / 32
    int64_t ld;            // floats per base row (a multiple of 4)
    int32_t tables, bits;
    const int32_t *rows;   // [m] the call's ids, each in [0, n0) (checked on the host)
    uint32_t *keep;        // [W] zero before lsh_remove_mark_kernel, which leaves the DROP bits; lsh_remove_rank_kernel turns a
                           // word into its KEEP bits (bits at positions >= n0 clear)
    uint32_t *word_rank;   // [W] kept rows below the word's first
    const float *old_base, *old_norms;
    const uint16_t *old_codes;  // [n0][tables]
    float *new_base, *new_norms;
    uint16_t *new_codes;        // [n1][tables]
    uint32_t *removed;          // [tables][2^bits] zero before lsh_remove_count_kernel: the rows that go, per bucket
    const int64_t *old_off;     // [tables][2^bits + 1]
    int64_t *new_off;
    const int32_t *old_ids;     // [tables][n0]
    int32_t *new_ids;           // [tables][n1]
    int64_t nchunks;            // (n0 + kWG - 1) / kWG chunks of bucket-id positions per table
    uint32_t *chunk_base;       // [tables][nchunks] kept entries of a chunk, then (lsh_remove_chunk_scan_kernel) of the chunks before it
    // what the host reads back, once: [0, tables) every table's new_off[2^bits]; [kRemoveMaxTables, + tables) the kept entries
    // of every table's ids; [2 * kRemoveMaxTables] the kept rows by the rank scan -- all n1 when every step agrees
    int64_t *gate;
};

__device__ __forceinline__ bool lsh_remove_kept(const LshRemoveArgs &a, int64_t r) {
    return r >= 0 && r < a.n0 && ((a.keep[r >> 5] >> (r & 31)) & 1u);
}
// the new id of a KEPT row: the kept rows below it
__device__ __forceinline__ int64_t lsh_remove_rank(const LshRemoveArgs &a, int64_t r) {
    return static_cast<int64_t>(a.word_rank[r >> 5]) + __popc(a.keep[r >> 5] & ((1u << (r & 31)) - 1u));
}

// 1. keep[w] |= the bits of the call's ids (DROP bits until the rank step)
static __global__ __launch_bounds__(kWG) void lsh_remove_mark_kernel(LshRemoveArgs a) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * kWG + threadIdx.x;
    if (i >= a.m) return;
    const int64_t r = a.rows[i];
    if (r < 0 || r >= a.n0) return;  // (the host has refused such a call)
    atomicOr(a.keep + (r >> 5), 1u << (r & 31));
}

// 2. ONE workgroup: drop bits -> keep bits, a block scan with a carry over the W words' popcounts (the scan of
// lsh_add_offsets_kernel): word_rank[w] and the total
static __global__ __launch_bounds__(kWG) void lsh_remove_rank_kernel(LshRemoveArgs a) {
    __shared__ uint32_t wsum[kNWave];
    int64_t carry = 0;
    for (int64_t w0 = 0; w0 < a.W; w0 += kWG) {
        const int64_t w = w0 + threadIdx.x;
        uint32_t k = 0;
        if (w < a.W) {
            const int64_t left = a.n0 - w * 32;  // rows the word stands for: 32, fewer in the last
            const uint32_t valid = left >= 32 ? 0xffffffffu : (1u << left) - 1u;
            k = ~a.keep[w] & valid;
            a.keep[w] = k;
        }
        uint32_t total;
        const int64_t before = carry + wg_exclusive_sum(static_cast<uint32_t>(__popc(k)), wsum, &total);
        if (w < a.W) a.word_rank[w] = static_cast<uint32_t>(before);
        carry += total;
    }
    if (threadIdx.x == 0) a.gate[2 * kRemoveMaxTables] = carry;
}

// 3. One wave per old row: a kept row's ld floats as whole float4s, its norm and its codes go to its rank.  Never in place.
static __global__ __launch_bounds__(kWG) void lsh_remove_rows_kernel(LshRemoveArgs a) {
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t r = static_cast<int64_t>(blockIdx.x) * kNWave + (threadIdx.x >> 6);
    if (!lsh_remove_kept(a, r)) return;  // (wave-uniform)
    const int64_t to = lsh_remove_rank(a, r);
    if (to >= a.n1) return;
    const float4 *src = reinterpret_cast<const float4 *>(a.old_base + r * a.ld);
    float4 *dst = reinterpret_cast<float4 *>(a.new_base + to * a.ld);
    for (int64_t j = lane; j < a.ld / 4; j += kWave) dst[j] = src[j];
    if (lane == 0) a.new_norms[to] = a.old_norms[r];
    if (lane < a.tables) a.new_codes[to * a.tables + lane] = a.old_codes[r * a.tables + lane];
}

// 6a. chunk_base[t][c] = the kept entries among positions [c * kWG, (c + 1) * kWG) of table t's ids.  blockIdx.y is the table.
static __global__ __launch_bounds__(kWG) void lsh_remove_chunk_count_kernel(LshRemoveArgs a) {
    __shared__ uint32_t wsum[kNWave];
    const int64_t t = blockIdx.y, p = static_cast<int64_t>(blockIdx.x) * kWG + threadIdx.x;
    const bool kept = p < a.n0 && lsh_remove_kept(a, a.old_ids[t * a.n0 + p]);
    uint32_t total;
    (void)wg_exclusive_sum(kept ? 1u : 0u, wsum, &total);
    if (threadIdx.x == 0 && static_cast<int64_t>(blockIdx.x) < a.nchunks) a.chunk_base[t * a.nchunks + blockIdx.x] = total;
}

// 6b. One workgroup per table: the chunks' counts become the kept entries before each chunk (block scan with a carry)
static __global__ __launch_bounds__(kWG) void lsh_remove_chunk_scan_kernel(LshRemoveArgs a) {
    __shared__ uint32_t wsum[kNWave];
    const int64_t t = blockIdx.x;
    uint32_t *base = a.chunk_base + t * a.nchunks;
    int64_t carry = 0;
    for (int64_t c0 = 0; c0 < a.nchunks; c0 += kWG) {
        const int64_t c = c0 + threadIdx.x;
        uint32_t total;
        const int64_t before = carry + wg_exclusive_sum(c < a.nchunks ? base[c] : 0u, wsum, &total);
        if (c < a.nchunks) base[c] = static_cast<uint32_t>(before);
        carry += total;
    }
    if (threadIdx.x == 0) a.gate[kRemoveMaxTables + t] = carry;
}

}  // namespace hg
