// lsh_add_kernels.hpp -- rows join the hash tables of a live handle (lsh.hip: hnswgpu_lsh_add): how many of the call's rows go to
// every bucket, the grown offsets, every new row's place, and the old members moved to theirs.  Integer work only: the codes are
// lsh_hash_kernel's (lsh_kernels.hpp), over the new rows alone.  Everything here is deterministic: counts are integer sums, a new
// row's place inside its bucket is its STABLE rank among the call's rows of that bucket (ballots and a popcount below the lane,
// walked in row order; never the order atomics happen to arrive in) -- the rule of ivf_add_place_kernel (ivf_add_kernels.hpp),
// but not its shape: there a workgroup per list reads all m assignments, here tables x 2^bits buckets (up to a million) would
// make that O(buckets x m), so ONE wave per table walks the call's rows once and keeps a cursor per bucket.
// No kernel here waits for another workgroup: the steps depend on each other through launch boundaries only, and every loop is
// bounded by m, n0 or 2^bits.
#pragma once
#include "kernels.hpp"

namespace hg {

constexpr int kLshAddLdsBuckets = 4096;  // buckets per table up to which the count and the cursors live in LDS (16 KB)

struct LshAddArgs {
    const uint16_t *codes;  // [n0 + m][tables] the grown codes (rows [n0, n0 + m) are the call's)
    int64_t n0, m;
    int32_t tables, bits;
    const int64_t *old_off;  // [tables][2^bits + 1] the buckets as they stand
    int64_t *new_off;        // [tables][2^bits + 1] ... and grown
    // [tables][2^bits] zero before lsh_add_count_kernel, which leaves the new rows per bucket; lsh_add_offsets_kernel turns a
    // bucket's count into its CURSOR: the position in the table's grown ids of the bucket's next new row
    uint32_t *cursor;
    const int32_t *old_ids;  // [tables][n0]
    int32_t *new_ids;        // [tables][n0 + m]
};

// cursor[t][b] = the call's rows with code b in table t.  Integer adds: the sums do not depend on their order.  blockIdx.y is
// the table; with few enough buckets a workgroup counts its rows in LDS and adds every bucket's count once.
__global__ __launch_bounds__(kWG) void lsh_add_count_kernel(LshAddArgs a) {
    __shared__ uint32_t hist[kLshAddLdsBuckets];
    const int t = blockIdx.y;
    const uint32_t nb = 1u << a.bits;
    const bool in_lds = nb <= static_cast<uint32_t>(kLshAddLdsBuckets);
    uint32_t *counts = a.cursor + static_cast<int64_t>(t) * nb;
    if (in_lds) {
        for (uint32_t b = threadIdx.x; b < nb; b += kWG) hist[b] = 0;
        __syncthreads();
    }
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * kWG + threadIdx.x; i < a.m; i += static_cast<int64_t>(gridDim.x) * kWG) {
        const uint32_t b = a.codes[(a.n0 + i) * a.tables + t];
        if (b >= nb) continue;  // (a code has `bits` bits)
        if (in_lds) atomicAdd(&hist[b], 1u);
        else atomicAdd(counts + b, 1u);
    }
    if (in_lds) {
        __syncthreads();
        for (uint32_t b = threadIdx.x; b < nb; b += kWG)
            if (hist[b]) atomicAdd(counts + b, hist[b]);
    }
}

// One workgroup per table, a block scan with a carry over the 2^bits + 1 entries: new_off[b] = old_off[b] + the call's rows of the
// buckets below b, so new_off[2^bits] = n0 + m when the counts are right (the host reads that entry back before it installs
// anything).  A bucket's old members keep the front of the grown bucket; its count becomes its cursor, the position behind them.
__global__ __launch_bounds__(kWG) void lsh_add_offsets_kernel(LshAddArgs a) {
    __shared__ uint32_t wsum[kNWave];
    const int t = blockIdx.x;
    const int64_t nb = static_cast<int64_t>(1) << a.bits;
    const int64_t *old_off = a.old_off + t * (nb + 1);
    int64_t *new_off = a.new_off + t * (nb + 1);
    uint32_t *cursor = a.cursor + t * nb;
    int64_t carry = 0;
    for (int64_t b0 = 0; b0 <= nb; b0 += kWG) {
        const int64_t b = b0 + threadIdx.x;
        uint32_t total;
        const int64_t shift = carry + wg_exclusive_sum(b < nb ? cursor[b] : 0u, wsum, &total);  // the call's rows of the buckets below b
        if (b <= nb) new_off[b] = old_off[b] + shift;
        if (b < nb) cursor[b] = static_cast<uint32_t>(old_off[b + 1] + shift);  // = new_off[b] + the bucket's old length
        carry += total;
    }
}

// What orders a cursor written in one step and read in the next, by another lane: the memory model, not timing.  The workgroup
// is ONE wave.  Cursors in LDS: a wavefront-scope fence + wave barrier (the idiom of lsh_merge_kernel's `seen` list).  Cursors in
// global memory: __syncthreads(), whose workgroup-scope fence makes the workgroup's stores visible to its own later loads.
template <bool IN_LDS>
__device__ __forceinline__ void lsh_add_cursor_sync() {
    if (IN_LDS) {
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
    } else {
        __syncthreads();
    }
}

// One WAVE per table (a workgroup of kWave threads) walks the call's rows in order, kWave at a time: new_ids[t][cursor[b] + rank]
// = n0 + i, rank = the EARLIER lanes of the step with the same code -- the lanes' codes matched bit by bit with ballots, a
// popcount below the lane -- and the last of equal lanes moves the cursor past the step's rows of its bucket.  The cursors live
// in LDS while 2^bits words fit (IN_LDS) and stay in a.cursor otherwise.  Ordering rule: within a step every lane READS its
// bucket's cursor, lsh_add_cursor_sync, the last lane of every bucket WRITES it, lsh_add_cursor_sync; so a read never races
// with a write of the same step, and the next step's reads see this step's writes.  About m / 64 dependent steps: fine for a
// batch, linear-but-serial for a bulk load (which should build the tables instead).
template <bool IN_LDS>
__global__ __launch_bounds__(kWave) void lsh_add_place_kernel(LshAddArgs a) {
    __shared__ uint32_t lcur[IN_LDS ? kLshAddLdsBuckets : 1];
    const int t = blockIdx.x, lane = threadIdx.x;
    const uint32_t nb = 1u << a.bits;
    const int64_t n1 = a.n0 + a.m;
    uint32_t *cursor = IN_LDS ? lcur : a.cursor + static_cast<int64_t>(t) * nb;
    int32_t *ids = a.new_ids + static_cast<int64_t>(t) * n1;
    if (IN_LDS) {
        for (uint32_t b = lane; b < nb; b += kWave) lcur[b] = a.cursor[static_cast<int64_t>(t) * nb + b];
        lsh_add_cursor_sync<IN_LDS>();
    }
    const unsigned long long below = (1ull << lane) - 1ull;
    auto code_of = [&](int64_t i) -> uint32_t { return i < a.m ? a.codes[(a.n0 + i) * a.tables + t] : 0u; };
    uint32_t next = code_of(lane);
    for (int64_t i0 = 0; i0 < a.m; i0 += kWave) {  // (wave-uniform: every lane reaches every ballot and every sync)
        const int64_t i = i0 + lane;
        const uint32_t code = next;
        next = code_of(i + kWave);  // (the next step's codes are on their way while this step's cursors are read and written)
        const bool in = i < a.m && code < nb;
        unsigned long long same = __ballot(in);  // the step's lanes with this lane's code
        for (int bit = 0; bit < a.bits; bit++) {
            const bool one = (code >> bit) & 1u;
            const unsigned long long ones = __ballot(in && one);
            same &= one ? ones : ~ones;
        }
        const uint32_t first = in ? cursor[code] : 0u;
        lsh_add_cursor_sync<IN_LDS>();
        if (in) {
            const int64_t pos = static_cast<int64_t>(first) + __popcll(same & below);
            if (pos < n1) ids[pos] = static_cast<int32_t>(a.n0 + i);
            if ((same >> lane) == 1ull) cursor[code] = first + static_cast<uint32_t>(__popcll(same));  // the last of equal lanes
        }
        lsh_add_cursor_sync<IN_LDS>();
    }
}

// One thread per (table, old position p): the row there moves with its bucket -- new_ids[t][p + new_off[t][b] - old_off[t][b]],
// b = the row's code.  old_ids is read contiguously; the code and the two offsets are gathered.
__global__ __launch_bounds__(kWG) void lsh_add_splice_kernel(LshAddArgs a) {
    const int64_t at = static_cast<int64_t>(blockIdx.x) * kWG + threadIdx.x;
    if (at >= a.n0 * a.tables) return;
    const int64_t t = at / a.n0, p = at - t * a.n0, n1 = a.n0 + a.m;
    const int64_t nb = static_cast<int64_t>(1) << a.bits;
    const int32_t r = a.old_ids[at];
    if (r < 0 || r >= a.n0) return;
    const int64_t b = a.codes[static_cast<int64_t>(r) * a.tables + t];
    if (b >= nb) return;
    const int64_t pos = p + a.new_off[t * (nb + 1) + b] - a.old_off[t * (nb + 1) + b];
    if (pos >= 0 && pos < n1) a.new_ids[t * n1 + pos] = r;
}

}  // namespace hg
