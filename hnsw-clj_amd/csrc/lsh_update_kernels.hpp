// lsh_update_kernels.hpp -- rows of a live handle with hash tables take new values (lsh.hip: hnswgpu_lsh_update).  Slot s of a
// call is its s-th smallest row id (ivf_update_ids.hpp).  Here: the call's rows into a staging matrix in slot order, their scatter
// (rows, norms, codes) into the staged copies, per table the entries that leave and join every bucket, the new offsets, the movers
// of a table grouped twice -- by the bucket they leave and by the bucket they join, ascending by row id inside a bucket -- and the
// placement of every entry.  Integer work and row copies only: the codes are lsh_hash_kernel's (lsh_kernels.hpp) and the norms
// row_norms_kernel's, over the m staged rows.  A row is a MOVER of table t when its new code there differs from its old one.
// With the two grouped lists ONE formula places every row r in its new bucket b of table t:
//     dest = new_off[t][b] + #old(b, < r) - #leavers(b, < r) + #joiners(b, < r)
// #old = the old members of b with an id below r: for an entry that stays, its old position minus old_off[t][b] (a bucket is
// ascending); for a joiner a lower bound in the old bucket.  The other two terms are lower bounds in b's segments of the grouped
// lists.  The n bucket entries are never sorted again and nothing loops over buckets x m.
// Everything here is deterministic: counts are integer sums, a mover's place in a grouped list is its STABLE rank among the movers
// of its bucket in slot order (the walk of lsh_add_place_kernel: ballots and a popcount below the lane, never the order atomics
// arrive in), and a destination is a function of the old arrays and the call alone.  No kernel waits for another workgroup: the
// steps depend on each other through launch boundaries only, every loop is bounded by n, m, 2^bits, ld or the logarithm of a
// bucket's length, and every index is checked against n / m / 2^bits before its store.
#pragma once
#include "kernels.hpp"
#include "lsh_add_kernels.hpp"  // kLshAddLdsBuckets, lsh_add_cursor_sync
#include "lsh_kernels.hpp"      // kLshMaxTables

namespace hg {

// words of the one readback (LshUpdateArgs::gate), kLshMaxTables of each: a table's new_off[2^bits], the entries that left its
// buckets, the entries that joined them, the entries lsh_update_keep_kernel + lsh_update_join_kernel stored
enum { LSH_UPD_TOTAL = 0, LSH_UPD_LEFT = 1, LSH_UPD_JOINED = 2, LSH_UPD_PLACED = 3, LSH_UPD_GATES = 4 };
constexpr int kLshUpdateGate = LSH_UPD_GATES * kLshMaxTables;

struct LshUpdateArgs {
    int64_t n, m, ld;
    int32_t dim, tables, bits;
    const int32_t *uid;      // [m] slot -> row id, ascending
    const int32_t *from;     // [m] slot -> position in the caller's arrays
    const float *raw;        // [m][dim] the caller's rows as they came
    float *stage;            // [m][ld] ... in slot order, padding zeroed
    const float *snorms;     // [m] their norms (row_norms_kernel)
    const uint16_t *scodes;  // [m][tables] their codes (lsh_hash_kernel)
    uint16_t *ocodes;        // [m][tables] the codes rows uid[s] had
    const uint16_t *old_codes;  // [n][tables]
    float *new_base, *new_norms;  // device copies of the old arrays before lsh_update_scatter_kernel
    uint16_t *new_codes;
    // which = 0 the buckets the movers LEAVE, 1 the buckets they JOIN; all [2][tables][...]:
    uint32_t *count;   // [2^bits] zero before lsh_update_count_kernel, which leaves the movers per bucket; lsh_update_offsets_kernel turns a
                       // bucket's count into its CURSOR, the place in the table's grouped list of the bucket's next mover
    uint32_t *seg;     // [2^bits + 1] the exclusive prefix of the counts: bucket b's movers are grouped[seg[b] .. seg[b + 1])
    int32_t *grouped;  // [m] the movers' row ids, by bucket, ascending inside a bucket
    const int64_t *old_off;  // [tables][2^bits + 1]
    int64_t *new_off;
    const int32_t *old_ids;  // [tables][n]
    int32_t *new_ids;
    unsigned long long *gate;  // [kLshUpdateGate] zero before lsh_update_offsets_kernel
};

// 1. One wave per slot: the caller's row `from[s]` becomes row s of the staging matrix (ld floats, the padding zero).
__global__ __launch_bounds__(kWG) void lsh_update_stage_kernel(LshUpdateArgs a) {
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t s = static_cast<int64_t>(blockIdx.x) * kNWave + (threadIdx.x >> 6);
    if (s >= a.m) return;  // (wave-uniform)
    const int64_t f = a.from[s];
    if (f < 0 || f >= a.m) return;
    const float *sp = a.raw + f * a.dim;
    float *dp = a.stage + s * a.ld;
    for (int64_t j = lane; j < a.ld; j += kWave) dp[j] = j < a.dim ? sp[j] : 0.0f;
}

// 2. One wave per slot: the staged row, its norm and its codes replace those of row uid[s] in the staged copies, and the codes the
// row had are kept per slot.  The ids are distinct, so no two slots write one row.
__global__ __launch_bounds__(kWG) void lsh_update_scatter_kernel(LshUpdateArgs a) {
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t s = static_cast<int64_t>(blockIdx.x) * kNWave + (threadIdx.x >> 6);
    if (s >= a.m) return;  // (wave-uniform)
    const int64_t r = a.uid[s];
    if (r < 0 || r >= a.n) return;
    const float4 *sp = reinterpret_cast<const float4 *>(a.stage + s * a.ld);
    float4 *dp = reinterpret_cast<float4 *>(a.new_base + r * a.ld);
    for (int64_t j = lane; j < a.ld / 4; j += kWave) dp[j] = sp[j];
    if (lane == 0) a.new_norms[r] = a.snorms[s];
    if (lane < a.tables) {
        a.ocodes[s * a.tables + lane] = a.old_codes[r * a.tables + lane];
        a.new_codes[r * a.tables + lane] = a.scodes[s * a.tables + lane];
    }
}

// the bucket slot i leaves (which = 0) or joins (1) in table t, or 2^bits when it stays (or a code is out of range: a code has `bits` bits)
__device__ __forceinline__ uint32_t lsh_update_mover_bucket(const LshUpdateArgs &a, int64_t i, int t, int which, uint32_t nb) {
    const uint32_t was = a.ocodes[i * a.tables + t], now = a.scodes[i * a.tables + t];
    return was != now && was < nb && now < nb ? (which ? now : was) : nb;
}

// 3. count[which][t][b] = the movers of table t that leave (join) bucket b.  Integer adds: the sums do not depend on their order.
// blockIdx.y is the table, blockIdx.z is `which`; with few enough buckets a workgroup counts in LDS and adds every bucket's count
// once (lsh_add_count_kernel).
__global__ __launch_bounds__(kWG) void lsh_update_count_kernel(LshUpdateArgs a) {
    __shared__ uint32_t hist[kLshAddLdsBuckets];
    const int t = blockIdx.y, which = blockIdx.z;
    const uint32_t nb = 1u << a.bits;
    const bool in_lds = nb <= static_cast<uint32_t>(kLshAddLdsBuckets);
    uint32_t *counts = a.count + (static_cast<int64_t>(which) * a.tables + t) * nb;
    if (in_lds) {
        for (uint32_t b = threadIdx.x; b < nb; b += kWG) hist[b] = 0;
        __syncthreads();
    }
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * kWG + threadIdx.x; i < a.m; i += static_cast<int64_t>(gridDim.x) * kWG) {
        const uint32_t b = lsh_update_mover_bucket(a, i, t, which, nb);
        if (b >= nb) continue;
        if (in_lds) atomicAdd(&hist[b], 1u);
        else atomicAdd(counts + b, 1u);
    }
    if (in_lds) {
        __syncthreads();
        for (uint32_t b = threadIdx.x; b < nb; b += kWG)
            if (hist[b]) atomicAdd(counts + b, hist[b]);
    }
}

// 4. One workgroup per table, two block scans with a carry over the 2^bits + 1 entries (lsh_add_offsets_kernel, ivf_update_offsets_kernel):
// seg[which][b] = the movers of the buckets below b, new_off[b] = old_off[b] - those that left + those that joined; a bucket's
// count becomes its cursor.  The totals go to the gate.
__global__ __launch_bounds__(kWG) void lsh_update_offsets_kernel(LshUpdateArgs a) {
    __shared__ uint32_t wsum[kNWave];
    const int t = blockIdx.x;
    const int64_t nb = static_cast<int64_t>(1) << a.bits;
    const int64_t *old_off = a.old_off + t * (nb + 1);
    int64_t *new_off = a.new_off + t * (nb + 1);
    uint32_t *cl = a.count + t * nb, *cj = a.count + (a.tables + t) * nb;
    uint32_t *sl = a.seg + t * (nb + 1), *sj = a.seg + (a.tables + t) * (nb + 1);
    int64_t left = 0, joined = 0;
    for (int64_t b0 = 0; b0 <= nb; b0 += kWG) {
        const int64_t b = b0 + threadIdx.x;
        uint32_t tl, tj;
        const int64_t bl = left + wg_exclusive_sum(b < nb ? cl[b] : 0u, wsum, &tl);
        const int64_t bj = joined + wg_exclusive_sum(b < nb ? cj[b] : 0u, wsum, &tj);
        if (b <= nb) {
            sl[b] = static_cast<uint32_t>(bl);
            sj[b] = static_cast<uint32_t>(bj);
            new_off[b] = old_off[b] - bl + bj;
        }
        if (b < nb) {
            cl[b] = static_cast<uint32_t>(bl);
            cj[b] = static_cast<uint32_t>(bj);
        }
        if (b == nb) {
            a.gate[LSH_UPD_TOTAL * kLshMaxTables + t] = static_cast<unsigned long long>(old_off[b] - bl + bj);
            a.gate[LSH_UPD_LEFT * kLshMaxTables + t] = static_cast<unsigned long long>(bl);
            a.gate[LSH_UPD_JOINED * kLshMaxTables + t] = static_cast<unsigned long long>(bj);
        }
        left += tl;
        joined += tj;
    }
}

// 5. One WAVE per (table, which) walks the slots in order, kWave at a time: grouped[cursor[b] + rank] = uid[i] for a mover i of
// bucket b, rank = the EARLIER lanes of the step with the same bucket, and the last of equal lanes moves the cursor past the
// step's movers of its bucket -- lsh_add_place_kernel's walk and its ordering rule (every lane READS its bucket's cursor,
// lsh_add_cursor_sync, the last lane of every bucket WRITES it, lsh_add_cursor_sync) over another source.  Slots ascend by row id,
// so a bucket's segment does.  The cursors live in LDS while 2^bits words fit (IN_LDS) and stay in a.count otherwise.  About
// m / 64 dependent steps, acceptable for the reason stated there.
template <bool IN_LDS>
__global__ __launch_bounds__(kWave) void lsh_update_group_kernel(LshUpdateArgs a) {
    __shared__ uint32_t lcur[IN_LDS ? kLshAddLdsBuckets : 1];
    const int t = blockIdx.x, which = blockIdx.y, lane = threadIdx.x;
    const uint32_t nb = 1u << a.bits;
    const int64_t list = static_cast<int64_t>(which) * a.tables + t;
    uint32_t *cursor = IN_LDS ? lcur : a.count + list * nb;
    int32_t *out = a.grouped + list * a.m;
    if (IN_LDS) {
        for (uint32_t b = lane; b < nb; b += kWave) lcur[b] = a.count[list * nb + b];
        lsh_add_cursor_sync<IN_LDS>();
    }
    const unsigned long long below = (1ull << lane) - 1ull;
    auto bucket_of = [&](int64_t i) -> uint32_t { return i < a.m ? lsh_update_mover_bucket(a, i, t, which, nb) : nb; };
    uint32_t next = bucket_of(lane);
    for (int64_t i0 = 0; i0 < a.m; i0 += kWave) {  // (wave-uniform: every lane reaches every ballot and every sync)
        const int64_t i = i0 + lane;
        const uint32_t b = next;
        next = bucket_of(i + kWave);  // (the next step's codes are on their way while this step's cursors are read and written)
        const bool in = b < nb;
        unsigned long long same = __ballot(in);  // the step's movers with this lane's bucket
        for (int bit = 0; bit < a.bits; bit++) {
            const bool one = (b >> bit) & 1u;
            const unsigned long long ones = __ballot(in && one);
            same &= one ? ones : ~ones;
        }
        const uint32_t first = in ? cursor[b] : 0u;
        lsh_add_cursor_sync<IN_LDS>();
        if (in) {
            const int64_t pos = static_cast<int64_t>(first) + __popcll(same & below);
            if (pos < a.m) out[pos] = a.uid[i];
            if ((same >> lane) == 1ull) cursor[b] = first + static_cast<uint32_t>(__popcll(same));  // the last of equal lanes
        }
        lsh_add_cursor_sync<IN_LDS>();
    }
}

// the entries of the ascending v[0, len) below r.  At most 32 steps.
__device__ __forceinline__ int64_t lsh_update_below(const int32_t *v, int64_t len, int32_t r) {
    int64_t lo = 0, hi = len;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (v[mid] < r) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// #joiners(b, < r) - #leavers(b, < r) of table t: lower bounds in bucket b's segments of the two grouped lists
__device__ __forceinline__ int64_t lsh_update_shift(const LshUpdateArgs &a, int64_t t, int64_t b, int32_t r) {
    const int64_t nb1 = (static_cast<int64_t>(1) << a.bits) + 1;
    const uint32_t *sl = a.seg + t * nb1 + b, *sj = a.seg + (a.tables + t) * nb1 + b;
    const uint32_t l0 = sl[0], l1 = sl[1], j0 = sj[0], j1 = sj[1];
    if (l0 > l1 || l1 > a.m || j0 > j1 || j1 > a.m) return -1 - a.n;  // (no such segment: the destination falls out of range)
    return lsh_update_below(a.grouped + (a.tables + t) * a.m + j0, j1 - j0, r) - lsh_update_below(a.grouped + t * a.m + l0, l1 - l0, r);
}

// a wave's stores into table t (wave-uniform), one add per wave
__device__ __forceinline__ void lsh_update_count_placed(const LshUpdateArgs &a, int64_t t, bool stored) {
    const unsigned long long b = __ballot(stored);
    if (b && (threadIdx.x & (kWave - 1)) == 0) atomicAdd(a.gate + LSH_UPD_PLACED * kLshMaxTables + t, static_cast<unsigned long long>(__popcll(b)));
}

// 6a. One thread per (table, old position p), blockIdx.y the table: the row there stays in its bucket unless its code in the table
// changed; #old(b, < r) = p - old_off[t][b].  old_ids is read contiguously; the codes, the offsets and the segments are gathered.
__global__ __launch_bounds__(kWG) void lsh_update_keep_kernel(LshUpdateArgs a) {
    const int64_t t = blockIdx.y, p = static_cast<int64_t>(blockIdx.x) * kWG + threadIdx.x;
    const int64_t nb = static_cast<int64_t>(1) << a.bits;
    bool stored = false;
    const int64_t r = p < a.n ? a.old_ids[t * a.n + p] : -1;
    if (r >= 0 && r < a.n) {
        const int64_t b = a.old_codes[r * a.tables + t];
        if (b < nb && a.new_codes[r * a.tables + t] == b) {
            const int64_t dest = a.new_off[t * (nb + 1) + b] + (p - a.old_off[t * (nb + 1) + b]) + lsh_update_shift(a, t, b, static_cast<int32_t>(r));
            if (dest >= 0 && dest < a.n) {
                a.new_ids[t * a.n + dest] = static_cast<int32_t>(r);
                stored = true;
            }
        }
    }
    lsh_update_count_placed(a, t, stored);
}

// 6b. One thread per (table, slot), blockIdx.y the table: a mover joins its new bucket at the place its row id gives it;
// #old(b, < r) is a lower bound in the old bucket.
__global__ __launch_bounds__(kWG) void lsh_update_join_kernel(LshUpdateArgs a) {
    const int64_t t = blockIdx.y, s = static_cast<int64_t>(blockIdx.x) * kWG + threadIdx.x;
    const int64_t nb = static_cast<int64_t>(1) << a.bits;
    bool stored = false;
    const int64_t b = s < a.m ? lsh_update_mover_bucket(a, s, static_cast<int>(t), 1, static_cast<uint32_t>(nb)) : nb;
    if (b < nb) {
        const int32_t r = a.uid[s];
        const int64_t o0 = a.old_off[t * (nb + 1) + b], o1 = a.old_off[t * (nb + 1) + b + 1];
        if (r >= 0 && r < a.n && o0 >= 0 && o0 <= o1 && o1 <= a.n) {
            const int64_t dest = a.new_off[t * (nb + 1) + b] + lsh_update_below(a.old_ids + t * a.n + o0, o1 - o0, r) + lsh_update_shift(a, t, b, r);
            if (dest >= 0 && dest < a.n) {
                a.new_ids[t * a.n + dest] = r;
                stored = true;
            }
        }
    }
    lsh_update_count_placed(a, t, stored);
}

}  // namespace hg
