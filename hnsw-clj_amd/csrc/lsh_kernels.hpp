// lsh_kernels.hpp -- the hybrid LSH index (src/hnsw/ann/hash/hybrid_lsh.clj) on the device: sign-projection hash, probe table,
// bucket scan, merge.  (Host side: lsh.hip; the contract: include/hnswgpu.h, "Hybrid LSH".)
//
// The reference probes, per table, the query's own bucket and the buckets one flipped bit away, keeps the `take` nearest rows of
// every probed bucket (search-bucket-brute-force, :147-193), concatenates the pieces in probe order, drops a row's later
// occurrences, sorts stably by distance and takes k (:330-342).  Here every candidate carries ord = its position in the query's
// probe stream (the sizes of the buckets probed before + its position in its own bucket):
//   lsh_hash_kernel         codes of base rows and of queries alike: bit i of table t = dot(plane[t][i], row) >= 0 in the GEMV order
//   lsh_probe_kernel        query codes -> one LshPair per (query, probe): the bucket's slice of `ids`, ord_base, take
//   lsh_bucket_scan_kernel  one wave per pair: the `take` smallest keys (distance, ord) of the bucket, and their rows
//   lsh_filtered_scan_kernel  the same over the bucket's rows whose bit is set in the pair's allow-mask (one body for both mask forms)
//   lsh_merge_kernel        one wave per query: the pairs' ascending lists merged by key, a row's later occurrences dropped, k out
// Truncation per probe comes BEFORE the dedup, as in the reference; a row's distance does not depend on the rows that share its
// step (finished in its own lane from its own sum), so equal rows have equal distance bits and the dedup only ever drops an
// entry that sorts behind its twin.
#pragma once
#include "kernels.hpp"

namespace hg {

constexpr int kLshMaxTables = 16, kLshMaxBits = 16, kLshMaxTake = 256, kLshMaxK = 256;
// lists a lane of the merge holds: 16 tables x (1 + 16 flipped bits) = 272 probes per query at the most
constexpr int kLshLanePairs = 5;
static_assert(kLshMaxTables * (1 + kLshMaxBits) <= kLshLanePairs * kWave, "a merge lane holds kLshLanePairs lists");

struct LshHashArgs {
    const float *planes;  // [tables * bits][ld], zero padded
    const float *rows;    // [n][ld], zero padded
    int64_t ld, n;
    int32_t tables, bits;
    uint16_t *codes;  // [n][tables]
};

// A wave keeps RB rows in registers and walks the hyperplanes (a few hundred KB at the most: L2-resident, each read once per RB
// rows); lane b collects the bits of row b.  lane_partial + rows_sum_to_lane are scan_kernel's with the hyperplane in the
// query's role: a bit is the sign test of the negated distance a DOT handle's hnswgpu_batch_distances returns.
template <int NCH, int RB>
__global__ __launch_bounds__(kWG) void lsh_hash_kernel(LshHashArgs a) {
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t row0 = (static_cast<int64_t>(blockIdx.x) * kNWave + (threadIdx.x >> 6)) * RB;
    if (row0 >= a.n) return;
    const int nvec = static_cast<int>(a.ld / 4);
    float4 r[RB][NCH];
#pragma unroll
    for (int b = 0; b < RB; b++) {
        const bool valid = row0 + b < a.n;
        load_row<NCH>(r[b], a.rows + (valid ? row0 + b : row0) * a.ld, nvec, lane, valid);
    }
    const int64_t myrow = row0 + lane;
    for (int t = 0; t < a.tables; t++) {
        uint32_t code = 0;
        for (int i = 0; i < a.bits; i++) {
            float4 pl[NCH];
            load_row<NCH>(pl, a.planes + (static_cast<int64_t>(t) * a.bits + i) * a.ld, nvec, lane, true);
            float s[RB];
#pragma unroll
            for (int b = 0; b < RB; b++) s[b] = lane_partial<NCH, false>(pl, r[b]);
            const float tot = rows_sum_to_lane<RB>(s, lane);  // lane b: row b's dot
            code |= (tot >= 0.0f ? 1u : 0u) << i;
        }
        if (lane < RB && myrow < a.n) a.codes[myrow * a.tables + t] = static_cast<uint16_t>(code);
    }
}

// One probed bucket of one query: ids[begin, end) (an index into the [tables][n] array), the position of its first row in
// the query's probe stream, and how many of its rows the probe keeps.
struct LshPair {
    int64_t begin, end;
    uint32_t ord_base;
    int32_t take;
    int32_t q;
    int32_t pad;
};

struct LshProbeArgs {
    const uint16_t *qcodes;  // [nq][tables]
    const int64_t *off;      // [tables][2^bits + 1]
    int64_t n;
    int32_t nq, tables, bits;
    int32_t probes, radius;  // clamped by the host: probes <= tables, radius <= bits
    int32_t take_main, take_flip;
    LshPair *pairs;  // [nq][probes * (1 + radius)], a query's pairs in probe order
};

// (hybrid_lsh.clj:307-327: per table the own bucket, then bit 0, 1, ... flipped.)  One thread per query; the host has
// checked that a query's probe stream stays below 2^32 rows.
__global__ void lsh_probe_kernel(LshProbeArgs a) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= a.nq) return;
    const int64_t nb1 = (static_cast<int64_t>(1) << a.bits) + 1;
    LshPair *out = a.pairs + static_cast<int64_t>(q) * a.probes * (1 + a.radius);
    uint32_t ord = 0;
    for (int t = 0; t < a.probes; t++) {
        const uint32_t code = a.qcodes[static_cast<int64_t>(q) * a.tables + t];
        for (int j = 0; j <= a.radius; j++) {
            const uint32_t b = j == 0 ? code : code ^ (1u << (j - 1));
            const int64_t *o = a.off + t * nb1 + b;
            LshPair p;
            p.begin = t * a.n + o[0];
            p.end = t * a.n + o[1];
            p.ord_base = ord;
            p.take = j == 0 ? a.take_main : a.take_flip;
            p.q = q;
            p.pad = 0;
            ord += static_cast<uint32_t>(p.end - p.begin);
            *out++ = p;
        }
    }
}

struct LshScanArgs {
    const float *rows;
    const float *row_norms;
    int64_t ld;
    const float *Q;
    int64_t qld;
    int32_t dim, metric;
    const LshPair *pairs;
    int64_t npairs;
    const int32_t *ids;  // [tables][n]: the buckets' rows
    int32_t take_max;    // slots per pair of the outputs (the larger of the two takes)
    uint64_t *keys;      // [npairs][take_max] ascending, all-ones padded
    int32_t *key_rows;   // [npairs][take_max] the keys' rows, -1 padded
    // lsh_filtered_scan_kernel only: the mask of pair p is allow + p.q * allow_stride, (n + 31) / 32 words indexed by row id
    const uint32_t *allow;
    int64_t allow_stride;  // words between the masks of two queries; 0: one mask shared by all
    int64_t n;
};

// ivf_gathered_step (filter_kernels.hpp) for a bucket: lane b (and every lane beyond RB, as row RB - 1) brings the ROW of a bucket
// position in `myrow` and that position's place in the probe stream in `myord`; the same loads, sums and finish in the same order,
// so a row's distance has the bits it has in every GEMV-order scan.  The key is built from the position in the probe stream,
// which here is not the row.  One step for both bucket scans: the unfiltered one brings consecutive positions, the filtered one
// whatever its queue holds.
template <int NCH, int RB, bool L2M>
__device__ __forceinline__ void lsh_gathered_step(const LshScanArgs &a, const float4 (&q)[NCH], float qn, int32_t myrow, uint32_t myord,
                                                  int nvalid, int take, int lane, bool regk, uint64_t &mine, uint64_t *mylist, int &cnt,
                                                  uint64_t &thr) {
    float4 r[RB][NCH];
    const int nvec = static_cast<int>(a.ld / 4);
    const float myrn = (!L2M && a.metric == METRIC_COS) ? a.row_norms[myrow] : 0.0f;
#pragma unroll
    for (int b = 0; b < RB; b++) {
        const int64_t row = __builtin_amdgcn_readlane(myrow, b);
        load_row<NCH>(r[b], a.rows + row * a.ld, nvec, lane, true);
    }
    float s[RB];
#pragma unroll
    for (int b = 0; b < RB; b++) s[b] = lane_partial<NCH, L2M>(q, r[b]);
    const float tot = rows_sum_to_lane<RB>(s, lane);  // lane b: row b's sum
    const float myd = L2M ? __builtin_sqrtf(tot) : finish_dist(a.metric, tot, qn, myrn);
#pragma unroll
    for (int b = 0; b < RB; b++) {
        if (b < nvalid) {  // wave-uniform
            const float d = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(myd), b));
            const uint64_t key = make_key(d, static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(myord), b)));
            if (key < thr) {
                if (regk) {
                    wave_insert_reg(mine, cnt, take, key, lane);
                    thr = wave_kth_reg(mine, take);  // ~0 until the list is full
                } else {
                    wave_insert(mylist, cnt, take, key, lane);
                    thr = cnt == take ? mylist[take - 1] : ~0ull;
                }
            }
        }
    }
}

// The epilogue of both bucket scans: the wave's list to keys[pair][take_max], from its registers (take <= 64) or from LDS, and
// each key's row beside it (the ord says where in the bucket it stands).
__device__ __forceinline__ void lsh_store_keys(const LshScanArgs &a, int64_t pair, const LshPair &p, int lane, bool regk, uint64_t mine,
                                               const uint64_t *mylist, int cnt) {
    for (int i = lane; i < a.take_max; i += kWave) {
        const uint64_t key = regk ? (i < kWave ? mine : ~0ull) : (i < cnt ? mylist[i] : ~0ull);
        const int64_t at = pair * a.take_max + i;
        a.keys[at] = key;
        a.key_rows[at] = key != ~0ull ? a.ids[p.begin + (static_cast<uint32_t>(key) - p.ord_base)] : -1;
    }
}

// Buckets are short (n / 2^bits rows on average): one WAVE per pair, kNWave pairs per workgroup.  The wave walks its bucket RB
// row ids at a time and keeps its `take` smallest keys in registers (take <= 64) or in LDS; no barrier is used, a wave without a
// pair leaves.  An empty bucket writes an all-ones list.  Dynamic LDS: [kNWave][take_max] keys when take_max > 64.
template <int NCH, int RB, bool L2M>
__global__ __launch_bounds__(kWG) void lsh_bucket_scan_kernel(LshScanArgs a) {
    extern __shared__ __align__(16) unsigned char smem[];
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = threadIdx.x >> 6;
    const int64_t pair = static_cast<int64_t>(blockIdx.x) * kNWave + wave;
    if (pair >= a.npairs) return;
    const LshPair p = a.pairs[pair];
    const int take = p.take;
    const bool regk = take <= kWave;
    uint64_t *mylist = reinterpret_cast<uint64_t *>(smem) + static_cast<size_t>(wave) * a.take_max;
    uint64_t mine = ~0ull, thr = ~0ull;
    int cnt = 0;
    if (p.begin < p.end) {
        float4 q[NCH];
        load_query<NCH>(q, a.Q + p.q * a.qld, a.dim, lane);
        const float qn = (!L2M && a.metric == METRIC_COS) ? query_norm<NCH>(q) : 0.0f;
        for (int64_t base = p.begin; base < p.end; base += RB) {
            const int64_t at = base + (lane < RB ? lane : RB - 1);
            const int32_t myrow = a.ids[at < p.end ? at : p.end - 1];
            const int64_t left = p.end - base;
            const int nvalid = __builtin_amdgcn_readfirstlane(static_cast<int>(left < RB ? left : RB));
            lsh_gathered_step<NCH, RB, L2M>(a, q, qn, myrow, p.ord_base + static_cast<uint32_t>(base - p.begin) + lane, nvalid, take, lane,
                                            regk, mine, mylist, cnt, thr);
        }
    }
    lsh_store_keys(a, pair, p, lane, regk, mine, mylist, cnt);
}

// ---- the allow-mask through the bucket scan ------------------------------------------------------------------------------------
// The reference's search over buckets that list only their passing rows, in bucket order: the bit is tested where the bucket is
// read (ivf_each_scan_kernel's pattern, filter_kernels.hpp).  One wave per pair as above; of a block of 64 bucket positions,
// lane i reads row = ids[pos] and the word of ITS PAIR's mask that holds the row's bit (a row outside [0, n) reads as clear), one
// ballot gives the block's passing lanes, and a passing lane's prefix popcount is its slot in the wave's queue in LDS (kWave + RB
// entries: fewer than RB left over, at most 64 new).  The queue holds positions RELATIVE to p.begin: the row is
// ids[p.begin + rel], the key's ord p.ord_base + rel -- the position in the UNFILTERED probe stream, monotone in the filtered
// one, so the epilogue and lsh_merge_kernel are the unfiltered search's.  Whenever RB positions are queued, RB go through
// lsh_gathered_step; what is left moves to the front, and the remainder after the last block is flushed with the clamped lane.
// No workgroup barrier (a wave without a pair has left): a wave's queue is its own, ordered by a wavefront fence + wave_barrier.
// Per probed position: 4 B of ids and a gathered mask word (rows ascend inside a bucket: so do a block's words); the f32 row
// only where the bit is set.
// LDS: [kNWave][kWave + RB] queued positions, then [kNWave][take_max] keys (take_max > 64)
__host__ __device__ constexpr size_t lsh_queue_bytes(int rb) { return sizeof(int32_t) * kNWave * (kWave + rb); }

// lane b's queued position of a step over que[0 .. nvalid): entry b, clamped into the step (every lane beyond RB as row RB - 1)
template <int RB>
__device__ __forceinline__ int32_t lsh_queued(const int32_t *que, int nvalid, int lane) {
    int at = lane < RB ? lane : RB - 1;
    at = at < nvalid ? at : nvalid - 1;
    return que[at];
}

template <int NCH, int RB, bool L2M>
__global__ __launch_bounds__(kWG) void lsh_filtered_scan_kernel(LshScanArgs a) {
    extern __shared__ __align__(16) unsigned char smem[];
    constexpr int kQueue = kWave + RB;
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = threadIdx.x >> 6;
    const int64_t pair = static_cast<int64_t>(blockIdx.x) * kNWave + wave;
    if (pair >= a.npairs) return;
    const LshPair p = a.pairs[pair];
    const int take = p.take;
    const bool regk = take <= kWave;
    int32_t *que = reinterpret_cast<int32_t *>(smem) + wave * kQueue;
    uint64_t *mylist = reinterpret_cast<uint64_t *>(smem + lsh_queue_bytes(RB)) + static_cast<size_t>(wave) * a.take_max;  // (16 * kQueue bytes in: aligned)
    uint64_t mine = ~0ull, thr = ~0ull;
    int cnt = 0;
    if (p.begin < p.end) {
        float4 q[NCH];
        load_query<NCH>(q, a.Q + p.q * a.qld, a.dim, lane);
        const float qn = (!L2M && a.metric == METRIC_COS) ? query_norm<NCH>(q) : 0.0f;
        const uint32_t *allow = a.allow + static_cast<int64_t>(p.q) * a.allow_stride;
        const int32_t *bucket = a.ids + p.begin;
        const int64_t len = p.end - p.begin;  // (a bucket holds n < 2^31 rows at the most: a queued position fits 32 bits)
        int have = 0;  // queued positions (wave-uniform), < RB between two blocks
        for (int64_t base = 0; base < len; base += kWave) {
            const int64_t rel = base + lane;
            const int64_t row = bucket[rel < len ? rel : len - 1];  // clamped, unconditional
            const bool in = rel < len && row >= 0 && row < a.n;
            const uint32_t w = allow[in ? row >> 5 : 0];
            const bool ok = in && ((w >> (row & 31)) & 1u);
            const unsigned long long m = __ballot(ok);
            if (ok) que[have + __popcll(m & ((1ull << lane) - 1ull))] = static_cast<int32_t>(rel);
            have += __popcll(m);
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            __builtin_amdgcn_wave_barrier();
            int head = 0;
            for (; have - head >= RB; head += RB) {
                const int32_t myrel = lsh_queued<RB>(que + head, RB, lane);
                lsh_gathered_step<NCH, RB, L2M>(a, q, qn, bucket[myrel], p.ord_base + static_cast<uint32_t>(myrel), RB, take, lane, regk, mine,
                                                mylist, cnt, thr);
            }
            const int rem = have - head;  // < RB
            if (head > 0 && rem > 0) {  // the leftovers to the front
                int32_t v = 0;
                if (lane < rem) v = que[head + lane];
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                __builtin_amdgcn_wave_barrier();
                if (lane < rem) que[lane] = v;
            }
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            __builtin_amdgcn_wave_barrier();
            have = rem;
        }
        if (have > 0) {
            const int32_t myrel = lsh_queued<RB>(que, have, lane);
            lsh_gathered_step<NCH, RB, L2M>(a, q, qn, bucket[myrel], p.ord_base + static_cast<uint32_t>(myrel), have, take, lane, regk, mine,
                                            mylist, cnt, thr);
        }
    }
    lsh_store_keys(a, pair, p, lane, regk, mine, mylist, cnt);
}

__device__ __forceinline__ uint64_t wave_min_u64(uint64_t v) {
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
        const uint64_t o = __shfl_xor(static_cast<unsigned long long>(v), off, kWave);
        v = o < v ? o : v;
    }
    return v;
}

struct LshMergeArgs {
    const uint64_t *keys;     // [nq][pp][take_max]
    const int32_t *key_rows;  // [nq][pp][take_max]
    int32_t nq, pp, take_max, k;
    int32_t *out_ids;  // [nq][k], -1 padded
    float *out_dist;   // [nq][k], +inf padded
};

// One wave per query.  Every probe's list is ascending, so the union in key order is a merge of the lists' heads: lane l holds
// the head (key and row) of lists l, l + 64, ...; the smallest head of the wave is the next entry of the union (keys are
// distinct: they carry their ord), its row is dropped when an earlier entry had it -- that one has the same distance and a
// smaller ord -- and emitted otherwise.  A row occurs once per table at the most, so k rows are out after k x probes steps or
// fewer; a step costs one dependent load, the winner's next head.
__global__ __launch_bounds__(kWave) void lsh_merge_kernel(LshMergeArgs a) {
    __shared__ int32_t seen[kLshMaxK];
    const int lane = threadIdx.x, q = blockIdx.x;
    const int64_t qbase = static_cast<int64_t>(q) * a.pp * a.take_max;
    const uint64_t *keys = a.keys + qbase;
    const int32_t *rows = a.key_rows + qbase;
    uint64_t hk[kLshLanePairs];
    int32_t hr[kLshLanePairs], cur[kLshLanePairs];
#pragma unroll
    for (int s = 0; s < kLshLanePairs; s++) {
        const int l = s * kWave + lane;
        cur[s] = 0;
        hk[s] = l < a.pp ? keys[static_cast<int64_t>(l) * a.take_max] : ~0ull;
        hr[s] = l < a.pp ? rows[static_cast<int64_t>(l) * a.take_max] : -1;
    }
    int32_t *out_ids = a.out_ids + static_cast<int64_t>(q) * a.k;
    float *out_dist = a.out_dist + static_cast<int64_t>(q) * a.k;
    int cnt = 0;
    while (cnt < a.k) {
        uint64_t m = hk[0];
#pragma unroll
        for (int s = 1; s < kLshLanePairs; s++) m = hk[s] < m ? hk[s] : m;
        const uint64_t w = wave_min_u64(m);
        if (w == ~0ull) break;
        const bool win = m == w;  // exactly one lane
        int32_t myrow = -1;
#pragma unroll
        for (int s = 0; s < kLshLanePairs; s++) {
            if (win && hk[s] == w) {
                myrow = hr[s];
                const int c = ++cur[s];
                const int64_t at = static_cast<int64_t>(s * kWave + lane) * a.take_max + c;
                hk[s] = c < a.take_max ? keys[at] : ~0ull;
                hr[s] = c < a.take_max ? rows[at] : -1;
            }
        }
        const int src = __ffsll(static_cast<unsigned long long>(__ballot(win))) - 1;
        const int32_t row = __shfl(myrow, src, kWave);
        bool dup = false;
        for (int base = 0; base < cnt; base += kWave) {
            const bool hit = __ballot(base + lane < cnt && seen[base + lane] == row) != 0;
            dup = dup || hit;
        }
        if (!dup) {
            if (lane == 0) {
                seen[cnt] = row;
                out_ids[cnt] = row;
                out_dist[cnt] = key_dist(w);
            }
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            __builtin_amdgcn_wave_barrier();
            cnt++;
        }
    }
    for (int i = cnt + lane; i < a.k; i += kWave) {
        out_ids[i] = -1;
        out_dist[i] = __uint_as_float(0x7f800000u);
    }
}

}  // namespace hg
