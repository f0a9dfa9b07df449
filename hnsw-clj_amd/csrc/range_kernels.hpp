// range_kernels.hpp -- exact range search: every row within a radius of a query, CSR results (hnswgpu_range_search).
//
// The answer's size depends on the data, so nothing here ends in a top-k selection.  Four steps, no atomic in any of them:
//
//   range_scan_kernel -- l2_group_kernel's walk (a query group resident in LDS, RB rows of a wave in registers, the distance
//   finished in lane b by lane_partial + rows_sum_to_lane + finish_dist / sqrtf: the bits of hnswgpu_batch_distances at every
//   batch size) with the store replaced by a compare and a ballot.  A wave owns 32 CONSECUTIVE rows of a tile -- one word of
//   every query's hit mask hits[q][row >> 5] -- and walks them in 32 / RB steps; lane q collects the steps' ballots of query q
//   in a register and stores the finished word: every word of every query is written exactly once, whole, zeros included.
//
//   counts -- hits[q] is an allow-mask in filter_kernels.hpp's format, so mask_count_kernel / mask_scan_kernel (mask =
//   blockIdx.y) give every query its per-block prefix sums and its total; range_lims_kernel scans the totals into lims, from
//   the running total of the slices before it (a device scalar: nothing is read back).
//
//   range_fill_kernel -- only hits get a second look: a workgroup takes one block of kMaskWordsPerWG words of one query, a set
//   bit's rank is the block's prefix + the words' popcounts below it, and the hit's distance is recomputed by a whole wave in
//   the gather arithmetic of hnswgpu_rerank (wave-strided f32 fma chain + butterfly): the bits the scan compared.  id and
//   distance go to lims[q] + rank: ascending row id by construction.
//
//   range_sort_kernel (HNSWGPU_RANGE_BY_DISTANCE) -- one workgroup per query, a bitonic network over make_key(distance, row
//   id), of any length: every merge runs in one direction (its first step mirrors the block), so the positions past the
//   segment's end behave as +inf keys that never move and their pairs are skipped.
#pragma once
#include "kernels.hpp"
#include "tile_args.hpp"

namespace hg {

constexpr int kRangeFillWords = 1024;    // words per workgroup of range_fill_kernel: mask_count_kernel's block (kMaskWordsPerWG)
constexpr int kRangeSortThreads = 1024;
constexpr int kRangeSortTile = 4096;     // keys of a segment that sort in LDS (32 KiB)

struct RangeArgs {
    const float *rows;
    const float *row_norms;
    int64_t ld;
    int64_t n;
    int32_t metric;
    // the slice's queries, numbered from 0
    const float *Qp;       // padded to stride ld (zero filled)
    const float *q_norms;  // cosine
    const float *radius;
    int32_t nq;
    int32_t tq;            // queries per group (filtered_group_queries)
    int32_t ngroups;
    int64_t chunk_rows;    // rows per workgroup of the scan: whole tiles, so whole words
    int64_t nwords;        // W = (n + 31) / 32
    uint32_t *hits;        // [nq][W]
    const uint32_t *blk;   // [nq][nblk]: hits of query q below block b (mask_scan_kernel)
    int32_t nblk;
    const unsigned long long *qtot;  // [nq]: hits of query q
    unsigned long long *run;         // [1]: results of the slices before this one; this one's added behind the scan
    int32_t first;                   // the call's first slice: *run counts from 0
    int64_t *lims;                   // the slice's part of the call's lims: [nq] (+ 1: the running total)
    int32_t *out_ids;                // the CALL's arrays: lims index them
    float *out_dist;
    int64_t cap;
};

__host__ inline size_t range_scan_lds_bytes(int64_t ld, int tq) {
    return sizeof(float) * static_cast<size_t>(tq) * static_cast<size_t>(ld) + 2 * sizeof(float) * static_cast<size_t>(tq);
}

template <int NCH, int RB, bool L2M>
__global__ __launch_bounds__(kTileThreads) void range_scan_kernel(RangeArgs a) {
    extern __shared__ __align__(16) unsigned char smem[];
    static_assert(32 % RB == 0, "a word is a whole number of steps");
    const int nvec = static_cast<int>(a.ld / 4);
    float4 *Bs = reinterpret_cast<float4 *>(smem);              // [tq][nvec] resident query group
    float *qn_s = reinterpret_cast<float *>(Bs + a.tq * nvec);  // [tq] query norms (cosine)
    float *rad_s = qn_s + a.tq;                                 // [tq] radii
    const int tid = threadIdx.x;
    const int lane = tid & (kWave - 1);
    const int wave = tid >> 6;
    // chunk-major: the workgroups of one chunk of rows run side by side and share its rows in L2 (filtered_group_kernel)
    const int g = blockIdx.x % a.ngroups;
    const int64_t chunk = blockIdx.x / a.ngroups;
    const int64_t r0 = chunk * a.chunk_rows;
    const int64_t r1 = r0 + a.chunk_rows < a.n ? r0 + a.chunk_rows : a.n;
    const int q0 = g * a.tq;
    const int cnt = a.nq - q0 < a.tq ? a.nq - q0 : a.tq;
    if (r0 >= r1 || cnt <= 0) return;

    if (tid < cnt) {
        qn_s[tid] = (!L2M && a.metric == METRIC_COS) ? a.q_norms[q0 + tid] : 0.0f;
        rad_s[tid] = a.radius[q0 + tid];
    }
    {
        constexpr int kQU = 16;  // 32 x 256 float4 at most = 16 per thread
        const int total = cnt * nvec;
        const float4 *src = reinterpret_cast<const float4 *>(a.Qp + static_cast<int64_t>(q0) * a.ld);  // the group's rows are contiguous
        for (int f0 = tid; f0 < total; f0 += kTileThreads * kQU) {
            float4 v[kQU];
            int fc[kQU];
#pragma unroll
            for (int u = 0; u < kQU; u++) {  // clamped, unconditional: all loads of a thread in flight together
                const int f = f0 + u * kTileThreads;
                fc[u] = f < total ? f : total - 1;
                v[u] = src[fc[u]];
            }
#pragma unroll
            for (int u = 0; u < kQU; u++) Bs[fc[u]] = v[u];  // (an index past the end re-writes element total - 1 with its own value)
        }
    }
    __syncthreads();

    // wave w of a tile: rows [tile + 32 w, tile + 32 w + 32) = word (tile >> 5) + w of every query
    for (int64_t wb = r0 + wave * 32; wb < r1; wb += kTileRows) {
        uint32_t word = 0;  // lane q: the hit bits of query slot q among this word's rows
#pragma unroll 1
        for (int s = 0; s < 32 / RB; s++) {
            const int64_t base = wb + s * RB;
            if (base >= r1) break;  // wave-uniform: the rest of the word lies past the rows, its bits stay clear
            float4 r[RB][NCH];
            const bool mine_in = lane < RB && base + lane < r1;
            const float myrn = (!L2M && a.metric == METRIC_COS && mine_in) ? a.row_norms[base + lane] : 0.0f;
#pragma unroll
            for (int b = 0; b < RB; b++) load_row<NCH>(r[b], a.rows + (base + b < r1 ? base + b : r1 - 1) * a.ld, nvec, lane, base + b < r1);
            for (int q = 0; q < cnt; q++) {
                const float qn = L2M ? 0.0f : qn_s[q];
                float4 qv[NCH];
#pragma unroll
                for (int c = 0; c < NCH; c++) {
                    const int i = c * kWave + lane;
                    qv[c] = i < nvec ? Bs[q * nvec + i] : make_float4(0.f, 0.f, 0.f, 0.f);
                }
                float sum[RB];
#pragma unroll
                for (int b = 0; b < RB; b++) sum[b] = lane_partial<NCH, L2M>(qv, r[b]);
                const float mine = rows_sum_to_lane<RB>(sum, lane);  // lane b: row b's sum
                const float d = L2M ? __builtin_sqrtf(mine) : finish_dist(a.metric, mine, qn, myrn);
                // (d <= radius is false for a NaN on either side)
                const unsigned long long m = __ballot(mine_in && d <= rad_s[q]);
                const uint32_t bits = static_cast<uint32_t>(m) << (s * RB);
                word |= lane == q ? bits : 0u;
            }
        }
        if (lane < cnt) a.hits[static_cast<int64_t>(q0 + lane) * a.nwords + (wb >> 5)] = word;
    }
}

// exclusive prefix sum of 64-bit v over the workgroup's NW waves; *tot: the workgroup's sum.  ws: NW entries of LDS.
template <int NW>
__device__ __forceinline__ unsigned long long wg_exclusive_scan64(unsigned long long v, unsigned long long *ws, unsigned long long *tot) {
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    unsigned long long inc = v;
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
        const unsigned long long t = __shfl_up(inc, off, kWave);
        inc += lane >= off ? t : 0ull;
    }
    if (lane == kWave - 1) ws[wave] = inc;
    __syncthreads();
    unsigned long long before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < NW; w++) {
        const unsigned long long c = ws[w];
        before += w < wave ? c : 0ull;
        all += c;
    }
    __syncthreads();
    *tot = all;
    return before + inc - v;
}

// One workgroup: lims[q] = results before the slice + hits of the slice's queries below q; the running total moves on and is
// the next entry of lims (the next slice rewrites it with the same value, the last slice's is lims[nq] of the call).
__global__ __launch_bounds__(kRangeSortThreads) void range_lims_kernel(RangeArgs a) {
    __shared__ unsigned long long ws[kRangeSortThreads / kWave];
    unsigned long long carry = a.first ? 0ull : *a.run;
    for (int i0 = 0; i0 < a.nq; i0 += kRangeSortThreads) {
        const int i = i0 + threadIdx.x;
        const unsigned long long v = i < a.nq ? a.qtot[i] : 0ull;
        unsigned long long tot;
        const unsigned long long ex = wg_exclusive_scan64<kRangeSortThreads / kWave>(v, ws, &tot);
        if (i < a.nq) a.lims[i] = static_cast<int64_t>(carry + ex);
        carry += tot;
    }
    // (every thread has read *a.run before the first barrier of the loop; nq >= 1)
    if (threadIdx.x == 0) {
        a.lims[a.nq] = static_cast<int64_t>(carry);
        *a.run = carry;
    }
}

// no rows, or no queries' worth of work: lims all zero
__global__ void range_zero_lims_kernel(int64_t *lims, int64_t cnt) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i < cnt) lims[i] = 0;
}

// Workgroup (block b, query q): the words [1024 b, 1024 b + 1024) of hits[q], four consecutive words per thread as in
// mask_count_kernel, so blk[q][b] + the threads' popcounts below is a word's prefix.  A wave then walks ITS lanes' words in
// lane order -- ascending row id -- and evaluates one hit at a time with all 64 lanes: the gather arithmetic, one wave per row.
template <int NCH, bool L2M>
__global__ __launch_bounds__(kWG) void range_fill_kernel(RangeArgs a) {
    __shared__ uint32_t ws[kNWave];
    const int lane = threadIdx.x & (kWave - 1);
    const int q = blockIdx.y;
    const uint32_t *hq = a.hits + static_cast<int64_t>(q) * a.nwords;
    const int64_t w0 = static_cast<int64_t>(blockIdx.x) * kRangeFillWords + threadIdx.x * 4;
    uint32_t m[4];
    uint32_t c = 0;
#pragma unroll
    for (int u = 0; u < 4; u++) {
        const int64_t w = w0 + u;
        m[u] = w < a.nwords ? hq[w] : 0u;  // (the scan left the bits at rows >= n clear)
        c += __popc(m[u]);
    }
    uint32_t tot;
    const uint32_t ex = wg_exclusive_sum(c, ws, &tot);
    if (tot == 0) return;  // workgroup-uniform
    const int64_t at0 = a.lims[q] + a.blk[static_cast<int64_t>(q) * a.nblk + blockIdx.x] + ex;  // where this thread's first hit goes
    const unsigned long long busy = __ballot(c != 0);
    if (busy == 0) return;  // wave-uniform
    const int nvec = static_cast<int>(a.ld / 4);
    float4 qv[NCH];
    {
        const float4 *qp = reinterpret_cast<const float4 *>(a.Qp + static_cast<int64_t>(q) * a.ld);
#pragma unroll
        for (int c4 = 0; c4 < NCH; c4++) {
            const int i = c4 * kWave + lane;
            qv[c4] = i < nvec ? qp[i] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
    const float qn = (!L2M && a.metric == METRIC_COS) ? a.q_norms[q] : 0.0f;
    const uint32_t at_lo = static_cast<uint32_t>(at0), at_hi = static_cast<uint32_t>(static_cast<unsigned long long>(at0) >> 32);
    for (unsigned long long rest = busy; rest; rest &= rest - 1) {
        const int src = __builtin_ctzll(rest);  // wave-uniform: the next lane with hits
        int64_t at = static_cast<int64_t>((static_cast<unsigned long long>(__builtin_amdgcn_readlane(at_hi, src)) << 32) |
                                          static_cast<uint32_t>(__builtin_amdgcn_readlane(at_lo, src)));
#pragma unroll
        for (int u = 0; u < 4; u++) {
            uint32_t x = __builtin_amdgcn_readlane(m[u], src);
            const int64_t row0 = (static_cast<int64_t>(blockIdx.x) * kRangeFillWords + (static_cast<int64_t>(threadIdx.x & ~(kWave - 1)) + src) * 4 + u) * 32;
            while (x) {  // wave-uniform
                const int64_t row = row0 + (__ffs(x) - 1);
                x &= x - 1;
                float4 r[NCH];
                load_row<NCH>(r, a.rows + row * a.ld, nvec, lane, true);
                const float s = wave_sum(lane_partial<NCH, L2M>(qv, r));
                if (lane == 0 && at < a.cap) {
                    const float rn = (!L2M && a.metric == METRIC_COS) ? a.row_norms[row] : 0.0f;
                    a.out_ids[at] = static_cast<int32_t>(row);
                    a.out_dist[at] = L2M ? __builtin_sqrtf(s) : finish_dist(a.metric, s, qn, rn);
                }
                at++;
            }
        }
    }
}

// ---- HNSWGPU_RANGE_BY_DISTANCE: a query's segment ascending by (distance, row id) ---------------------------------------
__device__ __forceinline__ void range_cmpswap(uint64_t &x, uint64_t &y) {
    const uint64_t lo = x < y ? x : y, hi = x < y ? y : x;
    x = lo;
    y = hi;
}

// pair i of a merge step over blocks of `size` keys: the mirror step (first of a merge) or the step at `stride`
__device__ __forceinline__ void range_pair(int64_t i, int64_t size, int64_t stride, bool mirror, int64_t &x, int64_t &y) {
    if (mirror) {
        const int64_t half = size >> 1, blk = i / half, off = i - blk * half;
        x = blk * size + off;
        y = blk * size + size - 1 - off;
    } else {
        const int64_t blk = i / stride, off = i - blk * stride;
        x = blk * 2 * stride + off;
        y = x + stride;
    }
}

// the steps of a merge that stay inside a tile of T keys held in LDS (keys past len: ~0, never the smaller of a pair)
__device__ __forceinline__ void range_sort_lds_steps(uint64_t *ks, int T, int64_t size_from, int64_t size_to, bool tail_only) {
    for (int64_t size = size_from; size <= size_to; size <<= 1) {
        // tail_only: the merge's wide steps ran in global memory; strides below T remain
        int64_t stride = tail_only ? T >> 1 : size >> 1;
        bool mirror = !tail_only;
        for (; stride >= 1; stride >>= 1, mirror = false) {
            for (int i = threadIdx.x; i < T / 2; i += kRangeSortThreads) {
                int64_t x, y;
                range_pair(i, mirror ? size : 2 * stride, stride, mirror, x, y);
                uint64_t kx = ks[x], ky = ks[y];
                range_cmpswap(kx, ky);
                ks[x] = kx;
                ks[y] = ky;
            }
            __syncthreads();
        }
    }
}

__global__ __launch_bounds__(kRangeSortThreads) void range_sort_kernel(RangeArgs a) {
    __shared__ uint64_t ks[kRangeSortTile];
    const int q = blockIdx.x;
    const int64_t s0 = a.lims[q] < a.cap ? a.lims[q] : a.cap;
    const int64_t s1 = a.lims[q + 1] < a.cap ? a.lims[q + 1] : a.cap;
    const int64_t len = s1 - s0;  // workgroup-uniform
    if (len < 2) return;
    int32_t *ids = a.out_ids + s0;
    float *dist = a.out_dist + s0;
    int64_t P = 2;
    while (P < len) P <<= 1;
    const int64_t tileP = P < kRangeSortTile ? P : kRangeSortTile;
    // every tile: keys into LDS, the merges up to the tile's size, ids and distances back
    for (int64_t t0 = 0; t0 < len; t0 += kRangeSortTile) {
        for (int i = threadIdx.x; i < tileP; i += kRangeSortThreads)
            ks[i] = t0 + i < len ? make_key(dist[t0 + i], static_cast<uint32_t>(ids[t0 + i])) : ~0ull;
        __syncthreads();
        range_sort_lds_steps(ks, static_cast<int>(tileP), 2, tileP, false);
        for (int i = threadIdx.x; i < tileP; i += kRangeSortThreads)
            if (t0 + i < len) {
                ids[t0 + i] = static_cast<int32_t>(static_cast<uint32_t>(ks[i]));
                dist[t0 + i] = key_dist(ks[i]);
            }
        __syncthreads();
    }
    // the wider merges: steps at strides >= a tile through global memory (a pair past the end holds a +inf key: skipped), the
    // rest per tile in LDS
    for (int64_t size = 2 * static_cast<int64_t>(kRangeSortTile); size <= P; size <<= 1) {
        bool mirror = true;
        for (int64_t stride = size >> 1; stride >= kRangeSortTile; stride >>= 1, mirror = false) {
            for (int64_t i = threadIdx.x; i < P / 2; i += kRangeSortThreads) {
                int64_t x, y;
                range_pair(i, mirror ? size : 2 * stride, stride, mirror, x, y);
                if (y < len) {
                    const int32_t ix = ids[x], iy = ids[y];
                    const float dx = dist[x], dy = dist[y];
                    if (make_key(dy, static_cast<uint32_t>(iy)) < make_key(dx, static_cast<uint32_t>(ix))) {
                        ids[x] = iy;
                        dist[x] = dy;
                        ids[y] = ix;
                        dist[y] = dx;
                    }
                }
            }
            __syncthreads();
        }
        for (int64_t t0 = 0; t0 < len; t0 += kRangeSortTile) {
            for (int i = threadIdx.x; i < kRangeSortTile; i += kRangeSortThreads)
                ks[i] = t0 + i < len ? make_key(dist[t0 + i], static_cast<uint32_t>(ids[t0 + i])) : ~0ull;
            __syncthreads();
            range_sort_lds_steps(ks, kRangeSortTile, size, size, true);
            for (int i = threadIdx.x; i < kRangeSortTile; i += kRangeSortThreads)
                if (t0 + i < len) {
                    ids[t0 + i] = static_cast<int32_t>(static_cast<uint32_t>(ks[i]));
                    dist[t0 + i] = key_dist(ks[i]);
                }
            __syncthreads();
        }
    }
}

}  // namespace hg
