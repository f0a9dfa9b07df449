// range_filtered_kernels.hpp -- range search under an allow-mask (hnswgpu_range_search_filtered[_each]): the rows a mask lets
// pass within a radius of a query, CSR results.  range_kernels.hpp's four steps, with the scan and the fill GATHERED:
//
//   pass list -- the mask (Each: the union of a query group's masks) compacted into the ascending list of passing row ids by
//   filter_kernels.hpp's count / scan / scatter (no atomic: the same list on every run); Each adds union_words_kernel's word per
//   union row, bit j = "query j of the group allows it".  The list's length p stays ON THE DEVICE (cnt[g]): nothing is read
//   back, so the lists hold n entries and every grid below is sized by n.
//
//   range_gather_scan_kernel -- range_scan_kernel's walk (query group and radii resident in LDS, RB rows of a wave in
//   registers, lane_partial + rows_sum_to_lane + finish_dist / sqrtf: the bits of hnswgpu_batch_distances) over list
//   POSITIONS: a wave owns 32 consecutive positions = one word of every query's hit mask IN PASS-LIST SPACE,
//   hits[q][pos >> 5].  Lane b fetches the id of position base + b (and that row's norm and, Each, its union word), readlane
//   makes the row addresses wave-uniform (filtered_group_kernel), and the step's ballot is shifted into lane q's register
//   word, stored once, whole.  Each: a query none of whose bits is set among the step's rows is skipped without touching its
//   LDS vector, and the ballot's predicate gains the row's bit.
//   The host does not know p, so the grid is the unfiltered scan's (nchunks x ngroups, chunk-major) and the kernel cuts the p
//   positions into nchunks chunks of whole tiles ITSELF: the passing rows spread over all workgroups whatever the mask's
//   density, and a workgroup whose chunk is empty leaves before it stages a query.  The count pass walks all W words of a
//   query, so the words past the list's end must read zero: every workgroup clears, of ITS n-sized chunk, the words at or
//   past ceil(p / 32) -- plain stores, no memset node (the call may be captured into a graph).
//
//   counts, lims -- unchanged: hit masks in pass-list space are allow-masks of n bits (p <= n; the bits at and past p are 0).
//
//   range_fill_gather_kernel -- range_fill_kernel with one indirection: a set bit at position pos is row list[pos].  Ascending
//   position is ascending row id, because the lists are ascending.
//
//   range_sort_kernel -- unchanged.
#pragma once
#include "range_kernels.hpp"

namespace hg {

struct RangeGatherArgs {
    RangeArgs r;                     // r.hits: [nq][W] in pass-list space; r.chunk_rows: the n-sized chunk (whole tiles)
    const int32_t *pass;             // Single: [n], every group's list.  Each: [ngroups][lstride], group g's union list
    const uint32_t *uw;              // Each: [ngroups][lstride], who of the group allows the row (union_words_kernel)
    const unsigned long long *cnt;   // entries of the list: [1], or Each [ngroups]
    int64_t lstride;                 // entries between two groups' lists; 0: one list
    int32_t nchunks;                 // workgroups per group
};

// the list of group g and its length as the kernels trust it: at most n entries
__device__ __forceinline__ int64_t range_list_len(const RangeGatherArgs &a, int g) {
    const unsigned long long p = a.cnt[a.lstride ? g : 0];
    return p < static_cast<unsigned long long>(a.r.n) ? static_cast<int64_t>(p) : a.r.n;
}

template <int NCH, int RB, bool L2M, bool EACH>
__global__ __launch_bounds__(kTileThreads) void range_gather_scan_kernel(RangeGatherArgs a) {
    extern __shared__ __align__(16) unsigned char smem[];
    static_assert(32 % RB == 0, "a word is a whole number of steps");
    const int nvec = static_cast<int>(a.r.ld / 4);
    float4 *Bs = reinterpret_cast<float4 *>(smem);                // [tq][nvec] resident query group
    float *qn_s = reinterpret_cast<float *>(Bs + a.r.tq * nvec);  // [tq] query norms (cosine)
    float *rad_s = qn_s + a.r.tq;                                 // [tq] radii
    const int tid = threadIdx.x;
    const int lane = tid & (kWave - 1);
    const int wave = tid >> 6;
    // chunk-major: the workgroups of one chunk of the list run side by side and share its rows in L2
    const int g = blockIdx.x % a.r.ngroups;
    const int64_t chunk = blockIdx.x / a.r.ngroups;
    const int q0 = g * a.r.tq;
    const int cnt = a.r.nq - q0 < a.r.tq ? a.r.nq - q0 : a.r.tq;
    if (cnt <= 0) return;
    const int64_t p = range_list_len(a, g);
    const int32_t *pass = a.pass + g * a.lstride;
    const uint32_t *uw = EACH ? a.uw + g * a.lstride : nullptr;

    // the words past the list's end, of this workgroup's n-sized chunk: zero
    {
        const int64_t wp = (p + 31) >> 5;
        int64_t z0 = chunk * a.r.chunk_rows >> 5, z1 = (chunk + 1) * a.r.chunk_rows >> 5;
        z0 = z0 > wp ? z0 : wp;
        z1 = z1 < a.r.nwords ? z1 : a.r.nwords;
        for (int q = 0; q < cnt; q++)
            for (int64_t w = z0 + tid; w < z1; w += kTileThreads) a.r.hits[static_cast<int64_t>(q0 + q) * a.r.nwords + w] = 0u;
    }
    // this workgroup's chunk of the p positions: whole tiles, nchunks of them cover the list
    const int64_t tiles = (p + kTileRows - 1) / kTileRows;
    const int64_t crows = (tiles + a.nchunks - 1) / a.nchunks * kTileRows;
    const int64_t r0 = chunk * crows;
    const int64_t r1 = r0 + crows < p ? r0 + crows : p;
    if (r0 >= r1) return;  // workgroup-uniform

    if (tid < cnt) {
        qn_s[tid] = (!L2M && a.r.metric == METRIC_COS) ? a.r.q_norms[q0 + tid] : 0.0f;
        rad_s[tid] = a.r.radius[q0 + tid];
    }
    {
        constexpr int kQU = 16;  // 32 x 256 float4 at most = 16 per thread
        const int total = cnt * nvec;
        const float4 *src = reinterpret_cast<const float4 *>(a.r.Qp + static_cast<int64_t>(q0) * a.r.ld);  // the group's rows are contiguous
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

    // wave w of a tile: positions [tile + 32 w, tile + 32 w + 32) = word (tile >> 5) + w of every query
    for (int64_t wb = r0 + wave * 32; wb < r1; wb += kTileRows) {
        uint32_t word = 0;  // lane q: the hit bits of query slot q among this word's positions
#pragma unroll 1
        for (int s = 0; s < 32 / RB; s++) {
            const int64_t base = wb + s * RB;
            if (base >= r1) break;  // wave-uniform: the rest of the word lies past the list, its bits stay clear
            float4 r[RB][NCH];
            // lane b (and every lane beyond RB, as row RB - 1): the id of position base + b, clamped into the chunk, its norm
            // and, Each, its word
            const int64_t mypos = base + (lane < RB ? lane : RB - 1);
            const bool mine_in = lane < RB && mypos < r1;
            int32_t myid = pass[mypos < r1 ? mypos : r1 - 1];
            myid = static_cast<uint32_t>(myid) < static_cast<uint64_t>(a.r.n) ? myid : 0;  // (a mask its owner rewrites during the call)
            const float myrn = (!L2M && a.r.metric == METRIC_COS) ? a.r.row_norms[myid] : 0.0f;
            uint32_t myw = 0, anyw = 0;
            if constexpr (EACH) myw = mypos < r1 ? uw[mypos] : 0u;  // (a position past the chunk's end: nobody's)
#pragma unroll
            for (int b = 0; b < RB; b++) {
                const int64_t row = __builtin_amdgcn_readlane(myid, b);
                load_row<NCH>(r[b], a.r.rows + row * a.r.ld, nvec, lane, true);
                if constexpr (EACH) anyw |= static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(myw), b));
            }
            for (int q = 0; q < cnt; q++) {
                if constexpr (EACH) {
                    if (!((anyw >> q) & 1u)) continue;  // wave-uniform: none of the RB rows is this query's
                }
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
                const float d = L2M ? __builtin_sqrtf(mine) : finish_dist(a.r.metric, mine, qn, myrn);
                // (d <= radius is false for a NaN on either side)
                const bool allowed = !EACH || ((myw >> q) & 1u);
                const unsigned long long m = __ballot(mine_in && allowed && d <= rad_s[q]);
                const uint32_t bits = static_cast<uint32_t>(m) << (s * RB);
                word |= lane == q ? bits : 0u;
            }
        }
        if (lane < cnt) a.r.hits[static_cast<int64_t>(q0 + lane) * a.r.nwords + (wb >> 5)] = word;
    }
}

// range_fill_kernel over hit masks in pass-list space: workgroup (block b, query q) takes the words [1024 b, 1024 b + 1024) of
// hits[q]; a set bit at position pos is row list[pos] of the query's group, evaluated by a whole wave in the gather arithmetic.
template <int NCH, bool L2M>
__global__ __launch_bounds__(kWG) void range_fill_gather_kernel(RangeGatherArgs g) {
    __shared__ uint32_t ws[kNWave];
    const RangeArgs &a = g.r;
    const int lane = threadIdx.x & (kWave - 1);
    const int q = blockIdx.y;
    const uint32_t *hq = a.hits + static_cast<int64_t>(q) * a.nwords;
    const int64_t w0 = static_cast<int64_t>(blockIdx.x) * kRangeFillWords + threadIdx.x * 4;
    uint32_t m[4];
    uint32_t c = 0;
#pragma unroll
    for (int u = 0; u < 4; u++) {
        const int64_t w = w0 + u;
        m[u] = w < a.nwords ? hq[w] : 0u;  // (the scan left the bits at positions >= p clear)
        c += __popc(m[u]);
    }
    uint32_t tot;
    const uint32_t ex = wg_exclusive_sum(c, ws, &tot);
    if (tot == 0) return;  // workgroup-uniform
    const int64_t at0 = a.lims[q] + a.blk[static_cast<int64_t>(q) * a.nblk + blockIdx.x] + ex;  // where this thread's first hit goes
    const unsigned long long busy = __ballot(c != 0);
    if (busy == 0) return;  // wave-uniform
    const int32_t *list = g.pass + static_cast<int64_t>(q / a.tq) * g.lstride;
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
            const int64_t pos0 = (static_cast<int64_t>(blockIdx.x) * kRangeFillWords + (static_cast<int64_t>(threadIdx.x & ~(kWave - 1)) + src) * 4 + u) * 32;
            while (x) {  // wave-uniform
                const int64_t pos = pos0 + (__ffs(x) - 1);  // < p <= n: a hit bit is a list position
                x &= x - 1;
                int64_t row = list[pos];
                row = static_cast<uint64_t>(row) < static_cast<uint64_t>(a.n) ? row : 0;
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

}  // namespace hg
