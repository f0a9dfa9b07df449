// ivf_range_kernels.hpp -- range search through the IVF lists (hnswgpu_ivf_range_search): every row of a query's PROBED lists
// within its radius, CSR results in the order of the query's candidate stream S(q) -- its probed lists in probe-table order,
// each in list order (ivf_flat.clj:281-288).  range_kernels.hpp's steps over a hit mask in STREAM space:
//
//   ivf_range_offsets_kernel -- a wave per query: woff[q][j] = the running sum of ceil(len(list(q, j)) / 32) over the query's
//   probes, woff[q][nprobe] its total.  A list always starts a fresh word, so the hit words of a (query, list) pair are the
//   LIST's words: a wave of the scan that owns 32 consecutive list positions owns one whole word of every query that probes the
//   list, whatever lies in front of the list in each query's stream.  The per-query stride Wq is the host's bound (the nprobe
//   largest word counts); the words between woff[q][nprobe] and Wq are cleared here by plain stores.
//
//   ivf_range_worklist_kernel -- one workgroup: the (query, list) pairs counted per list (the counts pair_order_kernel files
//   them by: its order[] holds list l's pairs at [ps[l], ps[l + 1])), a scan of the lists' item counts, and the items
//   (list, chunk of whole tiles, block of up to tq pairs) filled by bisection, chunk-major inside a list so that the blocks
//   reading the same rows are neighbours.
//
//   ivf_range_scan_kernel -- LIST-MAJOR: a workgroup takes one item, gathers the queries of its pairs -- not consecutive ones --
//   with their norms and radii into LDS, reads the list's rows contiguously from the list-ordered copy and walks them as
//   range_scan_kernel does (RB rows of a wave in registers, lane_partial + rows_sum_to_lane + finish_dist / sqrtf: the bits of
//   hnswgpu_batch_distances).  The step's ballot is shifted into lane s's register word and lane s stores it once, whole, at
//   hits[q(s)][woff[q(s)][j(s)] + word]: one writer per word, no atomic, zeros included.  A list is read once per block of tq
//   of the queries that probe it, not once per query.
//
//   counts, lims, sort -- unchanged: a hit mask in stream space is an allow-mask of Wq * 32 bits whose padding bits are clear.
//
//   ivf_range_fill_kernel -- range_fill_kernel's shape (a block of 1024 words of one query, rank = block prefix + popcounts
//   below) with the block's words dealt to the waves of several workgroups; a set bit of word w belongs to the probe j with
//   woff[q][j] <= w < woff[q][j + 1] (the query's woff row in LDS, bisected per word with hits), its position in the list is
//   32 (w - woff[q][j]) + bit, its id comes from the list's ids.  Ascending stream position by construction.
#pragma once
#include "range_kernels.hpp"

namespace hg {

constexpr int kIvfRangeMaxProbe = 1024;     // the fill's woff row in LDS; hnswgpu_ivf_search's own limit
constexpr int kIvfRangeMaxLists = 16384;    // pair_order_kernel's histogram (kOrderMaxLists)
constexpr int kIvfRangeListThreads = 1024;  // ivf_range_worklist_kernel
constexpr int kIvfRangeFillParts = 4;       // workgroups per (block of words, query) of ivf_range_fill_kernel: blockIdx.z

struct IvfRangeItem {
    int32_t list, chunk;   // rows [chunk * chunk_rows, ...) of the list
    int32_t pbegin, cnt;   // the pairs order[pbegin .. pbegin + cnt), 1 <= cnt <= tq
};

struct IvfRangeArgs {
    RangeArgs r;              // rows / row_norms: the list-ordered copy; n: list positions; nwords: Wq; hits: [nq][Wq] in stream space
    const int64_t *listoff;   // [nlist + 1]
    const int32_t *listids;   // [n]
    int32_t nlist;
    const int32_t *probes;    // the slice's [nq][nprobe], -1 = skip (ids outside [0, nlist) read as skip)
    int32_t nprobe;
    int32_t *woff;            // [nq][nprobe + 1]
    const int32_t *order;     // [nq * nprobe]: pair indices q * nprobe + j filed by list (pair_order_kernel)
    IvfRangeItem *items;      // [max_items]
    int32_t *nitems;
    int32_t max_items;
};

// the caller's (or the routing's) table [nq][src_np] -> [nq][dst_np]: an id outside [0, nlist) and a column past src_np are -1
__global__ void ivf_range_probes_kernel(const int32_t *src, int32_t src_np, int32_t *dst, int32_t dst_np, int64_t nq, int32_t nlist) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= nq * dst_np) return;
    const int64_t q = i / dst_np;
    const int32_t j = static_cast<int32_t>(i - q * dst_np);
    const int32_t l = j < src_np ? src[q * src_np + j] : -1;
    dst[i] = l >= 0 && l < nlist ? l : -1;
}

__global__ __launch_bounds__(kWG) void ivf_range_offsets_kernel(IvfRangeArgs a) {
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t q = static_cast<int64_t>(blockIdx.x) * kNWave + (threadIdx.x >> 6);
    if (q >= a.r.nq) return;
    const int32_t *pq = a.probes + q * a.nprobe;
    int32_t *wq = a.woff + q * (a.nprobe + 1);
    uint32_t carry = 0;
    for (int p0 = 0; p0 < a.nprobe; p0 += kWave) {
        const int p = p0 + lane;
        const int32_t l = p < a.nprobe ? pq[p] : -1;
        const uint32_t w = l >= 0 && l < a.nlist ? static_cast<uint32_t>((a.listoff[l + 1] - a.listoff[l] + 31) >> 5) : 0u;
        uint32_t incl = w;
        for (int off = 1; off < kWave; off <<= 1) {
            const uint32_t o = __shfl_up(incl, off, kWave);
            if (lane >= off) incl += o;
        }
        if (p < a.nprobe) wq[p] = static_cast<int32_t>(carry + incl - w);
        carry += __shfl(incl, kWave - 1, kWave);
    }
    if (lane == 0) wq[a.nprobe] = static_cast<int32_t>(carry);
    // the words no pair owns (the host's stride is a bound over all queries)
    uint32_t *hq = a.r.hits + q * a.r.nwords;
    for (int64_t w = static_cast<int64_t>(carry) + lane; w < a.r.nwords; w += kWave) hq[w] = 0u;
}

__host__ inline size_t ivf_range_worklist_lds_bytes(int nlist) { return 2 * sizeof(int32_t) * (static_cast<size_t>(nlist) + 2); }

// inclusive scan of part[0 .. 1024) in place (one value per thread of the workgroup)
__device__ __forceinline__ void ivf_range_scan1024(int32_t *part) {
    const int tid = threadIdx.x;
    for (int off = 1; off < kIvfRangeListThreads; off <<= 1) {
        const int add = tid >= off ? part[tid - off] : 0;
        __syncthreads();
        part[tid] += add;
        __syncthreads();
    }
}

__global__ __launch_bounds__(kIvfRangeListThreads) void ivf_range_worklist_kernel(IvfRangeArgs a) {
    extern __shared__ int32_t wl_s[];
    __shared__ int32_t part_p[kIvfRangeListThreads], part_i[kIvfRangeListThreads];
    int32_t *ps = wl_s;                // [nlist + 1]: counts, then the pairs filed below list l
    int32_t *is = wl_s + a.nlist + 2;  // [nlist + 1]: the items below list l
    const int tid = threadIdx.x, nl = a.nlist, tq = a.r.tq;
    const int64_t npairs = static_cast<int64_t>(a.r.nq) * a.nprobe;
    for (int i = tid; i <= nl; i += kIvfRangeListThreads) ps[i] = 0;
    __syncthreads();
    for (int64_t i = tid; i < npairs; i += kIvfRangeListThreads) {
        const int l = a.probes[i];
        if (l >= 0 && l < nl) atomicAdd(&ps[l], 1);
    }
    __syncthreads();
    // exclusive scans over the lists: every thread a contiguous range, then the 1024 range sums (pair_order_kernel)
    const int per = (nl + kIvfRangeListThreads - 1) / kIvfRangeListThreads, lo = tid * per < nl ? tid * per : nl, hi = lo + per < nl ? lo + per : nl;
    int sp = 0, si = 0;
    for (int l = lo; l < hi; l++) {
        const int c = ps[l];
        const int64_t len = a.listoff[l + 1] - a.listoff[l];
        const int nchunk = static_cast<int>((len + a.r.chunk_rows - 1) / a.r.chunk_rows);
        sp += c;
        si += (c + tq - 1) / tq * nchunk;
        is[l] = (c + tq - 1) / tq * nchunk;
    }
    part_p[tid] = sp;
    part_i[tid] = si;
    __syncthreads();
    ivf_range_scan1024(part_p);
    ivf_range_scan1024(part_i);
    int rp = part_p[tid] - sp, ri = part_i[tid] - si;
    for (int l = lo; l < hi; l++) {
        const int c = ps[l], it = is[l];
        ps[l] = rp;
        is[l] = ri;
        rp += c;
        ri += it;
    }
    if (tid == 0) {
        ps[nl] = part_p[kIvfRangeListThreads - 1];
        is[nl] = part_i[kIvfRangeListThreads - 1];
    }
    __syncthreads();
    const int nit = is[nl] < a.max_items ? is[nl] : a.max_items;  // (the host's bound holds: never cut)
    if (tid == 0) *a.nitems = nit;
    for (int i = tid; i < nit; i += kIvfRangeListThreads) {
        int l = 0, h = nl;  // the largest l with is[l] <= i: its items are [is[l], is[l + 1])
        while (h - l > 1) {
            const int mid = (l + h) >> 1;
            if (is[mid] <= i) l = mid;
            else h = mid;
        }
        const int c = ps[l + 1] - ps[l], nblk = (c + tq - 1) / tq, local = i - is[l];
        IvfRangeItem it;
        it.list = l;
        it.chunk = local / nblk;  // chunk-major
        const int b = local - it.chunk * nblk;
        it.pbegin = ps[l] + b * tq;
        it.cnt = c - b * tq < tq ? c - b * tq : tq;
        a.items[i] = it;
    }
}

template <int NCH, int RB, bool L2M>
__global__ __launch_bounds__(kTileThreads) void ivf_range_scan_kernel(IvfRangeArgs a) {
    extern __shared__ __align__(16) unsigned char smem[];
    static_assert(32 % RB == 0, "a word is a whole number of steps");
    __shared__ int32_t qs_s[32];   // slot s: its query ...
    __shared__ int64_t hw_s[32];   // ... and where the words of its pair begin in hits (-1: nowhere)
    const int nvec = static_cast<int>(a.r.ld / 4);
    float4 *Bs = reinterpret_cast<float4 *>(smem);                // [tq][nvec] the gathered queries
    float *qn_s = reinterpret_cast<float *>(Bs + a.r.tq * nvec);  // [tq] query norms (cosine)
    float *rad_s = qn_s + a.r.tq;                                 // [tq] radii
    const int tid = threadIdx.x;
    const int lane = tid & (kWave - 1);
    const int wave = tid >> 6;
    const int nit = *a.nitems < a.max_items ? *a.nitems : a.max_items;
    if (static_cast<int>(blockIdx.x) >= nit) return;  // past the work list: nothing staged
    const IvfRangeItem it = a.items[blockIdx.x];
    const int cnt = it.cnt < a.r.tq ? it.cnt : a.r.tq;
    const int64_t lb = a.listoff[it.list], len = a.listoff[it.list + 1] - lb;
    const int64_t lwords = (len + 31) >> 5;
    const int64_t r0 = it.chunk * a.r.chunk_rows;  // list positions
    const int64_t r1 = r0 + a.r.chunk_rows < len ? r0 + a.r.chunk_rows : len;
    if (r0 >= r1 || cnt <= 0) return;

    if (tid < cnt) {
        const int pair = a.order[it.pbegin + tid];
        const int q = pair / a.nprobe, j = pair - q * a.nprobe;
        const int64_t wo = a.woff[static_cast<int64_t>(q) * (a.nprobe + 1) + j];
        qs_s[tid] = q;
        hw_s[tid] = wo + lwords <= a.r.nwords ? static_cast<int64_t>(q) * a.r.nwords + wo : -1;
        qn_s[tid] = (!L2M && a.r.metric == METRIC_COS) ? a.r.q_norms[q] : 0.0f;
        rad_s[tid] = a.r.radius[q];
    }
    __syncthreads();
    {
        constexpr int kQU = 16;  // 32 x 256 float4 at most = 16 per thread
        const int total = cnt * nvec;
        const float4 *src = reinterpret_cast<const float4 *>(a.r.Qp);
        for (int f0 = tid; f0 < total; f0 += kTileThreads * kQU) {
            float4 v[kQU];
            int fc[kQU];
#pragma unroll
            for (int u = 0; u < kQU; u++) {  // clamped, unconditional: all loads of a thread in flight together
                const int f = f0 + u * kTileThreads;
                fc[u] = f < total ? f : total - 1;
                const int s = fc[u] / nvec;
                v[u] = src[static_cast<int64_t>(qs_s[s]) * nvec + (fc[u] - s * nvec)];
            }
#pragma unroll
            for (int u = 0; u < kQU; u++) Bs[fc[u]] = v[u];  // (an index past the end re-writes element total - 1 with its own value)
        }
    }
    __syncthreads();
    const int64_t myhw = lane < cnt ? hw_s[lane] : -1;
    const float *rows = a.r.rows + lb * a.r.ld;
    const float *norms = a.r.row_norms + lb;

    // wave w of a tile: list positions [tile + 32 w, tile + 32 w + 32) = word (tile >> 5) + w of the list
    for (int64_t wb = r0 + wave * 32; wb < r1; wb += kTileRows) {
        uint32_t word = 0;  // lane s: the hit bits of slot s among this word's rows
#pragma unroll 1
        for (int s = 0; s < 32 / RB; s++) {
            const int64_t base = wb + s * RB;
            if (base >= r1) break;  // wave-uniform: the rest of the word lies past the list, its bits stay clear
            float4 r[RB][NCH];
            const bool mine_in = lane < RB && base + lane < r1;
            const float myrn = (!L2M && a.r.metric == METRIC_COS && mine_in) ? norms[base + lane] : 0.0f;
#pragma unroll
            for (int b = 0; b < RB; b++) load_row<NCH>(r[b], rows + (base + b < r1 ? base + b : r1 - 1) * a.r.ld, nvec, lane, base + b < r1);
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
                const float d = L2M ? __builtin_sqrtf(mine) : finish_dist(a.r.metric, mine, qn, myrn);
                // (d <= radius is false for a NaN on either side)
                const unsigned long long m = __ballot(mine_in && d <= rad_s[q]);
                const uint32_t bits = static_cast<uint32_t>(m) << (s * RB);
                word |= lane == q ? bits : 0u;
            }
        }
        if (myhw >= 0) a.r.hits[myhw + (wb >> 5)] = word;  // (wb >> 5 < lwords: wb < len)
    }
}

// Workgroup (block b, query q, part z): the words [1024 b, 1024 b + 1024) of hits[q], four consecutive words per thread as in
// range_fill_kernel, so blk[q][b] + the popcounts below is a word's prefix -- kept per WORD in LDS, because a query's stream is
// short (nprobe lists: 124 words at 4 lists of 980 rows) and four words a thread would leave every hit to the block's first
// wave.  The words are dealt to the waves of the block's kIvfRangeFillParts workgroups instead (each computes the prefixes
// itself), and a wave evaluates the hits of ITS words one at a time with all 64 lanes.  A hit's row is found through the
// query's woff row and the list's offset, its id in the list's ids.
template <int NCH, bool L2M>
__global__ __launch_bounds__(kWG) void ivf_range_fill_kernel(IvfRangeArgs g) {
    __shared__ uint32_t ws[kNWave];
    __shared__ int32_t wo_s[kIvfRangeMaxProbe + 1];
    __shared__ uint32_t m_s[kRangeFillWords], pre_s[kRangeFillWords];  // the block's words and the block's hits below each
    const RangeArgs &a = g.r;
    const int lane = threadIdx.x & (kWave - 1);
    const int q = blockIdx.y;
    const int np = g.nprobe < kIvfRangeMaxProbe ? g.nprobe : kIvfRangeMaxProbe;
    const uint32_t *hq = a.hits + static_cast<int64_t>(q) * a.nwords;
    const int64_t w0 = static_cast<int64_t>(blockIdx.x) * kRangeFillWords + threadIdx.x * 4;
    uint32_t m[4];
    uint32_t c = 0;
#pragma unroll
    for (int u = 0; u < 4; u++) {
        const int64_t w = w0 + u;
        m[u] = w < a.nwords ? hq[w] : 0u;  // (the scan left the bits past a list's end clear, the offsets kernel the words past the stream's)
        c += __popc(m[u]);
    }
    uint32_t tot;
    uint32_t ex = wg_exclusive_sum(c, ws, &tot);
    if (tot == 0) return;  // workgroup-uniform
    for (int i = threadIdx.x; i <= np; i += kWG) wo_s[i] = g.woff[static_cast<int64_t>(q) * (g.nprobe + 1) + i];
#pragma unroll
    for (int u = 0; u < 4; u++) {
        m_s[threadIdx.x * 4 + u] = m[u];
        pre_s[threadIdx.x * 4 + u] = ex;
        ex += __popc(m[u]);
    }
    __syncthreads();
    const int64_t at0 = a.lims[q] + a.blk[static_cast<int64_t>(q) * a.nblk + blockIdx.x];  // where the block's first hit goes
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
    // the block's words dealt to the waves of its kIvfRangeFillParts workgroups, word wl to wave wl mod (parts x waves)
    const int64_t left = a.nwords - static_cast<int64_t>(blockIdx.x) * kRangeFillWords;
    const int nw = left < kRangeFillWords ? static_cast<int>(left) : kRangeFillWords;
    for (int wl = blockIdx.z * kNWave + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6); wl < nw; wl += kIvfRangeFillParts * kNWave) {
        uint32_t x = __builtin_amdgcn_readfirstlane(m_s[wl]);
        if (!x) continue;  // wave-uniform, as everything below
        const int64_t w = static_cast<int64_t>(blockIdx.x) * kRangeFillWords + wl;
        int j = 0, h = np;  // the probe that owns the word: the largest j with woff[j] <= w (probes without words are stepped over)
        while (h - j > 1) {
            const int mid = (j + h) >> 1;
            if (wo_s[mid] <= w) j = mid;
            else h = mid;
        }
        int32_t l = g.probes[static_cast<int64_t>(q) * g.nprobe + j];
        l = l >= 0 && l < g.nlist ? l : 0;  // (a word with a set bit belongs to a probed list)
        const int64_t pos0 = g.listoff[l] + (w - wo_s[j]) * 32;
        int64_t at = at0 + pre_s[wl];
        while (x) {
            int64_t row = pos0 + (__ffs(x) - 1);
            x &= x - 1;
            row = static_cast<uint64_t>(row) < static_cast<uint64_t>(a.n) ? row : 0;
            float4 r[NCH];
            load_row<NCH>(r, a.rows + row * a.ld, nvec, lane, true);
            const float s = wave_sum(lane_partial<NCH, L2M>(qv, r));
            if (lane == 0 && at < a.cap) {
                const float rn = (!L2M && a.metric == METRIC_COS) ? a.row_norms[row] : 0.0f;
                a.out_ids[at] = g.listids[row];
                a.out_dist[at] = L2M ? __builtin_sqrtf(s) : finish_dist(a.metric, s, qn, rn);
            }
            at++;
        }
    }
}

}  // namespace hg
