// filter_kernels.hpp -- filtered search (FilterableIndex/search-knn-filtered*, api/protocol.clj:34-41,97-102).
//
// One allow-mask per call, shared by its queries: (n + 31) / 32 words, row i may be returned iff bit (i & 31) of word
// i >> 5 is set; bits at positions >= n are ignored.  Two services are built on it:
//
//   few rows pass -- mask_compact turns the mask into the ascending list of passing row ids (popcounts and a scan, no
//   atomic: the list is the same on every run), filtered_group_kernel evaluates exactly those rows, each fetched once per
//   query GROUP, into a dense [query][position in the passing list] array, and the dense top-k selection + a decode
//   (position -> row id) finish the call.  The work per (row, query) pair is lane_partial + rows_sum_to_lane +
//   finish_dist: the GEMV summation order at every batch size, the bits hnswgpu_rerank and scan_kernel produce.  Ties go
//   to the lower position = the lower row id.
//
//   one mask per QUERY (the *_filtered_each entry points) -- the same chain over the UNION of a query group's masks:
//   mask_union_kernel ORs the group's masks, the three compaction launches run once for all groups (group = blockIdx.y),
//   union_words_kernel gives every union row one word with bit j = "query j of the group allows it", and the EACH form of
//   filtered_group_kernel fetches a union row once for the group and finishes a distance only for the queries whose bit
//   is set; every other (row, query) entry of the dense array holds kSkipDist, a key above +inf, and
//   filter_each_decode_kernel turns whatever the selection kept of those into -1 / +inf BY THE BIT, not by the value.
//
//   many rows pass -- the traversal runs untouched for min(ef, 1024) results and filter_take_kernel keeps the first k
//   passing entries of each query's result list, in list order.
//
//   IVF-FLAT (search-ivf-flat, ivf_flat.clj:261-294) -- the mask is turned round into LIST order (list_mask_kernel: bit pos
//   = the bit of row list_ids[pos]), compacted by the same three launches into the ascending list of passing list
//   POSITIONS, and cut at the list boundaries (list_foff_kernel).  A probed list's passing rows are then a segment of that
//   list, and ivf_filtered_scan_kernel -- the gathered form of scan_kernel's top-k body -- reads exactly those rows.  Keys
//   carry the position in the UNFILTERED candidate stream, so the merge and the decode of the unfiltered search finish it.
//
//   IVF-FLAT, one mask per QUERY (hnswgpu_ivf_search_filtered_each) -- no list-order mask (nq x L bits) and no compaction:
//   ivf_each_scan_kernel walks the UNFILTERED probed lists in scan_kernel's chunks, tests a row's bit in its query's mask where
//   it reads the list id (64 positions, one ballot), queues the passing positions per wave in LDS and runs RB of them at a time
//   through ivf_filtered_scan_kernel's step (ivf_gathered_step: one for both).  Same keys, same merge, same decode: the single-mask call's ids and bits.
#pragma once
#include "kernels.hpp"
#include "tile_args.hpp"

namespace hg {

// ---- mask -> ascending list of passing row ids -----------------------------------------------------------------
constexpr int kMaskThreads = 256;
constexpr int kMaskWordsPerThread = 4;  // consecutive words of one thread: its ids are consecutive in the list
constexpr int kMaskWordsPerWG = kMaskThreads * kMaskWordsPerThread;
constexpr int kMaskScanThreads = 1024;

struct MaskArgs {
    const uint32_t *allow;
    int64_t n;       // rows (>= 1)
    int64_t nwords;  // (n + 31) / 32
    uint32_t *blk;   // [nblk]: passing rows per workgroup of the count pass, then their exclusive prefix sums
    int32_t nblk;
    int32_t *pass_ids;          // [cap]
    int64_t cap;                // entries pass_ids holds (the count the scan produced)
    unsigned long long *total;  // [1]: passing rows
    // several masks in one launch, mask g = blockIdx.y (engine.hip: mask_count_scan / mask_scatter; mask_compact is one mask)
    int64_t allow_stride;  // words between two masks
    int64_t blk_stride;    // entries of blk between two masks
    int64_t pass_stride;   // entries of pass_ids between two lists
    int64_t total_stride;  // entries of total between two masks (0 or 1)
};

// the arguments of mask blockIdx.y
__device__ __forceinline__ MaskArgs mask_of_group(MaskArgs a) {
    const int64_t g = blockIdx.y;
    a.allow += g * a.allow_stride;
    a.blk += g * a.blk_stride;
    a.pass_ids += g * a.pass_stride;
    a.total += g * a.total_stride;
    return a;
}

// word w of the mask as the kernels see it: nothing past the mask, the last word trimmed to n
__device__ __forceinline__ uint32_t mask_word(const MaskArgs &a, int64_t w) {
    const uint32_t m = a.allow[w < a.nwords ? w : a.nwords - 1];  // clamped, unconditional
    const int tail = static_cast<int>(a.n & 31);
    const uint32_t keep = (w == a.nwords - 1 && tail) ? (1u << tail) - 1u : 0xffffffffu;
    return w < a.nwords ? m & keep : 0u;
}

// exclusive prefix sum of v over the NW waves of the workgroup; *tot: the workgroup's sum.  ws: NW words of LDS, free
// again on return.
template <int NW>
__device__ __forceinline__ uint32_t wg_exclusive_scan(uint32_t v, uint32_t *ws, uint32_t *tot) {
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
        const uint32_t t = __shfl_up(inc, off, kWave);
        inc += lane >= off ? t : 0u;
    }
    if (lane == kWave - 1) ws[wave] = inc;
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < NW; w++) {
        const uint32_t c = ws[w];
        before += w < wave ? c : 0u;
        all += c;
    }
    __syncthreads();
    *tot = all;
    return before + inc - v;
}

__global__ __launch_bounds__(kMaskThreads) void mask_count_kernel(MaskArgs a0) {
    const MaskArgs a = mask_of_group(a0);
    __shared__ uint32_t ws[kMaskThreads / kWave];
    const int64_t w0 = static_cast<int64_t>(blockIdx.x) * kMaskWordsPerWG + threadIdx.x * kMaskWordsPerThread;
    uint32_t c = 0;
#pragma unroll
    for (int u = 0; u < kMaskWordsPerThread; u++) c += __popc(mask_word(a, w0 + u));
    uint32_t tot;
    (void)wg_exclusive_scan<kMaskThreads / kWave>(c, ws, &tot);
    if (threadIdx.x == 0) a.blk[blockIdx.x] = tot;
}

// one workgroup: blk[] -> its exclusive prefix sums, *total = the sum
__global__ __launch_bounds__(kMaskScanThreads) void mask_scan_kernel(MaskArgs a0) {
    const MaskArgs a = mask_of_group(a0);
    __shared__ uint32_t ws[kMaskScanThreads / kWave];
    unsigned long long carry = 0;
    for (int i0 = 0; i0 < a.nblk; i0 += kMaskScanThreads) {
        const int i = i0 + threadIdx.x;
        const uint32_t v = i < a.nblk ? a.blk[i] : 0u;
        uint32_t tot;
        const uint32_t ex = wg_exclusive_scan<kMaskScanThreads / kWave>(v, ws, &tot);
        if (i < a.nblk) a.blk[i] = static_cast<uint32_t>(carry) + ex;  // below 2^31: row ids are int32
        carry += tot;
    }
    if (threadIdx.x == 0) *a.total = carry;
}

__global__ __launch_bounds__(kMaskThreads) void mask_scatter_kernel(MaskArgs a0) {
    const MaskArgs a = mask_of_group(a0);
    __shared__ uint32_t ws[kMaskThreads / kWave];
    const int64_t w0 = static_cast<int64_t>(blockIdx.x) * kMaskWordsPerWG + threadIdx.x * kMaskWordsPerThread;
    uint32_t m[kMaskWordsPerThread];
    uint32_t c = 0;
#pragma unroll
    for (int u = 0; u < kMaskWordsPerThread; u++) {
        m[u] = mask_word(a, w0 + u);
        c += __popc(m[u]);
    }
    uint32_t tot;
    int64_t off = static_cast<int64_t>(a.blk[blockIdx.x]) + wg_exclusive_scan<kMaskThreads / kWave>(c, ws, &tot);
#pragma unroll
    for (int u = 0; u < kMaskWordsPerThread; u++) {
        uint32_t x = m[u];
        while (x) {
            const int bit = __ffs(x) - 1;
            x &= x - 1;
            // (off < cap by construction; the check keeps a mask its owner rewrites during the call inside the list)
            if (off < a.cap) a.pass_ids[off] = static_cast<int32_t>((w0 + u) * 32 + bit);
            off++;
        }
    }
}

// no results: id -1 at distance +inf (what fill_empty writes on the host)
__global__ void filter_fill_kernel(int32_t *ids, float *dist, int64_t cnt) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= cnt) return;
    ids[i] = -1;
    dist[i] = __uint_as_float(0x7f800000u);
}

// position in the passing list -> row id (rerank_decode_kernel's job for candidate lists)
__global__ void filter_decode_kernel(const uint32_t *ord, int64_t cnt, const int32_t *pass_ids, int64_t p, int32_t *out_ids) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= cnt) return;
    const uint32_t o = ord[i];
    out_ids[i] = o < p ? pass_ids[o] : -1;  // 0xffffffff: padding
}

// ---- one mask per query: the union of a query group's masks, and who of the group allows a union row ----------------------
// A dense entry of a (union row, query) pair whose bit is clear.  As a key (make_key) it lies above +inf, so it loses against
// every passing entry of its query, one at distance +inf included; whether a selected entry IS one is decided by the bit.
constexpr uint32_t kSkipDist = 0x7fffffffu;

struct UnionArgs {
    const uint32_t *allow_each;  // [nq][nwords]
    int64_t n, nwords;
    int32_t nq, tq;
    uint32_t *um;                       // [ngroups][nwords]: OR of the group's masks, last word trimmed to n
    const int32_t *upass;               // [ngroups][pstride]: ascending set bits of um[g] (mask_scatter_kernel)
    const unsigned long long *up;       // [ngroups]: their number
    uint32_t *uw;                       // [ngroups][pstride]: bit j = allow bit of query g * tq + j for row upass[g][i]
    int64_t pstride;
    int32_t *q_cnt;                     // [nq]: up[group of q], what select_topk_kernel walks
};

__global__ __launch_bounds__(kMaskThreads) void mask_union_kernel(UnionArgs a) {
    const int64_t w = static_cast<int64_t>(blockIdx.x) * kMaskThreads + threadIdx.x;
    const int g = blockIdx.y;
    if (w >= a.nwords) return;
    const int q0 = g * a.tq;
    const int cnt = a.nq - q0 < a.tq ? a.nq - q0 : a.tq;
    uint32_t m = 0;
    for (int j = 0; j < cnt; j++) m |= a.allow_each[static_cast<int64_t>(q0 + j) * a.nwords + w];
    const int tail = static_cast<int>(a.n & 31);
    if (w == a.nwords - 1 && tail) m &= (1u << tail) - 1u;
    a.um[static_cast<int64_t>(g) * a.nwords + w] = m;
}

// (neighbouring threads read neighbouring union rows: mostly the same word of every mask)
__global__ __launch_bounds__(kMaskThreads) void union_words_kernel(UnionArgs a) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * kMaskThreads + threadIdx.x;
    const int g = blockIdx.y;
    const int64_t p = static_cast<int64_t>(a.up[g]) < a.pstride ? static_cast<int64_t>(a.up[g]) : a.pstride;
    if (i >= p) return;
    const int64_t row = a.upass[static_cast<int64_t>(g) * a.pstride + i];
    const int q0 = g * a.tq;
    const int cnt = a.nq - q0 < a.tq ? a.nq - q0 : a.tq;
    uint32_t word = 0;
    if (row >= 0 && row < a.n)
        for (int j = 0; j < cnt; j++)
            word |= ((a.allow_each[static_cast<int64_t>(q0 + j) * a.nwords + (row >> 5)] >> (row & 31)) & 1u) << j;
    a.uw[static_cast<int64_t>(g) * a.pstride + i] = word;
}

__global__ void union_qcnt_kernel(UnionArgs a) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= a.nq) return;
    const unsigned long long p = a.up[q / a.tq];
    a.q_cnt[q] = static_cast<int32_t>(p < static_cast<unsigned long long>(a.pstride) ? p : a.pstride);
}

// position in the group's union list -> row id and distance, for the cnt = nq * k selected entries of a slice.  An entry
// whose query does not allow the row (uw) is padding, whatever its distance reads.
__global__ void filter_each_decode_kernel(const uint32_t *ord, const float *sel_dist, int64_t cnt, int32_t k, UnionArgs a,
                                          int32_t *out_ids, float *out_dist) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= cnt) return;
    const int q = static_cast<int>(i / k);
    const int g = q / a.tq, j = q % a.tq;
    const uint32_t o = ord[i];
    const int64_t p = static_cast<int64_t>(a.up[g]) < a.pstride ? static_cast<int64_t>(a.up[g]) : a.pstride;
    const int64_t at = static_cast<int64_t>(g) * a.pstride + (o < p ? o : 0);
    const bool ok = o < p && ((a.uw[at] >> j) & 1u);
    out_ids[i] = ok ? a.upass[at] : -1;
    out_dist[i] = ok ? sel_dist[i] : __uint_as_float(0x7f800000u);
}

// ---- the gathered register-row group scan ------------------------------------------------------------------------
// l2_group_kernel (l2_kernels.hpp) over the rows pass_ids names: a workgroup keeps a group of queries resident in LDS, every
// wave holds RB rows in registers and walks the group's queries over them.  Row b of a step is pass_ids[base + b]; lane b
// fetches that id, and with it the row's norm, so the distance is finished in the lane that stores it: RB consecutive
// floats of dense[q][base ..], whose index IS the position in the passing list.
struct FilteredArgs {
    const float *rows;
    const float *row_norms;
    int64_t ld;
    int32_t metric;
    const float *Qp;       // queries padded to stride ld (zero filled)
    const float *q_norms;  // cosine
    int32_t nq;
    int32_t tq;            // queries per group: what the LDS holds at this ld (filtered_group_queries)
    int32_t ngroups;
    const int32_t *pass_ids;
    int64_t p;             // passing rows (>= 1)
    int64_t chunk_rows;    // positions of the passing list per workgroup
    float *out;            // dense[q * p + position]
    // EACH (one mask per query): pass_ids is [ngroups][pstride], group g's union list; p is not used
    const uint32_t *uw;            // [ngroups][pstride]: who of the group allows the row (union_words_kernel)
    const unsigned long long *up;  // [ngroups]: entries of group g's list
    int64_t pstride;               // also the row stride of `out`
};

// 32 queries up to ld 1024, 16 up to 2048, 8 up to 3072: 128 KiB / 128 KiB / 96 KiB of the CU's 160 KiB
__host__ __device__ inline int filtered_group_queries(int64_t ld) { return ld <= 1024 ? 32 : (ld <= 2048 ? 16 : 8); }
__host__ inline size_t filtered_group_lds_bytes(int64_t ld) {
    const size_t tq = static_cast<size_t>(filtered_group_queries(ld));
    return sizeof(float) * tq * static_cast<size_t>(ld) + sizeof(float) * tq;
}

// EACH: the list is the group's own (the union of its queries' masks), lane b loads the row's word beside id and norm, and a
// query is walked over a step's RB rows only if one of them carries its bit (anyw: wave-uniform); the store is the distance
// where the row's bit is set and kSkipDist elsewhere, so every entry of dense[q][0 .. up[g]) is written.
template <int NCH, int RB, bool L2M, bool EACH = false>
__global__ __launch_bounds__(kTileThreads) void filtered_group_kernel(FilteredArgs a) {
    extern __shared__ __align__(16) unsigned char smem[];
    const int nvec = static_cast<int>(a.ld / 4);
    float4 *Bs = reinterpret_cast<float4 *>(smem);            // [tq][nvec] resident query group
    float *qn_s = reinterpret_cast<float *>(Bs + a.tq * nvec);  // [tq] query norms (cosine)
    const int tid = threadIdx.x;
    const int lane = tid & (kWave - 1);
    const int wave = tid >> 6;
    // chunk-major: the workgroups of one chunk of the passing list run side by side and share its rows in L2
    const int g = blockIdx.x % a.ngroups;
    const int64_t chunk = blockIdx.x / a.ngroups;
    const int64_t r0 = chunk * a.chunk_rows;
    int64_t p = a.p, ostride = a.p;
    const int32_t *pass = a.pass_ids;
    const uint32_t *uw = nullptr;
    if constexpr (EACH) {
        const int64_t have = static_cast<int64_t>(a.up[g]);
        p = have < a.pstride ? have : a.pstride;
        ostride = a.pstride;
        pass = a.pass_ids + g * a.pstride;
        uw = a.uw + g * a.pstride;
    }
    const int64_t r1 = r0 + a.chunk_rows < p ? r0 + a.chunk_rows : p;
    const int q0 = g * a.tq;
    const int cnt = a.nq - q0 < a.tq ? a.nq - q0 : a.tq;
    if (r0 >= r1 || cnt <= 0) return;

    if (tid < cnt) qn_s[tid] = (!L2M && a.metric == METRIC_COS) ? a.q_norms[q0 + tid] : 0.0f;
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
            // ... and unconditional stores: an index past the end re-writes element total - 1 with its own value
#pragma unroll
            for (int u = 0; u < kQU; u++) Bs[fc[u]] = v[u];
        }
    }
    __syncthreads();

    for (int64_t base = r0 + wave * RB; base < r1; base += kTileWaves * RB) {
        float4 r[RB][NCH];
        // lane b (and every lane beyond RB, as row RB - 1): the id of row b, clamped into the chunk, and its norm
        const int64_t mypos = base + (lane < RB ? lane : RB - 1);
        const int32_t myid = pass[mypos < r1 ? mypos : r1 - 1];
        const float myrn = (!L2M && a.metric == METRIC_COS) ? a.row_norms[myid] : 0.0f;
        uint32_t myw = 0, anyw = 0;
        if constexpr (EACH) myw = mypos < r1 ? uw[mypos] : 0u;  // (a row past the chunk's end: nobody's)
#pragma unroll
        for (int b = 0; b < RB; b++) {
            const int64_t row = __builtin_amdgcn_readlane(myid, b);
            load_row<NCH>(r[b], a.rows + row * a.ld, nvec, lane, true);
            if constexpr (EACH) anyw |= static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(myw), b));
        }
        for (int q = 0; q < cnt; q++) {
            if constexpr (EACH) {
                if (!((anyw >> q) & 1u)) {  // wave-uniform: none of the RB rows is this query's
                    if (lane < RB && base + lane < r1)
                        a.out[static_cast<int64_t>(q0 + q) * ostride + (base + lane)] = __uint_as_float(kSkipDist);
                    continue;
                }
            }
            const float qn = L2M ? 0.0f : qn_s[q];
            float4 qv[NCH];
#pragma unroll
            for (int c = 0; c < NCH; c++) {
                const int i = c * kWave + lane;
                qv[c] = i < nvec ? Bs[q * nvec + i] : make_float4(0.f, 0.f, 0.f, 0.f);
            }
            float s[RB];
#pragma unroll
            for (int b = 0; b < RB; b++) s[b] = lane_partial<NCH, L2M>(qv, r[b]);
            const float mine = rows_sum_to_lane<RB>(s, lane);  // lane b: row b's sum
            if (lane < RB && base + lane < r1) {
                const float d = L2M ? __builtin_sqrtf(mine) : finish_dist(a.metric, mine, qn, myrn);
                a.out[static_cast<int64_t>(q0 + q) * ostride + (base + lane)] = (!EACH || ((myw >> q) & 1u)) ? d : __uint_as_float(kSkipDist);
            }
        }
    }
}

// ---- IVF-FLAT: the mask in list order, the passing positions per list, the gathered list scan ----------------------------
// lmask bit pos = allow bit of row list_ids[pos], for the L list positions; positions >= L are clear.  Lane i of a wave
// takes position 64 * wave + i: one ballot is two words.  Row ids are install_lists' (in [0, n)); one outside reads as clear.
__global__ __launch_bounds__(kMaskThreads) void list_mask_kernel(const uint32_t *allow, const int32_t *listids, int64_t L, int64_t n,
                                                                 uint32_t *lmask, int64_t lwords) {
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t gw = (static_cast<int64_t>(blockIdx.x) * kMaskThreads + threadIdx.x) >> 6;
    const int64_t pos = gw * kWave + lane;
    const int64_t row = listids[pos < L ? pos : L - 1];  // clamped, unconditional (L >= 1)
    const bool in = pos < L && row >= 0 && row < n;
    const uint32_t w = allow[in ? row >> 5 : 0];
    const unsigned long long m = __ballot(in && ((w >> (row & 31)) & 1u));
    if (lane < 2 && 2 * gw + lane < lwords) lmask[2 * gw + lane] = static_cast<uint32_t>(m >> (32 * lane));
}

// foff[l] = passing positions below list_off[l], l = 0 .. nlist: a lower bound in the ascending pass_pos[0 .. total).
// The total is read on the device (nobody has read it back) and trusted up to `cap`, the entries pass_pos holds.
__global__ void list_foff_kernel(const int32_t *pass_pos, const unsigned long long *total, int64_t cap, const int64_t *list_off,
                                 int nlist, int32_t *foff) {
    const int l = blockIdx.x * blockDim.x + threadIdx.x;
    if (l > nlist) return;
    const unsigned long long t = *total;
    int64_t lo = 0, hi = t < static_cast<unsigned long long>(cap) ? static_cast<int64_t>(t) : cap;
    const int64_t at = list_off[l];
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (pass_pos[mid] < at) lo = mid + 1;
        else hi = mid;
    }
    foff[l] = static_cast<int32_t>(lo);
}

// The gathered step of both filtered list scans: RB list positions (nvalid of them real, the rest clamped copies: the last step
// of a tile or of a wave's queue) -> distances -> the wave's top-k list.  Lane b (and every lane beyond RB, as row RB - 1)
// brings the position of row b in `mypos` and fetches its norm here, readlane makes the row address wave-uniform
// (filtered_group_kernel); lane_partial + rows_sum_to_lane + finish_dist are scan_kernel's, in its order, and a row's distance is
// finished in its own lane from its own sum: the same bits, whichever rows share its step.  Key: (distance, position in the
// UNFILTERED stream) -- monotone in the filtered one, and what merge_topk_kernel and ivf_decode_kernel expect.
template <int NCH, int RB, bool L2M>
__device__ __forceinline__ void ivf_gathered_step(const IvfGatherArgs &a, const float4 (&q)[NCH], float qn, const Pair &p, int32_t mypos,
                                                  int nvalid, int lane, bool regk, uint64_t &mine, uint64_t *mylist, int &cnt, uint64_t &thr) {
    float4 r[RB][NCH];
    const int nvec = static_cast<int>(a.ld / 4);
    const float myrn = (!L2M && a.metric == METRIC_COS) ? a.row_norms[mypos] : 0.0f;
#pragma unroll
    for (int b = 0; b < RB; b++) {
        const int64_t row = __builtin_amdgcn_readlane(mypos, b);
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
            const int64_t pos = __builtin_amdgcn_readlane(mypos, b);
            const uint64_t key = make_key(d, p.ord_base + static_cast<uint32_t>(pos - p.row_begin));
            if (key < thr) {
                if (regk) {
                    wave_insert_reg(mine, cnt, a.k, key, lane);
                    thr = wave_kth_reg(mine, a.k);  // ~0 until the list is full
                } else {
                    wave_insert(mylist, cnt, a.k, key, lane);
                    thr = cnt == a.k ? mylist[a.k - 1] : ~0ull;
                }
            }
        }
    }
}

// ... and their epilogue: the wave's list to partial[pair][chunk][wave][k], from its registers (k <= 64) or from LDS
__device__ __forceinline__ void ivf_store_partial(const IvfGatherArgs &a, int32_t pair, int32_t chunk, int wave, int lane, bool regk,
                                                  uint64_t mine, const uint64_t *mylist, int cnt) {
    uint64_t *dst = a.partial + ((static_cast<int64_t>(pair) * a.nchunks + chunk) * kNWave + wave) * a.k;
    if (regk) {
        if (lane < a.k) dst[lane] = mine;
    } else {
        for (int i = lane; i < a.k; i += kWave) dst[i] = i < cnt ? mylist[i] : ~0ull;
    }
}

// The list scan over the passing rows only.  A workgroup serves one (pair, chunk): the pair's list l comes from the probe
// table (-1: none), its candidates are pass_pos[foff[l] .. foff[l + 1]) -- list positions, ascending, so the filtered
// candidate stream is the unfiltered one with holes.  Nobody on the host knows a filtered list's length: workgroup c of a
// pair takes the tiles c, c + nchunks, ... (chunk_rows positions each) of the segment, whatever its length; one with no
// tile writes its all-ones lists and leaves.  Lane b fetches the position of row b, clamped into the tile, and the step does
// the rest.  (IvfFilteredArgs: tile_args.hpp, beside the other launch arguments the host side fills)
template <int NCH, int RB, bool L2M>
__global__ __launch_bounds__(kWG) void ivf_filtered_scan_kernel(IvfFilteredArgs a) {
    extern __shared__ __align__(16) unsigned char smem[];
    uint64_t *lists = reinterpret_cast<uint64_t *>(smem);  // [kNWave][k] (k > 64)
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = threadIdx.x >> 6;
    int32_t pair, chunk;
    if (!scan_work_item(a.order, a.run, a.npairs, a.nchunks, blockIdx.x, pair, chunk)) return;
    const Pair p = a.pairs[pair];
    const int32_t l = a.probes[pair];
    const int64_t s0 = l >= 0 ? a.foff[l] : 0, s1 = l >= 0 ? a.foff[l + 1] : 0;
    uint64_t *mylist = lists + wave * a.k;
    int cnt = 0;
    uint64_t thr = ~0ull;
    const bool regk = a.k <= kWave;
    uint64_t mine = ~0ull;
    if (s0 + static_cast<int64_t>(chunk) * a.chunk_rows < s1) {
        float4 q[NCH];
        load_query<NCH>(q, a.Q + p.q * a.qld, a.dim, lane);
        const float qn = (!L2M && a.metric == METRIC_COS) ? query_norm<NCH>(q) : 0.0f;
        for (int64_t t0 = s0 + static_cast<int64_t>(chunk) * a.chunk_rows; t0 < s1; t0 += static_cast<int64_t>(a.nchunks) * a.chunk_rows) {
            const int64_t t1 = t0 + a.chunk_rows < s1 ? t0 + a.chunk_rows : s1;
            for (int64_t base = t0 + wave * RB; base < t1; base += kNWave * RB) {
                const int64_t at = base + (lane < RB ? lane : RB - 1);
                const int32_t mypos = a.pass_pos[at < t1 ? at : t1 - 1];
                // (readfirstlane: the count is the same in every lane of the wave, and the step branches on it)
                const int nvalid = __builtin_amdgcn_readfirstlane(static_cast<int>(t1 - base));
                ivf_gathered_step<NCH, RB, L2M>(a, q, qn, p, mypos, nvalid, lane, regk, mine, mylist, cnt, thr);
            }
        }
    }
    ivf_store_partial(a, pair, chunk, wave, lane, regk, mine, mylist, cnt);
}

// ---- IVF-FLAT, one mask per query: the bit tested where the list is read ------------------------------------------------------
// A list-order mask per query would be nq x L bits of scratch and a compaction per query.  Instead a workgroup serves one
// (pair, chunk) of the UNFILTERED list -- positions [row_begin + chunk * chunk_rows, ...), which the host can plan as it plans
// scan_kernel's -- and wave w takes the chunk's blocks w, w + 4, ... of 64 positions.  Of a block, lane i reads
// row = list_ids[pos] and the word of ITS QUERY's mask that holds the row's bit (list_mask_kernel's clamping, a row outside
// [0, n) reads as clear), one ballot gives the block's passing lanes, and a passing lane's prefix popcount is its slot in the
// wave's queue of passing positions in LDS (kWave + RB entries: fewer than RB left over, at most 64 new).  Whenever the queue
// holds RB positions, RB of them go through the single-mask kernel's step (ivf_gathered_step); what is left moves to the front,
// and the remainder after the last block is flushed with the clamped lane.  A row's bits do not depend on which rows share its
// step, the keys and the partial lists are the single-mask kernel's: the top k of a query's keys is the single-mask call's,
// whatever the chunking.
// Per probed position: 4 B of list_ids and a gathered mask word; the f32 row only where the bit is set.
// (IvfEachArgs: tile_args.hpp)

// LDS: [kNWave][kWave + RB] queued positions, then [kNWave][k] keys (k > 64)
__host__ __device__ constexpr size_t ivf_each_queue_bytes(int rb) { return sizeof(int32_t) * kNWave * (kWave + rb); }

// lane b's position of a step over que[0 .. nvalid): entry b, clamped into the step (every lane beyond RB as row RB - 1)
template <int RB>
__device__ __forceinline__ int32_t ivf_each_queued(const int32_t *que, int nvalid, int lane) {
    int at = lane < RB ? lane : RB - 1;
    at = at < nvalid ? at : nvalid - 1;
    return que[at];
}

template <int NCH, int RB, bool L2M>
__global__ __launch_bounds__(kWG) void ivf_each_scan_kernel(IvfEachArgs a) {
    extern __shared__ __align__(16) unsigned char smem[];
    constexpr int kQueue = kWave + RB;
    int32_t *queues = reinterpret_cast<int32_t *>(smem);
    uint64_t *lists = reinterpret_cast<uint64_t *>(smem + ivf_each_queue_bytes(RB));  // (16 * kQueue bytes in: aligned)
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = threadIdx.x >> 6;
    int32_t pair, chunk;
    if (!scan_work_item(a.order, a.run, a.npairs, a.nchunks, blockIdx.x, pair, chunk)) return;
    const Pair p = a.pairs[pair];
    const int64_t r0 = p.row_begin + static_cast<int64_t>(chunk) * a.chunk_rows;
    const int64_t r1 = r0 + a.chunk_rows < p.row_end ? r0 + a.chunk_rows : p.row_end;
    uint64_t *mylist = lists + wave * a.k;
    int32_t *que = queues + wave * kQueue;
    int cnt = 0;
    uint64_t thr = ~0ull;
    const bool regk = a.k <= kWave;
    uint64_t mine = ~0ull;
    if (r0 < r1) {
        if (r0 + static_cast<int64_t>(wave) * kWave < r1) {  // wave-uniform: this wave has a block
            float4 q[NCH];
            load_query<NCH>(q, a.Q + p.q * a.qld, a.dim, lane);
            const float qn = (!L2M && a.metric == METRIC_COS) ? query_norm<NCH>(q) : 0.0f;
            const uint32_t *allow = a.allow_each + static_cast<int64_t>(p.q) * a.nwords;
            int have = 0;  // queued positions (wave-uniform), < RB between two blocks
            // wave w walks the chunk's blocks w, w + kNWave, ... of 64 positions
            for (int64_t base = r0 + static_cast<int64_t>(wave) * kWave; base < r1; base += kNWave * kWave) {
                const int64_t pos = base + lane;
                const int64_t row = a.listids[pos < r1 ? pos : r1 - 1];  // clamped, unconditional
                const bool in = pos < r1 && row >= 0 && row < a.n;
                const uint32_t w = allow[in ? row >> 5 : 0];
                const bool ok = in && ((w >> (row & 31)) & 1u);
                const unsigned long long m = __ballot(ok);
                if (ok) que[have + __popcll(m & ((1ull << lane) - 1ull))] = static_cast<int32_t>(pos);
                have += __popcll(m);
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                __builtin_amdgcn_wave_barrier();
                int head = 0;
                for (; have - head >= RB; head += RB)
                    ivf_gathered_step<NCH, RB, L2M>(a, q, qn, p, ivf_each_queued<RB>(que + head, RB, lane), RB, lane, regk, mine, mylist, cnt, thr);
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
            if (have > 0)
                ivf_gathered_step<NCH, RB, L2M>(a, q, qn, p, ivf_each_queued<RB>(que, have, lane), have, lane, regk, mine, mylist, cnt, thr);
        }
    }
    ivf_store_partial(a, pair, chunk, wave, lane, regk, mine, mylist, cnt);
}

// ---- the first k passing entries of a traversal's result list ----------------------------------------------------------
struct TakeArgs {
    const int32_t *ids_in;  // [nq][kk], -1 padded
    const float *dist_in;
    int32_t nq, kk, k;
    const uint32_t *allow;
    int64_t allow_stride;  // words between the masks of two queries; 0: one mask shared by all
    int64_t n;
    int32_t *out_ids;  // [nq][k]
    float *out_dist;
};

// One wave per query, 64 entries of the list per step: `id >= 0 && bit` -> ballot -> the prefix popcount is the output slot.
__global__ __launch_bounds__(kWG) void filter_take_kernel(TakeArgs a) {
    const int lane = threadIdx.x & (kWave - 1);
    const int q = blockIdx.x * kNWave + (threadIdx.x >> 6);
    if (q >= a.nq) return;  // uniform over the wave
    const int32_t *in = a.ids_in + static_cast<int64_t>(q) * a.kk;
    const float *din = a.dist_in + static_cast<int64_t>(q) * a.kk;
    int32_t *oi = a.out_ids + static_cast<int64_t>(q) * a.k;
    float *od = a.out_dist + static_cast<int64_t>(q) * a.k;
    const uint32_t *allow = a.allow + static_cast<int64_t>(q) * a.allow_stride;
    int taken = 0;
    for (int base = 0; base < a.kk && taken < a.k; base += kWave) {
        const int i = base + lane;
        const int ic = i < a.kk ? i : a.kk - 1;
        const int32_t id = in[ic];
        const float d = din[ic];
        const bool valid = i < a.kk && id >= 0 && id < a.n;
        const uint32_t w = allow[valid ? id >> 5 : 0];
        const bool ok = valid && ((w >> (id & 31)) & 1u);
        const unsigned long long m = __ballot(ok);
        const int slot = taken + __popcll(m & ((1ull << lane) - 1ull));
        if (ok && slot < a.k) {
            oi[slot] = id;
            od[slot] = d;
        }
        taken += __popcll(m);
    }
    if (taken > a.k) taken = a.k;
    for (int i = taken + lane; i < a.k; i += kWave) {
        oi[i] = -1;
        od[i] = __uint_as_float(0x7f800000u);
    }
}

}  // namespace hg
