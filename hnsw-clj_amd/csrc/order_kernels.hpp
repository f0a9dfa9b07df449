// order_kernels.hpp -- the ORDER in which a large launch of hnsw_wave_kernel (wave_kernels.hpp) deals its queries to the chip.
//
// That kernel's time follows the bytes that leave the XCD L2s, and queries that lie near each other read largely the same rows.
// Workgroups are dealt round-robin over the 8 XCDs, so with query qi in workgroup qi neighbouring queries meet in one L2 at one
// time only by chance.  Here every query gets a small integer KEY -- the nearest of P = min(256, n) pivot rows, the base rows
// i * floor(n / P): deterministic, no state to invalidate when the graph changes --, order[] = the query indices sorted by
// (key, index), and the traversal serves slot s with query order[(s % 8) * ceil(nq / 8) + s / 8]: consecutive entries of order[]
// run on one XCD at one time.  The key is a hint and nothing else: a pure function of the query and the index, judged on what the
// handle already has for the rejection test (the pivots' int8 rows against the query's 16-bit code, kernels.hpp: Query16), and
// results never depend on where a workgroup runs.
#pragma once
#include "kernels.hpp"

namespace hg {

constexpr int kOrderPivots = 256;  // bins of the counting sort
constexpr int kOrderQ = 8;         // queries per workgroup of the key pass: wave_sum8_int's eight totals per loaded pivot row
constexpr int kOrderSortWG = 1024;

struct OrderArgs {
    const float *Q;
    int64_t qld;
    int32_t dim;
    int32_t metric;
    int32_t nq;
    int64_t n;
    const uint32_t *qrows;  // int8 rows + per-row terms of the whole base (quantize_rows_kernel)
    const float4 *qmeta;
    int32_t *keys;          // [nq] out: index of the nearest pivot
    int32_t *order;         // [nq] out: query indices by (key, index)
};

// One workgroup of kOrderWaves waves per kOrderQ queries.  Wave w codes two of the queries (encode_query16) and leaves the code
// planes in LDS for the others; then every wave holds all eight codes in registers and takes a quarter of the pivots, RIF rows
// per trip with the next trip's rows already on their way (a wave has nothing else to hide the L2's latency behind: the first
// form, one wave over all 256 pivots with one trip in flight, took 142 us at the headline's 10,000 x 768 -- more than the 1 % of
// the traversal the order may cost).  The pivot table (196 KB at dim 768) is read once per eight queries and stays in L2.  The
// score is a monotone proxy of the metric from the exact code dot product (code_bounds' centre without its allowances): cosine
// -q'.v' / |v|, dot -q'.v', L2 |q'|^2 - 2 q'.v' + |v'|^2.  Smallest score wins, the first pivot among equals; a NaN score never
// wins (key 0 for a query without a code).
constexpr int kOrderWaves = 4;

template <int NCH>
__global__ __launch_bounds__(kOrderWaves *kWave) void hnsw_order_key_kernel(OrderArgs a) {
    constexpr int RIF = NCH <= 3 ? 4 : (NCH <= 6 ? 2 : 1);
    constexpr int QPW = kOrderQ / kOrderWaves;  // queries a wave codes
    __shared__ uint32_t s_code[kOrderQ][2 * NCH][kWave];
    __shared__ float s_scal[kOrderQ][2];
    __shared__ float s_best[kOrderWaves][kOrderQ];
    __shared__ int32_t s_piv[kOrderWaves][kOrderQ];
    const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
    const int q0 = blockIdx.x * kOrderQ;
    const int own = wave_sum8_row(lane);  // the query of this workgroup whose totals this lane receives
#pragma unroll
    for (int j = 0; j < QPW; j++) {
        const int b = wv * QPW + j;
        const int qi = q0 + b < a.nq ? q0 + b : a.nq - 1;  // past the batch: a valid query, its key is not written
        float4 q[NCH];
        load_query<NCH>(q, a.Q + static_cast<int64_t>(qi) * a.qld, a.dim, lane);
        Query16<NCH> qc;
        encode_query16<NCH>(q, qc);
#pragma unroll
        for (int c = 0; c < NCH; c++) {
            s_code[b][c][lane] = qc.hi[c];
            s_code[b][NCH + c][lane] = qc.lo[c];
        }
        if (lane == 0) {
            s_scal[b][0] = qc.sc.s;
            s_scal[b][1] = qc.sc.a2;
        }
    }
    __syncthreads();
    Query16<NCH> qc[kOrderQ];  // (the code planes only)
#pragma unroll
    for (int b = 0; b < kOrderQ; b++) {
#pragma unroll
        for (int c = 0; c < NCH; c++) {
            qc[b].hi[c] = s_code[b][c][lane];
            qc[b].lo[c] = s_code[b][NCH + c][lane];
        }
    }
    const float my_s = s_scal[own][0], my_a2 = s_scal[own][1];
    const int P = a.n < kOrderPivots ? static_cast<int>(a.n) : kOrderPivots;
    const int64_t stride = a.n / P;
    const int per = (P + kOrderWaves - 1) / kOrderWaves, pb = wv * per, pe = pb + per < P ? pb + per : P;  // this wave's pivots
    float best = __uint_as_float(0x7f800000u);
    int best_p = 0;
    uint32_t wa[RIF][NCH], wb[RIF][NCH];
    float4 ma[RIF], mb[RIF];
    // rows p0 .. p0 + RIF - 1 of this wave's range (past its end: its last row again, not scored)
    const auto fetch = [&](int p0, uint32_t (&w)[RIF][NCH], float4 (&mt)[RIF]) {
#pragma unroll
        for (int r = 0; r < RIF; r++) {
            const int64_t row = (p0 + r < pe ? p0 + r : pe - 1) * stride;  // < n
            const uint32_t *rp = a.qrows + (row * kWave + lane) * NCH;
#pragma unroll
            for (int c = 0; c < NCH; c++) w[r][c] = rp[c];
            mt[r] = a.qmeta[row];
        }
    };
    const auto score = [&](int p0, const uint32_t (&w)[RIF][NCH], const float4 (&mt)[RIF]) {
#pragma unroll
        for (int r = 0; r < RIF; r++) {
            int acc[kOrderQ];
#pragma unroll
            for (int b = 0; b < kOrderQ; b++) acc[b] = code_dot16<NCH>(qc[b], w[r]);
            const int tot = wave_sum8_int(acc, lane);
            const float dh = static_cast<float>(tot) * (my_s * mt[r].x);  // q' . v'
            float sc;
            if (a.metric == METRIC_L2) sc = my_a2 - 2.0f * dh + mt[r].x * mt[r].x * mt[r].z;
            else if (a.metric == METRIC_DOT) sc = -dh;
            else sc = -dh * mt[r].w;
            if (p0 + r < pe && sc < best) {
                best = sc;
                best_p = p0 + r;
            }
        }
    };
    if (pb < pe) {
        fetch(pb, wa, ma);
        for (int p0 = pb; p0 < pe; p0 += 2 * RIF) {
            fetch(p0 + RIF, wb, mb);
            score(p0, wa, ma);
            fetch(p0 + 2 * RIF, wa, ma);
            score(p0 + RIF, wb, mb);
        }
    }
    if ((lane & 7) == 0) {
        s_best[wv][own] = best;
        s_piv[wv][own] = best_p;
    }
    __syncthreads();
    if (threadIdx.x < kOrderQ && q0 + threadIdx.x < a.nq) {  // the waves in pivot order: the first pivot among equals
        float bs = s_best[0][threadIdx.x];
        int bp = s_piv[0][threadIdx.x];
#pragma unroll
        for (int w2 = 1; w2 < kOrderWaves; w2++) {
            if (s_best[w2][threadIdx.x] < bs) {
                bs = s_best[w2][threadIdx.x];
                bp = s_piv[w2][threadIdx.x];
            }
        }
        a.keys[q0 + threadIdx.x] = bp;
    }
}

// order[] = the query indices sorted by (key, index): a stable counting sort over kOrderPivots bins in ONE workgroup of WG threads.  Tiles
// of WG queries in index order; inside a tile a query's place = the bin's next free position + the queries of the same
// bin in earlier waves of the tile + those in lower lanes of its own wave.
template <int WG>
__global__ __launch_bounds__(WG) void hnsw_order_sort_kernel(const int32_t *keys, int32_t nq, int32_t *order) {
    constexpr int NWV = WG / kWave;
    __shared__ int32_t start[kOrderPivots];
    __shared__ int32_t scan[kOrderPivots];
    __shared__ int32_t wcnt[NWV][kOrderPivots];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wv = tid / kWave;
    if (tid < kOrderPivots) start[tid] = 0;
    for (int i = tid; i < NWV * kOrderPivots; i += WG) (&wcnt[0][0])[i] = 0;
    __syncthreads();
    for (int i = tid; i < nq; i += WG) atomicAdd(&start[keys[i] & (kOrderPivots - 1)], 1);
    __syncthreads();
    if (tid < kOrderPivots) scan[tid] = start[tid];
    __syncthreads();
    for (int off = 1; off < kOrderPivots; off <<= 1) {  // inclusive prefix sums of the bin counts
        const int32_t v = (tid < kOrderPivots && tid >= off) ? scan[tid - off] : 0;
        __syncthreads();
        if (tid < kOrderPivots) scan[tid] += v;
        __syncthreads();
    }
    if (tid < kOrderPivots) start[tid] = scan[tid] - start[tid];  // the bin's first position
    __syncthreads();
    for (int base = 0; base < nq; base += WG) {
        const int i = base + tid;
        const bool valid = i < nq;
        const int key = valid ? (keys[i] & (kOrderPivots - 1)) : 0;
        uint64_t same = __builtin_amdgcn_ballot_w64(valid);  // the valid lanes of this wave with this lane's key
#pragma unroll
        for (int bit = 0; bit < 8; bit++) {
            const bool one = (key >> bit) & 1;
            const uint64_t bm = __builtin_amdgcn_ballot_w64(one);
            same &= one ? bm : ~bm;
        }
        const int rank = __popcll(same & ((1ull << lane) - 1ull));
        if (valid && rank == 0) wcnt[wv][key] = __popcll(same);
        __syncthreads();
        if (valid) {
            int32_t pos = start[key] + rank;
            for (int w2 = 0; w2 < wv; w2++) pos += wcnt[w2][key];
            order[pos] = i;  // < nq: the bins were counted over the same keys
        }
        __syncthreads();
        if (tid < kOrderPivots) {
            int32_t s = 0;
            for (int w2 = 0; w2 < NWV; w2++) {
                s += wcnt[w2][tid];
                wcnt[w2][tid] = 0;
            }
            start[tid] += s;
        }
        __syncthreads();
    }
}

}  // namespace hg
