// dense_kernels.hpp -- the int8 lower bounds of a WHOLE batch against ALL rows, on the matrix cores, in front of a large launch
// of hnsw_wave_kernel (wave_kernels.hpp).
//
// That kernel's time follows the bytes that leave the XCD L2s, and over a third of them are int8 rows: at the headline
// (10,000 queries, 31,173 x 768 rows, ef 640) a query tests 4,190 neighbours, 13 % of the rows, so a launch reads every int8
// row about 1,344 times for an integer dot product each.  The dot product of two int8 codes is exact in any summation order:
// computed here as a tiled GEMM -- query codes (the two planes of Query16) x qrows -- and put through the very
// code_lower_bound the traversal calls, every (query, row) bound is the float the traversal would compute, bit for bit, and
// the traversal reads 4 bytes per fresh neighbour instead of an int8 row.  This moves a computation; it changes no decision.
//   1. hnsw_query_code_kernel: per query the two int8 planes of its 16-bit code in the row layout of qrows, plane after
//      plane (code row 2q = hi, 2q + 1 = lo), and its QueryScal -- by encode_query16, the traversal's and the key pass's own.
//   2. hnsw_dense_bounds_kernel: lb[q * lb_ld + row] for every query and row.
#pragma once
#include "kernels.hpp"

namespace hg {

typedef int dense_v4i __attribute__((ext_vector_type(4)));
typedef int dense_v16i __attribute__((ext_vector_type(16)));

constexpr int kDenseTQ = 128;    // queries per tile (256 code rows: hi and lo plane interleaved)
constexpr int kDenseTR = 128;    // base rows per tile; lb_ld is n rounded up to it
constexpr int kDenseKS = 128;    // bytes of K per staged step (rows are 256 NCH bytes: whole steps)
constexpr int kDensePanel = 8;   // row tiles of a super-panel (1,024 rows: 768 KB of int8 rows at dim 768, L2-resident)

struct QueryCodeArgs {
    const float *Q;
    int64_t qld;
    int32_t dim;
    int32_t nq;
    uint32_t *qcode;   // [2 nq][64 NCH] out
    QueryScal *qscal;  // [nq] out
};

// One wave per query.
template <int NCH>
__global__ __launch_bounds__(kWG) void hnsw_query_code_kernel(QueryCodeArgs a) {
    const int lane = threadIdx.x & (kWave - 1);
    const int qi = blockIdx.x * kNWave + (threadIdx.x >> 6);
    if (qi >= a.nq) return;  // (a whole wave)
    float4 q[NCH];
    load_query<NCH>(q, a.Q + static_cast<int64_t>(qi) * a.qld, a.dim, lane);
    Query16<NCH> qc;
    encode_query16<NCH>(q, qc);
    uint32_t *hi = a.qcode + (static_cast<int64_t>(2 * qi) * kWave + lane) * NCH, *lo = hi + kWave * NCH;
#pragma unroll
    for (int c = 0; c < NCH; c++) {
        hi[c] = qc.hi[c];
        lo[c] = qc.lo[c];
    }
    if (lane == 0) a.qscal[qi] = qc.sc;
}

struct DenseArgs {
    const uint32_t *qcode;   // hnsw_query_code_kernel's
    const QueryScal *qscal;
    const uint32_t *qrows;   // int8 rows + per-row terms of the whole base (quantize_rows_kernel)
    const float4 *qmeta;
    float *lb;               // [nq][lb_ld] out; columns n .. lb_ld - 1 are never written or read
    int64_t lb_ld;
    int64_t n;
    int32_t nq;
    int32_t kbytes;          // 256 NCH
    int32_t metric;
    int32_t nqt, nrt;        // tiles along the queries / the rows
    int32_t rp;              // row tiles per super-panel
    int32_t nsp;             // super-panels
};

// byte offset of 16-byte slot `ks` (0..7) of row `row` in a staged image of 128-byte rows.  ds_read_b128 serves four groups of
// 16 lanes over 64 banks (256 B); a fragment read has lane l on row l & 31 at one slot, and the XOR with (row >> 1) & 7 --
// beside the row's parity, which picks the half of the bank row -- puts the 16 rows of every group on 16 different slots.
__device__ __forceinline__ int dense_lds_off(int row, int ks) { return row * kDenseKS + ((ks ^ ((row >> 1) & 7)) << 4); }

// Tile (qt, rt): 128 queries x 128 rows, K as a run-time loop of 128-byte steps through LDS (the next step's operands are on
// their way from memory while this one is multiplied).  v_mfma_i32_32x32x32_i8 with the code rows as A and the base rows as B:
// lane l supplies bytes 16 (l >> 5) .. + 15 of row l & 31 of both -- any fixed permutation of K is fine as long as both
// operands use it, so qrows is read as it lies -- and receives C[(g & 3) + 8 (g >> 2) + 4 (l >> 5)][l & 31] in register g.
// Code rows 2q and 2q + 1 are the planes of query q: registers g and g + 1 (g even) are its ah and al, tot = 256 ah + al.
// Base rows lie along the 32-lane axis, so a store instruction writes two whole 128-byte lines.  Wave w multiplies code rows
// 128 (w >> 1) .. + 127 by rows 64 (w & 1) .. + 63: eight accumulators.
// Workgroup b runs on XCD b % 8 (observed, and used for speed only, as in hnsw_wave_kernel): the workgroups of one XCD walk the
// super-panels x, x + 8, ... of rp row tiles each, query tile by query tile -- what runs on an XCD at one time shares a few
// row panels and a few query panels out of its L2.
__global__ __launch_bounds__(kWG, 2) void hnsw_dense_bounds_kernel(DenseArgs a) {
    __shared__ __align__(16) unsigned char s_a[2 * kDenseTQ * kDenseKS];
    __shared__ __align__(16) unsigned char s_b[kDenseTR * kDenseKS];
    __shared__ QueryScal s_scal[kDenseTQ];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wv = tid >> 6;
    const int l31 = lane & 31, half = lane >> 5;
    const int xcd = blockIdx.x & 7, j = blockIdx.x >> 3;
    const int per = a.nqt * a.rp;
    const int sp = (j / per) * 8 + xcd, rem = j % per;
    const int qt = rem / a.rp, rt = sp * a.rp + rem % a.rp;
    if (sp >= a.nsp || rt >= a.nrt) return;  // (the whole workgroup)
    const int q0 = qt * kDenseTQ;
    const int64_t r0 = static_cast<int64_t>(rt) * kDenseTR;
    const int64_t K = a.kbytes;

    if (tid < kDenseTQ) s_scal[tid] = a.qscal[q0 + tid < a.nq ? q0 + tid : a.nq - 1];
    // this thread's 16-byte pieces of a step: slot tid & 7 of code rows (tid >> 3) + 32 i and of base rows (tid >> 3) + 32 i
    // (past the batch or the base: the last code row / base row again, its products are not stored)
    const int ks = tid & 7, rr = tid >> 3;
    const unsigned char *const pa = reinterpret_cast<const unsigned char *>(a.qcode) + ks * 16;
    const unsigned char *const pb = reinterpret_cast<const unsigned char *>(a.qrows) + ks * 16;
    const int64_t a_last = 2LL * a.nq - 1, b_last = a.n - 1;
    dense_v4i va[8], vb[4];  // (a native vector type: arrays of the uint4 struct stay in scratch memory)
#define HG_DENSE_FETCH(k0)                                                                       \
    do {                                                                                         \
        _Pragma("unroll") for (int i = 0; i < 8; i++) {                                          \
            const int64_t ar = static_cast<int64_t>(2 * q0) + rr + 32 * i;                       \
            va[i] = *reinterpret_cast<const dense_v4i *>(pa + (ar < a_last ? ar : a_last) * K + (k0)); \
        }                                                                                        \
        _Pragma("unroll") for (int i = 0; i < 4; i++) {                                          \
            const int64_t br = r0 + rr + 32 * i;                                                 \
            vb[i] = *reinterpret_cast<const dense_v4i *>(pb + (br < b_last ? br : b_last) * K + (k0)); \
        }                                                                                        \
    } while (0)
    dense_v16i acc[4][2];
#pragma unroll
    for (int sa = 0; sa < 4; sa++)
#pragma unroll
        for (int sb = 0; sb < 2; sb++)
#pragma unroll
            for (int g = 0; g < 16; g++) acc[sa][sb][g] = 0;
    const int arow = (wv >> 1) * 128 + l31, brow = (wv & 1) * 64 + l31;
    HG_DENSE_FETCH(0);
    for (int k0 = 0; k0 < a.kbytes; k0 += kDenseKS) {
#pragma unroll
        for (int i = 0; i < 8; i++) *reinterpret_cast<dense_v4i *>(s_a + dense_lds_off(rr + 32 * i, ks)) = va[i];
#pragma unroll
        for (int i = 0; i < 4; i++) *reinterpret_cast<dense_v4i *>(s_b + dense_lds_off(rr + 32 * i, ks)) = vb[i];
        __syncthreads();
        if (k0 + kDenseKS < a.kbytes) HG_DENSE_FETCH(k0 + kDenseKS);
#pragma unroll
        for (int u = 0; u < kDenseKS / 32; u++) {
            dense_v4i fa[4], fb[2];
#pragma unroll
            for (int sb = 0; sb < 2; sb++) fb[sb] = *reinterpret_cast<const dense_v4i *>(s_b + dense_lds_off(brow + 32 * sb, 2 * u + half));
#pragma unroll
            for (int sa = 0; sa < 4; sa++) fa[sa] = *reinterpret_cast<const dense_v4i *>(s_a + dense_lds_off(arow + 32 * sa, 2 * u + half));
#pragma unroll
            for (int sa = 0; sa < 4; sa++)
#pragma unroll
                for (int sb = 0; sb < 2; sb++) acc[sa][sb] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa[sa], fb[sb], acc[sa][sb], 0, 0, 0);
        }
        __syncthreads();
    }
#undef HG_DENSE_FETCH
    // ---- epilogue: lane = base row (two of them), 64 queries each
#pragma unroll
    for (int sb = 0; sb < 2; sb++) {
        const int64_t row = r0 + (wv & 1) * 64 + 32 * sb + l31;
        const float4 meta = a.qmeta[row < a.n ? row : a.n - 1];
#pragma unroll
        for (int sa = 0; sa < 4; sa++) {
#pragma unroll
            for (int g = 0; g < 8; g++) {
                const int ql = (wv >> 1) * 64 + 16 * sa + 4 * (g >> 1) + 2 * half + (g & 1);
                // 256 ah + al: the planes' own products may pass 2^31 where the range A is cut to the row length (Query16::kMax),
                // their sum does not -- unsigned arithmetic, as wave_sum8_int's
                const int tot = static_cast<int>(static_cast<unsigned>(acc[sa][sb][2 * g]) * 256u + static_cast<unsigned>(acc[sa][sb][2 * g + 1]));
                const float lb = code_lower_bound(a.metric, tot, s_scal[ql], meta, meta.w);
                if (q0 + ql < a.nq && row < a.n) a.lb[static_cast<int64_t>(q0 + ql) * a.lb_ld + row] = lb;
            }
        }
    }
}

}  // namespace hg
