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
constexpr int kDenseTR = 256;    // base rows per tile (a tile past n masks its stores)
constexpr int kDenseLd = 128;    // lb_ld is n rounded up to it: whole 128-byte lines per row of the table, whatever the tile
constexpr int kDenseKS = 128;    // bytes of K per staged step (rows are 256 NCH bytes: whole steps)
constexpr int kDensePanel = 4;   // row tiles of a super-panel (1,024 rows: 768 KB of int8 rows at dim 768, L2-resident)
constexpr int kDenseWG = 512;    // eight waves, two per SIMD, one workgroup per CU
constexpr int kDenseImage = (2 * kDenseTQ + kDenseTR) * kDenseKS;  // one staged K step: the code rows, then the base rows
constexpr int kDenseLds = 2 * kDenseImage + 2 * (kDenseTQ * 32 + kDenseTR * 16);  // two images, the QueryScal and row meta of two tiles: 144 KB

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
    int32_t nqt, nrt;        // tiles along the queries / the rows
    int32_t rp;              // row tiles per super-panel
    int32_t nsp;             // super-panels
    int32_t nvt;             // places of the tile walk: 8 ceil(nsp / 8) nqt rp; those past the last super-panel or row tile are empty
};

// the tiling of nq queries x n rows (the launch's; the tests' shapes follow it)
inline void dense_tiling(DenseArgs &d) {
    d.nqt = (d.nq + kDenseTQ - 1) / kDenseTQ;
    d.nrt = static_cast<int32_t>((d.n + kDenseTR - 1) / kDenseTR);
    d.rp = d.nrt / 8 < 1 ? 1 : d.nrt / 8 < kDensePanel ? d.nrt / 8 : kDensePanel;  // (few rows: narrower panels, so that every XCD has one)
    d.nsp = (d.nrt + d.rp - 1) / d.rp;
}
inline int64_t dense_walk_places(const DenseArgs &d) { return 8LL * ((d.nsp + 7) / 8) * d.nqt * d.rp; }

// byte offset of 16-byte slot `ks` (0..7) of row `row` in a staged image of 128-byte rows.  ds_read_b128 serves four groups of
// 16 lanes over 64 banks (256 B); a fragment read has lane l on row l & 31 at one slot, and the XOR with (row >> 1) & 7 --
// beside the row's parity, which picks the half of the bank row -- puts the 16 rows of every group on 16 different slots.
__device__ __forceinline__ int dense_lds_off(int row, int ks) { return row * kDenseKS + ((ks ^ ((row >> 1) & 7)) << 4); }

// Place v of the walk: the workgroups of XCD x = v % 8 walk the super-panels x, x + 8, ... of rp row tiles each, query tile by
// query tile -- what runs on an XCD at one time shares a few row panels and a few query panels out of its L2.
__device__ __forceinline__ bool dense_tile_at(const DenseArgs &a, int v, int &qt, int &rt) {
    const int xcd = v & 7, j = v >> 3, per = a.nqt * a.rp;
    const int sp = (j / per) * 8 + xcd, rem = j % per;
    qt = rem / a.rp;
    rt = sp * a.rp + rem % a.rp;
    return sp < a.nsp && rt < a.nrt;
}

// The bounds of a wave's 64 queries x 64 rows from its eight accumulators.  Lane = base row (two of them, 32 apart), registers =
// queries: a query's QueryScal is read once for both rows, the rows' meta is held across all queries, and a store instruction
// writes two whole 128-byte lines.  FULL: the tile lies inside the batch and the base, nothing is tested.
template <int METRIC, bool FULL>
__device__ __forceinline__ void dense_store_bounds(const dense_v16i (&acc)[4][2], const QueryScal *sc, const float4 (&meta)[2],
                                                   float *out, int64_t lb_ld, int nql, const bool (&row_ok)[2]) {
#pragma unroll
    for (int sa = 0; sa < 4; sa++) {
#pragma unroll
        for (int g = 0; g < 8; g++) {
            const int c = 16 * sa + 4 * (g >> 1) + (g & 1);  // + 2 (lane >> 5): sc, out and nql start at the lane's first query
            const QueryScal q = sc[c];
#pragma unroll
            for (int sb = 0; sb < 2; sb++) {
                // 256 ah + al: the planes' own products may pass 2^31 where the range A is cut to the row length (Query16::kMax),
                // their sum does not -- unsigned arithmetic, as wave_sum8_int's
                const int tot = static_cast<int>(static_cast<unsigned>(acc[sa][sb][2 * g]) * 256u + static_cast<unsigned>(acc[sa][sb][2 * g + 1]));
                const float lb = code_lower_bound(METRIC, tot, q, meta[sb], meta[sb].w);
                if (FULL || (c < nql && row_ok[sb])) out[c * lb_ld + 32 * sb] = lb;
            }
        }
    }
}

// A persistent workgroup of eight waves walks the places blockIdx.x, + gridDim.x, ... (gridDim.x is a multiple of 8: it stays on
// its XCD -- observed, and used for speed only, as in hnsw_wave_kernel).  Tile (qt, rt): 128 queries x 256 rows, K in 128-byte
// steps through two LDS images with one barrier per step, as one pipeline over all its tiles: a step multiplies out of one
// image, then writes the next step -- the next tile's first after this tile's last -- into the other and sends for the one
// after it.  A tile's bounds are computed and stored between its last step and the next tile's first, whose operands are in
// LDS by then: the stores drain behind that step's matrix work, and nothing waits for memory in between.  The QueryScal and
// row meta of a tile go through LDS too, fetched and written with the tile's first step.
// v_mfma_i32_32x32x32_i8 with the code rows as A and the base rows as B: lane l supplies bytes 16 (l >> 5) .. + 15 of row
// l & 31 of both -- any fixed permutation of K is fine as long as both operands use it, so qrows is read as it lies -- and
// receives C[(g & 3) + 8 (g >> 2) + 4 (l >> 5)][l & 31] in register g.  Code rows 2q and 2q + 1 are the planes of query q:
// registers g and g + 1 (g even) are its ah and al, tot = 256 ah + al.  Wave w multiplies code rows 128 (w >> 2) .. + 127 by
// rows 64 (w & 3) .. + 63: eight accumulators, six ds_read_b128 per eight MFMAs.
template <int METRIC>
__global__ __launch_bounds__(kDenseWG, 2) void hnsw_dense_bounds_kernel(DenseArgs a) {
    static_assert(sizeof(QueryScal) == 32 && sizeof(float4) == 16, "kDenseLds");
    extern __shared__ __align__(16) unsigned char smem[];  // image 0, image 1, QueryScal[2][kDenseTQ], meta[2][kDenseTR]
    QueryScal *const s_scal = reinterpret_cast<QueryScal *>(smem + 2 * kDenseImage);
    float4 *const s_meta = reinterpret_cast<float4 *>(smem + 2 * kDenseImage + 2 * kDenseTQ * 32);
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, half = lane >> 5;
    const int64_t K = a.kbytes;
    const int nk = a.kbytes / kDenseKS;  // (even)
    const int step = gridDim.x;
    int v = blockIdx.x, qt = 0, rt = 0;
    while (v < a.nvt && !dense_tile_at(a, v, qt, rt)) v += step;
    if (v >= a.nvt) return;  // (the whole workgroup)

    // this thread's 16-byte pieces of a step: slot tid & 7 of code rows (tid >> 3) + 64 i and of base rows (tid >> 3) + 64 i
    // (past the batch or the base: the last code row / base row again, its products are not stored), and its piece of the
    // tile's terms: half a QueryScal, and the meta of a row in threads 0 .. 255
    const int ks = tid & 7, rr = tid >> 3;
    const int64_t a_last = 2LL * a.nq - 1, b_last = a.n - 1;
    const unsigned char *pa[4], *pb[4];
    dense_v4i va[4], vb[4], vs;  // (a native vector type: arrays of the uint4 struct stay in scratch memory)
    float4 vm;
    int q0, par = 0;
    int64_t r0;
    // the addresses of tile (qt, rt), and its terms on their way
#define HG_DENSE_TILE()                                                                                               \
    do {                                                                                                              \
        q0 = qt * kDenseTQ;                                                                                           \
        r0 = static_cast<int64_t>(rt) * kDenseTR;                                                                     \
        _Pragma("unroll") for (int i = 0; i < 4; i++) {                                                               \
            const int64_t ar = 2LL * q0 + rr + 64 * i, br = r0 + rr + 64 * i;                                         \
            pa[i] = reinterpret_cast<const unsigned char *>(a.qcode) + (ar < a_last ? ar : a_last) * K + ks * 16;     \
            pb[i] = reinterpret_cast<const unsigned char *>(a.qrows) + (br < b_last ? br : b_last) * K + ks * 16;     \
        }                                                                                                             \
        const int tq = q0 + ((tid >> 1) & (kDenseTQ - 1));                                                            \
        const int64_t tr = r0 + (tid & (kDenseTR - 1));                                                               \
        vs = reinterpret_cast<const dense_v4i *>(a.qscal + (tq < a.nq ? tq : a.nq - 1))[tid & 1];                     \
        vm = a.qmeta[tr < a.n ? tr : a.n - 1];                                                                        \
    } while (0)
    // ... into half p of s_scal and s_meta (last read in the epilogue of the tile before this one's predecessor)
#define HG_DENSE_TERMS(p)                                                                                             \
    do {                                                                                                              \
        if (tid < 2 * kDenseTQ) reinterpret_cast<dense_v4i *>(s_scal + (p) * kDenseTQ)[tid] = vs;                     \
        if (tid < kDenseTR) s_meta[(p) * kDenseTR + tid] = vm;                                                        \
    } while (0)
#define HG_DENSE_FETCH(k0)                                                                               \
    do {                                                                                                 \
        _Pragma("unroll") for (int i = 0; i < 4; i++) va[i] = *reinterpret_cast<const dense_v4i *>(pa[i] + (k0)); \
        _Pragma("unroll") for (int i = 0; i < 4; i++) vb[i] = *reinterpret_cast<const dense_v4i *>(pb[i] + (k0)); \
    } while (0)
#define HG_DENSE_WRITE(im)                                                                                            \
    do {                                                                                                              \
        _Pragma("unroll") for (int i = 0; i < 4; i++)                                                                 \
            *reinterpret_cast<dense_v4i *>(smem + (im) * kDenseImage + dense_lds_off(rr + 64 * i, ks)) = va[i];       \
        _Pragma("unroll") for (int i = 0; i < 4; i++)                                                                 \
            *reinterpret_cast<dense_v4i *>(smem + (im) * kDenseImage + 2 * kDenseTQ * kDenseKS + dense_lds_off(rr + 64 * i, ks)) = vb[i]; \
    } while (0)
    // one K step of this wave through the matrix cores, out of image im
#define HG_DENSE_MUL(im)                                                                                              \
    do {                                                                                                              \
        const unsigned char *const s_a = smem + (im) * kDenseImage, *const s_b = s_a + 2 * kDenseTQ * kDenseKS;       \
        _Pragma("unroll") for (int u = 0; u < kDenseKS / 32; u++) {                                                   \
            dense_v4i fa[4], fb[2];                                                                                   \
            _Pragma("unroll") for (int sb = 0; sb < 2; sb++)                                                          \
                fb[sb] = *reinterpret_cast<const dense_v4i *>(s_b + dense_lds_off(brow + 32 * sb, 2 * u + half));     \
            _Pragma("unroll") for (int sa = 0; sa < 4; sa++)                                                          \
                fa[sa] = *reinterpret_cast<const dense_v4i *>(s_a + dense_lds_off(arow + 32 * sa, 2 * u + half));     \
            _Pragma("unroll") for (int sa = 0; sa < 4; sa++)                                                          \
                _Pragma("unroll") for (int sb = 0; sb < 2; sb++)                                                      \
                    acc[sa][sb] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa[sa], fb[sb], acc[sa][sb], 0, 0, 0);        \
        }                                                                                                             \
    } while (0)

    const int arow = (wv >> 2) * 128 + l31, brow = (wv & 3) * 64 + l31;
    HG_DENSE_TILE();
    HG_DENSE_FETCH(0);
    HG_DENSE_TERMS(0);
    HG_DENSE_WRITE(0);
    HG_DENSE_FETCH(kDenseKS);
    __syncthreads();
    for (;;) {
        // here image 0 holds step 0 of this tile, the registers hold step 1, and half par of the terms is this tile's
        dense_v16i acc[4][2];
#pragma unroll
        for (int sa = 0; sa < 4; sa++)
#pragma unroll
            for (int sb = 0; sb < 2; sb++)
#pragma unroll
                for (int g = 0; g < 16; g++) acc[sa][sb][g] = 0;
        const int eq0 = q0, epar = par;  // (this tile's, for its epilogue: the walk moves on two steps before it)
        const int64_t er0 = r0;
        bool more = false;
        for (int s = 0; s < nk; s += 2) {
            const bool last = s + 2 >= nk;
            HG_DENSE_MUL(0);
            HG_DENSE_WRITE(1);
            if (!last) {
                HG_DENSE_FETCH((s + 2) * kDenseKS);
            } else {
                v += step;
                while (v < a.nvt && !dense_tile_at(a, v, qt, rt)) v += step;
                more = v < a.nvt;
                if (more) {
                    par ^= 1;
                    HG_DENSE_TILE();
                    HG_DENSE_FETCH(0);
                }
            }
            __syncthreads();
            HG_DENSE_MUL(1);
            if (!last || more) {
                if (last) HG_DENSE_TERMS(par);
                HG_DENSE_WRITE(0);
                HG_DENSE_FETCH(last ? kDenseKS : (s + 3) * kDenseKS);
            }
            __syncthreads();
        }
        // ---- this tile's bounds
        const int cq = eq0 + (wv >> 2) * 64 + 2 * half;  // the lane's first query
        const int64_t crow = er0 + (wv & 3) * 64 + l31;  // and its first row
        const bool full = eq0 + kDenseTQ <= a.nq && er0 + kDenseTR <= a.n;
        const QueryScal *const sc = s_scal + epar * kDenseTQ + (wv >> 2) * 64 + 2 * half;
        const float4 *const sm = s_meta + epar * kDenseTR + (wv & 3) * 64 + l31;
        const float4 meta[2] = {sm[0], sm[32]};
        const bool row_ok[2] = {crow < a.n, crow + 32 < a.n};
        float *const out = a.lb + static_cast<int64_t>(cq) * a.lb_ld + crow;
        if (full) dense_store_bounds<METRIC, true>(acc, sc, meta, out, a.lb_ld, 0, row_ok);
        else dense_store_bounds<METRIC, false>(acc, sc, meta, out, a.lb_ld, a.nq - cq, row_ok);
        if (!more) break;
    }
#undef HG_DENSE_MUL
#undef HG_DENSE_WRITE
#undef HG_DENSE_FETCH
#undef HG_DENSE_TERMS
#undef HG_DENSE_TILE
}

}  // namespace hg
