// pcaf_kernels.hpp -- P-HNSW on one handle (src/hnsw/ann/dimreduct/pcaf.clj; C ABI: include/hnswgpu.h, "P-HNSW"; host: pcaf.hip).
//
// Three kernels, one launch each, and nothing of the shape [queries][rows] between them:
//   1. pcaf_project_kernel: X[m][dim] . P^T -> [m][Tp] on the f32 matrix cores (v_mfma_f32_32x32x2_f32) plus every projected
//      row's norm in the same pass.  Serves the build (X = the base rows), hnswgpu_pcaf_project, the query side of a search and
//      the rows hnswgpu_pcaf_add appends; its MAP form stores every row where a map names (hnswgpu_pcaf_update).
//   2. pcaf_filter_kernel: a workgroup owns <= 32 projected queries (the B operand, resident in LDS) and streams a contiguous
//      slab of projected rows past them, 32 rows per wave and step; the 32 x 32 accumulators become cosine distances, each is
//      tested against its query's running threshold and the survivors are collected per query in LDS; kf keys per query and
//      slab leave the kernel.
//   3. pcaf_refine_kernel: a workgroup per query merges its slabs' keys to kf candidates, gathers their f32 base rows, one
//      wave per row, with the pair arithmetic of gather_dist_kernel (the bits of hnswgpu_rerank), and writes the top k.
// Layout: a projected row is Tp = T rounded up to 8 floats, zero padded, rows back to back -- 32 rows of a step are ONE
// contiguous run of 32 * Tp * 4 bytes, fetched with 16-byte loads.  In LDS a row takes Tp + 4 floats: Tp / 4 is even, so the
// 16-byte reads of eight neighbouring rows fall on distinct banks.
// K order of a tile: the lanes of half h = lane >> 5 feed k = 8t + 4h + {0, 1, 2, 3} to four successive MFMAs of step t (the
// slot a k goes to is free as long as A and B agree, and one 16-byte LDS read then serves four instructions).
#pragma once
#include "kernels.hpp"
#include "tile_args.hpp"

namespace hg {

constexpr int kPcafMaxT = 256;    // n_components
constexpr int kPcafMaxKf = 128;   // candidates of phase 1
constexpr int kPcafProjRows = 128;  // X rows of a projection workgroup (32 per wave)
constexpr int kPcafProjK = 32;      // floats of dim per LDS chunk
constexpr int kPcafProjLd = kPcafProjK + 4;

__device__ __forceinline__ void pcaf_wave_sync() {  // LDS written by some lanes of a wave, read by others
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ f32x16 pcaf_mfma4(const float4 &x, const float4 &y, f32x16 acc) {
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(x.x, y.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(x.y, y.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(x.z, y.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(x.w, y.w, acc, 0, 0, 0);
    return acc;
}

// The `keep` smallest of the m <= 64 * PER distinct keys b[0 .. m) (LDS, one wave), ascending, into b[0 .. min(m, keep)):
// every lane ranks its keys against all m (broadcast reads), then each key goes to the slot its rank names.  All-ones entries
// may repeat; they rank behind every real key and land on one slot.
template <int PER>
__device__ __forceinline__ void pcaf_wave_cut(uint64_t *b, int m, int keep, int lane) {
    uint64_t mine[PER];
    int rank[PER];
#pragma unroll
    for (int p = 0; p < PER; p++) {
        const int i = p * kWave + lane;
        mine[p] = i < m ? b[i] : ~0ull;
        rank[p] = 0;
    }
    for (int j = 0; j < m; j++) {
        const uint64_t o = b[j];
#pragma unroll
        for (int p = 0; p < PER; p++) rank[p] += o < mine[p] ? 1 : 0;
    }
    pcaf_wave_sync();
#pragma unroll
    for (int p = 0; p < PER; p++)
        if (p * kWave + lane < m && rank[p] < keep) b[rank[p]] = mine[p];
    pcaf_wave_sync();
}

// ---- 1. projection ------------------------------------------------------------------------------------------------------
struct PcafProjectArgs {
    const float *X;   // [m][dim], row stride xld
    int64_t xld, m;
    int32_t dim;
    int32_t vec;      // X rows start on 16-byte boundaries (xld % 4 == 0 and the pointer is aligned)
    const float *P;   // [T][pld], zero padded to pld (a multiple of 4)
    int64_t pld;
    int32_t T, Tp;
    float *out;       // [m][Tp]
    float *norms;     // [m]
    // MAP only (hnswgpu_pcaf_update): row r of X is row dst[r] of out / norms, which hold n_dst rows; distinct per call
    const int32_t *dst;
    int64_t n_dst;
};

// 128 X rows per workgroup, 32 per wave, against all NT * 32 >= Tp components.  Per chunk of 32 floats of dim the workgroup
// stages the chunk of P (shared by its waves) and of its X rows in LDS, then every wave multiplies its 32 rows with the NT
// column tiles.  Epilogue: lane (li, half) holds component nt * 32 + li of rows 8 (reg >> 2) + 4 half + (reg & 3): the row
// goes out in 128-byte runs, and its sum of squares is an fmaf chain over the lane's tiles and a butterfly over the 32 lanes.
// MAP: the same body with a destination map in the epilogue -- row r's components and norm are stored at row dst[r] (checked
// against n_dst before the store).  A row's bits depend on its values and on P alone, never on r, on its slot in the 128-row block
// or on where it is stored: each accumulator entry is one row's sum over k, and the norm's butterfly runs over one row's 32 lanes.
template <int NT, bool MAP = false>
__global__ __launch_bounds__(kWG) void pcaf_project_kernel(PcafProjectArgs a) {
    __shared__ __align__(16) float Ps[NT * 32 * kPcafProjLd];
    __shared__ __align__(16) float Xs[kPcafProjRows * kPcafProjLd];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6, half = lane >> 5, li = lane & 31;
    const int64_t row0 = static_cast<int64_t>(blockIdx.x) * kPcafProjRows;
    f32x16 acc[NT];
#pragma unroll
    for (int nt = 0; nt < NT; nt++)
#pragma unroll
        for (int i = 0; i < 16; i++) acc[nt][i] = 0.0f;
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int k0 = 0; k0 < a.dim; k0 += kPcafProjK) {
        __syncthreads();  // the chunk before has been multiplied
#pragma unroll
        for (int u = 0; u < NT; u++) {
            const int f = tid + kWG * u, t = f >> 3, k = k0 + 4 * (f & 7);
            float4 v = zero;
            if (t < a.T && k < a.pld) v = *reinterpret_cast<const float4 *>(a.P + t * a.pld + k);
            *reinterpret_cast<float4 *>(Ps + t * kPcafProjLd + 4 * (f & 7)) = v;
        }
#pragma unroll
        for (int u = 0; u < kPcafProjRows * 8 / kWG; u++) {
            const int f = tid + kWG * u, r = f >> 3, k = k0 + 4 * (f & 7);
            float4 v = zero;
            if (row0 + r < a.m) {
                const float *x = a.X + (row0 + r) * a.xld;
                if (a.vec && k + 4 <= a.dim) {
                    v = *reinterpret_cast<const float4 *>(x + k);
                } else {
                    v.x = k + 0 < a.dim ? x[k + 0] : 0.0f;
                    v.y = k + 1 < a.dim ? x[k + 1] : 0.0f;
                    v.z = k + 2 < a.dim ? x[k + 2] : 0.0f;
                    v.w = k + 3 < a.dim ? x[k + 3] : 0.0f;
                }
            }
            *reinterpret_cast<float4 *>(Xs + r * kPcafProjLd + 4 * (f & 7)) = v;
        }
        __syncthreads();
#pragma unroll
        for (int t = 0; t < kPcafProjK / 8; t++) {
            const float4 av = *reinterpret_cast<const float4 *>(Xs + (wave * 32 + li) * kPcafProjLd + 8 * t + 4 * half);
#pragma unroll
            for (int nt = 0; nt < NT; nt++) {
                const float4 bv = *reinterpret_cast<const float4 *>(Ps + (nt * 32 + li) * kPcafProjLd + 8 * t + 4 * half);
                acc[nt] = pcaf_mfma4(av, bv, acc[nt]);
            }
        }
    }
#pragma unroll
    for (int reg = 0; reg < 16; reg++) {
        const int64_t row = row0 + wave * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * half;
        bool live = row < a.m;
        int64_t to = row;
        if (MAP) {
            to = live ? a.dst[row] : -1;
            live = to >= 0 && to < a.n_dst;
        }
        float s = 0.0f;
#pragma unroll
        for (int nt = 0; nt < NT; nt++) {
            const float v = acc[nt][reg];  // components >= T are exact zeros (P's rows there are)
            s = __builtin_fmaf(v, v, s);
            if (live && nt * 32 + li < a.Tp) a.out[to * a.Tp + nt * 32 + li] = v;
        }
#pragma unroll
        for (int off = 1; off < 32; off <<= 1) s = s + __shfl_xor(s, off, kWave);
        if (live && li == 0) a.norms[to] = __builtin_sqrtf(s);
    }
}

// ---- 2. filter ----------------------------------------------------------------------------------------------------------
struct PcafFilterArgs {
    const float *rows;       // projected rows [n][Tp]
    const float *row_norms;  // [n]
    int64_t n;
    const float *Q;          // projected queries [nq][Tp]
    const float *q_norms;
    int32_t nq, Tp, kf;
    int64_t slab_rows;       // a multiple of 32 * (waves of a workgroup)
    int32_t nslabs;
    uint64_t *keys;          // [nq][nslabs][kf]: make_key(projected cosine distance, row), ascending, all-ones padded
};

// dynamic LDS of a workgroup of nw waves (pcaf.hip sizes nw by it)
__host__ __device__ inline size_t pcaf_filter_lds(int Tp, int kf, int nw) {
    return sizeof(uint64_t) * 32 * (2 * kf + 1) + sizeof(float) * 32 * (Tp + 4) * (1 + nw) + sizeof(int32_t) * 36;
}

// One step of this wave's share of the slab from HBM into NV float4 registers per lane (exactly Tp / 8 of them are live): the
// 32 rows are one contiguous run, lane l takes float4 number 64 v + l of it.  Written out in place, not as a helper taking the
// array: register arrays handed to helpers by reference have ended up in scratch memory in this code base.
#define HG_PCAF_LOAD(r0_)                                                                                      \
    do {                                                                                                       \
        const int64_t left_ = r_end - (r0_);                                                                   \
        const int valid_ = left_ < 0 ? 0 : (left_ > 32 ? 32 : static_cast<int>(left_));                        \
        const float4 *src_ = reinterpret_cast<const float4 *>(a.rows + (r0_) * a.Tp);                          \
        _Pragma("unroll") for (int v = 0; v < NV; v++) if (v < nv) {                                           \
            const int f_ = v * kWave + lane;                                                                   \
            st[v] = f_ < valid_ * tv ? src_[f_] : make_float4(0.f, 0.f, 0.f, 0.f);                             \
        }                                                                                                      \
        rn_next = lane < valid_ ? a.row_norms[(r0_) + lane] : 0.0f;                                            \
    } while (0)

// grid = query blocks x slabs (blockIdx.x = block * nslabs + slab), nw = blockDim.x / 64 waves that step through the slab in
// lockstep, wave w taking rows [r + 32 w, r + 32 w + 32) of every nw * 32.  The next step's rows are in flight in registers
// while this step's sit in the wave's own LDS buffer and go through the matrix core.  Per query the workgroup keeps up to
// 2 kf keys in LDS and the kf-th best it has seen as a threshold; a lane appends what beats the threshold; when a buffer is
// full the workgroup stops at the step's barrier, a wave cuts the buffer back to its best kf (pcaf_wave_cut), the threshold
// drops and the lanes whose key found no room try again.
template <int NV>
__global__ __launch_bounds__(512) void pcaf_filter_kernel(PcafFilterArgs a) {
    extern __shared__ __align__(16) unsigned char pcaf_smem[];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6, half = lane >> 5, li = lane & 31;
    const int nw = blockDim.x >> 6, S = a.Tp + 4, cap = 2 * a.kf, tv = a.Tp >> 2, nv = a.Tp >> 3;
    uint64_t *buf = reinterpret_cast<uint64_t *>(pcaf_smem);  // [32][cap]
    uint64_t *thr = buf + 32 * cap;                           // [32]
    float *Qs = reinterpret_cast<float *>(thr + 32);          // [32][S]
    float *Rw = Qs + 32 * S + wave * 32 * S;                  // this wave's [32][S]
    int32_t *cnt = reinterpret_cast<int32_t *>(Qs + 32 * S * (1 + nw));  // [32]
    int32_t *flag = cnt + 32;
    const int qb = blockIdx.x / a.nslabs, slab = blockIdx.x % a.nslabs;
    const int q0 = qb * 32, qcnt = a.nq - q0 < 32 ? a.nq - q0 : 32;
    const int64_t r_begin = slab * a.slab_rows, r_end = r_begin + a.slab_rows < a.n ? r_begin + a.slab_rows : a.n;
    const int steps = static_cast<int>((r_end - r_begin + nw * 32 - 1) / (nw * 32));

    for (int f = tid; f < 32 * tv; f += blockDim.x) {
        const int q = f / tv, c = f % tv;
        const float4 v = q < qcnt ? reinterpret_cast<const float4 *>(a.Q + static_cast<int64_t>(q0 + q) * a.Tp)[c]
                                  : make_float4(0.f, 0.f, 0.f, 0.f);
        *reinterpret_cast<float4 *>(Qs + q * S + 4 * c) = v;
    }
    if (tid < 32) {
        thr[tid] = ~0ull;
        cnt[tid] = 0;
    }
    if (tid == 0) *flag = 0;
    const bool qok = li < qcnt;
    const float qn = qok ? a.q_norms[q0 + li] : 0.0f;
    int off[NV];
#pragma unroll
    for (int v = 0; v < NV; v++) {
        const int f = v * kWave + lane;
        off[v] = (f / tv) * S + (f % tv) * 4;
    }
    float4 st[NV];
    float rn_next = 0.0f;
    HG_PCAF_LOAD(r_begin + wave * 32);
    __syncthreads();

    for (int s = 0; s < steps; s++) {
        const int64_t r0 = r_begin + (static_cast<int64_t>(s) * nw + wave) * 32;
#pragma unroll
        for (int v = 0; v < NV; v++)
            if (v < nv) *reinterpret_cast<float4 *>(Rw + off[v]) = st[v];
        const float rn = rn_next;
        pcaf_wave_sync();
        if (s + 1 < steps) HG_PCAF_LOAD(r0 + static_cast<int64_t>(nw) * 32);
        f32x16 acc;
#pragma unroll
        for (int i = 0; i < 16; i++) acc[i] = 0.0f;
        for (int t = 0; t < nv; t++) {
            const float4 av = *reinterpret_cast<const float4 *>(Rw + li * S + 8 * t + 4 * half);
            const float4 bv = *reinterpret_cast<const float4 *>(Qs + li * S + 8 * t + 4 * half);
            acc = pcaf_mfma4(av, bv, acc);
        }
        // D[row i][query li], i = (reg & 3) + 8 (reg >> 2) + 4 half: distances in place of the dots, a bit per live entry
        float d[16];
        uint32_t pend = 0;
#pragma unroll
        for (int reg = 0; reg < 16; reg++) {
            const int i = (reg & 3) + 8 * (reg >> 2) + 4 * half;
            d[reg] = finish_dist(METRIC_COS, acc[reg], qn, __shfl(rn, i, kWave));
            if (qok && r0 + i < r_end) pend |= 1u << reg;
        }
        for (;;) {
            const uint64_t th = thr[li];
#pragma unroll
            for (int reg = 0; reg < 16; reg++) {
                if (!(pend & (1u << reg))) continue;
                const int i = (reg & 3) + 8 * (reg >> 2) + 4 * half;
                const uint64_t key = make_key(d[reg], static_cast<uint32_t>(r0 + i));
                bool done = true;
                if (key < th) {
                    const int pos = atomicAdd(&cnt[li], 1);
                    if (pos < cap) {
                        buf[li * cap + pos] = key;
                    } else {
                        *flag = 1;
                        done = false;
                    }
                }
                if (done) pend &= ~(1u << reg);
            }
            __syncthreads();
            const int over = *flag;
            __syncthreads();
            if (!over) break;
            for (int q = wave; q < 32; q += nw)
                if (cnt[q] >= cap) {  // (wave-uniform)
                    pcaf_wave_cut<(2 * kPcafMaxKf + kWave - 1) / kWave>(buf + q * cap, cap, a.kf, lane);
                    if (lane == 0) {
                        cnt[q] = a.kf;
                        thr[q] = buf[q * cap + a.kf - 1];
                    }
                }
            if (tid == 0) *flag = 0;
            __syncthreads();
        }
    }
    // (behind the last step's barriers nobody appends any more)
    for (int q = wave; q < qcnt; q += nw) {
        const int c = cnt[q] < cap ? cnt[q] : cap, have = c < a.kf ? c : a.kf;
        pcaf_wave_cut<(2 * kPcafMaxKf + kWave - 1) / kWave>(buf + q * cap, c, a.kf, lane);
        uint64_t *out = a.keys + (static_cast<int64_t>(q0 + q) * a.nslabs + slab) * a.kf;
        for (int j = lane; j < a.kf; j += kWave) out[j] = j < have ? buf[q * cap + j] : ~0ull;
    }
}
#undef HG_PCAF_LOAD

// ---- 2b. filter under an allow-mask -------------------------------------------------------------------------------------
// hnswgpu_pcaf_search_filtered[_each]: the kf nearest PASSING rows per query and slab.  Grid, query block, key buffer, cut and
// key output are pcaf_filter_kernel's (so pcaf_refine_kernel serves both); a step is 32 passing rows instead of 32 consecutive
// ones, and a row that no query of the block may see costs no HBM, no MFMA and no epilogue.
struct PcafMaskedArgs : PcafFilterArgs {
    const uint32_t *allow;  // (n + 31) / 32 words per mask, bit r & 31 of word r >> 5: row r passes
    int64_t allow_stride;   // EACH: words between the masks of two queries (the mask of query q is allow + q * allow_stride)
};

// pcaf_filter_lds plus two id buffers of 32 rows per wave (the row fetch runs a step ahead of the epilogue that names the rows)
__host__ __device__ inline size_t pcaf_filter_masked_lds(int Tp, int kf, int nw) {
    return pcaf_filter_lds(Tp, kf, nw) + sizeof(uint32_t) * 64 * nw;
}

// Mask word w of this lane: the mask's (shared) or the OR of the block's qcnt masks (EACH); 0 at and behind w_hi (the end of the
// wave's range, already cut to the mask's length); bits of rows >= n cleared.  One coalesced load per mask and 64 words.
template <bool EACH>
__device__ __forceinline__ uint32_t pcaf_mask_word(const PcafMaskedArgs &a, int q0, int qcnt, int64_t w, int64_t w_hi) {
    if (w >= w_hi) return 0u;
    uint32_t u = 0u;
    if (EACH) {
        const uint32_t *m = a.allow + static_cast<int64_t>(q0) * a.allow_stride + w;
#pragma unroll 4
        for (int q = 0; q < qcnt; q++) u |= m[q * a.allow_stride];
    } else {
        u = a.allow[w];
    }
    if (w == (a.n >> 5)) u &= (1u << (a.n & 31)) - 1u;  // (only the ragged last word has this index)
    return u;
}

// The next step of a wave from the 64 words it holds (lane l: word w0 + l, `mw` = its bits not yet taken): the rows of the
// first 32 set bits in row order go to ids[0 ..), their bits leave mw; returns how many (0: the words are used up).
__device__ __forceinline__ int pcaf_take_step(uint32_t &mw, int64_t w0, int lane, uint32_t *ids) {
    const int c = __popc(mw);
    int incl = c;
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
        const int t = __shfl_up(incl, off, kWave);
        if (lane >= off) incl += t;
    }
    const int tot = __builtin_amdgcn_readlane(incl, kWave - 1);
    int pos = incl - c;
    const uint32_t row0 = static_cast<uint32_t>(w0 + lane) << 5;
    while (mw != 0u && pos < 32) {
        ids[pos++] = row0 + static_cast<uint32_t>(__ffs(mw) - 1);
        mw &= mw - 1u;
    }
    return tot < 32 ? tot : 32;
}

// Build the wave's next step in id buffer nb_ and put its rows in flight: float4 number f = 64 v + lane of the step is column
// f % tv of row ids[f / tv] (pk[v] holds both), a projected row being one run of Tp * 4 bytes.  Words are walked from
// registers; when the 64 in hand are used up the prefetched 64 take their place and the 64 behind them are requested.
#define HG_PCAF_NEXT(nb_)                                                                                      \
    do {                                                                                                       \
        uint32_t *ids_ = idw + (nb_) * 32;                                                                     \
        valid_next = 0;                                                                                        \
        while (wcur < w_hi) {                                                                                  \
            valid_next = pcaf_take_step(mw, wcur, lane, ids_);                                                 \
            if (valid_next) break;                                                                             \
            wcur += kWave;                                                                                     \
            mw = mw_ahead;                                                                                     \
            mw_ahead = pcaf_mask_word<EACH>(a, q0, qcnt, wcur + kWave + lane, w_hi);                           \
        }                                                                                                      \
        pcaf_wave_sync();                                                                                      \
        if (valid_next) {                                                                                      \
            _Pragma("unroll") for (int v = 0; v < NV; v++) if (v < nv) {                                       \
                const int slot_ = pk[v] >> 16;                                                                 \
                st[v] = slot_ < valid_next                                                                     \
                            ? *reinterpret_cast<const float4 *>(a.rows + static_cast<int64_t>(ids_[slot_]) * a.Tp + (pk[v] & 0xffff)) \
                            : make_float4(0.f, 0.f, 0.f, 0.f);                                                 \
            }                                                                                                  \
            rn_next = lane < valid_next ? a.row_norms[ids_[lane]] : 0.0f;                                      \
        }                                                                                                      \
    } while (0)

// grid and LDS front as pcaf_filter_kernel; behind them `fin` (waves that have no further step) and per wave two id buffers.
// Wave w owns the mask words [w_lo, w_hi) of the slab (slab_rows is a multiple of nw * 32: whole words, the same number per
// wave) and turns them into steps of <= 32 passing rows; a step never spans two 64-word loads, so at most the last step of a
// load is partial, and words without a set bit make no step.  EACH: the words are the union over the block's queries, and lane
// li (query li) arms slot i only if its own mask has the row's bit (read from its own mask row: the wave has just read these
// words for the union).
// Barriers.  The waves of a workgroup have different numbers of steps, and every pass of the append loop has workgroup
// barriers, so the loop structure must not depend on a wave's own steps: every wave runs the SAME outer iterations, a wave
// without a step (valid == 0) skips only its LDS store, its fetch, its MFMAs and its epilogue -- code without a barrier -- and
// arrives at the append loop with pend == 0.  Inside the append loop the trip count depends on *flag alone, read by all waves
// between the same two barriers, as in pcaf_filter_kernel.  The outer loop ends on *fin == nw, read between those same two
// barriers: a wave adds itself to *fin exactly once, in the outer body before the append loop of the iteration in which it
// first has no next step, i.e. before barrier 1 of that iteration; nobody adds between barrier 1 and barrier 2 of any pass (the
// only code there is the two reads), and a wave that leaves barrier 2 and adds in the NEXT outer iteration does so after every
// wave has read.  A wave's next-step state only ever goes from "has one" to "has none", so *fin reaches nw, and the iteration
// in which it does still appends the last steps before anyone leaves.
template <int NV, bool EACH>
__global__ __launch_bounds__(512) void pcaf_filter_masked_kernel(PcafMaskedArgs a) {
    extern __shared__ __align__(16) unsigned char pcaf_smem[];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6, half = lane >> 5, li = lane & 31;
    const int nw = blockDim.x >> 6, S = a.Tp + 4, cap = 2 * a.kf, tv = a.Tp >> 2, nv = a.Tp >> 3;
    uint64_t *buf = reinterpret_cast<uint64_t *>(pcaf_smem);  // [32][cap]
    uint64_t *thr = buf + 32 * cap;                           // [32]
    float *Qs = reinterpret_cast<float *>(thr + 32);          // [32][S]
    float *Rw = Qs + 32 * S + wave * 32 * S;                  // this wave's [32][S]
    int32_t *cnt = reinterpret_cast<int32_t *>(Qs + 32 * S * (1 + nw));  // [32]
    int32_t *flag = cnt + 32, *fin = cnt + 33;
    uint32_t *idw = reinterpret_cast<uint32_t *>(cnt + 36) + wave * 64;  // this wave's [2][32]
    const int qb = blockIdx.x / a.nslabs, slab = blockIdx.x % a.nslabs;
    const int q0 = qb * 32, qcnt = a.nq - q0 < 32 ? a.nq - q0 : 32;
    const int64_t wpw = a.slab_rows / (32 * nw), w_all = (a.n + 31) >> 5;
    const int64_t w_lo = slab * (a.slab_rows >> 5) + wave * wpw, w_hi = w_lo + wpw < w_all ? w_lo + wpw : w_all;

    for (int f = tid; f < 32 * tv; f += blockDim.x) {
        const int q = f / tv, c = f % tv;
        const float4 v = q < qcnt ? reinterpret_cast<const float4 *>(a.Q + static_cast<int64_t>(q0 + q) * a.Tp)[c]
                                  : make_float4(0.f, 0.f, 0.f, 0.f);
        *reinterpret_cast<float4 *>(Qs + q * S + 4 * c) = v;
    }
    if (tid < 32) {
        thr[tid] = ~0ull;
        cnt[tid] = 0;
    }
    if (tid == 0) {
        *flag = 0;
        *fin = 0;
    }
    const bool qok = li < qcnt;
    const float qn = qok ? a.q_norms[q0 + li] : 0.0f;
    const uint32_t *own = a.allow + static_cast<int64_t>(qok ? q0 + li : q0) * a.allow_stride;  // (EACH: this lane's query's mask)
    int pk[NV];  // slot of the step << 16 | first float of the lane's float4 in the row
#pragma unroll
    for (int v = 0; v < NV; v++) {
        const int f = v * kWave + lane;
        pk[v] = ((f / tv) << 16) | ((f % tv) * 4);
    }
    float4 st[NV];
    float rn_next = 0.0f;
    int64_t wcur = w_lo;
    uint32_t mw = pcaf_mask_word<EACH>(a, q0, qcnt, wcur + lane, w_hi);
    uint32_t mw_ahead = pcaf_mask_word<EACH>(a, q0, qcnt, wcur + kWave + lane, w_hi);
    int valid_next, p = 0;
    bool told = false;
    HG_PCAF_NEXT(0);
    __syncthreads();

    for (;;) {
        const int valid = valid_next;  // (wave-uniform) rows of this wave's step; 0: the wave has run out
        const uint32_t *ids = idw + p * 32;
        float d[16];
        uint32_t pend = 0;
        if (valid) {
#pragma unroll
            for (int v = 0; v < NV; v++)
                if (v < nv) *reinterpret_cast<float4 *>(Rw + (pk[v] >> 16) * S + (pk[v] & 0xffff)) = st[v];
            const float rn = rn_next;
            pcaf_wave_sync();
            p ^= 1;
            HG_PCAF_NEXT(p);
            f32x16 acc;
#pragma unroll
            for (int i = 0; i < 16; i++) acc[i] = 0.0f;
            for (int t = 0; t < nv; t++) {
                const float4 av = *reinterpret_cast<const float4 *>(Rw + li * S + 8 * t + 4 * half);
                const float4 bv = *reinterpret_cast<const float4 *>(Qs + li * S + 8 * t + 4 * half);
                acc = pcaf_mfma4(av, bv, acc);
            }
            // D[slot i][query li], i = (reg & 3) + 8 (reg >> 2) + 4 half
#pragma unroll
            for (int reg = 0; reg < 16; reg++) {
                const int i = (reg & 3) + 8 * (reg >> 2) + 4 * half;
                d[reg] = finish_dist(METRIC_COS, acc[reg], qn, __shfl(rn, i, kWave));
                if (qok && i < valid) {
                    const uint32_t r = ids[i];
                    const bool pass = EACH ? ((own[r >> 5] >> (r & 31)) & 1u) != 0u : true;
                    if (pass) pend |= 1u << reg;
                }
            }
        }
        if (!valid_next && !told) {  // before barrier 1 below, once per wave
            told = true;
            if (lane == 0) atomicAdd(fin, 1);
        }
        int nfin;
        for (;;) {
            const uint64_t th = thr[li];
#pragma unroll
            for (int reg = 0; reg < 16; reg++) {
                if (!(pend & (1u << reg))) continue;
                const uint64_t key = make_key(d[reg], ids[(reg & 3) + 8 * (reg >> 2) + 4 * half]);
                bool done = true;
                if (key < th) {
                    const int pos = atomicAdd(&cnt[li], 1);
                    if (pos < cap) {
                        buf[li * cap + pos] = key;
                    } else {
                        *flag = 1;
                        done = false;
                    }
                }
                if (done) pend &= ~(1u << reg);
            }
            __syncthreads();
            const int over = *flag;
            nfin = *fin;
            __syncthreads();
            if (!over) break;
            for (int q = wave; q < 32; q += nw)
                if (cnt[q] >= cap) {  // (wave-uniform)
                    pcaf_wave_cut<(2 * kPcafMaxKf + kWave - 1) / kWave>(buf + q * cap, cap, a.kf, lane);
                    if (lane == 0) {
                        cnt[q] = a.kf;
                        thr[q] = buf[q * cap + a.kf - 1];
                    }
                }
            if (tid == 0) *flag = 0;
            __syncthreads();
        }
        if (nfin == nw) break;
    }
    // (behind the last step's barriers nobody appends any more)
    for (int q = wave; q < qcnt; q += nw) {
        const int c = cnt[q] < cap ? cnt[q] : cap, have = c < a.kf ? c : a.kf;
        pcaf_wave_cut<(2 * kPcafMaxKf + kWave - 1) / kWave>(buf + q * cap, c, a.kf, lane);
        uint64_t *out = a.keys + (static_cast<int64_t>(q0 + q) * a.nslabs + slab) * a.kf;
        for (int j = lane; j < a.kf; j += kWave) out[j] = j < have ? buf[q * cap + j] : ~0ull;
    }
}
#undef HG_PCAF_NEXT

// ---- 3. merge + refine --------------------------------------------------------------------------------------------------
struct PcafRefineArgs {
    const uint64_t *keys;  // [nq][nslabs][kf] from the filter
    int32_t nslabs, kf, k;
    const float *rows;     // the f32 base rows
    const float *row_norms;
    int64_t ld;
    const float *Q;        // the original queries, row stride qld
    int64_t qld;
    int32_t dim;
    int32_t *out_ids;      // [nq][k]
    float *out_dist;
};

// A workgroup of four waves per query.  Merge: every wave folds a quarter of the query's nslabs * kf keys into its best kf
// (append what beats the wave's threshold to a 256-key LDS buffer, cut it back when 64 more might not fit), wave 0 cuts the
// four lists to the kf candidates.  Refine: wave w takes candidates w, w + 4, ...: query and row in registers as float4, one
// fmaf chain per lane, the xor butterfly, cosine from the stored norms -- load_query / query_norm / load_row / lane_partial /
// wave_sum / finish_dist exactly as gather_dist_kernel runs them, so a candidate's distance has hnswgpu_rerank's bits.  Wave 0
// sorts the (exact distance, row) keys and writes min(k, candidates) results, -1 / +inf behind them.
template <int NCH>
__global__ __launch_bounds__(kWG) void pcaf_refine_kernel(PcafRefineArgs a) {
    __shared__ uint64_t wb[kNWave][4 * kWave];
    __shared__ uint64_t fin[kNWave * kPcafMaxKf];
    __shared__ int32_t wcnt[kNWave];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    const int64_t y = blockIdx.x;
    const int64_t L = static_cast<int64_t>(a.nslabs) * a.kf;
    const uint64_t *kq = a.keys + y * L;
    uint64_t th = ~0ull;
    int c = 0;
    uint64_t *mine = wb[wave];
    for (int64_t base = wave * kWave; base < L; base += kWG) {
        const int64_t i = base + lane;
        const uint64_t key = i < L ? kq[i] : ~0ull;
        uint64_t m = __ballot(key < th);
        if (m == 0) continue;
        if (c + __popcll(m) > 4 * kWave) {
            pcaf_wave_cut<4>(mine, c, a.kf, lane);
            c = c < a.kf ? c : a.kf;
            if (c == a.kf) th = mine[a.kf - 1];
            m = __ballot(key < th);
        }
        if (key < th) mine[c + __popcll(m & ((1ull << lane) - 1))] = key;
        c += __popcll(m);
        pcaf_wave_sync();
    }
    pcaf_wave_cut<4>(mine, c, a.kf, lane);
    c = c < a.kf ? c : a.kf;
    for (int j = lane; j < a.kf; j += kWave) fin[wave * a.kf + j] = j < c ? mine[j] : ~0ull;
    if (lane == 0) wcnt[wave] = c;
    __syncthreads();
    int ncand = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
    ncand = ncand < a.kf ? ncand : a.kf;
    if (wave == 0) pcaf_wave_cut<kNWave * kPcafMaxKf / kWave>(fin, kNWave * a.kf, a.kf, lane);
    __syncthreads();

    uint64_t *exact = wb[0];  // [ncand] (the waves' merge buffers are done with)
    float4 q[NCH];
    load_query<NCH>(q, a.Q + y * a.qld, a.dim, lane);
    const float qn = query_norm<NCH>(q);
    const int nvec = static_cast<int>(a.ld / 4);
    for (int j = wave; j < ncand; j += kNWave) {
        const uint32_t id = static_cast<uint32_t>(fin[j]);
        float4 r[NCH];
        load_row<NCH>(r, a.rows + static_cast<int64_t>(id) * a.ld, nvec, lane, true);
        const float s = wave_sum(lane_partial<NCH, false>(q, r));
        if (lane == 0) exact[j] = make_key(finish_dist(METRIC_COS, s, qn, a.row_norms[id]), id);
    }
    __syncthreads();
    if (wave != 0) return;
    pcaf_wave_cut<kPcafMaxKf / kWave>(exact, ncand, ncand, lane);
    for (int j = lane; j < a.k; j += kWave) {
        const bool have = j < ncand;
        a.out_ids[y * a.k + j] = have ? static_cast<int32_t>(static_cast<uint32_t>(exact[j])) : -1;
        a.out_dist[y * a.k + j] = have ? key_dist(exact[j]) : __builtin_inff();
    }
}

}  // namespace hg
