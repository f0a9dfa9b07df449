// pcaf_mutate_kernels.hpp -- rows join, leave and take new values on a live P-HNSW handle (pcaf.hip: hnswgpu_pcaf_add / _remove /
// _update; the contract: include/hnswgpu.h, "P-HNSW").  A row of such a handle has four pieces: its base row (ld floats), that
// row's norm, its projected row (Tp floats) and the projected row's norm.  The arithmetic is done elsewhere -- norms by
// row_norms_kernel (launch_norms), projected rows and their norms by pcaf_project_kernel and its MAP form (pcaf_kernels.hpp), the
// drop mask and the rank scan by lsh_remove_mark_kernel / lsh_remove_rank_kernel (remove_kernels.hpp, tables = 0) -- so what is
// here is row copies: the call's staged rows to the rows their ids name, and the kept rows' four pieces to their ranks.
// Nothing is moved in place: sources are the handle's arrays or the call's staging, destinations the call's staged arrays.  No
// kernel waits for another workgroup; every loop is bounded by ld or Tp, and every index is checked against n / n1 before its
// store.
#pragma once
#include "kernels.hpp"
#include "remove_kernels.hpp"

namespace hg {

// ---- update ---------------------------------------------------------------------------------------------------------------
struct PcafUpdateArgs {
    int64_t n, m, ld;
    const int32_t *ids;   // [m] slot -> row id, distinct, each in [0, n) (checked on the host)
    const float *stage;   // [m][ld] the call's rows in slot order, padding zero
    const float *snorms;  // [m] their norms (row_norms_kernel)
    float *new_base, *new_norms;  // device copies of the handle's arrays before this kernel
};

// One wave per slot: the staged row as ld / 4 float4s and its norm replace those of row ids[s] in the staged copies.  The ids
// are distinct, so no two slots write one row.
static __global__ __launch_bounds__(kWG) void pcaf_update_place_kernel(PcafUpdateArgs a) {
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t s = static_cast<int64_t>(blockIdx.x) * kNWave + (threadIdx.x >> 6);
    if (s >= a.m) return;  // (wave-uniform)
    const int64_t r = a.ids[s];
    if (r < 0 || r >= a.n) return;
    const float4 *sp = reinterpret_cast<const float4 *>(a.stage + s * a.ld);
    float4 *dp = reinterpret_cast<float4 *>(a.new_base + r * a.ld);
    for (int64_t j = lane; j < a.ld / 4; j += kWave) dp[j] = sp[j];
    if (lane == 0) a.new_norms[r] = a.snorms[s];
}

// ---- remove ---------------------------------------------------------------------------------------------------------------
struct PcafRemoveArgs {
    LshRemoveArgs r;  // n0, n1, m, W, ld, rows, keep, word_rank, old / new base and norms, gate; tables = 0
    int64_t Tp;       // floats per projected row (a multiple of 8)
    const float *old_low, *old_lnorms;  // [n0][Tp], [n0]
    float *new_low, *new_lnorms;        // [n1][Tp], [n1]
};

// One wave per old row, one pass: a kept row's base row, its norm, its projected row and that row's norm go to its rank (the
// kept rows below it).  The two rows move as whole float4s -- ld / 4 of one, Tp / 4 of the other, so at the reference's sizes a
// lane carries three of the base row and a quarter of the wave one of the projected row -- and both norms leave from lane 0.
static __global__ __launch_bounds__(kWG) void pcaf_remove_rows_kernel(PcafRemoveArgs a) {
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t r = static_cast<int64_t>(blockIdx.x) * kNWave + (threadIdx.x >> 6);
    if (!lsh_remove_kept(a.r, r)) return;  // (wave-uniform; rows >= n0 are not kept)
    const int64_t to = lsh_remove_rank(a.r, r);
    if (to < 0 || to >= a.r.n1) return;
    const float4 *bs = reinterpret_cast<const float4 *>(a.r.old_base + r * a.r.ld);
    float4 *bd = reinterpret_cast<float4 *>(a.r.new_base + to * a.r.ld);
    for (int64_t j = lane; j < a.r.ld / 4; j += kWave) bd[j] = bs[j];
    const float4 *ls = reinterpret_cast<const float4 *>(a.old_low + r * a.Tp);
    float4 *ld = reinterpret_cast<float4 *>(a.new_low + to * a.Tp);
    for (int64_t j = lane; j < a.Tp / 4; j += kWave) ld[j] = ls[j];
    if (lane == 0) {
        a.r.new_norms[to] = a.r.old_norms[r];
        a.new_lnorms[to] = a.old_lnorms[r];
    }
}

}  // namespace hg
