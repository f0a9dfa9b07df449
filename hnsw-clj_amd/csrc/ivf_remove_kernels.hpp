// ivf_remove_kernels.hpp -- rows leave the inverted lists of a live handle (ivf.hip: hnswgpu_ivf_remove).  The mask of the rows
// that go, every kept row's new id and the move of the kept base rows and norms are the kernels of remove_kernels.hpp, run
// with `tables == 0` (no codes are touched); so are the kept list positions per chunk of 256 and their scan, with d_listids as
// the one "table" (blockIdx.y == 0).  New here: the stable compaction of the list ids that also records where every old list
// position goes, the shrunken offsets, and the move of the list-order rows and norms.  Integer work and copies only.  A kept
// position's destination is a function of the mask and the old arrays alone -- the kept positions before it -- never the order
// atomics arrive in (there are none here).  No kernel waits for another workgroup, every loop is bounded by kWG or ld, and every
// index is checked against n1 / nlist before its store.
#pragma once
#include "remove_kernels.hpp"

namespace hg {

constexpr uint32_t kIvfRemoveGone = 0xffffffffu;  // IvfRemoveArgs::dest of a position whose row leaves

struct IvfRemoveArgs {
    // the mask, the ranks, the base rows and the chunk counts: tables == 0, old_ids = the list ids, new_ids unused.  Of its gate,
    // [2 * kRemoveMaxTables] is the rank scan's total and [kRemoveMaxTables] the kept list positions (lsh_remove_chunk_scan_kernel);
    // [0] is new_off[nlist] (ivf_remove_offsets_kernel)
    LshRemoveArgs r;
    int32_t nlist;
    const int64_t *old_off;  // [nlist + 1]
    int64_t *new_off;
    int32_t *new_ids;        // [n1] list order, the kept rows under their new ids
    uint32_t *dest;          // [n0] the new position of old list position p, or kIvfRemoveGone
    const float *old_lrows, *old_lnorms;  // list order, as they stand (unused on a handle whose lists are its base rows in place)
    float *new_lrows, *new_lnorms;
};

// The stable compaction (lsh_remove_ids_kernel, plus the record): a kept position p goes to the kept positions before p -- its
// chunk's base plus the kept positions before it in the chunk -- under its row's new id.  Lists are contiguous and the order of
// positions is kept, so every list's kept members stay together, in their order, and start at new_off of the list.
__global__ __launch_bounds__(kWG) void ivf_remove_ids_kernel(IvfRemoveArgs a) {
    __shared__ uint32_t wsum[kNWave];
    const int64_t p = static_cast<int64_t>(blockIdx.x) * kWG + threadIdx.x;
    const int64_t r = p < a.r.n0 ? a.r.old_ids[p] : -1;
    const bool kept = lsh_remove_kept(a.r, r);
    uint32_t total;
    const uint32_t before = wg_exclusive_sum(kept ? 1u : 0u, wsum, &total);
    if (p >= a.r.n0) return;
    const int64_t to = static_cast<int64_t>(a.r.chunk_base[blockIdx.x]) + before, id = kept ? lsh_remove_rank(a.r, r) : -1;
    const bool ok = kept && to < a.r.n1 && id < a.r.n1;
    a.dest[p] = ok ? static_cast<uint32_t>(to) : kIvfRemoveGone;
    if (ok) a.new_ids[to] = static_cast<int32_t>(id);
}

// new_off[l] = the kept positions before old_off[l]: the base of the chunk that holds position old_off[l] - 1 plus the kept
// positions of that chunk below old_off[l] (at most kWG of them, a wave's ballots: four rounds).  One wave per list boundary;
// every lane of the wave holds the same sum.  An emptied list keeps its place with two equal offsets.
__global__ __launch_bounds__(kWG) void ivf_remove_offsets_kernel(IvfRemoveArgs a) {
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t l = static_cast<int64_t>(blockIdx.x) * kNWave + (threadIdx.x >> 6);
    if (l > a.nlist) return;  // (wave-uniform)
    const int64_t off = a.old_off[l], b = off < a.r.n0 ? off : a.r.n0;
    int64_t before = 0;
    if (b > 0) {
        const int64_t c = (b - 1) / kWG;
        before = a.r.chunk_base[c];
        for (int64_t p0 = c * kWG; p0 < b; p0 += kWave) {  // (wave-uniform bounds)
            const int64_t p = p0 + lane;
            before += __popcll(__ballot(p < b && lsh_remove_kept(a.r, a.r.old_ids[p < b ? p : b - 1])));
        }
    }
    if (lane != 0) return;
    a.new_off[l] = before;
    if (l == a.nlist) a.r.gate[0] = before;
}

// One wave per OLD list position: a kept position's ld floats as whole float4s, and its norm, go to the recorded destination.
// Never in place.
__global__ __launch_bounds__(kWG) void ivf_remove_lrows_kernel(IvfRemoveArgs a) {
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t p = static_cast<int64_t>(blockIdx.x) * kNWave + (threadIdx.x >> 6);
    if (p >= a.r.n0) return;  // (wave-uniform)
    const uint32_t to = a.dest[p];
    if (to == kIvfRemoveGone || static_cast<int64_t>(to) >= a.r.n1) return;
    const float4 *src = reinterpret_cast<const float4 *>(a.old_lrows + p * a.r.ld);
    float4 *dst = reinterpret_cast<float4 *>(a.new_lrows + static_cast<int64_t>(to) * a.r.ld);
    for (int64_t j = lane; j < a.r.ld / 4; j += kWave) dst[j] = src[j];
    if (lane == 0) a.new_lnorms[to] = a.old_lnorms[p];
}

}  // namespace hg
