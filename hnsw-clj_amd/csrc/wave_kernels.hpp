// wave_kernels.hpp -- the HNSW traversal of LARGE launches: one wave per query, the candidate list as a main list in LDS plus an
// admission buffer in the wave's registers.
//
// search-layer-ultra (ultra_fast.clj:151-212) on the single-workgroup kernel (kernels.hpp: hnsw_search_kernel) merges every
// expansion's admitted neighbours into ONE sorted list by rank and scatter: every list entry is compared with every admitted
// neighbour, every expansion.  With one wave per query (the shape of every launch that fills the chip) that is the traversal's
// largest compute phase -- at the headline's ef 640 the merge took 2.9 of the 8.2 us an expansion takes per wave, the same again
// went into selecting the next candidate from LDS, and the launch ran no faster with the int8 rejection test than without
// (24 % fewer bytes, same time): THAT kernel is bound by instructions, not by memory.  This one is bound by memory: the
// headline launch (the DENSE instance, four rows in flight) fetches 57.65 GB past L2 in 8.56 ms -- 5.8 MB per query, 1,868 f32 rows
// of 3 KB of which nine in ten are admitted; 6.74 TB/s, 26.3 GB/s per CU, where a CU's path to memory carries 29-31 GB/s for random
// rows of an Infinity-Cache-resident table of this size (profiles/hnsw_dense_rows_ab.txt) -- so its time follows the bytes that
// leave L2 (hence the bounds table of the DENSE instances, and the 16-bit query code of the others' rejection test, kernels.hpp:
// Query16) and the dependent round trips a hop fetches them in (hence the rows in flight).  The list is hnsw_list.hpp's, the
// one the sequencer of solo_kernels.hpp keeps too, here without a mirror: nobody else reads it.  Ids, distance bits and both
// counters are hnsw_search_kernel's (the parity suite runs both).
#pragma once
#include "hnsw_list.hpp"

namespace hg {

// One trip of an expansion's gather: the f32 rows of the needed neighbours of ranks t0 .. t0 + R - 1 in flight together, their
// distances into cand_d (lane b takes the candidate of rank t0 + b and fetches its norm up front).
template <int NCH, int R, bool L2>
__device__ __forceinline__ void wave_gather_trip(const float *rows, int64_t ld, const float *row_norms, int metric,
                                                 const float4 (&q)[NCH], float qn, const int32_t *cand_id, float *cand_d, bool isset,
                                                 int rank, int t0, int nneed, int nvec, int lane) {
    float4 r[R][NCH];
    int myj = -1;
#pragma unroll
    for (int b = 0; b < R; b++) {
        const uint64_t hit = __builtin_amdgcn_ballot_w64(isset && rank == t0 + b);
        const int jb = hit ? __ffsll(static_cast<unsigned long long>(hit)) - 1 : -1;
        myj = lane == b ? jb : myj;
    }
    const int32_t myid = myj >= 0 ? cand_id[myj] : 0;
    const float myrn = (metric == METRIC_COS && myj >= 0) ? row_norms[myid] : 0.0f;
#pragma unroll
    for (int b = 0; b < R; b++) {
        const int32_t rid = __builtin_amdgcn_readlane(myid, b);
        load_row<NCH>(r[b], rows + static_cast<int64_t>(rid) * ld, nvec, lane, t0 + b < nneed);
    }
    float s[R];
#pragma unroll
    for (int b = 0; b < R; b++) s[b] = lane_partial<NCH, L2>(q, r[b]);
    const float mine = rows_sum_to_lane<R>(s, lane);  // lane b keeps candidate b's reduced sum
    if (myj >= 0) cand_d[myj] = finish_dist(metric, mine, qn, myrn) + 0.0f;
}

// One wave per query (workgroups of one wave; persistent: workgroup b serves slots b, b + gridDim.x, ...; a slot is a query).  VG = visited set in
// HBM stamps.  Build launches too (q_rows: the query is a base row, the best entry of every upper level <= the node's level is
// emitted for the linker, all ef candidates of layer 0 are the result); the repeat pass stays with hnsw_search_kernel.
// DENSE: the int8 bounds of the whole batch are in a table (dense_kernels.hpp; HnswArgs::lb) -- no query code, no int8 rows here.
template <int NCH, int RB, bool L2, bool VG, bool PARTS = false, bool DENSE = false>
__global__ __launch_bounds__(kWave) void hnsw_wave_kernel(HnswArgs a) {
    extern __shared__ __align__(16) unsigned char smem[];
    // LDS: [main: cap x 8] [img: 64 x 8] [cand_id | cand_d: kMaxDeg each] [bits: nwords]
    uint2 *const curA = reinterpret_cast<uint2 *>(smem);
    uint2 *const img = curA + a.cap;
    int32_t *const cand_id = reinterpret_cast<int32_t *>(img + kWave);
    float *const cand_d = reinterpret_cast<float *>(cand_id + kMaxDeg);
    uint32_t *const bits = reinterpret_cast<uint32_t *>(cand_d + kMaxDeg);
    uint32_t *stamps = VG ? a.vis + static_cast<int64_t>(blockIdx.x) * a.vis_stride : nullptr;
    const int lane = threadIdx.x;
    const int nvec = static_cast<int>(a.ld / 4);
    uint32_t gen = a.gen_base;
    // Ordered launches (order_kernels.hpp): the loop runs over SLOTS.  Workgroups b and b + 8 share an XCD (observed, and used for
    // speed only), so the slots of one XCD, s % 8 = x, take the x-th eighth of q_order[] front to back: queries with neighbouring
    // keys run on one XCD at one time.  The ragged end: the last eighths hold fewer than per8 queries, their surplus slots none.
    const int per8 = (a.nq + 7) >> 3;
    const int nslot = a.q_order ? 8 * per8 : a.nq;
    for (int slot = blockIdx.x; slot < nslot; slot += gridDim.x) {
        int qi = slot;
        if (a.q_order) {
            const int pos = (slot & 7) * per8 + (slot >> 3);
            if (pos >= a.nq) continue;
            qi = a.q_order[pos];
        }
        int64_t qrow = qi;
        int32_t entry = a.entry, max_level = a.max_level;
        uint32_t vis0 = 0;  // the row that owns bit 0 of the LDS visited set
        if (PARTS) {  // a forest launch (kernels.hpp, HnswArgs::items): qi is an item
            const int4 it = a.items[qi];
            if (it.y < 0) {
                hnsw_item_padding(a, qi, lane, kWave);
                continue;
            }
            // (one item per workgroup: the four words into SGPRs, where entry and max_level of a plain launch live)
            qrow = __builtin_amdgcn_readfirstlane(it.x);
            entry = __builtin_amdgcn_readfirstlane(it.y);
            max_level = __builtin_amdgcn_readfirstlane(it.z);
            vis0 = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(it.w));
        }
        const float *qptr = a.q_rows ? a.rows + static_cast<int64_t>(a.q_rows[qi]) * a.ld : a.Q + qrow * a.qld;
        float4 q[NCH];
        load_query<NCH>(q, qptr, a.dim, lane);
        const float qn = a.metric == METRIC_COS ? query_norm<NCH>(q) : 0.0f;
        Query16<NCH> qc;  // the query's side of the rejection test
        if (!DENSE && a.qrows != nullptr) encode_query16<NCH>(q, qc);
        const int qlevel = a.q_levels ? a.q_levels[qi] : -1;
        int64_t n_eval = 0, n_hop = 0, n_exact = 0;
        int len = 0;
        bool over = false;
        {  // seed: the entry point (ultra_fast.clj:358-359)
            float4 r[NCH];
            load_row<NCH>(r, a.rows + static_cast<int64_t>(entry) * a.ld, nvec, lane, true);
            const float s = wave_sum(lane_partial<NCH, L2>(q, r));
            const float d = finish_dist(a.metric, s, qn, a.metric == METRIC_COS ? a.row_norms[entry] : 0.0f);
            if (lane == 0) curA[0] = make_uint2(__float_as_uint(d + 0.0f), static_cast<uint32_t>(entry));
            len = 1;
            n_eval = 1;
        }
        const int top_l = (a.ref_start && qlevel >= 0 && qlevel < max_level) ? qlevel : max_level;
        for (int level = top_l; level >= 0; level--) {
            const int ef_l = level > 0 ? 1 : a.ef;
            // fresh visited set per layer (:156); entries carried from the level above are marked
            if (VG) {
                gen++;
            } else {
                for (int w = lane; w < a.nwords; w += kWave) bits[w] = 0;
            }
            if (len > ef_l) len = ef_l;
            // the reference re-evaluates its entry points at every layer (:162-167); the values are reused here, but counted so
            // that `evals` is the reference's number of distance calls
            if (level != top_l) n_eval += len;
            for (int i = lane; i < len; i += kWave) {
                uint2 e = curA[i];
                e.y &= ~kExpanded;
                curA[i] = e;
                if (VG) atomicExch(&stamps[e.y], gen);
                else atomicOr(&bits[(PARTS ? e.y - vis0 : e.y) >> 5], 1u << ((PARTS ? e.y - vis0 : e.y) & 31));
            }
            const int deg = level == 0 ? a.M0 : a.M;
            HnswList<false> L;
            L.main = curA;
            L.img = img;
            L.lane = lane;
            L.cap = a.cap;
            L.overflow = false;
            L.begin_level(len, ef_l);
            for (;;) {
                uint32_t node;
                if (!L.pop(node)) break;
                const int32_t *adj = level == 0 ? a.l0_adj + static_cast<int64_t>(node) * a.M0
                                                : a.up_adj + (a.up_off[node] + (level - 1)) * a.M;
                const int nbr = lane < deg ? adj[lane] : -1;
                bool fresh = false;
                if (nbr >= 0 && nbr < a.n) {
                    if (VG) {
                        fresh = atomicExch(&stamps[nbr], gen) != gen;
                    } else {
                        const uint32_t vb = PARTS ? static_cast<uint32_t>(nbr) - vis0 : static_cast<uint32_t>(nbr);
                        const uint32_t bit = 1u << (vb & 31);
                        const uint32_t old = atomicOr(&bits[vb >> 5], bit);
                        fresh = !(old & bit);
                    }
                }
                const uint64_t fm = __builtin_amdgcn_ballot_w64(fresh);
                n_hop++;
                if (fm == 0) continue;
                const int nc = __popcll(fm);
                if (fresh) cand_id[__popcll(fm & ((1ull << lane) - 1ull))] = nbr;  // adjacency order
                n_eval += nc;
                const bool list_full = L.full();
                const float worst0 = list_full ? L.worst : 0.0f;
                // ---- rejection test on the int8 rows (kernels.hpp: quantize_rows_kernel): with a full list a neighbour whose
                //      LOWER BOUND is already >= the worst cannot be admitted (:195-198) -- it gets +inf and no f32 fetch
                uint64_t needmask = nc >= 64 ? ~0ull : ((1ull << nc) - 1ull);
                if constexpr (DENSE) {
                    // ... read from the table, one bound per fresh neighbour: indexed by the QUERY (ordered launches permute slots)
                    if (list_full) {
                        const float lb = lane < nc ? a.lb[static_cast<int64_t>(qi) * a.lb_ld + cand_id[lane]] : 0.0f;
                        const bool need = lane < nc && !(lb >= worst0);  // NaN: needs the exact distance
                        if (lane < nc) cand_d[lane] = __uint_as_float(0x7f800000u);  // overwritten below if needed
                        needmask = __builtin_amdgcn_ballot_w64(need);
                    }
                } else if (a.qrows != nullptr && list_full) {
                    uint64_t wmask = 0;
                    const int own = wave_sum8_row(lane);  // the row of a step whose total this lane receives
                    for (int j0 = 0; j0 < nc; j0 += 8) {
                        const int myj = j0 + own;
                        const bool ok = (lane & 7) == 0 && myj < nc;
                        const float4 mymeta = ok ? a.qmeta[cand_id[myj]] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                        const int lj = j0 + lane;
                        const int32_t ids8 = cand_id[(lane < 8 && lj < nc) ? lj : j0];  // past nc: a valid row, unused
                        uint32_t w[8][NCH];
#pragma unroll
                        for (int b = 0; b < 8; b++) {
                            const int32_t rid = __builtin_amdgcn_readlane(ids8, b);
                            const uint32_t *rp = a.qrows + (static_cast<int64_t>(rid) * kWave + lane) * NCH;
#pragma unroll
                            for (int cc = 0; cc < NCH; cc++) w[b][cc] = rp[cc];
                        }
                        int acc[8];
#pragma unroll
                        for (int b = 0; b < 8; b++) acc[b] = code_dot16<NCH>(qc, w[b]);
                        const int tot = wave_sum8_int(acc, lane);
                        const float lb = code_lower_bound(a.metric, tot, qc.sc, mymeta, mymeta.w);
                        const bool need = ok && !(lb >= worst0);  // NaN: needs the exact distance
                        if (ok) cand_d[myj] = __uint_as_float(0x7f800000u);  // overwritten below if needed
                        const uint64_t m8 = ((__builtin_amdgcn_ballot_w64(need) & 0x0101010101010101ull) * 0x0102040810204080ull) >> 56;
                        wmask |= m8 << j0;
                    }
                    needmask = wmask;
                }
                // ---- gather rows + distances of the neighbours that need them, RB rows per trip (lane b takes the candidate of
                //      rank t0 + b and fetches its norm up front)
                const int nneed = __popcll(needmask);
                n_exact += nneed;
                const bool isset = (needmask >> lane) & 1ull;
                const int rank = __popcll(needmask & ((1ull << lane) - 1ull));
                // (768-float rows with the table and four rows in flight: a last trip of one or two rows is the two-row trip --
                // nneed is wave-uniform, and a row's distance does not depend on the trip that fetched it)
                constexpr bool kShortTrip = DENSE && NCH == 3 && RB == 4;
                for (int t0 = 0; t0 < nneed; t0 += RB) {
                    if (kShortTrip && nneed - t0 <= 2)
                        wave_gather_trip<NCH, 2, L2>(a.rows, a.ld, a.row_norms, a.metric, q, qn, cand_id, cand_d, isset, rank, t0, nneed,
                                                     nvec, lane);
                    else
                        wave_gather_trip<NCH, RB, L2>(a.rows, a.ld, a.row_norms, a.metric, q, qn, cand_id, cand_d, isset, rank, t0, nneed,
                                                      nvec, lane);
                }
                // ---- admission: lane j = the j-th fresh neighbour
                const float cdist = lane < nc ? cand_d[lane] : 0.0f;
                const uint32_t cid = lane < nc ? static_cast<uint32_t>(cand_id[lane]) : 0u;
                uint64_t smask = __builtin_amdgcn_ballot_w64(lane < nc && (!list_full || cdist < worst0));
                if (smask) {
                    L.make_room(smask, cdist, cid);
                    L.admit(smask, cdist, cid);
                }
            }
            len = L.end_level();
            over = over || L.overflow;
            if (a.q_rows && level > 0 && level <= qlevel && lane == 0) {  // build: the nearest node of this layer, for the linker
                a.up_out_ids[static_cast<int64_t>(qi) * a.up_stride + (level - 1)] = len > 0 ? static_cast<int32_t>(curA[0].y & ~kExpanded) : -1;
                a.up_out_dist[static_cast<int64_t>(qi) * a.up_stride + (level - 1)] = len > 0 ? __uint_as_float(curA[0].x) : 0.0f;
            }
        }
        // ---- results: ascending, take k (:362-370; the distances are reused, not recomputed)
        const int real = len < a.ef ? len : a.ef;
        for (int i = lane; i < a.k; i += kWave) {
            const bool ok = i < real;
            a.out_ids[static_cast<int64_t>(qi) * a.k + i] = ok ? static_cast<int32_t>(curA[i].y & ~kExpanded) : -1;
            a.out_dist[static_cast<int64_t>(qi) * a.k + i] = ok ? __uint_as_float(curA[i].x) : __uint_as_float(0x7f800000u);
        }
        if (lane == 0) {
            if (a.again && over) a.again[atomicAdd(a.again_cnt, 1)] = qi;
            if (a.stats) {
                a.stats[2 * static_cast<int64_t>(qi)] = n_eval;
                a.stats[2 * static_cast<int64_t>(qi) + 1] = n_hop;
            }
            if (a.rej_stats) {
                atomicAdd(a.rej_stats, static_cast<unsigned long long>(n_exact));
                atomicAdd(a.rej_stats + 1, static_cast<unsigned long long>(n_eval));
            }
        }
    }
    if (a.host_flag) {
        __threadfence_system();  // this thread's results (host memory) are visible system-wide ...
        if (lane == 0) {
            if (atomicAdd(a.done_cnt, 1u) == gridDim.x - 1) {  // the last workgroup: every result is out
                atomicExch(a.done_cnt, 0u);
                __threadfence();
                *a.host_again = a.again_cnt ? atomicAdd(a.again_cnt, 0) : 0;
                __threadfence_system();
                __hip_atomic_store(a.host_flag, a.flag_val, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
            }
        }
    }
}

}  // namespace hg
