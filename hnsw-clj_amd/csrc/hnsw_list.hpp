// hnsw_list.hpp -- the candidate list of the one-wave HNSW traversals: hnsw_wave_kernel (wave_kernels.hpp: one wave per query) and
// the sequencer of hnsw_solo_kernel (solo_kernels.hpp: one query over several CUs).
//
// The list is TWO sorted sequences: the main list in LDS and an admission buffer of up to 64 entries in the wave's registers (lane
// k = the k-th smallest).  The reference's `nearest` (ultra_fast.clj:158) is main[0, pm) + buffer[0, pb), pm + pb <= ef; its
// `candidates` are the unexpanded entries of both.  An admitted neighbour (:195-198) enters the buffer by one ballot and one lane
// shift (several at once: one pass decides them exactly as the reference's loop would); the entry it pushes out of `nearest`
// (:203-204) is the later of main[pm - 1] and buffer[pb - 1] -- a pointer moves, nothing else.  Evicted entries stay where they
// are: the next candidate is the smaller of the first unexpanded entries of either sequence, out of two register windows, and it is
// expanded iff it is still <= the worst of `nearest` (:175-178) -- the reference's own loop, instead of hnsw_search_kernel's
// positional merge of every expansion (one wave moved ~6 blocks of a 640-entry list per admission: 4 us per expansion).  Every 63
// admissions, and when the layer is done, the buffer is merged into the main list in place (per-lane binary searches).
#pragma once
#include "kernels.hpp"

#include <type_traits>

namespace hg {

// LDS accesses that another wave of the workgroup must see in program order: volatile, and EXPLICITLY in the LDS address space
// (a volatile access through a generic pointer is a flat instruction with a wait behind it: the compiler does not infer the
// address space of volatile accesses)
#define HG_LDS __attribute__((address_space(3)))
template <class T>
__device__ __forceinline__ volatile HG_LDS T *ldsv(T *p) {
    return (volatile HG_LDS T *)p;
}
template <class T>
__device__ __forceinline__ HG_LDS T *ldsp(T *p) {
    return (HG_LDS T *)p;
}

// Scalar decisions compare ORDERABLE KEYS of the distance bits with integer instructions: a float compare of two uniform values is
// a vector instruction whose result the scalar unit then waits ~25 cycles for.
__device__ __forceinline__ uint32_t wl_key(uint32_t b) {
    return b ^ (static_cast<uint32_t>(static_cast<int32_t>(b) >> 31) | 0x80000000u);
}

// The list of ONE wave's traversal of one layer.  All scalars are wave-uniform.
// MIRRORED: the buffer's LDS image is also its MIRROR, which other waves of the workgroup read while the traversal runs (the solo
// kernel's fetchers look ahead through it).  Then every access to the image is volatile and in the LDS address space, an entry's
// two words are stored separately, and the list publishes what those waves follow in sc[]: [0] the first unexpanded index of the
// main list, [1] its length, [3] the buffer's entries.  They are hints: a reader may meet the middle of an update.
template <bool MIRRORED>
struct HnswList {
    using Image = std::conditional_t<MIRRORED, volatile HG_LDS uint2 *, uint2 *>;
    uint2 *main;    // LDS [cap] (distance bits, node | expanded flag), ascending
    Image img;      // LDS [64]: the buffer's image while it is merged (MIRRORED: and whenever publish() has run)
    volatile HG_LDS int32_t *sc;  // (MIRRORED) LDS scalars
    int lane, cap, ef_l;
    int lm, pm;                 // main entries; those of them in `nearest`
    float bd;                   // buffer, lane k: distance (+inf behind the entries) ...
    uint32_t bi;                // ... and node | expanded flag
    int nb, pb;                 // buffer entries; those of them in `nearest`
    uint64_t bun;               // bit k: buffer entry k is unexpanded
    float fd;                   // front window of the main list, lane l: entry fbase + l
    uint32_t fi;
    int fbase;
    uint64_t fun;               // bit l: entry fbase + l exists and is unexpanded
    float td;                   // tail window: distance of main entry tbase + l (the entries around pm)
    int tbase;
    float worst;                // of `nearest`, while it holds ef entries
    uint32_t worst_k;
    bool overflow;              // ties with the worst may have been cut off: the query is repeated with a larger list
    bool dirty;                 // (MIRRORED) the buffer differs from its mirror
    bool dirty_sc;              // (MIRRORED) ... only its entry count does
    unsigned long long merges;  // (MIRRORED) merges of the buffer into the main list, a diagnostic

    __device__ __forceinline__ bool full() const { return pm + pb >= ef_l; }
    __device__ __forceinline__ void put(int i, uint32_t dbits, uint32_t node) {
        if constexpr (MIRRORED) {
            img[i].x = dbits;
            img[i].y = node;
        } else {
            img[i] = make_uint2(dbits, node);
        }
    }
    __device__ __forceinline__ int first_unexpanded() const {  // of the main list, as far as the front window shows
        return fun ? fbase + __ffsll(static_cast<unsigned long long>(fun)) - 1 : fbase + kWave;
    }
    __device__ __forceinline__ void load_front(int from) {
        fbase = from;
        const int i = fbase + lane;
        uint2 e = make_uint2(0u, kExpanded);
        if (i < lm) e = main[i];
        fd = __uint_as_float(e.x);
        fi = e.y;
        fun = __builtin_amdgcn_ballot_w64(i < lm && !(e.y & kExpanded));
    }
    __device__ __forceinline__ void load_tail() {
        tbase = pm > kWave ? pm - kWave : 0;
        const int i = tbase + lane;
        td = i < lm ? __uint_as_float(main[i].x) : 0.0f;
    }
    __device__ __forceinline__ void top_worst() {  // the later of main[pm - 1] and buffer[pb - 1]: the worst of `nearest`
        const int im = pm - 1 - tbase, ib = pb - 1;
        const uint32_t wmb = static_cast<uint32_t>(__builtin_amdgcn_readlane(__float_as_int(td), im > 0 ? im : 0));
        const uint32_t wbb = static_cast<uint32_t>(__builtin_amdgcn_readlane(__float_as_int(bd), ib > 0 ? ib : 0));
        const uint32_t km = pm > 0 ? wl_key(wmb) : 0u, kb2 = pb > 0 ? wl_key(wbb) : 0u;
        worst_k = kb2 >= km ? kb2 : km;
        worst = __uint_as_float(kb2 >= km ? wbb : wmb);
    }
    // The first `entries` of main are the layer's entry points; overflow (and merges) are the caller's to clear.
    __device__ __forceinline__ void begin_level(int entries, int ef) {
        ef_l = ef;
        lm = entries;
        pm = entries;
        bd = __uint_as_float(0x7f800000u);
        bi = kExpanded;
        nb = pb = 0;
        bun = 0;
        load_front(0);
        load_tail();
        top_worst();
        if constexpr (MIRRORED) {
            dirty = false;
            dirty_sc = false;
            if (lane == 0) {
                sc[0] = 0;
                sc[1] = lm;
                sc[3] = 0;
            }
        }
    }
    // Merge the buffer into the main list, in place: buffer entry k goes to k + (main entries <= it), main entry i to i + (buffer
    // entries < it) -- the main entries are the older ones.  Blocks from the tail down to the first position that changes; an
    // entry moves towards the tail by at most 64, into blocks already read.
    __device__ __forceinline__ void compact() {
        if (nb == 0) return;
        if constexpr (MIRRORED) merges++;
        if (lane < nb) put(lane, __float_as_uint(bd), bi);
        // (the first unexpanded main entry, in the coordinates before the merge: nothing in front of it or of minP moves)
        const int first_un = first_unexpanded();
        int lo = 0, hi = lm;  // upper bound of bd in the main list
        for (int span = lm; span > 0; span >>= 1) {
            const int mid = (lo + hi) >> 1;
            const float v = __uint_as_float(main[mid < lm ? mid : lm - 1].x);
            const bool act = lo < hi;
            const bool go = act && v <= bd;
            lo = go ? mid + 1 : lo;
            hi = (act && !go) ? mid : hi;
        }
        const int Pk = lane + lo;
        const int minP = __builtin_amdgcn_readlane(Pk, 0);
        const int total = lm + nb;
        const bool isfull = full();
        for (int base = ((lm - 1) / kWave) * kWave; base >= 0 && base + kWave > minP; base -= kWave) {
            const int i = base + lane;
            const bool valid_i = i < lm;
            uint2 e = make_uint2(0u, 0u);
            if (valid_i) e = main[i];
            const float de = __uint_as_float(e.x);
            int l2 = 0, h2 = nb;  // lower bound of de in the buffer
#pragma unroll
            for (int it = 0; it < 7; it++) {
                const int mid = (l2 + h2) >> 1;
                const float v = __uint_as_float(img[mid < nb ? mid : nb - 1].x);
                const bool act = l2 < h2;
                const bool go = act && v < de;
                l2 = go ? mid + 1 : l2;
                h2 = (act && !go) ? mid : h2;
            }
            const int Pe = i + l2;
            if (valid_i && Pe < cap && Pe != i) main[Pe] = e;
        }
        if (lane < nb && Pk < cap) main[Pk] = make_uint2(__float_as_uint(bd), bi);
        if (isfull) {
            // behind `nearest` only what ties its worst can still be expanded (:175-178): that run stays (hnsw_search_kernel's
            // ghosts), as far as the list has room
            const uint32_t wbits = main[ef_l - 1].x;
            int phys = (total < cap ? total : cap) - ef_l;
            const bool more = phys > kWave || total > cap;
            phys = phys > kWave ? kWave : phys;
            const bool tie = lane < phys && main[ef_l + (lane < phys ? lane : 0)].x == wbits;
            const uint64_t nt = ~__builtin_amdgcn_ballot_w64(tie);
            const int run = nt ? __ffsll(static_cast<unsigned long long>(nt)) - 1 : kWave;
            if (run == phys && more) overflow = true;
            lm = ef_l + run;
            pm = ef_l;
        } else {
            lm = total;
            pm = total;
        }
        nb = 0;
        pb = 0;
        bun = 0;
        bi = kExpanded;
        bd = __uint_as_float(0x7f800000u);
        if constexpr (MIRRORED) dirty = true;
        load_front(first_un < minP ? first_un : minP);
        load_tail();
    }
    // The next candidate (:170-178): the smaller of the first unexpanded entries of the two sequences (a tie: the main list's,
    // it is the older one); false when none is left that is <= the worst of `nearest` (nothing behind it can qualify either).
    __device__ __forceinline__ bool pop(uint32_t &node) {
        while (fun == 0 && fbase + kWave < lm) load_front(fbase + kWave);
        if ((fun | bun) == 0) return false;
        const int lf = fun ? __ffsll(static_cast<unsigned long long>(fun)) - 1 : 0;
        const int kb = bun ? __ffsll(static_cast<unsigned long long>(bun)) - 1 : 0;
        const uint32_t dmk = fun ? wl_key(static_cast<uint32_t>(__builtin_amdgcn_readlane(__float_as_int(fd), lf))) : 0xffffffffu;
        const uint32_t dbk = bun ? wl_key(static_cast<uint32_t>(__builtin_amdgcn_readlane(__float_as_int(bd), kb))) : 0xffffffffu;
        const uint32_t nm = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(fi), lf));
        const uint32_t nbf = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(bi), kb));
        const bool take_main = fun != 0 && dmk <= dbk;
        if (full() && (take_main ? dmk : dbk) > worst_k) return false;
        node = take_main ? nm : nbf;
        if (take_main) {
            if (lane == lf) {
                fi |= kExpanded;
                main[fbase + lf].y = fi;
            }
            fun &= fun - 1;
            if constexpr (MIRRORED) {
                if (lane == 0) sc[0] = first_unexpanded();
            }
        } else {
            if (lane == kb) {
                bi |= kExpanded;
                if constexpr (MIRRORED) img[kb].y = bi;
            }
            bun &= bun - 1;
        }
        return true;
    }
    // Admission (:195-204) of the fresh neighbours in `smask` (lane j: distance `dist`, node `id`; adjacency order; already
    // known to be < the worst the expansion found, or `nearest` not full), in two steps: make_room, then admit.  At least one
    // survivor: with none the caller takes neither step.
    //
    // 63 admissions at most between two merges: the buffer has 64 lanes, and the tail window of 64 main entries shows main[pm - 1]
    // through 63 evictions, and 63 admissions cause no more.  64 survivors at once (64 layer-0 slots, all fresh) could push 64
    // main entries out: pm would arrive at tbase and the window's lane 0 be main[pm], an entry that has LEFT `nearest`, read as
    // its worst.  So the first of them goes alone and the window is loaded again behind it; the other 63 follow together (the
    // buffer then holds 64).
    __device__ __forceinline__ void make_room(uint64_t &smask, float dist, uint32_t id) {
        if (nb + __popcll(smask) <= kWave - 1) return;
        compact();
        top_worst();
        if (smask == ~0ull) {
            admit_one(0, dist, id);
            load_tail();
            smask &= smask - 1;
        }
    }
    __device__ __forceinline__ void admit(uint64_t smask, float dist, uint32_t id) {
        if (smask & (smask - 1)) {
            // two or more: one pass in adjacency order decides every admission exactly as the sequential loop would -- a survivor
            // is admitted iff fewer than ef of {`nearest` as the expansion found it, the survivors before it} are <= it (the
            // entries those have pushed out of `nearest` meanwhile were larger than it anyway) -- and collects the merge counts;
            // the admitted ones enter the buffer together (a scatter through its LDS image), and what they push out of `nearest`
            // (:203-204) is the nev largest of its two tails, found by all lanes at once (a merge-path split)
            int before = 0, arank = 0, cball = 0, shb = 0;
            uint64_t am = 0;
            const bool tvalid = tbase + lane < pm;
#pragma unroll 1
            for (uint64_t mm = smask; mm; mm &= mm - 1) {
                const int sv = __ffsll(static_cast<unsigned long long>(mm)) - 1;
                const float ds = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(dist), sv));
                const int cb = __popcll(__builtin_amdgcn_ballot_w64(lane < pb && bd <= ds));
                const int cw = __popcll(__builtin_amdgcn_ballot_w64(tvalid && td <= ds));
                const int bs = __builtin_amdgcn_readlane(before, sv);
                // (smaller than every main entry the tail window shows, and the window does not start at 0: at most ef - 64
                // main + buffer entries are <= it, and fewer than 64 survivors precede it)
                const int tm = (cw == 0 && tbase > 0) ? 0 : tbase + cw;
                const bool adm = tm + cb + bs < ef_l;
                before += (lane > sv && ds <= dist) ? 1 : 0;
                if (adm) {
                    am |= 1ull << sv;
                    shb += (ds < bd) ? 1 : 0;
                    arank += (ds < dist || (ds == dist && sv < lane)) ? 1 : 0;
                    cball = lane == sv ? cb : cball;
                }
            }
            const int nadm = __popcll(am);
            if (nadm == 0) return;
            const bool isadm = (am >> lane) & 1ull;
            if (lane < nb) put(lane + shb, __float_as_uint(bd), bi);
            if (isadm) put(cball + arank, __float_as_uint(dist), id);
            nb += nadm;
            if constexpr (MIRRORED) {
                const uint32_t ex = img[lane].x, ey = img[lane].y;
                bd = lane < nb ? __uint_as_float(ex) : __uint_as_float(0x7f800000u);
                bi = lane < nb ? ey : kExpanded;
            } else {
                const uint2 e = img[lane];
                bd = lane < nb ? __uint_as_float(e.x) : __uint_as_float(0x7f800000u);
                bi = lane < nb ? e.y : kExpanded;
            }
            bun = __builtin_amdgcn_ballot_w64(lane < nb && !(bi & kExpanded));
            const int pbn = pb + nadm;
            const int nev = pm + pbn > ef_l ? pm + pbn - ef_l : 0;
            if (nev) {
                // lane e: e entries leave the main list's tail, nev - e the buffer's.  Right iff what stays is before what
                // leaves: main entries are the older ones (a tie: the buffer entry leaves)
                const int e = lane, eb = nev - lane;
                const bool feas = e <= nev && e <= pm && eb <= pbn;
                const int i_mk = pm - e - 1, i_me = pm - e, i_bk = pbn - eb - 1, i_be = pbn - eb;
                const float m_keep = __uint_as_float(main[i_mk > 0 ? i_mk : 0].x);
                const float m_ev = __uint_as_float(main[(feas && e > 0) ? i_me : 0].x);
                const float b_keep = __uint_as_float(img[(feas && i_bk > 0) ? i_bk : 0].x);
                const float b_ev = __uint_as_float(img[(feas && eb > 0) ? i_be : 0].x);
                const bool ca = i_mk < 0 || eb == 0 || m_keep <= b_ev;
                const bool cb2 = i_bk < 0 || e == 0 || b_keep < m_ev;
                const uint64_t okm = __builtin_amdgcn_ballot_w64(feas && ca && cb2);
                int em = okm ? __ffsll(static_cast<unsigned long long>(okm)) - 1 : -1;
                if (em < 0) {  // (cannot happen for comparable distances; NaNs: one at a time, the sequential rule)
                    em = 0;
                    int pmm = pm, pbb = pbn;
                    for (int t = 0; t < nev; t++) {
                        const uint32_t wmb = pmm > 0 ? main[pmm - 1].x : 0u;
                        const uint32_t wbb = pbb > 0 ? img[pbb - 1].x : 0u;
                        if (pmm > 0 && (pbb == 0 || wl_key(wmb) > wl_key(wbb))) {
                            pmm--;
                            em++;
                        } else {
                            pbb--;
                        }
                    }
                }
                pm -= em;
                pb = pbn - (nev - em);
            } else {
                pb = pbn;
            }
            top_worst();
            if constexpr (MIRRORED) dirty_sc = true;  // (the mirror IS the buffer now)
            return;
        }
        admit_one(__ffsll(static_cast<unsigned long long>(smask)) - 1, dist, id);
    }
    // ONE survivor (lane j): straight into its place
    __device__ __forceinline__ void admit_one(int j, float dist, uint32_t id) {
        const uint32_t djb = static_cast<uint32_t>(__builtin_amdgcn_readlane(__float_as_int(dist), j));
        const uint32_t idj = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(id), j));
        if (full() && wl_key(djb) >= worst_k) return;  // (:195-198, a strict <)
        const float dj = __uint_as_float(djb);
        // behind the buffer entries <= it (ties: admission order; lanes >= nb hold +inf)
        const int r0 = __popcll(__builtin_amdgcn_ballot_w64(bd <= dj));
        const int r = r0 < nb ? r0 : nb;  // (an infinite distance: behind everything)
        const float sd = __uint_as_float(wave_shr1(__float_as_uint(bd)));
        const uint32_t si = wave_shr1(bi);
        bd = lane > r ? sd : (lane == r ? dj : bd);
        bi = lane > r ? si : (lane == r ? idj : bi);
        const uint64_t lowm = (1ull << r) - 1ull;
        bun = (bun & lowm) | ((bun & ~lowm) << 1) | (1ull << r);
        nb++;
        pb++;
        {  // (:203-204) if `nearest` now holds ef + 1, its worst leaves it: the later of the two tails (a tie: the buffer's, it
           // is the younger).  Straight-line: integer selects on the keys, no branch.
            const int over = pm + pb > ef_l ? 1 : 0;
            const int im = pm - 1 - tbase;
            const uint32_t wmb = static_cast<uint32_t>(__builtin_amdgcn_readlane(__float_as_int(td), im > 0 ? im : 0));
            const uint32_t wbb = static_cast<uint32_t>(__builtin_amdgcn_readlane(__float_as_int(bd), pb - 1));
            const int evm = (over && pm > 0 && wl_key(wmb) > wl_key(wbb)) ? 1 : 0;
            pm -= evm;
            pb -= over - evm;
        }
        top_worst();
        if constexpr (MIRRORED) dirty = true;
    }
    // (MIRRORED) after an expansion's admissions: the other waves see the buffer through its mirror
    __device__ __forceinline__ void publish() {
        static_assert(MIRRORED, "only a mirrored list has readers");
        if (dirty) ((uint2 *)img)[lane] = make_uint2(__float_as_uint(bd), bi);  // (a plain store of the whole entry)
        if (dirty || dirty_sc) {
            if (lane == 0) {  // (plain stores: hints, and the LDS takes a wave's stores in order)
                int32_t *const s = (int32_t *)sc;
                s[3] = nb;
                s[1] = lm;
                s[0] = first_unexpanded();
            }
            asm volatile("" ::: "memory");
            dirty = false;
            dirty_sc = false;
        }
    }
    __device__ __forceinline__ int end_level() {
        compact();
        return lm;
    }
};

}  // namespace hg
