/*
 * hnswgpu.h -- C ABI of libhnswgpu.so: the MI355X (gfx950) distance engine behind hnsw-clj's
 * index/search API.  This header is the drop-in boundary: every entry point names the reference
 * interface (file:line under damesek/hnsw-clj) it replaces.  INTEGRATION.md shows the Clojure
 * (Panama FFM / JNI) binding a maintainer adds on the reference side.
 *
 * Conventions
 *  - extern "C", plain pointers and sizes only.  Every function returns 0 on success or a negative
 *    HNSWGPU_E* code; hnswgpu_last_error() returns a thread-local message.  No exception crosses
 *    the boundary.
 *  - Host-pointer entry points: the caller owns every host buffer; the library copies or consumes
 *    it before returning.  `_dev` entry points take DEVICE pointers (e.g. a torch tensor's
 *    data_ptr) plus a hipStream_t passed as void* (NULL = HIP's default stream); they only
 *    enqueue work and do not synchronise.  Calls on different streams are ordered against each
 *    other with events (they share the index's scratch buffers).
 *  - Row ids are dense int32 in [0, n); the String-id <-> row table stays on the Clojure side
 *    (UltraNode.id is a String, src/hnsw/ultra_fast.clj:99).
 *  - Results are ascending by distance; fewer than k results are padded with id -1 / +inf
 *    (the reference returns shorter seqs: test/hnsw/core_test.clj:90-96, ultra_fast.clj:349-351).
 *  - Metrics: COSINE = 1 - dot/(|a||b|), 1.0 when a norm is 0 (ultra_fast.clj:53-95);
 *    L2 = sqrt(sum (a-b)^2), rooted (ultra_fast.clj:43-51); DOT = -dot (ordering key for
 *    simd-optimized/dot-product, simd_optimized.clj:283-293).
 *  - Arithmetic is float32 on the device (the reference is float64): ids identical to the f64
 *    reference order, distances within 1e-4 relative (BASELINE.json north_star).
 *  - An index handle is safe for concurrent *_search calls from several host threads (calls are
 *    serialised on the handle's stream); set_* / build calls must not overlap searches.
 */
#ifndef HNSWGPU_H
#define HNSWGPU_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HNSWGPU_VERSION 104

#define HNSWGPU_COSINE 0
#define HNSWGPU_L2 1
#define HNSWGPU_DOT 2

#define HNSWGPU_OK 0
#define HNSWGPU_EINVAL (-1)   /* bad argument (null pointer, k < 1, dim unsupported ...)       */
#define HNSWGPU_EHIP (-2)     /* HIP runtime error; message has the hipError string            */
#define HNSWGPU_ESTATE (-3)   /* index lacks what the call needs (no graph / no IVF lists)      */
#define HNSWGPU_ENOMEM (-4)   /* host or device allocation failed                               */
#define HNSWGPU_ELIMIT (-5)   /* a documented limit exceeded (dim > 3072, ef > 4096, k > 1024)  */

typedef struct hnswgpu_index hnswgpu_index;

int hnswgpu_version(void);
const char *hnswgpu_last_error(void);
int hnswgpu_device_count(int32_t *count);

/* ---- index lifetime ----------------------------------------------------------------------------
 * Replaces the data-map of the reference indexes: ConcurrentHashMap<String,UltraNode{double[]}>
 * (ultra_fast.clj:99-111) / IVFFlatIndex.data-map (ivf_flat.clj:22-27).  `base` is n x dim float32
 * row-major host memory; it is copied to one contiguous HBM matrix (rows padded to 16 B) and the
 * per-row norms are precomputed on the device (ivf_flat.clj:171-177, simd_optimized.clj:206-216).
 * n == 0 is legal (empty index: every search returns no results, ultra_fast.clj:349-351). */
int hnswgpu_create(const float *base, int64_t n, int32_t dim, int32_t metric, int32_t device,
                   hnswgpu_index **out);
/* Same, from a device-resident n x dim matrix with row stride ld floats (copied). */
int hnswgpu_create_dev(const float *d_base, int64_t n, int32_t dim, int64_t ld, int32_t metric, int32_t device,
                       void *stream, hnswgpu_index **out);
int hnswgpu_destroy(hnswgpu_index *idx);
int hnswgpu_info(const hnswgpu_index *idx, int64_t *n, int32_t *dim, int32_t *metric, int32_t *has_graph,
                 int32_t *nlist);
int hnswgpu_sync(hnswgpu_index *idx);

/* ---- distance seams ------------------------------------------------------------------------------
 * hnswgpu_pair_distance: the :distance-fn signature (fn ^double [^doubles a ^doubles b])
 *   (ultra_fast.clj:43-95, simd_optimized.clj:145-160,283-293), one pair, computed on the device.
 * hnswgpu_batch_distances: simd-optimized/batch-cosine-distances, batch-euclidean-distances
 *   [query vectors] -> distances (simd_optimized.clj:164-184): q vs base rows ids[0..m) (ids NULL =
 *   rows 0..m-1).  This is the gather-dot used per hop inside HNSW (ultra_fast.clj:185-204).
 * hnswgpu_norms: simd-optimized/precompute-norms (simd_optimized.clj:206-216).
 * hnswgpu_exact_knn: bench/compute-exact-knn (src/hnsw/bench.clj:72-84) and
 *   simd-optimized/top-k-distances (simd_optimized.clj:271-280): brute force over the full base. */
int hnswgpu_pair_distance(int32_t metric, const float *a, const float *b, int32_t dim, int32_t device, float *out);
int hnswgpu_batch_distances(hnswgpu_index *idx, const float *q, const int32_t *ids, int32_t m, float *out);
int hnswgpu_norms(hnswgpu_index *idx, float *out_norms);
int hnswgpu_exact_knn(hnswgpu_index *idx, const float *Q, int32_t nq, int32_t k, int32_t *out_ids,
                      float *out_dist);
int hnswgpu_exact_knn_dev(hnswgpu_index *idx, const float *d_Q, int32_t nq, int32_t k, int32_t *d_out_ids,
                          float *d_out_dist, void *stream);

/* ---- HNSW ---------------------------------------------------------------------------------------
 * Graph layout (what UltraGraph's nodes / neighbor HashSets flatten to, ultra_fast.clj:99-111):
 *   levels[n]                node level
 *   l0_adj[n * M0]           layer-0 neighbours, -1 padded, adjacency-array order
 *   up_off[n + 1]            prefix sum of levels: node i's layers 1..levels[i] are the blocks
 *                            up_off[i] .. up_off[i+1]-1 of up_adj
 *   up_adj[up_off[n] * M]    one block of M neighbours (-1 padded) per (node, layer >= 1)
 *   entry, max_level         entry point and its level
 * hnswgpu_set_graph uploads a graph built elsewhere (e.g. by the reference's own insert-single);
 * hnswgpu_hnsw_build builds one on the device (batched insertion; replaces build-index /
 * insert-batch ultra_fast.clj:303-344); hnswgpu_get_graph exports it in the same layout.
 * hnswgpu_hnsw_search replaces search-knn (ultra_fast.clj:346-374) for a batch of queries -- the
 * seam of BatchSearchIndex/search-batch* (api/protocol.clj:58-67) and parallel-search-futures
 * (helper/parallel_search.clj:15-49).  ef is explicit; the reference's value is max(k, 50)
 * (ultra_fast.clj:355): pass ef <= 0 to get it.  stats (optional, nq x 2 int64): distance
 * evaluations and expansions per query.
 * Ties: the reference still expands a candidate whose distance EQUALS the current ef-th distance
 * (ultra_fast.clj:175-178, `<=`).  The traversal kernel keeps up to 32 such evicted-but-tied candidates per
 * query; a query that had more (hundreds of duplicated rows) is repeated on the device, in the same call, with the
 * largest candidate list the LDS holds, so results and counters are the reference's on such data too. */
int hnswgpu_set_graph(hnswgpu_index *idx, const int32_t *levels, const int32_t *l0_adj, int32_t M0,
                      const int64_t *up_off, const int32_t *up_adj, int32_t M, int32_t entry, int32_t max_level);
int hnswgpu_hnsw_build(hnswgpu_index *idx, int32_t M, int32_t ef_construction, int64_t seed);
/* The same with build options.  flags = 0 is hnswgpu_hnsw_build: batched insertion, every node linked to its m closest
 * candidates (insert-single / prune-connections-ultra, ultra_fast.clj:216-299).
 *   HNSWGPU_BUILD_SEQUENTIAL  insert-single itself: one row at a time, the walk starting at min(level, entry-level) with the
 *                             entry point (ultra_fast.clj:247-248), an over-full neighbour pruned at once (:264-266).  The
 *                             graph equals the CPU restatement's (oracle/oracle.c: orc_hnsw_build_ex) edge for edge; one
 *                             launch round trip per row -- the parity mode, not the fast one.
 *   HNSWGPU_BUILD_HEURISTIC   links chosen by get-neighbors-heuristic (src/hnsw/graph.clj:162-198, the builder behind
 *                             README's hnsw.hnsw-search): candidates ascending by (distance, id), one is taken unless it
 *                             is closer to an already taken one than to the node itself -- for the new node's own links
 *                             (from all its ef_construction candidates) and for an over-full neighbour list
 *                             (prune-connections, graph.clj:208-232).  Clusters stay connected to each other: on the
 *                             survey's clustered-normalised 31k x 768 set recall@10 goes from 0.02 (closest-m, at any ef)
 *                             to 0.98.  The pair distances run on the device (heuristic_select_kernel).
 *   HNSWGPU_BUILD_SYMMETRIC   with HEURISTIC: an edge a pruning drops is removed from the other node's list as well
 *                             (graph.clj:226-231)
 *   HNSWGPU_BUILD_EXTEND      with HEURISTIC: extend-candidates? for the new node's own selection (graph.clj:191-195)
 * hnswgpu_hnsw_add inserts with the options the handle's graph was built with (batched).  The index file carries them: a
 * graph that came back through hnswgpu_load keeps its builder.  A graph installed by hnswgpu_set_graph has none: rows
 * added to it are linked to their m closest candidates. */
#define HNSWGPU_BUILD_SEQUENTIAL 1
#define HNSWGPU_BUILD_HEURISTIC 2
#define HNSWGPU_BUILD_SYMMETRIC 4
#define HNSWGPU_BUILD_EXTEND 8
int hnswgpu_hnsw_build_ex(hnswgpu_index *idx, int32_t M, int32_t ef_construction, int64_t seed, int32_t flags);
/* insert-single on a LIVE index (src/hnsw/ultra_fast.clj:216-275, reached by add-vector! src/hnsw/api.clj:30-33 and add!
 * src/hnsw/api/simple.clj:31-42): `m` more rows (m x dim floats) join the base matrix and the installed graph.  Their row
 * ids are n, n + 1, ...; their levels continue the seeded java.util.Random sequence (row i takes its i-th draw: the same
 * `seed` as the build gives the levels a from-scratch build of all rows would draw); they are inserted in batches, by
 * the search kernel and the linker of hnswgpu_hnsw_build, against the CURRENT graph (any graph with M0 = 2 M:
 * hnswgpu_hnsw_build's, or one installed by hnswgpu_set_graph / hnswgpu_load -- its edge distances, which the reference's
 * pruning sorts by (:279-299), are recomputed on the device).  Not concurrent with searches on the same handle (they
 * wait); IVF lists must be built / installed AFTER the rows they cover have been added (a handle that holds lists and
 * no graph grows through hnswgpu_ivf_add). */
int hnswgpu_hnsw_add(hnswgpu_index *idx, const float *rows, int64_t m, int32_t ef_construction, int64_t seed);
/* Rows leave a LIVE graph.  The reference has no delete (pure_hnsw.clj:16 is a todo): what is restated is the list layout;
 * the repair rule is this project's own, and tests/hnsw_remove_model.py is its one specification.  `rows` is m row ids of
 * the handle in host memory, in any order; an id named twice is removed once.  The kept rows are renumbered densely in their
 * old order: the new id of a kept row r is the number of kept rows below r.  *n_after (may be NULL) gets the rows the handle
 * holds afterwards.
 *   - Base rows, norms and the base-order int8 rows with their meta (where the handle has them) are, bit for bit, what
 *     hnswgpu_create(the kept rows in their old order) + hnswgpu_set_rejection_test(same mode) holds: rows and norms are
 *     copied, the int8 rows made again over the moved rows.
 *   - The graph: the kept rows' levels in order, up_off their prefix sum; M, M0 and the builder flags stay.  Every layer's
 *     list of a kept node that loses no member keeps its members in their order under their new ids, -1 padded.
 *   - A list that loses at least one member is selected again from the OLD graph alone -- the adjacency as it stood when
 *     the call began; all lists are repaired from it at once, never from another list's repaired state.  For node u on
 *     layer lc (width w = M0 on layer 0, M above): the candidates are u's kept old neighbours joined with the kept members
 *     of the layer-lc lists of u's removed neighbours, without u, each once (one hop through what left, as FreshDiskANN's
 *     delete consolidation: at most w * w <= 4096 ids); d(u, c) by the traversal's arithmetic on the stored norms;
 *     ascending by (distance, id); then what the handle's builder does to an over-full list: with
 *     HNSWGPU_BUILD_HEURISTIC get-neighbors-heuristic without extend-candidates (prune-connections, graph.clj:208-232),
 *     otherwise -- a graph installed by hnswgpu_set_graph included -- the first min(w, C).  The list is written in
 *     selection order under the new ids, -1 padded; a list whose candidates are all gone becomes empty, which is legal.
 *   - What a repair does NOT do: HNSWGPU_BUILD_SYMMETRIC is not applied -- a repair changes only the list it repairs and
 *     adds no back edge; nothing deeper than one hop is looked at; badly connected nodes are not inserted again.
 *   - The result DEPENDS on how a removal is split over calls: each call repairs through its own removed rows only, so
 *     two calls give the rule applied twice, not the rule applied to the union.  (hnswgpu_ivf_remove and
 *     hnswgpu_lsh_remove are the opposite: their results do not depend on the split.)
 *   - The entry point: kept -> its new id, max_level unchanged; gone -> the kept row of the highest level, the lowest old
 *     id among equals, whose level becomes max_level.  No row left: entry -1, max_level 0, and the handle still has its
 *     (empty) graph with M / M0 / builder flags: searches answer with padding and hnswgpu_hnsw_add grows it again.
 *   - The per-graph verdict of the mode-1 rejection test (hnswgpu_hnsw_rejection_state) is RESET, as wherever a graph is
 *     replaced: the next large launch measures the shrunken graph.
 *   - Everything happens on the device, in one chain on the handle's stream (hnsw_remove_kernels.hpp): only the m ids go
 *     up, and no destination is decided by the order atomics arrive in.  Between the list pass and the gather the host
 *     reads two totals (candidates, lists to repair) to size the candidate arrays -- there is no cap to overflow.
 *   - Failure-atomic, like hnswgpu_hnsw_add: nothing is changed in place, every new array is staged under the handle's
 *     lock with its streams quiesced, and the handle takes them over only after ONE readback -- the new graph for the host
 *     mirrors, and three counts: the rank scan's total must be n - (distinct ids), the new up_off[n_after] must be the
 *     kept rows' levels summed on the host, and the list pass must have seen n_after kept rows (HNSWGPU_EHIP otherwise).
 *     On any failure the staged arrays are freed and the handle is what it was.  Searches from other threads wait and see
 *     the old or the new index.
 *   - Cost and quality, measured on one MI355X (profiles/hnsw_remove.txt: 31,173 x 768 clustered-normalised, heuristic
 *     graph, M 16, ef_construction 200): removing m = 1 / 1,024 / 8,192
 *     scattered rows takes 2.09 / 3.52 / 6.34 ms (host clock around the call, median of five) against 110 / 111 / 115 ms for
 *     hnswgpu_create + hnswgpu_hnsw_build_ex over the kept rows from host memory -- 0.019 / 0.032 / 0.055 of the rebuild.
 *     recall@10 of 1,000 held-out queries against the exact neighbours among the kept rows, repaired / merely compacted /
 *     freshly built: after 10 % of the rows left 0.978 / 0.980 / 0.987 at ef 640 and 0.604 / 0.616 / 0.617 at ef 100 (within
 *     noise of each other); after 40 % left 0.993 / 0.972 / 0.998 at ef 640 and 0.669 / 0.559 / 0.727 at ef 100.  The gap to
 *     the fresh build is the limit of a one-hop repair without back edges.
 * Returns, checked in this order: -1 for a null handle (before m == 0 and before any HIP call), for m < 0, and for null
 * rows with m > 0; 0 for m == 0 (nothing happens, *n_after = n, whatever the handle holds); -3 for a handle without a
 * graph, for a forest, and for one that also holds IVF lists or LSH tables -- the message names which; -1 for an id outside
 * [0, n), checked on the host array before anything is enqueued.  The handle is untouched in every one of these cases.
 * Out of scope: forests, hnswgpu_group_* and sharded.py; handles that hold a graph together with lists or tables; restoring
 * symmetry after a repair; repair deeper than one hop; reinserting badly connected nodes; tombstones. */
int hnswgpu_hnsw_remove(hnswgpu_index *idx, const int32_t *rows, int64_t m, int64_t *n_after);
/* Rows of a LIVE graph take new values.  The reference has no update (its to-do list names "Update existing vectors"); the
 * rule is this project's own -- the two rules above, composed under stable ids -- and tests/hnsw_update_model.py is its one
 * specification.  `ids` is m row ids in host memory, in any order; `rows` is m x dim float32 in host memory; row ids[i]
 * takes the values rows[i].  n, every row id and EVERY ROW'S LEVEL stay as they are: the handle's levels are still the
 * seed's draws by id, and a later hnswgpu_hnsw_add with the build's seed continues the sequence as before.  Let U be the
 * ids of the call.
 *   1. Unlink -- hnswgpu_hnsw_remove's repair with U as the rows that left, but nothing is renumbered.  Every list of a node
 *      outside U that holds no member of U stays as it is.  A list that holds a member of U is selected again from the OLD
 *      graph alone -- the adjacency as it stood when the call began; all lists are repaired from it at once.  For node u on
 *      layer lc (width w = M0 on layer 0, M above): the candidates are u's old neighbours outside U joined with the members
 *      outside U of the layer-lc lists of u's neighbours in U, without u, each once; d(u, c) by the traversal's arithmetic
 *      on the stored norms; ascending by (distance, id); then what the handle's builder does to an over-full list: with
 *      HNSWGPU_BUILD_HEURISTIC get-neighbors-heuristic without extend-candidates, otherwise -- a graph installed by
 *      hnswgpu_set_graph included -- the first min(w, C).  HNSWGPU_BUILD_SYMMETRIC is not applied: a repair changes only the
 *      list it repairs and adds no back edge; nothing deeper than one hop is looked at.  No row of U takes part in any of
 *      these distances: the old and the new base give the same bits.  Every list of every row of U becomes empty: after
 *      this step no edge leads into U or out of it.
 *   2. Values -- base rows of U take the new values, padding columns zero; their norms come from the kernel hnswgpu_create
 *      uses; the base-order int8 rows and meta are made again where the handle has them.  After the call base, norms, int8
 *      rows and meta equal, bit for bit, what hnswgpu_create(base with the new values) +
 *      hnswgpu_set_rejection_test(same mode) holds.
 *   3. The entry point the insertion starts from: outside U -> it stays, with max_level; in U -> hnswgpu_hnsw_remove's rule:
 *      the row outside U of the highest level, the lowest id among equals, whose level becomes the top; every row in U -> the
 *      lowest id of U with its own level, and the insertion starts behind it -- hnswgpu_hnsw_add on an empty graph.
 *   4. Re-insert -- the rows of U in ascending id order AS hnswgpu_hnsw_add INSERTS ROWS: the same search kernel and linker,
 *      the handle's builder flags without HNSWGPU_BUILD_SEQUENTIAL (a graph from hnswgpu_set_graph links to the m closest),
 *      the levels the rows already have, against the graph of step 1; batches by the builder's size rule with
 *      done = (n - |U|) + the rows inserted so far; rows of one batch do not see each other; entry and top move behind a
 *      batch in which a row's level exceeds the top.  Reverse edges, over-full lists and their pruning as add handles them.
 *   - Updating the LAST m rows of a handle equals, edge for edge and bit for bit, hnswgpu_hnsw_remove(those rows) followed
 *     by hnswgpu_hnsw_add(the new values, the same ef_construction, the build's seed).
 *   - The result DEPENDS on how an update is split over calls: two calls give the rule applied twice.  Within one call the
 *     order of `ids` does not matter.
 *   - Updating a row to the values it already has does NOT leave the graph unchanged: the row is unlinked and linked again
 *     (hnswgpu_ivf_update is the opposite: such a row stays where it is).
 *   - The per-graph verdict of the mode-1 rejection test (hnswgpu_hnsw_rejection_state) is RESET, as hnswgpu_hnsw_remove
 *     resets it.
 *   - The device work of the unlink is one chain on the handle's stream (hnsw_update_kernels.hpp, and hnsw_remove_kernels.hpp
 *     instantiated without the renumbering): the mark mask of U, the m uploaded rows and their norms scattered into copies of
 *     base and norms, the pass over all n + up_blocks lists (untouched lists copied, U's lists cleared, candidates counted),
 *     the scan whose two totals size the candidate arrays (no cap to overflow), gather, distances, the per-task sort, the
 *     selection, the scatter under the old ids.  No destination is decided by the order atomics arrive in.
 *   - Failure-atomic, like hnswgpu_hnsw_add: everything is staged under the handle's lock with its streams quiesced.  ONE
 *     readback brings the unlinked graph down for the linker, with three counts the host knows in advance: rows marked
 *     == m, lists cleared == m + the levels of U summed, rows outside U seen == n - m (HNSWGPU_EHIP otherwise, the handle
 *     untouched).  The insertion searches then run against the staged arrays; on any failure the handle is restored to
 *     exactly what it was.  Searches from other threads wait and see the old or the new index.
 *   - Cost and quality, measured on one MI355X (profiles/hnsw_update.txt: 31,173 x 768 clustered-normalised, heuristic
 *     graph, M 16, ef_construction 200; the new values are rows of other clusters): updating m = 1 / 1,024 / 8,192
 *     scattered rows takes 9.2 / 12.7 / 27.2 ms (host clock around the call, median of five) against 107 / 115 / 114 ms for
 *     hnswgpu_create + hnswgpu_hnsw_build_ex over the new base from host memory -- 0.09 / 0.11 / 0.24 of the rebuild -- and
 *     9.4 / 12.1 / 26.8 ms for hnswgpu_hnsw_remove + hnswgpu_hnsw_add of the same rows: the update costs what the pair costs
 *     and keeps ids and levels.  The update was faster than the rebuild at every m measured; the call copies the base once
 *     and its insertion grows with m, so larger shares than 8,192 of 31,173 were not timed.  recall@10 of 1,000 held-out
 *     queries against the exact neighbours in the new base, updated / freshly built / remove + add: after 10 % of the rows
 *     took new values 0.847 / 0.979 / 0.842 at ef 640 and 0.495 / 0.614 / 0.498 at ef 100; after 40 % 0.937 / 0.991 / 0.937
 *     at ef 640 and 0.515 / 0.661 / 0.519 at ef 100.  The update equals remove + add within noise and is BELOW a fresh
 *     build: the rows of a new cluster arrive in few batches whose rows do not see each other (hnswgpu_hnsw_add's batched
 *     insertion), so where recall matters more than the 4-10x in time, or most rows move to new regions, rebuild.
 * Returns, checked in this order, the handle untouched in every case: -1 for a null handle (before m == 0 and before any
 * HIP call); -1 for m < 0; -1 for null ids or rows with m > 0; HNSWGPU_ELIMIT for ef_construction outside [1, 4096], as
 * hnswgpu_hnsw_add; 0 for m == 0 (nothing happens); -3 for a handle without a graph, for a forest, for one that also holds
 * IVF lists or LSH tables, and for a graph with M0 != 2 M -- the message names which; -1 for an id outside [0, n); -1 for an
 * id named twice (the message names both positions) -- both checked on the host array before anything is enqueued.
 * Out of scope: forests; hnswgpu_group_* and sharded.py; handles that hold a graph together with lists or tables; new level
 * draws; repair deeper than one hop; restoring symmetry after the unlink; in-place patching that avoids the per-call copy of
 * the base. */
int hnswgpu_hnsw_update(hnswgpu_index *idx, const int32_t *ids, const float *rows, int64_t m, int32_t ef_construction);
int hnswgpu_graph_sizes(const hnswgpu_index *idx, int32_t *M, int32_t *M0, int64_t *up_blocks, int32_t *entry,
                        int32_t *max_level);
int hnswgpu_get_graph(const hnswgpu_index *idx, int32_t *levels, int32_t *l0_adj, int64_t *up_off,
                      int32_t *up_adj);
int hnswgpu_hnsw_search(hnswgpu_index *idx, const float *Q, int32_t nq, int32_t k, int32_t ef, int32_t *out_ids,
                        float *out_dist, int64_t *stats);
int hnswgpu_hnsw_search_dev(hnswgpu_index *idx, const float *d_Q, int32_t nq, int32_t k, int32_t ef,
                            int32_t *d_out_ids, float *d_out_dist, int64_t *d_stats, void *stream);

/* ---- A forest: several HNSW sub-graphs on one handle, searched in one launch ------------------------
 * The reference's indexes of many small graphs -- partitioned-hnsw (partitioned_hnsw.clj:149-196: every partition searched for
 * k' results, concatenated, stable-sorted, take k) and ivf-hnsw (ivf_hnsw.clj:286-325: the num-probes nearest partitions'
 * graphs searched for 2k each, merged) -- on ONE handle.  The handle's rows are grouped by part: part p is the contiguous
 * range [part_off[p], part_off[p + 1]); the caller permutes its rows and keeps the row -> id table.
 * hnswgpu_set_graph_parts: hnswgpu_set_graph's arrays (adjacency holds handle row ids) + the part tables.  Checked as
 *   hnswgpu_set_graph checks, and: part_off[0] == 0, part_off[nparts] == n, part_off monotone; every edge stays inside its
 *   part; an empty part has part_entry[p] == -1; otherwise part_entry[p] lies in the part, levels[part_entry[p]] >=
 *   part_max_level[p], and no node of the part is above part_max_level[p].  Any violation: HNSWGPU_EINVAL, and the handle
 *   keeps what it had.
 * hnswgpu_hnsw_build_parts: every non-empty part built as hnswgpu_hnsw_build_ex(M, ef_construction, seed, flags) builds a
 *   handle over that part's rows alone -- edge for edge, after the id shift by part_off[p].  The forest is installed once:
 *   on any error the handle keeps what it had.
 * hnswgpu_graph_parts: the part tables (arrays may be NULL to read only nparts); HNSWGPU_ESTATE without a forest.
 * hnswgpu_hnsw_search_parts / _dev: probes is [nq][nprobe] part ids, -1 = skip (as hnswgpu_ivf_search_lists); NULL = every
 *   part in order (nprobe is then the number of parts, the argument is ignored).  Item (q, r) -- query q, its r-th probe p --
 *   holds bit for bit the ids (shifted by part_off[p]: handle rows), distances and stats pair that
 *   hnswgpu_hnsw_search(k_part, ef) returns on a handle over part p's rows alone with part p's graph (ef <= 0: max(k_part,
 *   50)); a skipped probe, an empty part or a part id out of range is an all-padding list (-1 / +inf, stats 0).  The result
 *   is hnswgpu_merge_lists_dev of a query's items in probe order: stable, ties go to the earlier probe, take k (k <= 1024).
 *   stats (optional): [nq][nprobe][2].  All items run in ONE traversal launch (+ the tie repeat pass, per item); the _dev
 *   entry only enqueues on `stream`; the host entry stages one caller's batch (no call combining).
 * On a handle that holds a forest: hnswgpu_get_graph works; hnswgpu_graph_sizes reports entry = -1 and the largest
 *   max_level; hnswgpu_info has_graph = 1; hnswgpu_hnsw_search*, the filtered searches, hnswgpu_hnsw_add, hnswgpu_hnsw_remove and
 *   hnswgpu_save return HNSWGPU_ESTATE; hnswgpu_set_graph / hnswgpu_hnsw_build* replace the forest with a plain graph, and the other way
 *   round.
 * Out of scope: the several-CU kernel for forest launches (the single-query latency of the hybrid indexes: a handful of items
 *   run one workgroup each); save / load, add, filtered search and groups on a forest; a device-side forest builder. */
int hnswgpu_set_graph_parts(hnswgpu_index *idx, const int32_t *levels, const int32_t *l0_adj, int32_t M0, const int64_t *up_off,
                            const int32_t *up_adj, int32_t M, int32_t nparts, const int64_t *part_off, const int32_t *part_entry,
                            const int32_t *part_max_level);
int hnswgpu_hnsw_build_parts(hnswgpu_index *idx, int32_t nparts, const int64_t *part_off, int32_t M, int32_t ef_construction,
                             int64_t seed, int32_t flags);
int hnswgpu_graph_parts(const hnswgpu_index *idx, int32_t *nparts, int64_t *part_off, int32_t *part_entry, int32_t *part_max_level);
int hnswgpu_hnsw_search_parts(hnswgpu_index *idx, const float *Q, int32_t nq, int32_t k_part, int32_t ef, const int32_t *probes,
                              int32_t nprobe, int32_t k, int32_t *out_ids, float *out_dist, int64_t *stats);
int hnswgpu_hnsw_search_parts_dev(hnswgpu_index *idx, const float *d_Q, int32_t nq, int32_t k_part, int32_t ef, const int32_t *d_probes,
                                  int32_t nprobe, int32_t k, int32_t *d_out_ids, float *d_out_dist, int64_t *d_stats, void *stream);

/* ---- IVF-FLAT -------------------------------------------------------------------------------------
 * hnswgpu_ivf_build: build-ivf-flat-index :partition-method :kmeans (ivf_flat.clj:137-211):
 *   k-means++ seeding with java.util.Random(seed) (:32-60), max_iter Lloyd iterations (:92-131),
 *   final assignment, inverted lists in index order.  seed 42 is the reference's.
 * hnswgpu_set_ivf / hnswgpu_get_ivf: import / export centroids (nlist x dim f32), list_off[nlist+1],
 *   list_ids[n] (row ids in list order).
 * hnswgpu_kmeans_assign: assign-to-nearest-centroid for every base row (ivf_flat.clj:79-90):
 *   strict <, lowest index wins ties.
 * hnswgpu_ivf_search: search-ivf-flat (ivf_flat.clj:236-294) with explicit nprobe for a batch of
 *   queries: centroid routing (:261-269), brute-force scan of the probed lists with precomputed
 *   norms (:217-234), merge, take k.  out_probes optional (nq x nprobe list ids).
 *   Two summation orders exist for this call (cosine / dot).  The GEMV order (wave-strided f32 chain + butterfly) serves
 *   EVERY batch size on a handle with the int8 and half-precision copies of its lists (hnswgpu_set_rejection_test 1 / 2
 *   with dim >= 128, the default; k <= 256 -- divided by (mean list length / 1024) on lists longer than 2048 rows on
 *   average: k <= 36 at 7800 rows per list): only the candidates whose bounds can still reach the k nearest are evaluated
 *   at all, and nq queries in one call return bit for bit what nq single calls return.  Without the copies (mode 0,
 *   dim < 128, HNSWGPU_IVF_HALF=0 leaves a boundary of 48) or for k > 256, the GEMV order serves up to 12 (query, list)
 *   pairs per list (nq * nprobe <= 12 * nlist: one GEMV per pair; from 1.5 pairs per list the pairs of a list share one
 *   pass over its rows -- same chain, same bits) and larger batches are grouped by list and scanned by the f32-MFMA tile
 *   kernel (k-ordered f32 chain): both orders are within 1e-6 of the f64 reference, but there a query's distance BITS (and
 *   the order of candidates that tie within that) depend on which side of the boundary its batch falls.  Calls combined from
 *   concurrent host threads never change the kernel a call would get alone.  Euclidean: one arithmetic throughout. */
int hnswgpu_ivf_build(hnswgpu_index *idx, int32_t nlist, int32_t max_iter, int64_t seed);
/* Rows join the inverted lists of a LIVE handle (the IVF side of add-vector! src/hnsw/api.clj:30-33; the reference's
 * IVFFlatIndex is an immutable record, so what is restated is its assignment rule and its list order).
 * `rows` is m x dim float32 host memory; the rows join the base matrix as rows n, n + 1, ..., n + m - 1.  The norms grow
 * with it, and so do the base-order int8 rows if the handle has them.
 *   - Centroids do not move.  Each new row goes to its nearest centroid: strict <, lowest list index wins ties
 *     (assign-to-nearest-centroid, ivf_flat.clj:79-90).  The arithmetic is ONE order at every m -- the GEMV-order scan,
 *     never the MFMA tile path hnswgpu_kmeans_assign may take -- so a row's list never depends on the batch it came in.
 *   - Each list keeps its old members in their old order and receives its new members behind them, ascending by row id
 *     ("inverted lists in index order", :137-211).  m rows in one call or in any split of calls give the same lists.
 *   - After the call everything a search reads equals, bit for bit, what hnswgpu_create(all rows) +
 *     hnswgpu_set_rejection_test(same mode) + hnswgpu_set_ivf(same centroids, merged lists) holds: list offsets, ids,
 *     rows and norms in list order, their int8 and half-precision copies, the list-length bookkeeping, and what
 *     hnswgpu_get_ivf / hnswgpu_save export.  The first-search verdict of a mode-1 handle (hnswgpu_ivf_stream_state) is
 *     kept, not measured again.  A handle whose lists are its base rows in place (identity list_ids) gets list-order
 *     copies of its own once the merged lists are no longer the identity.
 *   - Failure-atomic, like hnswgpu_hnsw_add: every new array is staged under the handle's lock with its streams
 *     quiesced; on any failure the staged arrays are freed and the handle is what it was.  Searches from other threads
 *     wait and then see either the old or the new index.  An allow-mask of a filtered search simply is longer at the
 *     next call; scratch sized by n grows on demand.
 *   - Cost: one pass over the base and the list rows on the device per CALL (copies and re-quantisation; no host pass
 *     over the rows, no upload of old rows) plus nlist workgroups that each read the call's m assignments -- add rows
 *     in batches.
 * Returns (all checked before `rows` is read): HNSWGPU_EINVAL for a null handle, m < 0 or null rows; 0 for m == 0
 * (nothing happens); HNSWGPU_ESTATE without lists, on a handle that holds an HNSW graph (the rows would be missing from
 * the graph) and on a shard (hnswgpu_set_ivf_shard); HNSWGPU_ELIMIT for n + m >= 2^31.
 * Out of scope: a handle with both a graph and lists, hnswgpu_group_*, and sharded.ShardedIVF (rebuild those).
 * hnswgpu_hnsw_add still refuses a handle with lists. */
int hnswgpu_ivf_add(hnswgpu_index *idx, const float *rows, int64_t m);
/* Rows leave the inverted lists of a LIVE handle (the reference's IVFFlatIndex has no remove either; what is restated is
 * again its list order, "inverted lists in index order", ivf_flat.clj:137-211).  The contract is that of hnswgpu_lsh_remove,
 * on lists instead of tables.  `rows` is m row ids of the handle in host memory, in any order; an id named twice is removed
 * once.  The kept rows are renumbered densely in their old order: the new id of a kept row r is the number of kept rows
 * below r.  *n_after (may be NULL) gets the rows the handle holds afterwards.
 *   - Centroids do not move.  Every list keeps its kept members in their order under their new ids; an emptied list stays,
 *     with two equal offsets.
 *   - After the call the handle holds, bit for bit, what hnswgpu_create(the kept rows in their old order) +
 *     hnswgpu_set_rejection_test(same mode) + hnswgpu_set_ivf(same centroids, compacted lists) holds: base, norms, the
 *     base-order int8 rows and their meta where the handle has them, list offsets and ids, rows and norms in list order,
 *     their int8 and half-precision copies, the list-length bookkeeping, and what hnswgpu_get_ivf / hnswgpu_save export.
 *     The first-search verdict of a mode-1 handle (hnswgpu_ivf_stream_state) is kept, not measured again.  A handle whose
 *     lists are its base rows in place (identity list_ids) stays that way: the compacted ids are again the identity.
 *     It is the permanent form of hnswgpu_ivf_search_filtered: a search after the removal finds the rows, under their new
 *     ids, and the distance bits that the filtered search found before it under the mask of the kept rows.
 *   - Everything happens on the device, in one chain on the handle's stream: only the m ids go up, rows and norms are
 *     copied (not computed again), the int8 rows, the int8 tiles and the half copy are made again over the moved rows by
 *     what makes them for fresh lists (their layout depends on position), and every entry's destination is a function of
 *     the mask and the old arrays alone (prefix counts of kept entries), never of the order atomics arrive in.
 *   - Failure-atomic, like hnswgpu_ivf_add: nothing is changed in place, every new array is staged under the handle's
 *     lock with its streams quiesced, and the handle takes them over only after ONE readback -- the new offsets and ids
 *     for the host mirrors, and three counts that must all equal n - (distinct ids): the rank scan's total, the last new
 *     offset and the compacted list entries (HNSWGPU_EHIP otherwise).  On any failure the staged arrays are freed and the
 *     handle is what it was.  Searches from other threads wait and see the old or the new index.  Peak memory: the old
 *     plus the new arrays for the length of the call, as for add.
 *   - Cost: one device copy of the kept rows in base and in list order plus their re-quantisation per CALL, whatever m
 *     is -- remove rows in batches.  Measured on one MI355X (profiles/ivf_remove.txt: 31,173 x 768, 24 lists, mode 1):
 *     1.31 / 1.10 / 1.26 ms for m = 1 / 1,024 / 8,192 against 2.05 / 2.00 / 1.60 ms for the rebuild over the kept rows
 *     from host memory -- faster at every m measured, by less the more rows leave (0.64, 0.55, 0.79 of the rebuild); the
 *     kernels are 0.14 ms of a call, the rest is allocating and freeing the staged arrays and the readback.
 * Returns, checked in this order: -1 for a null handle (before m == 0 and before any HIP call), for m < 0, and for null
 * rows with m > 0; 0 for m == 0 (nothing happens, *n_after = n, whatever the handle holds); -3 for a handle without lists,
 * and for one that also holds an HNSW graph, a forest or LSH tables, and for a shard (hnswgpu_set_ivf_shard) -- those
 * would keep the old numbering; the message names which; -1 for an id outside [0, n), checked on the host array before
 * anything is enqueued.  The handle is untouched in every one of these cases.  Removing every row is legal: it leaves the
 * empty handle with lists that hnswgpu_ivf_search answers with padding, and hnswgpu_ivf_add can grow it again.
 * Out of scope: hnswgpu_group_*, sharded.ShardedIVF and shards (rebuild those); handles with both a graph and lists, and
 * forests (a plain graph alone shrinks through hnswgpu_hnsw_remove); moving centroids or re-clustering after heavy removal.
 * hnswgpu_lsh_remove still refuses a handle with lists. */
int hnswgpu_ivf_remove(hnswgpu_index *idx, const int32_t *rows, int64_t m, int64_t *n_after);
/* Rows of a LIVE handle with inverted lists take new values under their ids ("Update existing vectors", the open item of the
 * reference's to-do list, README.md:172-176; its IVFFlatIndex is an immutable record, so what is restated is its assignment
 * rule and its list order).  `ids` is m row ids of the handle in host memory, in any order; `rows` is m x dim float32 host
 * memory; row ids[i] takes the values rows[i].  n, every row id and the centroids stay as they are -- unlike
 * hnswgpu_ivf_remove + hnswgpu_ivf_add, which hand the row a new id and shift every id above it.
 *   - Assignment.  Each updated row is assigned to its nearest centroid by its NEW values: strict <, lowest list index wins
 *     ties (assign-to-nearest-centroid, ivf_flat.clj:79-90).  The arithmetic is the one order hnswgpu_ivf_add uses at every m
 *     -- the GEMV-order scan, never the MFMA tile path -- so a row's list never depends on the batch it was updated in.
 *   - Stayers.  A row whose nearest centroid is the list it already sits in keeps its list POSITION; only its values, its
 *     norm and their compact copies change.  Updating rows to the values they already have changes nothing, bit for bit.
 *   - Movers.  A row whose nearest centroid is another list leaves its old list, which closes up (the remaining members keep
 *     their order), and joins the new one behind the members that remain there, ascending by row id among the call's movers:
 *     new list l = (old members of l in their old order, without the movers that left) ++ (the call's movers into l,
 *     ascending by row id).  A list every member of which leaves stays, with two equal offsets; an empty list may receive its
 *     first rows.  (tests/ivf_update_model.py states the rule in numpy.)
 *   - After the call everything a search reads equals, bit for bit, what hnswgpu_create(the base with the new values) +
 *     hnswgpu_set_rejection_test(same mode) + hnswgpu_set_ivf(same centroids, the lists of the rule) holds: base, norms, the
 *     base-order int8 rows and their meta where the handle has them, list offsets and ids, rows and norms in list order,
 *     their int8 tiles and the half copy, the list-length bookkeeping, and what hnswgpu_get_ivf / hnswgpu_save export.  The
 *     first-search verdict of a mode-1 handle (hnswgpu_ivf_stream_state) is kept, not measured again.  A handle whose lists
 *     are its base rows in place (identity list_ids) stays so exactly when the new list_ids are again the identity, and gets
 *     list-order copies of its own otherwise.
 *   - The result DEPENDS on how an update is split over calls: the movers of a later call stand behind the movers of an
 *     earlier one, whatever their ids -- two calls give the rule applied twice, not the rule applied to the union
 *     (hnswgpu_hnsw_remove's caveat, not the independence of hnswgpu_ivf_add).  Within one call the order of `ids` does not
 *     matter.
 *   - Everything happens on the device, in one chain on the handle's stream: the m ids (sorted on the host: slot s of the
 *     call is the s-th smallest id) and the m rows go up once; norms by the kernel hnswgpu_create uses; every destination is
 *     a function of the old arrays and the call alone (prefix counts of the positions that remain, a mover's stable rank in
 *     slot order), never of the order atomics arrive in.
 *   - Failure-atomic, like hnswgpu_ivf_add and hnswgpu_ivf_remove: nothing is changed in place, every new array is staged
 *     under the handle's lock with its streams quiesced, and the handle takes them over only after ONE readback -- the new
 *     offsets and ids for the host mirrors, and a gate of counts: the last new offset == n, positions that left == positions
 *     that joined == movers, stayers + movers == m (HNSWGPU_EHIP otherwise).  On any failure the staged arrays are freed and
 *     the handle is what it was.  Searches from other threads wait and see the old or the new index.  Peak memory: the old
 *     plus the new arrays for the length of the call.
 *   - Cost: one device copy of the base and of the list rows plus their re-quantisation per CALL, whatever m is -- update
 *     rows in batches.  Measured on one MI355X (profiles/ivf_update.txt: 31,173 x 768, 24 lists, mode 1): 0.99 / 1.23 /
 *     1.99 ms for m = 1 / 1,024 / 8,192 scattered rows against 2.05 / 2.06 / 2.06 ms for the rebuild over the base with
 *     the new values from host memory -- faster at every m measured, by less the more rows a call carries (0.48, 0.60, 0.96
 *     of the rebuild) -- and against 1.95 / 2.24 / 2.72 ms for hnswgpu_ivf_remove + hnswgpu_ivf_add of the same rows, which
 *     loses the ids; the device chain is 0.19 / 0.21 / 0.35 ms of a call, the rest is the upload of the rows, allocating
 *     and freeing the staged arrays and the readback.
 * Returns, checked in this order, the handle untouched in every case: -1 for a null handle (before m == 0 and before any HIP
 * call), for m < 0, and for null ids or rows with m > 0; 0 for m == 0 (nothing happens); -3 for a handle without lists, for
 * one that also holds an HNSW graph, a forest or LSH tables (their copies of the row would go stale) and for a shard
 * (hnswgpu_set_ivf_shard); the message names which; -1 for an id outside [0, n) and for an id named twice (two values for one
 * row have no defined winner), both checked on the host array before anything is enqueued; -1 for a new row with no nearest
 * centroid (NaN).
 * Out of scope: handles with both a graph and lists (LSH tables take new values through hnswgpu_lsh_update, a plain graph
 * through hnswgpu_hnsw_update), forests, hnswgpu_group_*,
 * sharded.ShardedIVF and shards (rebuild those); a plain handle without lists; moving centroids or re-clustering after heavy
 * drift; in-place patching that avoids the per-call copy of the base and the list rows. */
int hnswgpu_ivf_update(hnswgpu_index *idx, const int32_t *ids, const float *rows, int64_t m);
int hnswgpu_set_ivf(hnswgpu_index *idx, const float *centroids, int32_t nlist, const int64_t *list_off,
                    const int32_t *list_ids);
int hnswgpu_get_ivf(const hnswgpu_index *idx, float *centroids, int64_t *list_off, int32_t *list_ids);
int hnswgpu_kmeans_assign(hnswgpu_index *idx, const float *centroids, int32_t nlist, int32_t *out_assign,
                          float *out_dist);
int hnswgpu_kmeanspp(hnswgpu_index *idx, int32_t nlist, int64_t seed, int32_t *out_rows);
/* compute-centroid (ivf_flat.clj:66-77, lightning.clj:24-35) for caller-given lists: f64 mean in list order,
 * stored f32; an empty list yields the zero vector (lightning.clj:118-120). */
int hnswgpu_list_means(hnswgpu_index *idx, int32_t nlist, const int64_t *list_off, const int32_t *list_ids,
                       float *out_centroids);
int hnswgpu_ivf_search(hnswgpu_index *idx, const float *Q, int32_t nq, int32_t k, int32_t nprobe,
                       int32_t *out_ids, float *out_dist, int32_t *out_probes);
int hnswgpu_ivf_search_dev(hnswgpu_index *idx, const float *d_Q, int32_t nq, int32_t k, int32_t nprobe,
                           int32_t *d_out_ids, float *d_out_dist, void *stream);
/* Same scan with caller-chosen lists instead of centroid routing: probes[nq][nprobe] list ids
 * (-1 = skip).  This is search-ivf-flat's :use-centroids false path (the :turbo mode's random
 * partitions, ivf_flat.clj:243-251,271-272) and lightning's partition scan (lightning.clj:144-187). */
int hnswgpu_ivf_search_lists(hnswgpu_index *idx, const float *Q, int32_t nq, int32_t k, int32_t nprobe,
                             const int32_t *probes, int32_t *out_ids, float *out_dist);

/* ---- one IVF index over several GPUs --------------------------------------------------------------------
 * The reference shards an index with threads: split, search every part, concatenate, sort, take k
 * (ann/partition/partitioned_hnsw.clj:149-196).  For IVF-FLAT the split that keeps ONE index is by inverted list:
 * the centroid table is replicated (nlist x dim), every WHOLE list lives on exactly one GPU, every GPU routes a
 * query to the same nprobe lists (ivf_flat.clj:261-269) and scans the probed lists it holds (:281-288); the
 * per-GPU top-k lists are all-gathered and merged (:291-294).
 * hnswgpu_set_ivf_shard: like hnswgpu_set_ivf on a handle whose base holds only this shard's rows; lists the
 *   shard does not hold have list_off[l] == list_off[l+1].  global_list_len[l] = rows of list l in the WHOLE index:
 *   a search then numbers its candidates by their position in the candidate stream of the whole index.
 * hnswgpu_ivf_search_shard_dev: hnswgpu_ivf_search_dev plus d_out_order[nq][k] (uint32, 0xffffffff padded): that
 *   position.  On an ordinary index (hnswgpu_set_ivf / hnswgpu_ivf_build) it is the position in the index's own stream.
 * hnswgpu_merge_keyed_dev: [nshard][nq][k] (global id, distance, order) -> [nq][k] ascending by (distance, order):
 *   bit for bit the result (ids, distances, tie order) of searching the unsharded index with the same batch.
 * hnswgpu_list_sums: the f64 column sums of compute-centroid (ivf_flat.clj:66-77) for caller-given lists, without
 *   the division -- one shard's contribution to a Lloyd update over a row-sharded base (sums of all shards are
 *   added, e.g. by an RCCL all-reduce, then divided by the global member count).  out_sums: nlist x dim doubles. */
int hnswgpu_set_ivf_shard(hnswgpu_index *idx, const float *centroids, int32_t nlist, const int64_t *list_off,
                          const int32_t *list_ids, const int64_t *global_list_len);
/* Mode-1 handles measure, at their first IVF search, what the int8 bounds separate on their rows, and keep the survivor
 * stream only where it helps (the verdict chooses the kernel path, hence -- for cosine / dot batches past the tile
 * boundary -- the summation order).  The shards of ONE index must share ONE verdict: hnswgpu_ivf_stream_state measures
 * now (if it has not yet) and reports it (1 = stream off), hnswgpu_ivf_set_stream_state installs a verdict without
 * measuring.  hnswgpu_group_set_ivf and sharded.ShardedIVF take the OR over the shards and push it to every member.
 * A shard also decides everything that depends on the mean list length (largest k the stream serves, sample sizes) from
 * the WHOLE index's list lengths (global_list_len), not from the rows it holds. */
int hnswgpu_ivf_stream_state(hnswgpu_index *idx, int32_t *off);
int hnswgpu_ivf_set_stream_state(hnswgpu_index *idx, int32_t off);
int hnswgpu_ivf_search_shard_dev(hnswgpu_index *idx, const float *d_Q, int32_t nq, int32_t k, int32_t nprobe,
                                 int32_t *d_out_ids, float *d_out_dist, uint32_t *d_out_order, void *stream);
int hnswgpu_merge_keyed_dev(int32_t device, const int32_t *d_ids, const float *d_dist, const uint32_t *d_order,
                            int32_t nshard, int32_t nq, int32_t k, int32_t *d_out_ids, float *d_out_dist, void *stream);
int hnswgpu_list_sums(hnswgpu_index *idx, int32_t nlist, const int64_t *list_off, const int32_t *list_ids,
                      double *out_sums);

/* ---- multi-GPU merge --------------------------------------------------------------------------------
 * Merge `nshard` per-shard top-k lists (what RCCL all-gather delivers) into the global top-k:
 * the partitioned_hnsw.clj:171-196 gather/sort/take-k step.  d_ids/d_dist: [nshard][nq][k] device
 * arrays of GLOBAL ids (-1 padded) and distances; ties keep the lower shard first. */
int hnswgpu_merge_topk_dev(int32_t device, const int32_t *d_ids, const float *d_dist, int32_t nshard, int32_t nq,
                           int32_t k, int32_t *d_out_ids, float *d_out_dist, void *stream);

/* Same merge with different input and output widths: [nshard][nq][k_in] lists -> [nq][k_out].  This is
 * partitioned-hnsw's "k-per-partition results from every partition, sort, take k"
 * (partitioned_hnsw.clj:149-196, :201-231) and ivf-hnsw's "2k from every probed partition graph, sort,
 * take k" (hybrid/ivf_hnsw.clj:312-325). */
int hnswgpu_merge_lists_dev(int32_t device, const int32_t *d_ids, const float *d_dist, int32_t nshard, int32_t nq,
                            int32_t k_in, int32_t k_out, int32_t *d_out_ids, float *d_out_dist, void *stream);

/* ---- re-rank and dense distances --------------------------------------------------------------------
 * hnswgpu_rerank: per query, exact distances to its own candidate rows cand[q][0..m) (-1 or out-of-range
 * = skipped), STABLE ascending sort (ties keep the candidate order, like Collections/sort), first k.
 * Replaces P-HNSW's refine phase (ann/dimreduct/pcaf.clj:239-253), search-knn's final re-rank of the
 * layer-0 result (ultra_fast.clj:362-370) and top-k-distances (simd_optimized.clj:271-280).
 * Arithmetic: the gather order (wave-strided f32 fma chain + butterfly), as hnswgpu_batch_distances. */
int hnswgpu_rerank(hnswgpu_index *idx, const float *Q, int32_t nq, const int32_t *cand, int32_t m, int32_t k,
                   int32_t *out_ids, float *out_dist);
int hnswgpu_rerank_dev(hnswgpu_index *idx, const float *d_Q, int32_t nq, const int32_t *d_cand, int32_t m,
                       int32_t k, int32_t *d_out_ids, float *d_out_dist, void *stream);
/* out[q * n + row] = distance(query q, base row) for every row: batch-cosine-distances
 * (simd_optimized.clj:176-184) over a whole query batch, and -- on an index whose rows are a projection
 * matrix with metric DOT -- P-HNSW's project-vector-simd (pcaf.clj:47-80; out = -projection).
 * Cosine / dot with nq >= 16 runs on the MFMA tile kernel (tile order), otherwise the GEMV kernel. */
int hnswgpu_dense_distances(hnswgpu_index *idx, const float *Q, int32_t nq, float *out);
int hnswgpu_dense_distances_dev(hnswgpu_index *idx, const float *d_Q, int32_t nq, float *d_out, void *stream);

/* ---- filtered search ----------------------------------------------------------------------------------------
 * FilterableIndex/search-knn-filtered* (src/hnsw/api/protocol.clj:34-41) and its default, default-filtered-search
 * (protocol.clj:97-102: search 3k, keep what passes the predicate, take k), with the predicate evaluated by the caller
 * into ONE allow-mask per call, shared by the call's queries like the reference's one filter-fn per call:
 *   allow: (n + 31) / 32 words; row i may be returned iff (allow[i >> 5] >> (i & 31)) & 1.  Bits at positions >= n are
 *   ignored.  The mask is an argument, not handle state: nothing is kept or persisted, and after hnswgpu_hnsw_add the
 *   next call simply brings a longer mask.  A null mask is an error (-1); n == 0: the host entry points behave as the
 *   unfiltered ones do.
 * hnswgpu_exact_knn_filtered (protocol.clj:34-41,97-102): the k nearest of the PASSING rows, exact, for every metric --
 *   the mask is compacted into the ascending list of passing row ids and exactly those rows are scanned, each fetched
 *   once per group of queries.  Distances in the gather order (wave-strided f32 fma chain + butterfly, the bits of
 *   hnswgpu_rerank / hnswgpu_batch_distances) at EVERY batch size -- no matrix-core order: a query's bits never depend
 *   on its batch.  Ties go to the lower row id; fewer than k passing rows: -1 / +inf padding.  k <= 1024.
 *   The _dev entry reads the number of passing rows (8 bytes) back once, between the compaction's scan and its scatter,
 *   and the calling thread waits for `stream` there: unlike the other _dev entry points it does synchronise, once.
 * hnswgpu_hnsw_search_filtered (protocol.clj:34-41,97-102): the traversal of hnswgpu_hnsw_search, untouched -- same
 *   list, expansions and stats.  With ef' the effective ef (ef <= 0: max(k, 50); at least k) and kk = min(ef', 1024), the
 *   result is the first k passing entries among the first kk entries of the traversal's result list, in list order,
 *   -1 / +inf padded.  ef' = 3k is default-filtered-search itself; a larger ef looks further; an all-ones mask returns
 *   hnswgpu_hnsw_search's results bit for bit.  The host entry stages one caller's batch (it is not combined with
 *   concurrent callers: their masks differ). */
int hnswgpu_exact_knn_filtered(hnswgpu_index *idx, const float *Q, int32_t nq, int32_t k, const uint32_t *allow,
                               int32_t *out_ids, float *out_dist);
int hnswgpu_exact_knn_filtered_dev(hnswgpu_index *idx, const float *d_Q, int32_t nq, int32_t k, const uint32_t *d_allow,
                                   int32_t *d_out_ids, float *d_out_dist, void *stream);
int hnswgpu_hnsw_search_filtered(hnswgpu_index *idx, const float *Q, int32_t nq, int32_t k, int32_t ef, const uint32_t *allow,
                                 int32_t *out_ids, float *out_dist, int64_t *stats);
int hnswgpu_hnsw_search_filtered_dev(hnswgpu_index *idx, const float *d_Q, int32_t nq, int32_t k, int32_t ef,
                                     const uint32_t *d_allow, int32_t *d_out_ids, float *d_out_dist, int64_t *d_stats,
                                     void *stream);
/* One allow-mask per QUERY of a batch: the reference's callers are many threads, each with one query and its own filter-fn
 *   (protocol.clj:34-41), and a service with per-user visibility brings one predicate per query.
 *   allow_each: [nq][W] words, W = (n + 31) / 32, row-major; row q is query q's mask in exactly the format and meaning of
 *   `allow` above (row i may be returned for q iff its bit is set in row q; bits at positions >= n are ignored; an argument,
 *   never handle state).  A null mask is -1, nq == 0 is 0, n == 0: the host entries fill the padding; k <= 1024; a handle
 *   that holds a forest is -3, as for every search.
 * hnswgpu_exact_knn_filtered_each: result row q is, in ids and distance bits, what
 *   hnswgpu_exact_knn_filtered(idx, Q + q * dim, 1, k, allow_each + q * W, ...) returns: gather order at every batch size,
 *   ties to the lower row id, -1 / +inf padding where fewer than k of query q's OWN rows pass (however many pass for other
 *   queries of the batch), and never a row whose bit is clear for q.  Queries are served in the groups of the single-mask
 *   call (32 / 16 / 8 consecutive queries by row length); a group walks the UNION of its queries' passing rows, fetches a
 *   union row once and finishes a distance only for the queries that allow it -- so callers that sort a batch by mask
 *   (equal masks adjacent) get the single-mask call's cost, and no batch fetches more than nq single calls would.
 *   The _dev entry reads the groups' passing counts (8 bytes per query group, one copy) back once and the calling thread
 *   waits for `stream` there, as hnswgpu_exact_knn_filtered_dev does.  The dense scratch of a slice of groups is bounded
 *   by HNSWGPU_TUNE_FILTER_EACH_MB.
 * hnswgpu_hnsw_search_filtered_each: the traversal of hnswgpu_hnsw_search, untouched; result row q equals
 *   hnswgpu_hnsw_search_filtered with mask q; stats are the unfiltered traversal's.  The _dev entry only enqueues.
 * The host entries stage one caller's batch and take no part in the call combiner.
 * Out of scope: combining concurrent single-query filtered callers into one _each launch (it would change the path of the
 *   existing entry points); forests, groups and shards.  (The IVF list scan's _each form: below, behind
 *   hnswgpu_ivf_search_filtered.) */
int hnswgpu_exact_knn_filtered_each(hnswgpu_index *idx, const float *Q, int32_t nq, int32_t k, const uint32_t *allow_each,
                                    int32_t *out_ids, float *out_dist);
int hnswgpu_exact_knn_filtered_each_dev(hnswgpu_index *idx, const float *d_Q, int32_t nq, int32_t k,
                                        const uint32_t *d_allow_each, int32_t *d_out_ids, float *d_out_dist, void *stream);
int hnswgpu_hnsw_search_filtered_each(hnswgpu_index *idx, const float *Q, int32_t nq, int32_t k, int32_t ef,
                                      const uint32_t *allow_each, int32_t *out_ids, float *out_dist, int64_t *stats);
int hnswgpu_hnsw_search_filtered_each_dev(hnswgpu_index *idx, const float *d_Q, int32_t nq, int32_t k, int32_t ef,
                                          const uint32_t *d_allow_each, int32_t *d_out_ids, float *d_out_dist,
                                          int64_t *d_stats, void *stream);
/* hnswgpu_ivf_search_filtered (search-ivf-flat, src/hnsw/ann/partition/ivf_flat.clj:236-294, behind
 *   FilterableIndex/search-knn-filtered*, protocol.clj:34-41): the allow-mask through the list scan, instead of
 *   default-filtered-search's "search 3k, drop, keep k" (protocol.clj:97-102), which returns about 3k * p / n rows when p of n
 *   rows pass and reads every row of every probed list whatever the mask says.  Routing is hnswgpu_ivf_search's
 *   (ivf_flat.clj:261-269) and does not see the mask; out_probes (optional, [nq][nprobe], -1 padded) is what that call
 *   reports.  Result: the query's candidate stream -- the probed lists concatenated in probe order, each in list order
 *   (:281-288) -- with the rows whose bit is clear dropped, the k nearest of the rest ascending by (distance, position in
 *   the stream), -1 / +inf padded when fewer than k pass.  Only the passing rows of the probed lists are read.  `allow` is
 *   the mask above: indexed by ROW id, not by list position.  k, nprobe and nq are checked as hnswgpu_ivf_search checks
 *   them; a handle without lists is -3.
 *   Distances in the gather order (wave-strided f32 fma chain + butterfly: the bits of hnswgpu_rerank and
 *   hnswgpu_exact_knn_filtered) at EVERY batch size and for every metric, behind a routing in the same order -- never the
 *   matrix-core tile order: a query's bits depend neither on its batch nor on the rejection mode, the handle's first-search
 *   measurement (not triggered, not read) or the presence of the int8 / half copies of the lists.  An all-ones mask returns
 *   hnswgpu_ivf_search's ids and distance bits wherever that call runs in this order: Euclidean always, cosine / dot at
 *   one query, and every batch on a handle with the compact copies.
 *   The _dev entry enqueues only and does NOT synchronise: the list of passing positions is sized by the number of list
 *   positions and nothing is read back.  The host entry stages one caller's batch (it is not combined with concurrent
 *   callers: their masks differ).
 *   One handle only.  hnswgpu_group_* and a set of hnswgpu_set_ivf_shard handles are out of scope: their members number
 *   rows locally, and a mask over the rows of the whole index needs a split per member, which is the caller's to make. */
int hnswgpu_ivf_search_filtered(hnswgpu_index *idx, const float *Q, int32_t nq, int32_t k, int32_t nprobe,
                                const uint32_t *allow, int32_t *out_ids, float *out_dist, int32_t *out_probes);
int hnswgpu_ivf_search_filtered_dev(hnswgpu_index *idx, const float *d_Q, int32_t nq, int32_t k, int32_t nprobe,
                                    const uint32_t *d_allow, int32_t *d_out_ids, float *d_out_dist, void *stream);
/* hnswgpu_ivf_search_filtered_each: one allow-mask per QUERY through the list scan.  allow_each is the [nq][W] array of the
 *   _each calls above (W = (n + 31) / 32, row-major, row q is query q's mask in ROW-id space, bits at positions >= n are
 *   ignored, an argument and never handle state).  Result row q is, in ids and distance bits, what
 *   hnswgpu_ivf_search_filtered(idx, Q + q * dim, 1, k, nprobe, allow_each + q * W, ...) returns: the unfiltered routing
 *   in the gather order, distances in the gather order, ascending by (distance, position in the UNFILTERED candidate
 *   stream), -1 / +inf padded where fewer than k of query q's OWN rows pass, and never a row whose bit is clear for q.
 *   out_probes (host entry, optional) is what the single-mask call reports, -1 padded when nprobe > nlist.  A null idx or a
 *   null mask is -1, arguments are checked as hnswgpu_ivf_search checks them, nq == 0 is 0, n == 0 behaves as the
 *   unfiltered call, a handle without lists is -3.
 *   How: no list-order mask and no compaction.  The scan walks the UNFILTERED probed lists in chunks the host plans from
 *   the list lengths; of every 64 list positions a wave reads the row ids, tests each row's bit in its query's mask, and
 *   queues the passing positions; only their f32 rows are fetched.  Per probed position that is 4 bytes of list ids and
 *   a gathered mask word -- the price of having no per-query compaction, where the single-mask call reads nothing for a
 *   failing position.  The scratch is that of an unfiltered scan of the batch and does not grow with nq x n.
 *   The _dev entry only enqueues: it does NOT synchronise and reads nothing back.  The host entry stages one caller's
 *   batch, masks included, and takes no part in the call combiner.  One handle only, as the single-mask call. */
int hnswgpu_ivf_search_filtered_each(hnswgpu_index *idx, const float *Q, int32_t nq, int32_t k, int32_t nprobe,
                                     const uint32_t *allow_each, int32_t *out_ids, float *out_dist, int32_t *out_probes);
int hnswgpu_ivf_search_filtered_each_dev(hnswgpu_index *idx, const float *d_Q, int32_t nq, int32_t k, int32_t nprobe,
                                         const uint32_t *d_allow_each, int32_t *d_out_ids, float *d_out_dist, void *stream);

/* ---- persistence ------------------------------------------------------------------------------------------
 * One flat binary file (header + plain arrays; layout in hnsw-clj_amd/csrc/persist.hip) with the base
 * vectors, the graph and the IVF lists -- replaces helper/index-io's save-index / load-index, an EDN
 * pr-str of every node (src/hnsw/helper/index_io.clj:10-80) and api/save, api/load-index which throw
 * (src/hnsw/api.clj:40-50).  String ids are the caller's to store.  load judges the header against the documented limits
 * and the size of the file before it reads the body (unknown flag or builder bits are a corrupt header, not ignored), and
 * re-validates the graph and the lists: a damaged file is an error code, never a search over it.  The header's last word
 * holds the HNSWGPU_BUILD_* flags of the graph, so a loaded graph grows (hnswgpu_hnsw_add) as the saved one would have;
 * files from before the word had a meaning hold 0 there and load as they did (the version stays 1).  Saving what was loaded
 * gives the same bytes. */
int hnswgpu_save(hnswgpu_index *idx, const char *path);
int hnswgpu_load(const char *path, int32_t device, hnswgpu_index **out);

/* ---- measurement --------------------------------------------------------------------------------------
 * With profiling on, the dominant kernel of each search call is bracketed by hipEvents on the
 * launch stream.  which: 0 = IVF list scan, 1 = HNSW traversal, 2 = k-means assignment scan.
 * Returns the accumulated kernel ms and launch count since the last reset (forces a stream sync). */
int hnswgpu_set_profiling(hnswgpu_index *idx, int32_t on);
/* Process-wide counters of the kernel variants launches have taken since the library was loaded -- so that a test (or a
 * benchmark line) can say WHICH path produced the results it checked, not only that the rule would have chosen it. */
#define HNSWGPU_COUNT_BOUNDS_TWO_BLOCKS 0 /* IVF bounds pass with two 32-query column blocks per staged row (stream_bounds_kernel<.., QB = 2>) */
#define HNSWGPU_COUNT_HNSW_SOLO 1         /* small HNSW launches that spread a query over several CUs (solo_kernels.hpp) */
#define HNSWGPU_COUNT_HNSW_HELPERS 2      /* small HNSW launches of the round-2 helper kernel */
#define HNSWGPU_COUNT_HNSW_REJECTION 3    /* HNSW traversal launches with the int8 rejection test on */
#define HNSWGPU_COUNT_HNSW_PLAIN 4        /* ... and with every neighbour evaluated in f32 */
#define HNSWGPU_COUNT_HNSW_WAVE 5         /* large HNSW launches on the one-wave-per-query kernel with the admission buffer (wave_kernels.hpp) */
#define HNSWGPU_COUNT_ROUTE_TAIL_WAVES 6   /* IVF routing tails launched with one wave per query (ivf_route_tail_wave_kernel) */
#define HNSWGPU_COUNT_HNSW_ORDERED 7       /* ... of those, launches that dealt their queries in the order of their nearest pivot row (HNSWGPU_TUNE_HNSW_ORDER) */
#define HNSWGPU_COUNT_FILTERED_EACH_GROUPS 8 /* query groups served by the one-mask-per-query group scan (filtered_group_kernel<.., EACH>), added per launch */
#define HNSWGPU_COUNT_N 9
int hnswgpu_launch_count(int32_t which, int64_t *out);
/* The HNSW traversal decides most neighbours (those that cannot enter a full result list, ultra_fast.clj:195-198) from
 * an int8 copy of the rows: a lower bound of the distance that is already >= the list's worst needs no f32 row
 * (hnsw-clj_amd/csrc/kernels.hpp: quantize_rows_kernel; results and counters are unchanged by construction).  The
 * traversals code the QUERY in 16 bits (it sits in registers; kernels.hpp: Query16): hnswgpu_hnsw_rejection_bounds, below,
 * returns THEIR bounds.  This entry returns the bounds of the same rows with the query in int8 as well -- the form the
 * IVF bounds pass uses, and the lower side of hnswgpu_distance_bounds bit for bit -- for query q[dim] against rows
 * ids[0..m): out[i] <= the distance hnswgpu_batch_distances reports for the same pair, NaN where the test abstains -- so
 * the property can be checked from outside.
 * hnswgpu_set_rejection_test: mode 0 = off (no int8 copy is made: saves n * dim bytes; the bounds entry then fails),
 * 1 = launches of at least two queries per CU, where the traversal is bandwidth-bound, and only for dim >= 128 (an int8
 * row of a shorter vector saves no cache line) (default), 2 = every launch, every dim.  The same setting decides whether
 * the IVF lists get their int8 copy (and with it the half-precision copy, below) for the bounds pass of the list scan;
 * in mode 1 the first IVF search of a handle measures once what those bounds separate on its rows (32 list rows as
 * queries) and keeps the bounds pass only if it leaves less than a quarter of the candidates -- on rows without cluster
 * structure (i.i.d. gaussian) it leaves everything, and the handle takes the plain f32 scans instead; mode 2 forces it
 * (every batch size; k <= 256, fewer on very long lists: see hnswgpu_ivf_search).
 * HNSWGPU_PREFILTER=<mode> in the environment sets the default of new handles.  Results never depend on the mode. */
int hnswgpu_rejection_bounds(hnswgpu_index *idx, const float *q, const int32_t *ids, int32_t m, float *out);
/* The bounds the HNSW traversals' own test computes: int8 rows against the 16-bit query code, by the device functions
 * hnsw_wave_kernel and hnsw_search_kernel call.  out_lb[i] <= the distance hnswgpu_batch_distances reports, NaN where the
 * test abstains; tighter than hnswgpu_rejection_bounds by the query's share of the slack (about half of it on rows and
 * queries of similar spread).  "16-bit" is the code's storage, two int8 planes: its range is +-16255 (15 bits with the
 * sign) up to dim 1024 and +-11008 / 8256 / 5504 at dims up to 1536 / 2048 / 3072, so that the integer dot product of a
 * whole row fits 32 bits; the query's share of the slack is 1 / 128 ... 1 / 43 of the int8 code's.  A query whose largest
 * component is below 1e-18 gets no bounds (NaN). */
int hnswgpu_hnsw_rejection_bounds(hnswgpu_index *idx, const float *q, const int32_t *ids, int32_t m, float *out_lb);
/* The same with the UPPER bounds beside them (out_ub, may be NULL): out_lb[i] <= distance <= out_ub[i].  The IVF search's
 * bounds pass (hnsw-clj_amd/csrc/stream_kernels.hpp) derives a query's threshold from upper bounds -- k candidates whose
 * upper bound is at most tau put the k-th nearest distance at or below tau -- and drops candidates whose lower bound is
 * above it: both sides have to hold for its result to be the full f32 scan's. */
int hnswgpu_distance_bounds(hnswgpu_index *idx, const float *q, const int32_t *ids, int32_t m, float *out_lb,
                            float *out_ub);
/* Batches with 1.5 M candidates and more (48 queries x 32 lists of ~1000 rows) put a second filter between the int8 bounds and the f32 rows: a HALF-precision copy of
 * the list rows (fp16 with a power-of-two scale per row, 2 * dim bytes per row, made with the int8 copy; HNSWGPU_IVF_HALF=0
 * in the environment leaves it out) whose bounds are ~70 times narrower -- the survivors of the int8 pass meet it first,
 * and f32 rows are fetched for little more than k candidates per query instead of ~3 % of the probed lists.  This entry
 * reports those bounds for `m` rows of the LIST order (positions as hnswgpu_get_ivf's list_ids numbers them) against one
 * query, by the kernel the searches run: out_lb[i] <= distance <= out_ub[i], NaN where a row or the query has no bound. */
int hnswgpu_ivf_half_bounds(hnswgpu_index *idx, const float *q, const int32_t *list_rows, int32_t m, float *out_lb,
                            float *out_ub);
/* Large batches (from 512 queries and half a query per list; rows of whole 128-element steps) put the
 * half-precision rows of a query's NEAREST list -- where nearly all of its int8 survivors sit -- through the matrix
 * cores, once per list for all the queries it is nearest to (v_mfma_f32_16x16x32_f16, the query split into two fp16
 * planes), instead of fetching a half row per (query, survivor).  This entry reports those bounds for the list rows
 * [row_begin, row_end) (positions in list order) against `nq` queries, by the kernel the searches run:
 * out_lb[q * len + r] <= distance(q, row_begin + r) <= out_ub[q * len + r], NaN where a row or the query has no bound. */
int hnswgpu_ivf_home_bounds(hnswgpu_index *idx, const float *Q, int32_t nq, int64_t row_begin, int64_t row_end,
                            float *out_lb, float *out_ub);
int hnswgpu_set_rejection_test(hnswgpu_index *idx, int32_t mode);
/* While profiling is on the traversal counts the neighbours it evaluated and the f32 rows it had to fetch for them
 * (everything with the test off): the bytes a search really moved = neighbours * (int8 row + 16 B) + f32_rows * 4 * dim. */
int hnswgpu_get_rejection_stats(hnswgpu_index *idx, int64_t *f32_rows, int64_t *neighbours, int32_t reset);
/* Mode 1 measures what the traversal's int8 test decides on THIS graph (its first large launch counts f32 rows fetched /
 * neighbours evaluated; nothing blocks: a later launch reads the counters) and evaluates every neighbour in f32 from then
 * on where the test left more than 65 % of the rows to fetch (HNSWGPU_TUNE_HNSW_CALIBRATE_PCT) -- on such rows the int8 stage
 * costs bytes instead of saving them.  state: 0 = not measured yet, 1 = measured, not yet read, 2 = decided; off: the
 * verdict; frac: f32 rows / neighbours of the measured launch.  Results never depend on it. */
int hnswgpu_hnsw_rejection_state(hnswgpu_index *idx, int32_t *state, int32_t *off, double *frac);
/* Device time between events around the timed launches while hnswgpu_set_profiling is on.  which: 0 the IVF / exact scan kernels,
 * 1 the HNSW traversal, 2 the assignment scan, 3 the device chain of hnswgpu_ivf_update (first launch to last, one per call). */
int hnswgpu_get_profile(hnswgpu_index *idx, int32_t which, double *total_ms, int64_t *launches, int32_t reset);
/* Debug read-back of the last ORDERED traversal launch on this handle (HNSWGPU_TUNE_HNSW_ORDER): *nq = its queries (0: none
 * yet), and the first min(cap, *nq) entries of its order[] (the query indices sorted by (key, index)) and of keys[] (per query:
 * the index of its nearest pivot row).  Either array may be NULL.  Waits for the device. */
int hnswgpu_hnsw_last_order(hnswgpu_index *idx, int32_t *order, int32_t *keys, int32_t cap, int32_t *nq);
/* The dense bounds table.  A large batch tests a sizeable share of ALL rows per query (about 6.5 ef neighbours), so a launch
 * reads every int8 row hundreds of times for one integer dot product each.  Eligible launches -- a plain (unfiltered, no
 * forest, no build) search on the one-wave-per-query kernel with the rejection test on -- may instead compute the test's
 * lower bound of every (query, row) pair in front of the traversal, as one int8 GEMM on the matrix cores (query codes x int8
 * rows, hnsw-clj_amd/csrc/dense_kernels.hpp), into a table of nq x (n rounded up to 128) floats; the traversal then reads 4
 * bytes per neighbour.  The integer dot product is exact in any order and the bound comes from the same device function:
 * every entry is the float hnswgpu_hnsw_rejection_bounds reports, bit for bit, NaN where the test abstains -- results,
 * counters and hnswgpu_get_rejection_stats never depend on it.
 * mode: 1 = by the rule of hnsw_launch_plan (default), 0 = never, 2 = every eligible launch (tests).  budget_mb: the largest
 * table of one launch, MiB (default 2048; negative = leave as it is); a launch whose table would be larger runs without.
 * The table is scratch of the handle, grown on demand (hnswgpu_hnsw_dense_bounds_state: bytes). */
int hnswgpu_set_hnsw_dense_bounds(hnswgpu_index *idx, int32_t mode, int64_t budget_mb);
/* mode and budget as set, the launches on this handle that used the table so far, the device bytes its scratch holds now.
 * Any pointer may be NULL. */
int hnswgpu_hnsw_dense_bounds_state(hnswgpu_index *idx, int32_t *mode, int64_t *budget_mb, int64_t *launches, int64_t *bytes);
/* f32 rows a wave keeps in flight in launches with the table on 768-float rows (513 to 768 elements; every other width keeps
 * its fixed count).  rows: 0 = four from 7.5 KiB of LDS per workgroup (ef 320 on a 31k-row index), where fewer workgroups fit a CU
 * anyway, two below (default; the measured table is beside the rule in hnsw_launch_plan), 2 / 4 = forced (A/B, tests), negative
 * = leave as it is.  *rows_set: the setting; *launches_four: the launches on this handle that kept four rows in flight so far.
 * Either pointer may be NULL.  Results, counters and hnswgpu_get_rejection_stats never depend on it. */
int hnswgpu_hnsw_dense_rows(hnswgpu_index *idx, int32_t rows, int32_t *rows_set, int64_t *launches_four);
/* Diagnostic / test entry: the table alone, by the kernels the searches run, for nq host queries (row stride qld >= dim
 * floats) against all n rows: out[q * n + r], nq x n floats on the host. */
int hnswgpu_hnsw_dense_bounds(hnswgpu_index *idx, const float *Q, int32_t nq, int64_t qld, float *out);

/* ---- tuning and test switches --------------------------------------------------------------------------------------
 * One process-wide table of 64-bit values.  NONE of them changes what a search returns within the contract of the path
 * it selects (ids, distance bits, tie order -- the GEMV and the MFMA summation orders differ in the last bits, and
 * TILE_PAIRS / TILE / IVF_CODES / PREFILTER choose between them exactly as the batch size otherwise does): they pick
 * between equivalent schedules, or shrink scratch buffers so that tests reach the fallback paths at test size
 * (tests/test_gpu_parity.py).  The library calls getenv for SIX names only, once, when it is loaded (the keys marked
 * `env`); no search path reads the environment.  HNSWGPU_TUNE_DEFAULT as the value restores a key's default.
 * Diagnostic switches that make results WRONG on purpose (kernels with their epilogue cut out, for ablation timing)
 * exist only in -DHG_DIAG builds (tools/build_stamps.sh), not in this library. */
#define HNSWGPU_TUNE_DEFAULT INT64_MIN
#define HNSWGPU_TUNE_TILE_PAIRS 0 /* (query, list) pairs per list beyond which a cosine / dot IVF batch takes the f32 MFMA tile scan (k-ordered sums) instead of the GEMV-order paths; 0 = the handle's own rule (never on handles with int8 + half-precision list rows, 12 without).  env HNSWGPU_TILE_PAIRS */
#define HNSWGPU_TUNE_PREFILTER 1 /* default hnswgpu_set_rejection_test mode of NEW handles (0 / 1 / 2).  env HNSWGPU_PREFILTER */
#define HNSWGPU_TUNE_IVF_HALF 2 /* 0 = no half-precision copy of the IVF list rows (+50 % of the base).  env HNSWGPU_IVF_HALF */
#define HNSWGPU_TUNE_IVF_CALIBRATE 3 /* 0 = mode-1 handles skip the first-search measurement of what the int8 bounds separate.  env HNSWGPU_IVF_CALIBRATE */
#define HNSWGPU_TUNE_BUILD_THREADS 4 /* host threads of the HNSW linker (0 = min(16, cores)); the graph does not depend on it.  env HNSWGPU_BUILD_THREADS */
#define HNSWGPU_TUNE_PREFETCH 5 /* helper workgroups per query of small HNSW launches (0 = none; default 8 for launches that spread a query over several CUs, 4 for the round-2 helpers).  env HNSWGPU_PREFETCH */
#define HNSWGPU_TUNE_SEED_BOUNDS 6 /* 0 = every k-means++ round a full f32 pass (A/B) */
#define HNSWGPU_TUNE_TILE_WGS 7 /* target workgroup count of the tile scan's work list */
#define HNSWGPU_TUNE_TILE_PERSIST 8 /* tiles per work item of the persistent tile scan (0 = one workgroup per item) */
#define HNSWGPU_TUNE_STREAM_BUCKET 9 /* capacity of a list's bucket of (query, list) pairs; tests: tiny buckets force the fallback */
#define HNSWGPU_TUNE_STREAM_WGS 10 /* target workgroup count of the bounds pass */
#define HNSWGPU_TUNE_FINISH_ORDER 11 /* batch size from which queries are served in the order of their nearest list (0 = never) */
#define HNSWGPU_TUNE_STREAM_CAP 12 /* survivors per query that fit; tests: a tiny list forces the f32-scan fallback */
#define HNSWGPU_TUNE_STREAM_MID 13 /* batch size from which the half-precision pass runs (-1 = by candidate count, 0 = never, 1 = always) */
#define HNSWGPU_TUNE_STREAM_NARROW 14 /* bounds-pass epilogue: -1 auto, 0 lane = query, 1 lane = row */
#define HNSWGPU_TUNE_FINISH_ADAPT 15 /* 0 = short survivor lists are not spread over all waves (A/B) */
#define HNSWGPU_TUNE_FINISH_BISECT 16 /* smallest k whose final merge bisects the key space (A/B) */
#define HNSWGPU_TUNE_FINISH_SLICES 17 /* workgroups per query of the finish kernel (0 = auto) */
#define HNSWGPU_TUNE_FINISH_SPAN 18 /* entries a finish wave looks at per step (0 = auto) */
#define HNSWGPU_TUNE_STREAM_HEAVY 19 /* 0 = no separate service of heavy queries */
#define HNSWGPU_TUNE_STREAM_HEAVY_MEAN 20 /* a heavy query has this many times the batch's mean survivors (default 4) */
#define HNSWGPU_TUNE_STREAM_HEAVY_MIN 21 /* ... and at least this many (default 4096) */
#define HNSWGPU_TUNE_MID_SLICES 22 /* workgroups per query of the half-precision pass (0 = auto) */
#define HNSWGPU_TUNE_MID_COMPACT 23 /* 0 = the half-precision pass does not compact the list (A/B) */
#define HNSWGPU_TUNE_IVF_CODES 24 /* 0 = never the survivor stream, N = from N queries per batch (default 1) */
#define HNSWGPU_TUNE_SCAN_ORDER 25 /* 0 = GEMV list scans never run in list order (A/B) */
#define HNSWGPU_TUNE_IVF_FUSED 26 /* 0 = never the fused two-launch search, 1 = small batches (default), 2 = every GEMV-path batch */
#define HNSWGPU_TUNE_IVF_GROUP 27 /* 0 = never the register-row group kernel, 2 = from half a pair per list */
#define HNSWGPU_TUNE_STREAM_ROUTE 28 /* largest batch routed by the one-launch routing kernel (default 12) */
#define HNSWGPU_TUNE_STREAM_GROUP 29 /* queries from which the bounds pass groups the pairs by list (default 5) */
#define HNSWGPU_TUNE_ROUTE_GROUP 30 /* queries from which a GEMV-order batch routes through the group kernel (default 1024) */
#define HNSWGPU_TUNE_MID_WIDE 31 /* 0 = never eight waves per query in the half-precision pass (A/B) */
#define HNSWGPU_TUNE_MERGE_W 32 /* waves per query of merge_topk_kernel (0 = auto) */
#define HNSWGPU_TUNE_SCAN_BLOCKS 33 /* target workgroup count of the GEMV scan (0 = auto) */
#define HNSWGPU_TUNE_ROUTE_WGS 34 /* target workgroup count of the routing distance pass */
#define HNSWGPU_TUNE_TILE 35 /* -1 auto, 0 never the MFMA tile kernel, 1 whenever possible */
#define HNSWGPU_TUNE_SELECT_W 36 /* waves per query of select_topk_kernel (0 = auto) */
#define HNSWGPU_TUNE_HNSW_NW 37 /* waves per query of the traversal kernel: 1 / 2 / 4 (0 = by batch size) */
#define HNSWGPU_TUNE_VIS_GLOBAL 38 /* 1 = the traversal's visited set in HBM stamps whatever the index size (tests) */
#define HNSWGPU_TUNE_PF_HINTS 39 /* unexpanded list entries kept evaluated ahead of the traversal by its helpers (solo launches: the fetchers' window, default 8 below ef 256 and 16 from there; round-2 helpers: entries posted per expansion, default 4) */
#define HNSWGPU_TUNE_PF_EVAL 40 /* 0 = the helpers only warm the L2 (A/B) */
#define HNSWGPU_TUNE_ZEROCOPY 41 /* 0 = small synchronous HNSW calls stage through copies instead of mapped pinned memory (A/B) */
#define HNSWGPU_TUNE_BUILD_TIMING 42 /* 1 = hnswgpu_hnsw_build prints where its time went to stderr */
#define HNSWGPU_TUNE_BUILD_BATCH 43 /* largest insertion batch of hnswgpu_hnsw_build / hnswgpu_hnsw_add (default and cap 16384, at least 1).  The batch-size rule: with `done` rows in the graph the next batch holds min(BUILD_BATCH, max(1, done / 8), 2048 + done / 64, rows left) rows (integer divisions) -- never more than 1/8 of the graph it is searched against, and from 18,725 rows on 2048 + done / 64.  A build starts at done = 1 (row 0 is the entry point), hnswgpu_hnsw_add at the rows the index holds.  The rows of a batch are searched against the graph as it stood when the batch began, so the graph depends on this value (1 = one row per batch); HNSWGPU_BUILD_SEQUENTIAL ignores it */
#define HNSWGPU_TUNE_STREAM_HOME 44 /* the home-list pass of large IVF batches (every list once through the matrix cores in half precision for all the queries it is nearest to): -1 from 512 queries and half a query per list, 0 never, 1 whenever the batch is served in the order of its nearest lists */
#define HNSWGPU_TUNE_HOME_CHUNK 45 /* rows per work item of the home-list pass (a multiple of 64; 0 = auto) */
#define HNSWGPU_TUNE_HOME_DEPTH 46 /* operand loads in flight per wave of the home-list pass: 4 / 8 / 12 / 16 / 24, the largest that divides the 32-element steps of a row and does not exceed this (default 12) */
#define HNSWGPU_TUNE_HOME_STRAYS 47 /* home-list batches: a query the bounds pass appended no more than this many candidates to skips the per-survivor half-precision pass (the finish kernel fetches their f32 rows; default 32) */
#define HNSWGPU_TUNE_ROUTE_MFMA 48 /* centroid distances of IVF batches on the f32 matrix cores in the GEMV order (the same bits): -1 from 256 queries (cosine / dot, rows of 256 / 512 / 768 elements), 0 never, 1 whenever possible, > 1 that many slices of the table per group of 16 queries */
#define HNSWGPU_TUNE_STREAM_WIDE2 49 /* bounds pass of large batches with several 32-query column blocks per group (a staged list row meets 64 / 128 queries): -1 = two blocks from 256 (query, list) pairs per list, 0 never, 1 = two blocks and 4 = four blocks (measured slower: A/B, tests) whenever the wide deferring epilogue runs */
#define HNSWGPU_TUNE_SOLO 50 /* small HNSW launches, one query over several CUs (an owner workgroup keeps the reference's order, helper workgroups evaluate and chase ahead of it): 1 = from ef 96 (default), 2 = always, 0 = never (the round-2 helpers) */
#define HNSWGPU_TUNE_SOLO_CHASE 51 /* 0 = the helpers only evaluate what the owner asks for (A/B) */
#define HNSWGPU_TUNE_SOLO_SLOTS 52 /* log2 of the slots per query of the helpers' node-keyed tables (0 = auto) */
#define HNSWGPU_TUNE_HNSW_CALIBRATE 53 /* 0 = rejection mode 1 never measures what the traversal's int8 test decides (it then stays on for every large launch) */
#define HNSWGPU_TUNE_HNSW_CALIBRATE_PCT 54 /* the int8 test of the traversal is switched off for a graph when it leaves more than this many percent of the neighbours' f32 rows to fetch (default 65) */
#define HNSWGPU_TUNE_HNSW_WAVE 55 /* large HNSW launches on the one-wave-per-query kernel with the admission buffer: 1 = launches that fill the chip with one wave per query, and every launch from ef 640 (default), 0 = never (A/B), 2 = every launch it can serve (tests) */
#define HNSWGPU_TUNE_FINISH_DIRECT 56 /* small IVF batches (16 and more finish workgroups per query): survivor lists of up to this many entries hand a key per survivor straight to the query's last workgroup instead of per-wave / per-workgroup top-k lists (default 1024 = the most; 0 = never: A/B) */
#define HNSWGPU_TUNE_WORKLIST_FOLD 57 /* 0 = the bounds pass's work list of a small IVF batch stays a launch of its own instead of extra workgroups of the routing tail's launch (A/B) */
#define HNSWGPU_TUNE_SEED_HALF 58 /* 0 = a query's first threshold from f32 rows of its nearest list even where the half-precision copy exists (A/B; default 1: the k-th smallest upper bound of the sampled rows' half-precision copies, half the bytes) */
#define HNSWGPU_TUNE_BUILD_KEEP_ROWS 59 /* 0 = the builder's heuristic selection fetches the already selected rows again for every candidate instead of keeping them in registers (A/B; the graph does not depend on it) */
#define HNSWGPU_TUNE_QUERY_WAVES 60 /* the per-query kernels of large IVF batches (home-list selection) with one WAVE per query, four queries per workgroup, instead of a workgroup per query: -1 from 2048 queries, 0 never, 1 wherever a wave can serve a query (k <= 64) */
#define HNSWGPU_TUNE_HNSW_ORDER 61 /* launches of the one-wave-per-query kernel serve their queries in the order of their nearest pivot row (min(256, n) base rows at a fixed stride, judged on the int8 rows), dealt so that neighbouring queries run on one XCD at one time -- a hint for the L2s, results never depend on it: 1 = search launches on handles with int8 rows from a batch size (default), 0 = never (A/B), 2 = every such launch (tests) */
#define HNSWGPU_TUNE_FILTER_EACH_MB 62 /* hnswgpu_exact_knn_filtered_each: bound of the dense distance scratch of one slice of query groups, in MiB (default 2048, the single-mask call's bound; at least one group per slice) */
#define HNSWGPU_TUNE_COUNT 63
int hnswgpu_set_tuning(int32_t key, int64_t value);
int hnswgpu_get_tuning(int32_t key, int64_t *value, int32_t *is_set);

/* ---- Hybrid LSH (hnsw-clj_amd/csrc/lsh.hip, lsh_kernels.hpp) -------------------------------------------------------
 * The reference's hnsw.ann.hash.hybrid-lsh (src/hnsw/ann/hash/hybrid_lsh.clj): `tables` hash tables of sign projections
 * over the handle's rows.  Bit i of a row's code in table t is dot(row, plane[t][i]) >= 0.0 (:33-45), bit i at position i
 * (:47-55); a bucket lists its rows in row order (:105-129).  The dot is the engine's GEMV-order dot with the plane in the
 * query's role -- the sign of the negated distance hnswgpu_batch_distances returns on a DOT handle -- and ONE kernel hashes
 * base rows and queries: a base row used as a query lands in its own buckets.
 *   hnswgpu_lsh_build: the planes from java.util.Random(seed) as build-lsh-index consumes it (:24-31, :80-84): tables x
 *     proj_dim x dim nextGaussian draws, table by table, row by row; a table keeps its first `bits` rows (NUM-HASH-BITS of
 *     PROJECTION-DIM, :12-14, :117).  proj_dim (>= bits) only keeps a JVM user's seed on the same hyperplanes; the
 *     reference's index is (8, 12, 64, 42).  The draws are rounded to float.  Replaces tables the handle has.  n == 0 is legal.
 *   hnswgpu_set_lsh: the same from the caller's hyperplanes [tables][bits][dim].
 *   hnswgpu_lsh_sizes: (0, 0) for a handle without tables.
 *   hnswgpu_lsh_get: planes [tables][bits][dim], codes [n][tables], off [tables][2^bits + 1] (bucket b of table t is
 *     ids[t][off[t][b] .. off[t][b + 1]), rows ascending), ids [tables][n]; every output may be null.
 *   hnswgpu_lsh_hash: codes [nq][tables] of arbitrary vectors under the handle's planes.
 *   hnswgpu_lsh_search / _dev: search-hybrid-multiprobe's sequential branch (:305-342; the parallel branch differs in the order
 *     of ties only).  For table t = 0 .. min(num_probes, tables) - 1: the query's own bucket, of which the take_main nearest
 *     rows are kept, then for j = 0 .. min(probe_radius, bits) - 1 the bucket with bit j flipped, take_flip rows each (a bucket
 *     with no more rows than its take is kept whole, :153; otherwise a stable sort by distance, :188-193).  The pieces are
 *     concatenated in probe order, a row's later occurrences dropped, the rest sorted stably by distance and cut to k
 *     (:330-342).  The reference calls it with take_main = 2 k, take_flip = k; search-hybrid (:195-259) is radius 0 with
 *     take_main = 3 k (parallel, the default) or 2 k.  Truncation per probe comes BEFORE the dedup.  out [nq][k] ascending,
 *     padded with -1 / +inf where fewer than k distinct rows were found.  The metric is the handle's (the reference computes
 *     cosine whatever :distance-fn says, :157-166: its query-norm is never nil); distances have the bits of every GEMV-order
 *     scan.  _dev only enqueues on `stream` (device arrays, no synchronise, no readback); the host entry stages one caller's
 *     batch and takes no part in the combining of concurrent callers.
 * Errors: -1 null pointers, k < 1, take_* < 1, num_probes < 1, probe_radius < 0, tables < 1; nq == 0 returns 0; -3 a handle
 * without tables; -5 tables > 16, bits outside 1 .. 16, k > 256, take_* > 256, or a probe stream of one query
 * (probes x (1 + radius) x n rows) of 2^32 rows or more.
 * hnswgpu_hnsw_add and hnswgpu_ivf_add return -3 on a handle with tables (the tables would miss the new rows).  The tables
 * are NOT part of the index file: hnswgpu_save writes what it writes without them, a loaded handle has none (build them again
 * from the seed, or install the exported planes).  Groups, shards and forests do not know them.
 *
 *   hnswgpu_lsh_add: rows join a LIVE handle with tables (the reference's HybridIndex has no add; what is restated is its bucket
 *     order, :105-129: a bucket lists its rows in insertion order, which is row order).  `rows` is m x dim float32 host memory;
 *     the rows get ids n .. n + m - 1 and join the base matrix, the norms, the base-order int8 rows where the handle has them,
 *     and every table's buckets behind a bucket's present members, in row order.  The planes do not change, and the new rows
 *     are hashed by the kernel that hashed the old ones: a row's code does not depend on whether it came by build or by add,
 *     and m rows in one call or in any split of calls give the same tables.
 *     After the call the handle holds, bit for bit, what hnswgpu_create(all n + m rows) + hnswgpu_set_rejection_test(same
 *     mode) + hnswgpu_set_lsh(the same planes) holds: what hnswgpu_lsh_get exports, the ids and distance bits of
 *     hnswgpu_lsh_search / _dev, hnswgpu_exact_knn, hnswgpu_norms, hnswgpu_batch_distances, hnswgpu_lsh_hash, and the bytes
 *     hnswgpu_save writes (still without the tables).
 *     Everything happens on the device, in one chain on the handle's stream: no old row is uploaded, no code or bucket id is
 *     read back, and the placement is deterministic by construction (a new row's place is its stable rank among the call's
 *     rows of its bucket, never the order atomics arrive in).  Failure-atomic, like hnswgpu_ivf_add: every new array is staged
 *     under the handle's lock with its streams quiesced; the handle takes them over only after the last step, and after one
 *     small readback has shown that every table's grown buckets hold n + m rows (HNSWGPU_EHIP otherwise); on any failure the
 *     staged arrays are freed and the handle is what it was.  Searches from other threads wait and see the old or the new index.
 *     Cost: one device copy of the base, the codes and the bucket ids per CALL plus about m / 64 dependent steps of one wave per
 *     table -- add rows in batches; a bulk load should build the tables instead.
 *     Returns, checked in this order: -1 for a null handle or m < 0; 0 for m == 0 (nothing happens, whatever `rows` and the
 *     handle are); -1 for null rows; -3 for a handle without tables, and for one that also holds an HNSW graph, a forest, IVF
 *     lists or a shard's lists (those structures would miss the rows; the message names which); -5 for n + m >= 2^31 - 1,
 *     before `rows` is read.  n == 0 is legal.
 *
 *   hnswgpu_lsh_remove: rows leave a LIVE handle with tables (the reference's HybridIndex has no remove either; what is
 *     restated is again its bucket order).  `rows` is m row ids of the handle in host memory, in any order; an id named twice
 *     is removed once.  The kept rows are renumbered densely in their old order: the new id of a kept row r is the number of
 *     kept rows below r.  *n_after (may be NULL) gets the rows the handle holds afterwards.
 *     After the call the handle holds, bit for bit, what hnswgpu_create(the kept rows in their old order) +
 *     hnswgpu_set_rejection_test(same mode) + hnswgpu_set_lsh(the same planes) holds: base, norms, the base-order int8 rows and
 *     their meta where the handle has them, and what hnswgpu_lsh_get exports -- codes [n1][tables], per table off[2^bits + 1]
 *     and ids[n1], rows ascending inside a bucket (a bucket's kept members stay in their order; the rank is monotone) -- hence
 *     the ids and distance bits of hnswgpu_lsh_search / _dev, hnswgpu_exact_knn, hnswgpu_norms, hnswgpu_batch_distances,
 *     hnswgpu_lsh_hash, and the bytes hnswgpu_save writes (still without the tables).  It is the permanent form of
 *     hnswgpu_lsh_search_filtered: a search after the removal finds the rows, under their new ids, and the distance bits that
 *     the filtered search found before it under the mask of the kept rows.
 *     Everything happens on the device, in one chain on the handle's stream: only the m ids go up, norms and codes are copied
 *     (not computed again), no code or bucket id is read back, and every entry's destination is a function of the mask and the
 *     old arrays alone (prefix counts of kept entries), never of the order atomics arrive in.  Failure-atomic, like
 *     hnswgpu_lsh_add: nothing is changed in place, every new array is staged under the handle's lock with its streams
 *     quiesced, and the handle takes them over only after ONE small readback has shown that the rank scan, every table's last
 *     offset and every table's compacted ids all count n - (distinct ids) rows (HNSWGPU_EHIP otherwise); on any failure the
 *     staged arrays are freed and the handle is what it was.  Searches from other threads wait and see the old or the new
 *     index.  Peak memory: the old plus the new arrays for the length of the call, as for add.  Cost: one device copy of the
 *     kept rows, codes and bucket ids per CALL, whatever m is -- remove rows in batches.
 *     Returns, checked in this order: -1 for a null handle (before m == 0 and before any HIP call), for m < 0, and for null
 *     rows with m > 0; 0 for m == 0 (nothing happens, *n_after = n, whatever the handle holds); -3 for a handle without
 *     tables, and for one that also holds an HNSW graph, a forest, IVF lists or a shard's lists (those structures would keep
 *     the old numbering; the message names which); -1 for an id outside [0, n), checked on the host array before anything is
 *     enqueued.  The handle is untouched in every one of these cases.  Removing every row is legal: it leaves an empty handle
 *     with tables (planes, all-zero offsets), the state hnswgpu_lsh_add accepts, and that handle can be grown again.
 *
 *   hnswgpu_lsh_update: rows of a LIVE handle with tables take new values under their ids ("Update existing vectors", the open
 *     item of the reference's to-do list, README.md:172-176; its HybridIndex is an immutable record, so what is restated is
 *     again its bucket order).  `ids` is m row ids of the handle in host memory, in any order; `rows` is m x dim float32 host
 *     memory; row ids[i] takes the values rows[i].  n, every row id and the planes stay as they are -- unlike
 *     hnswgpu_lsh_remove + hnswgpu_lsh_add, which hand the row a new id and shift every id above it.
 *     - Equivalence.  After the call the handle holds, bit for bit, what hnswgpu_create(the base with the new values) +
 *       hnswgpu_set_rejection_test(same mode) + hnswgpu_set_lsh(the same planes) holds: base and norms, the base-order int8
 *       rows and their meta where the handle has them, and what hnswgpu_lsh_get exports -- codes [n][tables], per table
 *       off[2^bits + 1] and ids[n], rows ascending inside a bucket -- hence the ids and distance bits of hnswgpu_lsh_search /
 *       _dev / _filtered / _filtered_each, hnswgpu_exact_knn, hnswgpu_norms, hnswgpu_batch_distances, hnswgpu_lsh_hash, and the
 *       bytes hnswgpu_save writes (still without the tables).
 *     - Hashing.  lsh_hash_kernel hashes the new values under the handle's planes: a row's code does not depend on whether it
 *       came by build, add or update.  NaN and zero rows are accepted as hnswgpu_lsh_add accepts them and hash as they would
 *       on a fresh handle (dot >= 0.0 is false for NaN), so the equivalence holds for them.
 *     - Stayers and movers, per table.  A row whose code in table t is unchanged keeps its bucket there.  A row whose code in
 *       table t changed leaves its bucket of table t, which closes up, and joins its new bucket at the place its row id gives
 *       it among the members -- a merge, not an append as in hnswgpu_ivf_update.  A row may move in some tables and stay in
 *       others.  Updating rows to the values they already have changes nothing, bit for bit.
 *     - Independence of the split.  An update changes no id and a bucket is ascending by row id, so different rows give the
 *       same handle whether they are updated in one call, in any split of calls, or in any order of `ids` -- the opposite of
 *       hnswgpu_ivf_update's caveat, the independence of hnswgpu_lsh_add and hnswgpu_lsh_remove.
 *     - Everything happens on the device, in one chain on the handle's stream: the m ids (sorted on the host: slot s of the
 *       call is the s-th smallest id) and the m rows go up once; norms by the kernel hnswgpu_create uses; the int8 rows made as
 *       hnswgpu_lsh_add makes them, over the new base; no code or bucket id is read back; every destination is a function of
 *       the old arrays and the call alone -- for row r in its new bucket b of table t,
 *       new_off[t][b] + #old members of b below r - #leavers of b below r + #joiners of b below r --, never of the order
 *       atomics arrive in.
 *     - Failure-atomic, like the other mutations: nothing is changed in place, every new array is staged under the handle's
 *       lock with its streams quiesced, and the handle takes them over only after ONE small readback of a gate of counts -- per
 *       table: the last new offset == n, entries that left == entries that joined, entries placed == n (HNSWGPU_EHIP
 *       otherwise).  On any failure the staged arrays are freed and the handle is what it was.  Searches from other threads
 *       wait and see the old or the new index.  Peak memory: the old plus the new arrays for the length of the call.
 *     - Cost: one device copy of the base, the codes and the bucket ids (O(n x tables) entries) per CALL, whatever m is, plus
 *       O(m x tables x log) searches and about m / 64 dependent steps of one wave per table -- update rows in batches.
 *       Measured on one MI355X (profiles/lsh_update.txt: 31,173 x 768 cosine, 8 tables x 12 bits): 0.48 / 0.65 / 1.54 ms for
 *       m = 1 / 1,024 / 8,192 scattered rows against 2.29 / 2.29 / 2.27 ms for the rebuild over the base with the new values
 *       from host memory -- faster at every m measured, by less the more rows a call carries (0.21, 0.29, 0.68 of the
 *       rebuild) -- and against 0.88 / 1.03 / 1.76 ms for hnswgpu_lsh_remove + hnswgpu_lsh_add of the same rows, which loses
 *       the ids.  The kernels and device copies are 0.23 / 0.26 / 0.45 ms of a call (the serial walk that groups the movers
 *       is 0.005 / 0.024 / 0.19 ms of that, the placement of the entries that stay 0.05 ms at every m); the rest is the
 *       upload of the rows, allocating and freeing the staged arrays and the readback.
 *     Returns, checked in this order, the handle untouched in every case: -1 for a null handle (before m == 0 and before any
 *     HIP call), for m < 0, and for null ids or rows with m > 0; 0 for m == 0 (nothing happens); -3 for a handle without
 *     tables; -3 for a handle that also holds an HNSW graph, a forest, IVF lists or a shard's lists (their copies of the row
 *     would go stale; the message names which); -1 for an id outside [0, n) and for an id named twice (two values for one row
 *     have no defined winner), both checked on the host array before anything is enqueued.
 *     Out of scope: HNSW updates; handles that hold tables and another structure; groups, shards and forests; the tables in
 *     the index file; in-place patching that avoids the per-call copy of the base. */
int hnswgpu_lsh_build(hnswgpu_index *idx, int32_t tables, int32_t bits, int32_t proj_dim, int64_t seed);
int hnswgpu_set_lsh(hnswgpu_index *idx, const float *planes, int32_t tables, int32_t bits);
int hnswgpu_lsh_sizes(hnswgpu_index *idx, int32_t *tables, int32_t *bits);
int hnswgpu_lsh_get(hnswgpu_index *idx, float *planes, uint16_t *codes, int64_t *off, int32_t *ids);
int hnswgpu_lsh_hash(hnswgpu_index *idx, const float *Q, int32_t nq, uint16_t *codes);
int hnswgpu_lsh_add(hnswgpu_index *idx, const float *rows, int64_t m);
int hnswgpu_lsh_remove(hnswgpu_index *idx, const int32_t *rows, int64_t m, int64_t *n_after);
int hnswgpu_lsh_update(hnswgpu_index *idx, const int32_t *ids, const float *rows, int64_t m);
int hnswgpu_lsh_search(hnswgpu_index *idx, const float *Q, int32_t nq, int32_t k, int32_t num_probes, int32_t probe_radius,
                       int32_t take_main, int32_t take_flip, int32_t *out_ids, float *out_dist);
int hnswgpu_lsh_search_dev(hnswgpu_index *idx, const float *d_Q, int32_t nq, int32_t k, int32_t num_probes,
                           int32_t probe_radius, int32_t take_main, int32_t take_flip, int32_t *d_out_ids, float *d_out_dist,
                           void *stream);

/* hnswgpu_lsh_search_filtered / _each / _dev: the allow-mask through the bucket scan (lsh_filtered_scan_kernel).  As for
 * hnswgpu_ivf_search_filtered, post-filtering ("search 3 k, drop what fails, keep k") is the wrong rule here, and more so: the
 * candidate set is already cut per probe, before the dedup, to take_main / take_flip rows of each bucket, so when a fraction
 * p of the rows passes about 3 k p results survive, and every row of every probed bucket is read whatever the mask says.
 * Instead the bit is tested where the bucket is read, and only the passing rows are fetched.
 *   Semantics: search-hybrid-multiprobe (:305-342) run over buckets that list only their passing rows, in bucket order.  For
 *     each probed bucket of a query, in the UNFILTERED probe order (table by table; own bucket, then bit 0, 1, ... flipped),
 *     the rows whose bit is clear are dropped and the `take` nearest of the rest are kept (take_main for the own bucket,
 *     take_flip for a neighbour; a bucket with no more passing rows than its take is kept whole, otherwise the order is by
 *     (distance, position in the bucket)).  The pieces are concatenated in probe order, a row's later occurrences dropped,
 *     the rest sorted stably by distance and cut to k; truncation still comes before the dedup; -1 / +inf padding.
 *   Equivalence: the result is what hnswgpu_lsh_search returns on a handle created over the passing rows alone (in row
 *     order) with hnswgpu_set_lsh(the same planes), with ids mapped back: ids and distance bits are equal.  "Filter first,
 *     then take" is the point: it differs from post-filtering wherever a bucket has more than `take` rows.  An all-ones
 *     mask returns hnswgpu_lsh_search's ids and distance bits.
 *   Keys carry the position in the unfiltered probe stream, which is monotone in the filtered one, so ties resolve as in
 *     the sub-index; the probe table, the key epilogue and the merge are the unfiltered search's.  Distances have the bits
 *     of every GEMV-order scan: a row's bits depend neither on which rows share its step nor on the mask.
 *   Mask: exactly that of the other filtered calls.  `allow` is (n + 31) / 32 words indexed by row id, bits at positions
 *     >= n are ignored; it is an argument, never handle state: nothing is kept or persisted, and after hnswgpu_lsh_add the
 *     next call brings a longer mask.  allow_each is [nq][W] row-major; result row q equals the single-mask call with query
 *     q and mask q.
 *   Cost per probed position: 4 B of bucket ids and a gathered mask word; the f32 row only where the bit is set.
 *   _dev entries only enqueue on `stream`: no synchronise, no readback (nothing needs a count: the wave that reads a bucket
 *     filters it).  Host entries stage one caller's batch, masks included (as hnswgpu_ivf_search_filtered_each stages its
 *     own), and take no part in the combining of concurrent callers.
 *   Errors: everything hnswgpu_lsh_search checks, in its order; nq == 0 returns 0; a null mask is -1 (when nq > 0); -3 a
 *     handle without tables; n == 0 fills the padding as the unfiltered call does; the 2^32 probe-stream limit is unchanged
 *     (it is about the unfiltered stream, which the keys still number).
 *   Out of scope: groups, shards and forests (they do not know the tables); the tables in the index file; combining
 *     concurrent filtered callers. */
int hnswgpu_lsh_search_filtered(hnswgpu_index *idx, const float *Q, int32_t nq, int32_t k, int32_t num_probes,
                                int32_t probe_radius, int32_t take_main, int32_t take_flip, const uint32_t *allow,
                                int32_t *out_ids, float *out_dist);
int hnswgpu_lsh_search_filtered_dev(hnswgpu_index *idx, const float *d_Q, int32_t nq, int32_t k, int32_t num_probes,
                                    int32_t probe_radius, int32_t take_main, int32_t take_flip, const uint32_t *d_allow,
                                    int32_t *d_out_ids, float *d_out_dist, void *stream);
int hnswgpu_lsh_search_filtered_each(hnswgpu_index *idx, const float *Q, int32_t nq, int32_t k, int32_t num_probes,
                                     int32_t probe_radius, int32_t take_main, int32_t take_flip, const uint32_t *allow_each,
                                     int32_t *out_ids, float *out_dist);
int hnswgpu_lsh_search_filtered_each_dev(hnswgpu_index *idx, const float *d_Q, int32_t nq, int32_t k, int32_t num_probes,
                                         int32_t probe_radius, int32_t take_main, int32_t take_flip,
                                         const uint32_t *d_allow_each, int32_t *d_out_ids, float *d_out_dist, void *stream);

/* ---- ONE index over several GPUs (hnsw-clj_amd/csrc/group.hip) ---------------------------------------------------
 * The reference shards inside one process: search-partitioned scatters a query to its partitions, takes a top-k per
 * partition, concatenates, sorts and takes k (src/hnsw/ann/partition/partitioned_hnsw.clj:149-196).  A group gives the
 * JVM host the same from one call: it owns one engine handle per device and every device works on its own stream.
 *   hnswgpu_group_create: `devices` = the GPUs of the group (one GPU may be named several times: several handles on it).
 *   hnswgpu_group_set_ivf: ONE IVF-FLAT index (base rows, centroids, lists as for hnswgpu_set_ivf) -- centroids
 *     replicated, whole inverted lists dealt to the devices balanced by row count (longest list first onto the least
 *     loaded device), every device routes a batch identically and scans the probed lists it holds.
 *   hnswgpu_group_ivf_search: the per-device top-k lists are moved to devices[0] by peer copies (nq * k * 12 bytes per
 *     device, xGMI between GPUs) and merged by (distance, position in the candidate stream of the WHOLE index): ids,
 *     distances and tie order are bit for bit those of hnswgpu_ivf_search on the unsharded index (ivf_flat.clj:291-294).
 *   hnswgpu_group_hnsw_build / _hnsw_search: contiguous row ranges, one independent sub-graph per device
 *     (= PartitionedHNSWIndex, partitioned_hnsw.clj:23-27), each searched with the full k; merge by distance, ties to the
 *     lower device (the reference's stable sort of the concatenation).
 *   hnswgpu_group_member: the sub-index device i holds (info / export; do not destroy it).
 * Row ids in and out are rows of the caller's base matrix.  Calls on one group are serialised. */
typedef struct hnswgpu_group hnswgpu_group;
int hnswgpu_group_create(const int32_t *devices, int32_t ndev, int32_t dim, int32_t metric, hnswgpu_group **out);
int hnswgpu_group_destroy(hnswgpu_group *g);
int hnswgpu_group_info(const hnswgpu_group *g, int32_t *ndev, int64_t *n, int32_t *kind, int64_t *rows_per_device);
int hnswgpu_group_set_ivf(hnswgpu_group *g, const float *base, int64_t n, const float *centroids, int32_t nlist,
                          const int64_t *list_off, const int32_t *list_ids);
int hnswgpu_group_ivf_search(hnswgpu_group *g, const float *Q, int32_t nq, int32_t k, int32_t nprobe, int32_t *out_ids,
                             float *out_dist);
int hnswgpu_group_hnsw_build(hnswgpu_group *g, const float *base, int64_t n, int32_t M, int32_t ef_construction,
                             int64_t seed);
int hnswgpu_group_hnsw_search(hnswgpu_group *g, const float *Q, int32_t nq, int32_t k, int32_t ef, int32_t *out_ids,
                              float *out_dist);
hnswgpu_index *hnswgpu_group_member(hnswgpu_group *g, int32_t i);

#ifdef __cplusplus
}
#endif
#endif /* HNSWGPU_H */
