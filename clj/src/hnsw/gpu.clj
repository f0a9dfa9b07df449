(ns hnsw.gpu
  "MI355X engine behind hnsw-clj's index/search API (libhnswgpu.so, C ABI: include/hnswgpu.h).

   Binding: java.lang.foreign (Panama FFM, JDK 22+; the reference already requires Java 21+),
   so no native glue is needed.  A JNI alternative is in clj/native/hnswgpu_jni.c.

   UNVERIFIED: this image has no JVM, so this namespace has never been loaded.  The C ABI it calls is
   exercised end to end by tests/test_gpu_parity.py through ctypes with the same signatures.

   Drop-in surface (same names / argument meaning as the reference):
     (build-index data & {:keys [M ef-construction distance-fn]})   ; hnsw.ultra-fast/build-index
     (search-knn index query-vec k)                                  ; hnsw.ultra-fast/search-knn
     (search-batch index queries k)                                  ; BatchSearchIndex/search-batch*
     (build-ivf-index data & {:keys [num-partitions max-iterations]}) ; hnsw.ann.partition.ivf-flat/build-index
     (search-ivf index query-vec k & {:keys [num-probes]})
     (search-ivf-batch index queries k & {:keys [num-probes]})
     (batch-distances index query-vec)                               ; simd-optimized/batch-cosine-distances
     (top-k-distances index query-vec k)                             ; simd-optimized/top-k-distances
     (add-vector! index new-data)                                    ; hnsw.api/add-vector!, insert-single on a live index
     (remove-vectors! index ids)                                     ; ... and leave the graph again: hnswgpu_hnsw_remove
     (update-vectors! index new-data)                                ; ... and take new values under their ids: hnswgpu_hnsw_update
     (add-ivf-vectors! index new-data)                               ; the same for a live IVF-FLAT index: hnswgpu_ivf_add
     (remove-ivf-vectors! index ids)                                 ; ... and leave it: hnswgpu_ivf_remove
     (update-ivf-vectors! index new-data)                            ; ... and take new values under their ids: hnswgpu_ivf_update
     (build-lsh-index data :metric :cosine)                          ; hnsw.ann.hash.hybrid-lsh/build-lsh-index: (Random. 42), 8 x 12 bits
     (add-lsh-vectors! index new-data)                               ; rows join a live hybrid-LSH index: hnswgpu_lsh_add
     (remove-lsh-vectors! index ids)                                 ; ... and leave it: hnswgpu_lsh_remove
     (update-lsh-vectors! index new-data)                            ; ... and take new values under their ids: hnswgpu_lsh_update
     (search-lsh index query-vec k :mode :balanced)                  ; hybrid-lsh/search-knn (search-hybrid-multiprobe)
     (search-lsh-batch index queries k :mode :balanced)
     (search-lsh-filtered index query-vec k filter-fn :mode :balanced) ; the allow-mask through the bucket scan: hnswgpu_lsh_search_filtered
     (search-lsh-batch-filtered-each index queries k filter-fns)      ; one predicate per query: hnswgpu_lsh_search_filtered_each
     (from-ultra-graph graph)                                        ; a graph built by the reference's own insert-single
     (from-ivf-flat-index ivf)                                       ; an IVFFlatIndex built by the reference's own k-means
     (save idx path) / (load-index path ids)                         ; helper/index-io save-index / load-index
     (search-knn-filtered index query-vec k filter-fn)               ; FilterableIndex/search-knn-filtered*, on the device
     (search-batch-filtered-each index queries k filter-fns)          ; ... for a batch, one predicate per query, in one chain of launches
     (search-ivf-filtered index query-vec k filter-fn :num-probes 4)  ; ... through the IVF list scan: the k nearest passing rows
     (search-ivf-batch-filtered-each index queries k filter-fns)      ; ... for a batch, one predicate per query, in one chain of launches
   and, at the bottom, the extend-type that makes GpuIndex an ANNIndex / BatchSearchIndex / FilterableIndex / PersistableIndex next to the
   records src/hnsw/api/unified.clj:30-95 extends."
  (:require [hnsw.api.protocol :as proto])
  (:import [java.lang.foreign Arena FunctionDescriptor Linker MemorySegment SymbolLookup ValueLayout]
           [java.lang.invoke MethodHandle]))

(def ^:private ^Linker linker (Linker/nativeLinker))
(def ^:private lookup
  (delay (SymbolLookup/libraryLookup (or (System/getProperty "hnswgpu.lib") "libhnswgpu.so") (Arena/global))))

(defn- fn-handle ^MethodHandle [^String sym ^FunctionDescriptor desc]
  (.downcallHandle linker (.orElseThrow (.find ^SymbolLookup @lookup sym)) desc (make-array java.lang.foreign.Linker$Option 0)))

(def ^:private I ValueLayout/JAVA_INT)
(def ^:private L ValueLayout/JAVA_LONG)
(def ^:private P ValueLayout/ADDRESS)

(def ^:private h-create   (delay (fn-handle "hnswgpu_create" (FunctionDescriptor/of I (into-array [P L I I I P])))))
(def ^:private h-destroy  (delay (fn-handle "hnswgpu_destroy" (FunctionDescriptor/of I (into-array [P])))))
(def ^:private h-build    (delay (fn-handle "hnswgpu_hnsw_build_ex" (FunctionDescriptor/of I (into-array [P I I L I])))))
(def ^:private h-search   (delay (fn-handle "hnswgpu_hnsw_search" (FunctionDescriptor/of I (into-array [P P I I I P P P])))))
(def ^:private h-ivfbuild (delay (fn-handle "hnswgpu_ivf_build" (FunctionDescriptor/of I (into-array [P I I L])))))
(def ^:private h-ivfsearch (delay (fn-handle "hnswgpu_ivf_search" (FunctionDescriptor/of I (into-array [P P I I I P P P])))))
(def ^:private h-setgraph (delay (fn-handle "hnswgpu_set_graph" (FunctionDescriptor/of I (into-array [P P P I P P I I I])))))
(def ^:private h-setivf   (delay (fn-handle "hnswgpu_set_ivf" (FunctionDescriptor/of I (into-array [P P I P P])))))
(def ^:private h-batchd   (delay (fn-handle "hnswgpu_batch_distances" (FunctionDescriptor/of I (into-array [P P P I P])))))
(def ^:private h-exact    (delay (fn-handle "hnswgpu_exact_knn" (FunctionDescriptor/of I (into-array [P P I I P P])))))
(def ^:private h-save     (delay (fn-handle "hnswgpu_save" (FunctionDescriptor/of I (into-array [P P])))))
(def ^:private h-load     (delay (fn-handle "hnswgpu_load" (FunctionDescriptor/of I (into-array [P I P])))))
(def ^:private h-info     (delay (fn-handle "hnswgpu_info" (FunctionDescriptor/of I (into-array [P P P P P P])))))
(def ^:private h-rejmode  (delay (fn-handle "hnswgpu_set_rejection_test" (FunctionDescriptor/of I (into-array [P I])))))
(def ^:private h-error    (delay (fn-handle "hnswgpu_last_error" (FunctionDescriptor/of P (into-array ValueLayout [])))))

(defn- check [rc]
  (when-not (zero? (int rc))
    (let [^MemorySegment msg (.invokeWithArguments ^MethodHandle @h-error [])]
      (throw (ex-info (str "libhnswgpu: " (.getString (.reinterpret msg 512) 0)) {:code rc})))))

(def ^:private metric-of {:cosine 0 :l2 1 :euclidean 1 :dot 2})

(defrecord GpuIndex [handle ids dim kind])

(defn- floats-of ^MemorySegment [^Arena arena rows dim]
  ;; [id double-array] pairs -> one contiguous float32 matrix (the engine stores f32)
  (let [n (count rows)
        seg (.allocate arena (* 4 (long n) (long dim)) 16)]
    (dotimes [i n]
      (let [^doubles v (nth rows i)]
        (dotimes [j dim]
          (.setAtIndex seg ValueLayout/JAVA_FLOAT (+ (* (long i) dim) j) (float (aget v j))))))
    seg))

(defn- create [data metric kind]
  (with-open [arena (Arena/ofConfined)]
    (let [ids (mapv first data)
          vecs (mapv second data)
          dim (if (seq vecs) (alength ^doubles (first vecs)) 1)
          base (floats-of arena vecs dim)
          out (.allocate arena 8 8)]
      (check (.invokeWithArguments ^MethodHandle @h-create
                                   [base (long (count ids)) (int dim) (int (metric-of metric 0)) (int 0) out]))
      (->GpuIndex (.get out P 0) ids dim kind))))

(def ^:private build-flag {:sequential 1 :heuristic 2 :symmetric 4 :extend 8})   ; include/hnswgpu.h: HNSWGPU_BUILD_*

(defn build-index
  "hnsw.ultra-fast/build-index (src/hnsw/ultra_fast.clj:334-344): data = seq of [id ^doubles vector].
   :select :closest   the m closest candidates (insert-single / prune-connections-ultra, ultra_fast.clj:216-299; default)
           :heuristic get-neighbors-heuristic for a node's links and for an over-full list (src/hnsw/graph.clj:162-232),
                      the dropped edge leaving the pruned list only
           :graph-clj the same, the dropped edge removed from both lists (prune-connections, graph.clj:226-231): what
                      hnsw.ann.graph.pure-hnsw/build-index builds
   :sequential? true  insert-single's own order and start level (slow: one launch round trip per row)."
  [data & {:keys [M ef-construction metric seed select sequential?]
           :or {M 16 ef-construction 200 metric :cosine seed 42 select :closest sequential? false}}]
  (let [idx (create data metric :hnsw)
        flags (bit-or (case select :closest 0 :heuristic 2 :graph-clj 6)
                      (if sequential? (build-flag :sequential) 0))]
    (check (.invokeWithArguments ^MethodHandle @h-build [(:handle idx) (int M) (int ef-construction) (long seed) (int flags)]))
    idx))

(def ^:private h-add (delay (fn-handle "hnswgpu_hnsw_add" (FunctionDescriptor/of I (into-array [P P L I L])))))

(defn add-vector!
  "hnsw.api/add-vector! (src/hnsw/api.clj:30-33) / ultra-fast insert-single (src/hnsw/ultra_fast.clj:216-275) on a live
   GpuIndex: the new [id ^doubles vector] pairs join the base matrix and the graph; returns the index with their ids
   appended (a GpuIndex is a value: keep the returned one).  One call per batch of new vectors is the efficient shape."
  [idx new-data & {:keys [ef-construction seed] :or {ef-construction 200 seed 42}}]
  (with-open [arena (Arena/ofConfined)]
    (check (.invokeWithArguments ^MethodHandle @h-add
                                 [(:handle idx) (floats-of arena (mapv second new-data) (:dim idx)) (long (count new-data))
                                  (int ef-construction) (long seed)])))
  (update idx :ids into (map first new-data)))

(def ^:private h-ivfadd (delay (fn-handle "hnswgpu_ivf_add" (FunctionDescriptor/of I (into-array [P P L])))))

(defn add-ivf-vectors!
  "add-vector! (src/hnsw/api.clj:30-33) for a live IVF-FLAT GpuIndex (the reference's IVFFlatIndex is an immutable record): the new
   [id ^doubles vector] pairs join the base matrix, each behind the present members of its nearest partition (ivf_flat.clj:79-90);
   the centroids stay.  Returns the index with their ids appended.  One call per batch of new vectors is the efficient shape."
  [idx new-data]
  (with-open [arena (Arena/ofConfined)]
    (check (.invokeWithArguments ^MethodHandle @h-ivfadd
                                 [(:handle idx) (floats-of arena (mapv second new-data) (:dim idx)) (long (count new-data))])))
  (update idx :ids into (map first new-data)))

(declare ints-of)

(def ^:private h-ivfremove (delay (fn-handle "hnswgpu_ivf_remove" (FunctionDescriptor/of I (into-array [P P L P])))))

(defn remove-ivf-vectors!
  "The inverse of add-ivf-vectors! (the reference's IVFFlatIndex has no remove; what is restated is its list order,
   ivf_flat.clj:137-211): the vectors with the given ids leave the base matrix and their partitions, a partition's kept members
   stay in their order, the centroids stay, and the kept rows are renumbered densely in their old order (hnswgpu_ivf_remove).  An
   unknown id throws before the device is touched.  Returns the index with the ids removed.  One call per batch is the efficient
   shape: a call copies the kept rows once, whatever it removes.  Unverified like the rest of this namespace: no JVM where the
   library is built."
  [idx ids]
  (let [gone (set ids)
        known (set (:ids idx))]
    (when-let [bad (first (remove known gone))]
      (throw (ex-info "remove-ivf-vectors!: unknown id" {:id bad})))
    (if (empty? gone)
      idx
      (let [rows (vec (keep-indexed (fn [i id] (when (gone id) i)) (:ids idx)))]
        (with-open [arena (Arena/ofConfined)]
          (let [n-after (.allocate arena 8 8)]
            (check (.invokeWithArguments ^MethodHandle @h-ivfremove
                                         [(:handle idx) (ints-of arena rows) (long (count rows)) n-after]))
            (let [kept (vec (remove gone (:ids idx)))]
              (assert (= (count kept) (.getAtIndex n-after L 0)))
              (assoc idx :ids kept))))))))

(def ^:private h-ivfupdate (delay (fn-handle "hnswgpu_ivf_update" (FunctionDescriptor/of I (into-array [P P P L])))))

(defn update-ivf-vectors!
  "\"Update existing vectors\" (the open item of the reference's to-do list; its IVFFlatIndex is an immutable record) for a live
   IVF-FLAT GpuIndex: new-data is a seq of [id ^doubles vector]; the vector stored under each id takes the new values and moves to
   its nearest partition if that is another one (ivf_flat.clj:79-90) -- behind the members that remain there --, and keeps its id;
   a vector whose partition stays keeps its place in it; the centroids stay (hnswgpu_ivf_update).  An unknown id, an id that names
   several rows and an id given twice throw before the device is touched.  Returns the index (its ids are unchanged).  One call
   per batch is the efficient shape: a call copies the rows once, whatever it updates.  Unverified like the rest of this
   namespace: no JVM where the library is built."
  [idx new-data]
  (let [rows-of (reduce (fn [m [i id]] (update m id (fnil conj []) i)) {} (map-indexed vector (:ids idx)))
        ids (mapv first new-data)]
    (doseq [id ids]
      (when-not (contains? rows-of id) (throw (ex-info "update-ivf-vectors!: unknown id" {:id id})))
      (when (> (count (rows-of id)) 1) (throw (ex-info "update-ivf-vectors!: the id names several rows" {:id id}))))
    (when-not (or (empty? ids) (apply distinct? ids))
      (throw (ex-info "update-ivf-vectors!: an id is given twice" {})))
    (when (seq ids)
      (with-open [arena (Arena/ofConfined)]
        (check (.invokeWithArguments ^MethodHandle @h-ivfupdate
                                     [(:handle idx) (ints-of arena (mapv (comp first rows-of) ids))
                                      (floats-of arena (mapv second new-data) (:dim idx)) (long (count ids))]))))
    idx))

(def ^:private h-hnswremove (delay (fn-handle "hnswgpu_hnsw_remove" (FunctionDescriptor/of I (into-array [P P L P])))))

(defn remove-vectors!
  "The inverse of add-vector! for a live HNSW GpuIndex (the reference has no delete: pure_hnsw.clj:16 is a todo; the repair rule
   is the engine's own, hnswgpu_hnsw_remove): the vectors with the given ids leave the base matrix and the graph, the kept rows are
   renumbered densely in their old order, a neighbour list that loses no member stays as it is, and a list that loses one is
   selected again -- as the index's builder prunes an over-full list -- from its kept members and the kept members of the lists of
   the members that left.  No back edges are added, and the result depends on how a removal is split over calls.  An unknown id
   throws before the device is touched.  Returns the index with the ids removed.  One call per batch is the efficient shape.
   Unverified like the rest of this namespace: no JVM where the library is built."
  [idx ids]
  (let [gone (set ids)
        known (set (:ids idx))]
    (when-let [bad (first (remove known gone))]
      (throw (ex-info "remove-vectors!: unknown id" {:id bad})))
    (if (empty? gone)
      idx
      (let [rows (vec (keep-indexed (fn [i id] (when (gone id) i)) (:ids idx)))]
        (with-open [arena (Arena/ofConfined)]
          (let [n-after (.allocate arena 8 8)]
            (check (.invokeWithArguments ^MethodHandle @h-hnswremove
                                         [(:handle idx) (ints-of arena rows) (long (count rows)) n-after]))
            (let [kept (vec (remove gone (:ids idx)))]
              (assert (= (count kept) (.getAtIndex n-after L 0)))
              (assoc idx :ids kept))))))))

(def ^:private h-hnswupdate (delay (fn-handle "hnswgpu_hnsw_update" (FunctionDescriptor/of I (into-array [P P P L I])))))

(defn update-vectors!
  "\"Update existing vectors\" (the open item of the reference's to-do list; the rule is the engine's own, hnswgpu_hnsw_update) for
   a live HNSW GpuIndex: new-data is a seq of [id ^doubles vector]; the vector stored under each id takes the new values and keeps
   its id and its level.  It is unlinked as remove-vectors! unlinks a vector that leaves -- nothing is renumbered -- and inserted
   again as add-vector! inserts one, with :ef-construction (default 200).  The result depends on how an update is split over calls,
   and a vector updated to the values it has is still linked anew.  An unknown id, an id that names several rows and an id given
   twice throw before the device is touched.  Returns the index (its ids are unchanged).  One call per batch is the efficient
   shape: a call copies the rows once, whatever it updates.  Unverified like the rest of this namespace: no JVM where the library
   is built."
  [idx new-data & {:keys [ef-construction] :or {ef-construction 200}}]
  (let [rows-of (reduce (fn [m [i id]] (update m id (fnil conj []) i)) {} (map-indexed vector (:ids idx)))
        ids (mapv first new-data)]
    (doseq [id ids]
      (when-not (contains? rows-of id) (throw (ex-info "update-vectors!: unknown id" {:id id})))
      (when (> (count (rows-of id)) 1) (throw (ex-info "update-vectors!: the id names several rows" {:id id}))))
    (when-not (or (empty? ids) (apply distinct? ids))
      (throw (ex-info "update-vectors!: an id is given twice" {})))
    (when (seq ids)
      (with-open [arena (Arena/ofConfined)]
        (check (.invokeWithArguments ^MethodHandle @h-hnswupdate
                                     [(:handle idx) (ints-of arena (mapv (comp first rows-of) ids))
                                      (floats-of arena (mapv second new-data) (:dim idx)) (long (count ids)) (int ef-construction)]))))
    idx))

;; ---- hybrid LSH (hnsw.ann.hash.hybrid-lsh): hnswgpu_lsh_build / hnswgpu_lsh_search ----
(def ^:private h-lshbuild  (delay (fn-handle "hnswgpu_lsh_build" (FunctionDescriptor/of I (into-array [P I I I L])))))
(def ^:private h-lshset    (delay (fn-handle "hnswgpu_set_lsh" (FunctionDescriptor/of I (into-array [P P I I])))))
(def ^:private h-lshsearch (delay (fn-handle "hnswgpu_lsh_search" (FunctionDescriptor/of I (into-array [P P I I I I I I P P])))))

(defn build-lsh-index
  "hnsw.ann.hash.hybrid-lsh/build-lsh-index (src/hnsw/ann/hash/hybrid_lsh.clj:66-145): data = seq of [id ^doubles vector].  The
   defaults are the reference's constants (:12-14) and its (Random. 42): the same hyperplanes, rounded to float.  :planes, a seq of
   tables of `bits` ^doubles rows, installs the caller's matrices instead (hnswgpu_set_lsh).  The metric is the handle's (the
   reference computes cosine whatever :distance-fn says)."
  [data & {:keys [metric tables bits projection-dim seed planes]
           :or {metric :cosine tables 8 bits 12 projection-dim 64 seed 42}}]
  (let [idx (create data metric :hybrid-lsh)]
    (if planes
      (with-open [arena (Arena/ofConfined)]
        (check (.invokeWithArguments ^MethodHandle @h-lshset
                                     [(:handle idx) (floats-of arena (vec (apply concat planes)) (:dim idx))
                                      (int (count planes)) (int (count (first planes)))])))
      (check (.invokeWithArguments ^MethodHandle @h-lshbuild
                                   [(:handle idx) (int tables) (int bits) (int projection-dim) (long seed)])))
    idx))

(def ^:private h-lshadd (delay (fn-handle "hnswgpu_lsh_add" (FunctionDescriptor/of I (into-array [P P L])))))

(defn add-lsh-vectors!
  "add-vector! (src/hnsw/api.clj:30-33) for a live hybrid-LSH GpuIndex (the reference's index has no add; what is restated is its
   bucket order, hybrid_lsh.clj:105-129): the new [id ^doubles vector] pairs join the base matrix and, hashed under the index's
   hyperplanes, every table's buckets behind a bucket's present members.  Returns the index with their ids appended.  One call per
   batch of new vectors is the efficient shape."
  [idx new-data]
  (with-open [arena (Arena/ofConfined)]
    (check (.invokeWithArguments ^MethodHandle @h-lshadd
                                 [(:handle idx) (floats-of arena (mapv second new-data) (:dim idx)) (long (count new-data))])))
  (update idx :ids into (map first new-data)))

(def ^:private h-lshremove (delay (fn-handle "hnswgpu_lsh_remove" (FunctionDescriptor/of I (into-array [P P L P])))))

(defn remove-lsh-vectors!
  "The inverse of add-lsh-vectors! (the reference's index has no remove either; what is restated is its bucket order,
   hybrid_lsh.clj:105-129): the vectors with the given ids leave the base matrix and every table's buckets, a bucket's kept members
   stay in their order, and the kept rows are renumbered densely in their old order (hnswgpu_lsh_remove).  An unknown id throws
   before the device is touched.  Returns the index with the ids removed.  One call per batch is the efficient shape: a call
   copies the kept rows once, whatever it removes.  Unverified like the rest of this namespace: no JVM where the library is built."
  [idx ids]
  (let [gone (set ids)
        known (set (:ids idx))]
    (when-let [bad (first (remove known gone))]
      (throw (ex-info "remove-lsh-vectors!: unknown id" {:id bad})))
    (if (empty? gone)
      idx
      (let [rows (vec (keep-indexed (fn [i id] (when (gone id) i)) (:ids idx)))]
        (with-open [arena (Arena/ofConfined)]
          (let [n-after (.allocate arena 8 8)]
            (check (.invokeWithArguments ^MethodHandle @h-lshremove
                                         [(:handle idx) (ints-of arena rows) (long (count rows)) n-after]))
            (let [kept (vec (remove gone (:ids idx)))]
              (assert (= (count kept) (.getAtIndex n-after L 0)))
              (assoc idx :ids kept))))))))

(def ^:private h-lshupdate (delay (fn-handle "hnswgpu_lsh_update" (FunctionDescriptor/of I (into-array [P P P L])))))

(defn update-lsh-vectors!
  "\"Update existing vectors\" (the open item of the reference's to-do list; its HybridIndex is an immutable record) for a live
   hybrid-LSH GpuIndex: new-data is a seq of [id ^doubles vector]; the vector stored under each id takes the new values, is hashed
   again under the index's hyperplanes and, in every table where its code changed, moves to its new bucket at the place its row
   gives it (hybrid_lsh.clj:105-129: a bucket lists its rows in row order), and keeps its id (hnswgpu_lsh_update).  An unknown id, an
   id that names several rows and an id given twice throw before the device is touched.  Returns the index (its ids are
   unchanged).  One call per batch is the efficient shape: a call copies the rows once, whatever it updates.  Unverified like the
   rest of this namespace: no JVM where the library is built."
  [idx new-data]
  (let [rows-of (reduce (fn [m [i id]] (update m id (fnil conj []) i)) {} (map-indexed vector (:ids idx)))
        ids (mapv first new-data)]
    (doseq [id ids]
      (when-not (contains? rows-of id) (throw (ex-info "update-lsh-vectors!: unknown id" {:id id})))
      (when (> (count (rows-of id)) 1) (throw (ex-info "update-lsh-vectors!: the id names several rows" {:id id}))))
    (when-not (or (empty? ids) (apply distinct? ids))
      (throw (ex-info "update-lsh-vectors!: an id is given twice" {})))
    (when (seq ids)
      (with-open [arena (Arena/ofConfined)]
        (check (.invokeWithArguments ^MethodHandle @h-lshupdate
                                     [(:handle idx) (ints-of arena (mapv (comp first rows-of) ids))
                                      (floats-of arena (mapv second new-data) (:dim idx)) (long (count ids))]))))
    idx))

(def ^:private lsh-modes {:turbo [2 1] :fast [4 1] :balanced [6 2] :accurate [8 3] :precise [8 4]})   ; hybrid_lsh.clj:350-364

(declare results)

(defn search-lsh-batch
  "search-hybrid-multiprobe (hybrid_lsh.clj:261-342, the order of its sequential branch) for a batch in one call: 2k rows of the own
   bucket, k of every one-bit neighbour, per probed table; :mode as search-knn's (:350-364), or :num-probes / :probe-radius."
  [idx queries k & {:keys [mode num-probes probe-radius]}]
  (let [[p r] (lsh-modes mode (lsh-modes :balanced))
        p (or num-probes p)
        r (or probe-radius r)]
    (if (empty? (:ids idx))
      (mapv (constantly []) queries)
      (with-open [arena (Arena/ofConfined)]
        (let [nq (count queries)
              q (floats-of arena (vec queries) (:dim idx))
              ids (.allocate arena (* 4 nq k) 4)
              ds (.allocate arena (* 4 nq k) 4)]
          (check (.invokeWithArguments ^MethodHandle @h-lshsearch
                                       [(:handle idx) q (int nq) (int k) (int p) (int r) (int (* 2 k)) (int k) ids ds]))
          (mapv #(results idx ids ds % k) (range nq)))))))

(defn search-lsh
  "hybrid-lsh/search-knn (hybrid_lsh.clj:350-364) for one query."
  [idx query-vec k & opts]
  (first (apply search-lsh-batch idx [query-vec] k opts)))

;; ---- hybrid LSH filtered search: the allow-mask through the bucket scan (hnswgpu_lsh_search_filtered / _each) ----
(def ^:private h-lshsearch-filtered
  (delay (fn-handle "hnswgpu_lsh_search_filtered" (FunctionDescriptor/of I (into-array [P P I I I I I I P P P])))))
(def ^:private h-lshsearch-filtered-each
  (delay (fn-handle "hnswgpu_lsh_search_filtered_each" (FunctionDescriptor/of I (into-array [P P I I I I I I P P P])))))

(defn- lsh-mask-of
  "filter-fn on the caller's ids -> the (n + 31) / 32 words of an allow-mask (bit (i & 31) of word i >> 5, indexed by row)."
  ^ints [idx filter-fn words]
  (let [m (int-array words)]
    (doseq [i (range (count (:ids idx))) :when (filter-fn (nth (:ids idx) i))]
      (aset m (quot i 32) (unchecked-int (bit-or (aget m (quot i 32)) (bit-shift-left 1 (rem i 32))))))
    m))

(defn search-lsh-batch-filtered
  "search-knn-filtered* over the probed buckets for a batch with ONE predicate on the caller's ids, evaluated once per row here
   into the call's allow-mask.  The device tests the bit where a bucket is read and keeps the 2k / k nearest PASSING rows of every
   probed bucket: search-hybrid-multiprobe over buckets that list only the passing rows -- not protocol.clj:97-102's search 3k,
   drop, keep k.  :mode / :num-probes / :probe-radius as search-lsh-batch."
  [idx queries k filter-fn & {:keys [mode num-probes probe-radius]}]
  (let [[p r] (lsh-modes mode (lsh-modes :balanced))
        p (or num-probes p)
        r (or probe-radius r)]
    (if (or (empty? (:ids idx)) (empty? queries))
      (mapv (constantly []) queries)
      (with-open [arena (Arena/ofConfined)]
        (let [nq (count queries)
              words (quot (+ (count (:ids idx)) 31) 32)
              mask (.allocate arena (* 4 words) 4)
              _ (MemorySegment/copy (MemorySegment/ofArray (lsh-mask-of idx filter-fn words)) 0 mask 0 (* 4 words))
              q (floats-of arena (vec queries) (:dim idx))
              ids (.allocate arena (* 4 nq k) 4)
              ds (.allocate arena (* 4 nq k) 4)]
          (check (.invokeWithArguments ^MethodHandle @h-lshsearch-filtered
                                       [(:handle idx) q (int nq) (int k) (int p) (int r) (int (* 2 k)) (int k) mask ids ds]))
          (mapv #(results idx ids ds % k) (range nq)))))))

(defn search-lsh-filtered
  "One query through search-lsh-batch-filtered: seq of {:id :distance} ascending, fewer than k when fewer passing rows are found."
  [idx query-vec k filter-fn & opts]
  (first (apply search-lsh-batch-filtered idx [query-vec] k filter-fn opts)))

(defn search-lsh-batch-filtered-each
  "search-lsh-batch-filtered with one predicate PER QUERY (filter-fns: as many as queries): result q is
   (search-lsh-filtered idx (nth queries q) k (nth filter-fns q) ...).  An identical predicate is evaluated once; the batch goes
   through one hnswgpu_lsh_search_filtered_each call, equal predicates adjacent, and the caller's order is restored.  One
   predicate for the whole batch: search-lsh-batch-filtered."
  [idx queries k filter-fns & {:keys [mode num-probes probe-radius] :as opts}]
  (assert (= (count queries) (count filter-fns)) "one filter-fn per query")
  (cond
    (empty? queries) []
    (empty? (:ids idx)) (mapv (constantly []) queries)
    (every? #(identical? % (first filter-fns)) filter-fns)
    (apply search-lsh-batch-filtered idx queries k (first filter-fns) (mapcat identity opts))
    :else
    (let [[p r] (lsh-modes mode (lsh-modes :balanced))
          p (or num-probes p)
          r (or probe-radius r)
          words (quot (+ (count (:ids idx)) 31) 32)
          distinct-fns (vec (distinct filter-fns))
          fn-no (into {} (map-indexed (fn [i f] [f i]) distinct-fns))
          masks (mapv #(lsh-mask-of idx % words) distinct-fns)
          qs (vec (sort-by (fn [q] [(fn-no (nth filter-fns q)) q]) (range (count queries))))
          nq (count qs)
          out (object-array nq)]
      (with-open [arena (Arena/ofConfined)]
        (let [mask (.allocate arena (* 4 words nq) 4)
              _ (doseq [[j q] (map-indexed vector qs)]
                  (MemorySegment/copy (MemorySegment/ofArray ^ints (masks (fn-no (nth filter-fns q)))) 0
                                      mask (* 4 words j) (* 4 words)))
              qa (floats-of arena (mapv #(nth queries %) qs) (:dim idx))
              ids (.allocate arena (* 4 nq k) 4)
              ds (.allocate arena (* 4 nq k) 4)]
          (check (.invokeWithArguments ^MethodHandle @h-lshsearch-filtered-each
                                       [(:handle idx) qa (int nq) (int k) (int p) (int r) (int (* 2 k)) (int k) mask ids ds]))
          (doseq [[j q] (map-indexed vector qs)]
            (aset out q (results idx ids ds j k)))))
      (vec out))))

(defn- results [idx ^MemorySegment ids ^MemorySegment ds q k]
  (vec (for [i (range k)
             :let [id (.getAtIndex ids I (+ (* (long q) k) i))]
             :when (>= id 0)]
         {:id (nth (:ids idx) id) :distance (double (.getAtIndex ds ValueLayout/JAVA_FLOAT (+ (* (long q) k) i)))})))

(defn search-batch
  "All queries in one kernel launch -> vector of result vectors (BatchSearchIndex/search-batch*,
   src/hnsw/api/protocol.clj:58-67; replaces helper/parallel_search.clj:15-49)."
  [idx queries k & {:keys [ef] :or {ef 0}}]
  (with-open [arena (Arena/ofConfined)]
    (let [nq (count queries)
          q (floats-of arena (vec queries) (:dim idx))
          ids (.allocate arena (* 4 nq k) 4)
          ds (.allocate arena (* 4 nq k) 4)]
      (check (.invokeWithArguments ^MethodHandle @h-search
                                   [(:handle idx) q (int nq) (int k) (int ef) ids ds MemorySegment/NULL]))
      (mapv #(results idx ids ds % k) (range nq)))))

(defn search-knn
  "hnsw.ultra-fast/search-knn (src/hnsw/ultra_fast.clj:346-374): seq of {:id :distance} ascending."
  [idx ^doubles query-vec k]
  (first (search-batch idx [query-vec] k)))

;; ---- a forest: several HNSW sub-graphs on one handle, searched in one launch (include/hnswgpu.h: hnswgpu_hnsw_build_parts) ----
(def ^:private h-buildparts
  (delay (fn-handle "hnswgpu_hnsw_build_parts" (FunctionDescriptor/of I (into-array [P I P I I L I])))))
(def ^:private h-searchparts
  (delay (fn-handle "hnswgpu_hnsw_search_parts" (FunctionDescriptor/of I (into-array [P P I I I P I I P P P])))))

(defn build-forest
  "hnsw.ann.partition.partitioned-hnsw/build-index (src/hnsw/ann/partition/partitioned_hnsw.clj:46-143) and the graphs of
   hnsw.ann.hybrid.ivf-hnsw (src/hnsw/ann/hybrid/ivf_hnsw.clj:172-280) on ONE handle: `partitions` is a seq of partitions, each a
   seq of [id ^doubles vector]; their rows are laid out one partition behind the other (the id table follows that order) and every
   partition gets the graph build-index would give it alone.  An empty partition is allowed.  :select as in build-index."
  [partitions & {:keys [M ef-construction metric seed select] :or {M 16 ef-construction 200 metric :cosine seed 42 select :closest}}]
  (let [idx (create (vec (apply concat partitions)) metric :hnsw-forest)
        offs (long-array (reductions + 0 (map count partitions)))]
    (with-open [arena (Arena/ofConfined)]
      (let [seg (.allocate arena (* 8 (alength offs)) 8)]
        (dotimes [i (alength offs)] (.setAtIndex seg L (long i) (aget offs i)))
        (check (.invokeWithArguments ^MethodHandle @h-buildparts
                                     [(:handle idx) (int (count partitions)) seg (int M) (int ef-construction) (long seed)
                                      (int (case select :closest 0 :heuristic 2 :graph-clj 6))]))))
    (assoc idx :nparts (count partitions))))

(defn search-forest-batch
  "search-partitioned (partitioned_hnsw.clj:149-196) / search-ivf-hnsw (ivf_hnsw.clj:286-325) for a batch, in one traversal launch:
   every probed partition's graph is searched for k-part results per query, the lists are merged in probe order (a stable sort of
   the concatenation), take k.  :probes = per query a seq of partition numbers (-1 = none; all the same length), nil = every
   partition in order."
  [idx queries k-part k & {:keys [ef probes] :or {ef 0}}]
  (with-open [arena (Arena/ofConfined)]
    (let [nq (count queries)
          q (floats-of arena (vec queries) (:dim idx))
          nprobe (if probes (count (first probes)) (:nparts idx))
          pr (if probes
               (let [seg (.allocate arena (* 4 (long nq) (long nprobe)) 4)]
                 (doseq [[i row] (map-indexed vector probes) [j p] (map-indexed vector row)]
                   (.setAtIndex seg I (+ (* (long i) nprobe) (long j)) (int p)))
                 seg)
               MemorySegment/NULL)
          ids (.allocate arena (* 4 nq k) 4)
          ds (.allocate arena (* 4 nq k) 4)]
      (check (.invokeWithArguments ^MethodHandle @h-searchparts
                                   [(:handle idx) q (int nq) (int k-part) (int ef) pr (int nprobe) (int k) ids ds MemorySegment/NULL]))
      (mapv #(results idx ids ds % k) (range nq)))))

(defn search-batch-routed
  "search-batch with the crossover the device offers and the reference has no word for: the traversal evaluates E(ef) rows per
   query, gathered at random; the exact scan (hnswgpu_exact_knn: every row once per batch through the matrix cores) answers at
   recall 1.0 -- the cheaper way to at least the same recall once E(ef) >= n / 3 (31k x 768: 1.5M QPS exact against 0.78M through
   the graph at ef 640, 90k at ef 3200).  E(ef) comes from the traversal's own counters (the `stats` argument of
   hnswgpu_hnsw_search: evals, expansions per query) on up to 32 of the queries.  The neighbours of a routed batch are the
   exact ones: at least as good as the graph's, not necessarily the same (hnsw-clj_amd/ultra_fast.py: search_batch route=True)."
  [idx queries k & {:keys [ef] :or {ef 0}}]
  (with-open [arena (Arena/ofConfined)]
    (let [pilot (vec (take 32 queries))
          np (count pilot)
          q (floats-of arena pilot (:dim idx))
          ids (.allocate arena (* 4 np k) 4)
          ds (.allocate arena (* 4 np k) 4)
          st (.allocate arena (* 16 np) 8)]
      (check (.invokeWithArguments ^MethodHandle @h-search [(:handle idx) q (int np) (int k) (int ef) ids ds st]))
      (let [evals (/ (reduce + (map #(.getAtIndex st ValueLayout/JAVA_LONG (* 2 (long %))) (range np))) (double np))]
        (if (>= evals (/ (count (:ids idx)) 3.0))
          (let [nq (count queries)
                qa (floats-of arena (vec queries) (:dim idx))
                ia (.allocate arena (* 4 nq k) 4)
                da (.allocate arena (* 4 nq k) 4)]
            (check (.invokeWithArguments ^MethodHandle @h-exact [(:handle idx) qa (int nq) (int k) ia da]))
            (mapv #(results idx ia da % k) (range nq)))
          (search-batch idx queries k :ef ef))))))

;; ---- filtered search (FilterableIndex/search-knn-filtered*, src/hnsw/api/protocol.clj:34-41,97-102) ----
(def ^:private h-exact-filtered
  (delay (fn-handle "hnswgpu_exact_knn_filtered" (FunctionDescriptor/of I (into-array [P P I I P P P])))))
(def ^:private h-search-filtered
  (delay (fn-handle "hnswgpu_hnsw_search_filtered" (FunctionDescriptor/of I (into-array [P P I I I P P P P])))))

(defn filtered-plan
  "[:scan | :graph, ef'] for n rows of which p pass (hnsw-clj_amd/ultra_fast.py: filtered_plan): the reference over-fetches by 3
   (protocol.clj:101), so a result list must hold ef-need = ceil(3 k n / p) entries to expect 3k passing ones; the exact scan of
   the passing rows serves the call when nothing passes, when ef-need exceeds the 1024 list entries the filtered traversal
   looks at, or when p <= ef'."
  [n p k ef]
  (let [ef0 (if (pos? ef) ef (max k 50))]
    (if (zero? p)
      [:scan ef0]
      (let [ef-need (quot (+ (* 3 k n) (dec p)) p)
            ef2 (max ef0 ef-need)]
        [(if (or (> ef-need 1024) (<= p ef2)) :scan :graph) ef2]))))

(defn search-batch-filtered
  "search-knn-filtered* for a batch with ONE predicate on the caller's ids, evaluated once per row here into the call's
   allow-mask ((n + 31) / 32 words, bit (i & 31) of word i >> 5).  :graph walks the graph at ef' and keeps the first k passing
   entries of every result list; :scan returns the EXACT k nearest passing rows."
  [idx queries k filter-fn & {:keys [ef] :or {ef 0}}]
  (with-open [arena (Arena/ofConfined)]
    (let [n (count (:ids idx))
          nq (count queries)
          words (quot (+ n 31) 32)
          mask (.allocate arena (* 4 (max words 1)) 4)
          _ (.fill mask (byte 0))
          p (reduce (fn [p i]
                      (if (filter-fn (nth (:ids idx) i))
                        (let [w (quot i 32)]
                          (.setAtIndex mask I (long w) (unchecked-int (bit-or (.getAtIndex mask I (long w))
                                                                               (bit-shift-left 1 (rem i 32)))))
                          (inc p))
                        p))
                    0 (range n))
          [plan ef2] (filtered-plan n p k ef)
          q (floats-of arena (vec queries) (:dim idx))
          ids (.allocate arena (* 4 nq k) 4)
          ds (.allocate arena (* 4 nq k) 4)]
      (if (= plan :scan)
        (check (.invokeWithArguments ^MethodHandle @h-exact-filtered [(:handle idx) q (int nq) (int k) mask ids ds]))
        (check (.invokeWithArguments ^MethodHandle @h-search-filtered
                                     [(:handle idx) q (int nq) (int k) (int ef2) mask ids ds MemorySegment/NULL])))
      (mapv #(results idx ids ds % k) (range nq)))))

(def ^:private h-exact-filtered-each
  (delay (fn-handle "hnswgpu_exact_knn_filtered_each" (FunctionDescriptor/of I (into-array [P P I I P P P])))))
(def ^:private h-search-filtered-each
  (delay (fn-handle "hnswgpu_hnsw_search_filtered_each" (FunctionDescriptor/of I (into-array [P P I I I P P P P])))))

(defn search-batch-filtered-each
  "search-knn-filtered* for a batch with one predicate PER QUERY (filter-fns: as many as queries): result q is
   (search-knn-filtered idx (nth queries q) k (nth filter-fns q)).  An identical predicate is evaluated once.  filtered-plan is
   applied per query; the :scan queries go in one hnswgpu_exact_knn_filtered_each call, ordered so that equal predicates are
   adjacent (a query group then shares the rows it fetches), the :graph queries in one hnswgpu_hnsw_search_filtered_each call
   per distinct ef'; the caller's order is restored.  One predicate for the whole batch: search-batch-filtered."
  [idx queries k filter-fns & {:keys [ef] :or {ef 0}}]
  (assert (= (count queries) (count filter-fns)) "one filter-fn per query")
  (if (and (seq filter-fns) (every? #(identical? % (first filter-fns)) filter-fns))
    (search-batch-filtered idx queries k (first filter-fns) :ef ef)
    (let [n (count (:ids idx))
          words (max 1 (quot (+ n 31) 32))
          distinct-fns (vec (distinct filter-fns))
          fn-no (into {} (map-indexed (fn [i f] [f i]) distinct-fns))
          masks (mapv (fn [f]                                   ; per distinct predicate: its words and its passing count
                        (let [m (int-array words)]
                          [m (reduce (fn [p i]
                                       (if (f (nth (:ids idx) i))
                                         (do (aset m (quot i 32) (unchecked-int (bit-or (aget m (quot i 32)) (bit-shift-left 1 (rem i 32)))))
                                             (inc p))
                                         p))
                                     0 (range n))]))
                      distinct-fns)
          call-of (fn [q] (let [[plan ef2] (filtered-plan n (second (masks (fn-no (nth filter-fns q)))) k ef)]
                            (if (= plan :scan) [:scan 0] [:graph ef2])))
          out (object-array (count queries))]
      (doseq [[[plan ef2] qs] (group-by call-of (range (count queries)))]
        (with-open [arena (Arena/ofConfined)]
          (let [qs (vec (sort-by (fn [q] [(fn-no (nth filter-fns q)) q]) qs))
                nq (count qs)
                mask (.allocate arena (* 4 words nq) 4)
                _ (doseq [[j q] (map-indexed vector qs)]
                    (MemorySegment/copy (MemorySegment/ofArray ^ints (first (masks (fn-no (nth filter-fns q))))) 0
                                        mask (* 4 words j) (* 4 words)))
                qa (floats-of arena (mapv #(nth queries %) qs) (:dim idx))
                ids (.allocate arena (* 4 nq k) 4)
                ds (.allocate arena (* 4 nq k) 4)]
            (if (= plan :scan)
              (check (.invokeWithArguments ^MethodHandle @h-exact-filtered-each [(:handle idx) qa (int nq) (int k) mask ids ds]))
              (check (.invokeWithArguments ^MethodHandle @h-search-filtered-each
                                           [(:handle idx) qa (int nq) (int k) (int ef2) mask ids ds MemorySegment/NULL])))
            (doseq [[j q] (map-indexed vector qs)]
              (aset out q (results idx ids ds j k))))))
      (vec out))))

(defn search-knn-filtered
  "One query through search-batch-filtered: seq of {:id :distance} ascending, fewer than k when fewer rows pass."
  [idx ^doubles query-vec k filter-fn]
  (first (search-batch-filtered idx [query-vec] k filter-fn)))

(defn build-ivf-index
  "hnsw.ann.partition.ivf-flat/build-index (src/hnsw/ann/partition/ivf_flat.clj:137-211,300-303)."
  [data & {:keys [num-partitions max-iterations metric] :or {num-partitions 24 max-iterations 10 metric :cosine}}]
  (let [idx (create data metric :ivf)]
    (check (.invokeWithArguments ^MethodHandle @h-ivfbuild [(:handle idx) (int num-partitions) (int max-iterations) (long 42)]))
    idx))

(defn search-ivf
  "search-ivf-flat (ivf_flat.clj:236-294) with an explicit :num-probes (mode presets :243-247 map to 1/2/4/8/12)."
  [idx ^doubles query-vec k & {:keys [num-probes] :or {num-probes 4}}]
  (with-open [arena (Arena/ofConfined)]
    (let [q (floats-of arena [query-vec] (:dim idx))
          ids (.allocate arena (* 4 k) 4)
          ds (.allocate arena (* 4 k) 4)]
      (check (.invokeWithArguments ^MethodHandle @h-ivfsearch
                                   [(:handle idx) q (int 1) (int k) (int num-probes) ids ds MemorySegment/NULL]))
      (results idx ids ds 0 k))))

(defn search-ivf-batch
  "All queries against the inverted lists in one call (the batch seam of search-ivf-flat)."
  [idx queries k & {:keys [num-probes] :or {num-probes 4}}]
  (with-open [arena (Arena/ofConfined)]
    (let [nq (count queries)
          q (floats-of arena (vec queries) (:dim idx))
          ids (.allocate arena (* 4 nq k) 4)
          ds (.allocate arena (* 4 nq k) 4)]
      (check (.invokeWithArguments ^MethodHandle @h-ivfsearch
                                   [(:handle idx) q (int nq) (int k) (int num-probes) ids ds MemorySegment/NULL]))
      (mapv #(results idx ids ds % k) (range nq)))))

;; ---- IVF-FLAT filtered search: the allow-mask through the list scan (hnswgpu_ivf_search_filtered) ----
(def ^:private h-ivfsearch-filtered
  (delay (fn-handle "hnswgpu_ivf_search_filtered" (FunctionDescriptor/of I (into-array [P P I I I P P P P])))))

(defn search-ivf-batch-filtered
  "search-knn-filtered* over the probed lists for a batch with ONE predicate on the caller's ids, evaluated once per row here
   into the call's allow-mask ((n + 31) / 32 words, bit (i & 31) of word i >> 5, indexed by row).  The device scans exactly
   the passing rows of the probed lists and returns the k nearest of them -- not protocol.clj:97-102's search 3k, drop, keep k."
  [idx queries k filter-fn & {:keys [num-probes] :or {num-probes 4}}]
  (with-open [arena (Arena/ofConfined)]
    (let [n (count (:ids idx))
          nq (count queries)
          words (quot (+ n 31) 32)
          mask (.allocate arena (* 4 (max words 1)) 4)
          _ (.fill mask (byte 0))
          _ (doseq [i (range n) :when (filter-fn (nth (:ids idx) i))]
              (let [w (quot i 32)]
                (.setAtIndex mask I (long w) (unchecked-int (bit-or (.getAtIndex mask I (long w)) (bit-shift-left 1 (rem i 32)))))))
          q (floats-of arena (vec queries) (:dim idx))
          ids (.allocate arena (* 4 nq k) 4)
          ds (.allocate arena (* 4 nq k) 4)]
      (check (.invokeWithArguments ^MethodHandle @h-ivfsearch-filtered
                                   [(:handle idx) q (int nq) (int k) (int num-probes) mask ids ds MemorySegment/NULL]))
      (mapv #(results idx ids ds % k) (range nq)))))

(defn search-ivf-filtered
  "One query through search-ivf-batch-filtered: seq of {:id :distance} ascending, fewer than k when fewer probed rows pass."
  [idx ^doubles query-vec k filter-fn & {:keys [num-probes] :or {num-probes 4}}]
  (first (search-ivf-batch-filtered idx [query-vec] k filter-fn :num-probes num-probes)))

(def ^:private h-ivfsearch-filtered-each
  (delay (fn-handle "hnswgpu_ivf_search_filtered_each" (FunctionDescriptor/of I (into-array [P P I I I P P P P])))))

(defn search-ivf-batch-filtered-each
  "search-ivf-batch-filtered with one predicate PER QUERY (filter-fns: as many as queries): result q is
   (search-ivf-filtered idx (nth queries q) k (nth filter-fns q) :num-probes num-probes).  An identical predicate is evaluated
   once; the batch goes through one hnswgpu_ivf_search_filtered_each call, equal predicates adjacent, and the caller's order is
   restored.  One predicate for the whole batch: search-ivf-batch-filtered."
  [idx queries k filter-fns & {:keys [num-probes] :or {num-probes 4}}]
  (assert (= (count queries) (count filter-fns)) "one filter-fn per query")
  (cond
    (empty? queries) []
    (every? #(identical? % (first filter-fns)) filter-fns)
    (search-ivf-batch-filtered idx queries k (first filter-fns) :num-probes num-probes)
    :else
    (let [n (count (:ids idx))
          words (max 1 (quot (+ n 31) 32))
          distinct-fns (vec (distinct filter-fns))
          fn-no (into {} (map-indexed (fn [i f] [f i]) distinct-fns))
          masks (mapv (fn [f]
                        (let [m (int-array words)]
                          (doseq [i (range n) :when (f (nth (:ids idx) i))]
                            (aset m (quot i 32) (unchecked-int (bit-or (aget m (quot i 32)) (bit-shift-left 1 (rem i 32))))))
                          m))
                      distinct-fns)
          qs (vec (sort-by (fn [q] [(fn-no (nth filter-fns q)) q]) (range (count queries))))
          nq (count qs)
          out (object-array nq)]
      (with-open [arena (Arena/ofConfined)]
        (let [mask (.allocate arena (* 4 words nq) 4)
              _ (doseq [[j q] (map-indexed vector qs)]
                  (MemorySegment/copy (MemorySegment/ofArray ^ints (masks (fn-no (nth filter-fns q)))) 0
                                      mask (* 4 words j) (* 4 words)))
              qa (floats-of arena (mapv #(nth queries %) qs) (:dim idx))
              ids (.allocate arena (* 4 nq k) 4)
              ds (.allocate arena (* 4 nq k) 4)]
          (check (.invokeWithArguments ^MethodHandle @h-ivfsearch-filtered-each
                                       [(:handle idx) qa (int nq) (int k) (int num-probes) mask ids ds MemorySegment/NULL]))
          (doseq [[j q] (map-indexed vector qs)]
            (aset out q (results idx ids ds j k)))))
      (vec out))))

;; ===== the simd-optimized batch seams =====

(defn batch-distances
  "simd-optimized/batch-cosine-distances / batch-euclidean-distances [query vectors] (src/hnsw/simd_optimized.clj:164-184)
   against the vectors the index already holds: distances from query-vec to every row, in row order (a double-array)."
  ^doubles [idx ^doubles query-vec]
  (with-open [arena (Arena/ofConfined)]
    (let [n (count (:ids idx))
          q (floats-of arena [query-vec] (:dim idx))
          out (.allocate arena (* 4 (long n)) 4)]
      (check (.invokeWithArguments ^MethodHandle @h-batchd [(:handle idx) q MemorySegment/NULL (int n) out]))
      (let [res (double-array n)]
        (dotimes [i n] (aset res i (double (.getAtIndex out ValueLayout/JAVA_FLOAT (long i)))))
        res))))

(defn top-k-distances
  "simd-optimized/top-k-distances (src/hnsw/simd_optimized.clj:271-280): exact k nearest rows -> [[row-index distance] ...]."
  [idx ^doubles query-vec k]
  (with-open [arena (Arena/ofConfined)]
    (let [q (floats-of arena [query-vec] (:dim idx))
          ids (.allocate arena (* 4 k) 4)
          ds (.allocate arena (* 4 k) 4)]
      (check (.invokeWithArguments ^MethodHandle @h-exact [(:handle idx) q (int 1) (int k) ids ds]))
      (vec (for [i (range k)
                 :let [id (.getAtIndex ids I (long i))]
                 :when (>= id 0)]
             [id (double (.getAtIndex ds ValueLayout/JAVA_FLOAT (long i)))])))))

;; ===== INTEGRATION.md section 5: serve an index the reference itself built =====

(defn- ints-of ^MemorySegment [^Arena arena coll]
  (let [seg (.allocate arena (* 4 (long (max 1 (count coll)))) 4)]
    (doseq [[i v] (map-indexed vector coll)] (.setAtIndex seg I (long i) (int v)))
    seg))

(defn- longs-of ^MemorySegment [^Arena arena coll]
  (let [seg (.allocate arena (* 8 (long (max 1 (count coll)))) 8)]
    (doseq [[i v] (map-indexed vector coll)] (.setAtIndex seg L (long i) (long v)))
    seg))

(defn from-ultra-graph
  "An UltraGraph built by the reference's own insert-single (src/hnsw/ultra_fast.clj:216-275) -> GpuIndex.
   Flattens UltraNode{id vector level neighbors} (:99-102; neighbors = Object[level+1] of HashSet<String>) into the
   arrays of include/hnswgpu.h: ids -> rows in iteration order of the node map; every neighbour set padded with -1
   to M0 = max-M (level 0) / M (levels >= 1); up_off = prefix sum of the node levels."
  [graph & {:keys [metric] :or {metric :cosine}}]
  (let [nodes (vec (.values ^java.util.Map (.nodes graph)))
        row-of (into {} (map-indexed (fn [i nd] [(.id nd) i]) nodes))
        M (int (.M graph))
        M0 (int (.max-M graph))
        idx (create (mapv (fn [nd] [(.id nd) (.vector nd)]) nodes) metric :hnsw)
        levels (mapv #(int (.level %)) nodes)
        up-off (vec (reductions + 0 levels))
        ;; a neighbour id the node map does not hold, or a set larger than the layer's width, is a broken graph: say so
        ;; here instead of an NPE inside ints-of / a silently truncated HashSet
        pad (fn [ids width]
              (let [rows (mapv (fn [id] (or (row-of id)
                                            (throw (ex-info "neighbour id is not a node of the graph" {:id id}))))
                               ids)]
                (when (> (count rows) width)
                  (throw (ex-info "neighbour set larger than the layer's width (M0 / M)" {:size (count rows) :width width})))
                (take width (concat rows (repeat -1)))))
        nbrs (fn [nd lv] (seq ^java.util.Set (aget ^objects (.neighbors nd) (int lv))))
        l0 (mapcat #(pad (nbrs % 0) M0) nodes)
        up (mapcat (fn [nd] (mapcat #(pad (nbrs nd %) M) (range 1 (inc (.level nd))))) nodes)
        entry (row-of (.get ^java.util.concurrent.atomic.AtomicReference (.entry-point graph)))]
    (with-open [arena (Arena/ofConfined)]
      (check (.invokeWithArguments ^MethodHandle @h-setgraph
                                   [(:handle idx) (ints-of arena levels) (ints-of arena l0) M0
                                    (longs-of arena up-off) (ints-of arena up) M (int entry) (int (nth levels entry))])))
    idx))

(defn from-ivf-flat-index
  "An IVFFlatIndex built by the reference's own k-means (src/hnsw/ann/partition/ivf_flat.clj:137-211) -> GpuIndex:
   centroids + list membership go to hnswgpu_set_ivf (rows = the partitions' vectors, partition by partition)."
  [ivf & {:keys [metric] :or {metric :cosine}}]
  (let [parts (:partitions ivf)
        rows (vec (mapcat identity parts))                 ; [[id ^doubles vec] ...], list by list
        idx (create rows metric :ivf)
        off (vec (reductions + 0 (map count parts)))]
    (with-open [arena (Arena/ofConfined)]
      (check (.invokeWithArguments ^MethodHandle @h-setivf
                                   [(:handle idx) (floats-of arena (vec (:centroids ivf)) (:dim idx)) (int (count parts))
                                    (longs-of arena off) (ints-of arena (range (count rows)))])))
    idx))

;; ===== persistence (helper/index-io save-index / load-index, src/hnsw/helper/index_io.clj:10-80) =====

(defn set-rejection-test!
  "Tuning knob with no counterpart in the reference: the engine decides neighbours / candidates that cannot reach the
   result from an int8 copy of the rows (+25 % memory) and reads f32 rows only for the rest; results never depend on it.
   mode :off (no copy), :auto (default: large HNSW batches, IVF batches of 9+ queries, dim >= 128) or :always."
  [idx mode]
  (check (.invokeWithArguments ^MethodHandle @h-rejmode [(:handle idx) (int ({:off 0 :auto 1 :always 2} mode))]))
  idx)

(defn save
  "One flat binary file (base + graph + lists); the String ids go beside it as EDN -- the engine knows rows only."
  [idx ^String path]
  (with-open [arena (Arena/ofConfined)]
    (check (.invokeWithArguments ^MethodHandle @h-save [(:handle idx) (.allocateFrom arena path)])))
  (spit (str path ".ids.edn") (pr-str {:ids (:ids idx) :kind (:kind idx)}))
  true)

(defn load-index
  "Index instance from `save`'s files; nil if the file does not exist (index_io.clj:41-48 returns nil too)."
  [^String path & {:keys [device] :or {device 0}}]
  (when (.exists (java.io.File. path))
    (with-open [arena (Arena/ofConfined)]
      (let [out (.allocate arena 8 8)
            dim (.allocate arena 4 4)]
        (check (.invokeWithArguments ^MethodHandle @h-load [(.allocateFrom arena path) (int device) out]))
        (let [h (.get out P 0)
              {:keys [ids kind]} (read-string (slurp (str path ".ids.edn")))]
          (check (.invokeWithArguments ^MethodHandle @h-info
                                       [h MemorySegment/NULL dim MemorySegment/NULL MemorySegment/NULL MemorySegment/NULL]))
          (->GpuIndex h ids (.get dim I 0) kind))))))

(defn close! [idx]
  (check (.invokeWithArguments ^MethodHandle @h-destroy [(:handle idx)])))

;; ===== ONE index over several GPUs (include/hnswgpu.h: hnswgpu_group_*) =====
;; search-partitioned's scatter / per-partition top-k / gather / sort / take k (src/hnsw/ann/partition/
;; partitioned_hnsw.clj:149-196) as one native call: the group owns one engine handle per GPU.

(def ^:private h-gcreate  (delay (fn-handle "hnswgpu_group_create" (FunctionDescriptor/of I (into-array [P I I I P])))))
(def ^:private h-gdestroy (delay (fn-handle "hnswgpu_group_destroy" (FunctionDescriptor/of I (into-array [P])))))
(def ^:private h-gsetivf  (delay (fn-handle "hnswgpu_group_set_ivf" (FunctionDescriptor/of I (into-array [P P L P I P P])))))
(def ^:private h-givf     (delay (fn-handle "hnswgpu_group_ivf_search" (FunctionDescriptor/of I (into-array [P P I I I P P])))))
(def ^:private h-gbuild   (delay (fn-handle "hnswgpu_group_hnsw_build" (FunctionDescriptor/of I (into-array [P P L I I L])))))
(def ^:private h-ghnsw    (delay (fn-handle "hnswgpu_group_hnsw_search" (FunctionDescriptor/of I (into-array [P P I I I P P])))))

(defrecord GpuGroup [handle ids dim kind devices])

(defn- group-create [devices dim metric]
  (with-open [arena (Arena/ofConfined)]
    (let [out (.allocate arena 8 8)]
      (check (.invokeWithArguments ^MethodHandle @h-gcreate
                                   [(ints-of arena devices) (int (count devices)) (int dim) (int (metric-of metric 0)) out]))
      (.get out P 0))))

(defn build-partitioned-index
  "hnsw.ann.partition.partitioned-hnsw/build-partitioned-hnsw (partitioned_hnsw.clj:46-143) across GPUs: contiguous row
   ranges, one HNSW sub-graph per device of `devices` (e.g. (range 8)), built on the devices."
  [data devices & {:keys [M ef-construction metric seed] :or {M 16 ef-construction 200 metric :cosine seed 42}}]
  (with-open [arena (Arena/ofConfined)]
    (let [ids (mapv first data)
          vecs (mapv second data)
          dim (alength ^doubles (first vecs))
          h (group-create (vec devices) dim metric)]
      (check (.invokeWithArguments ^MethodHandle @h-gbuild
                                   [h (floats-of arena vecs dim) (long (count ids)) (int M) (int ef-construction) (long seed)]))
      (->GpuGroup h ids dim :hnsw (vec devices)))))

(defn group-from-ivf-flat-index
  "An IVFFlatIndex (the reference's own k-means, ivf_flat.clj:137-211) served by several GPUs: centroids replicated, whole
   inverted lists dealt to the devices by row count.  Answers equal the one-GPU index's bit for bit."
  [ivf devices & {:keys [metric] :or {metric :cosine}}]
  (with-open [arena (Arena/ofConfined)]
    (let [parts (:partitions ivf)
          rows (vec (mapcat identity parts))
          dim (alength ^doubles (second (first rows)))
          off (vec (reductions + 0 (map count parts)))
          h (group-create (vec devices) dim metric)]
      (check (.invokeWithArguments ^MethodHandle @h-gsetivf
                                   [h (floats-of arena (mapv second rows) dim) (long (count rows))
                                    (floats-of arena (vec (:centroids ivf)) dim) (int (count parts))
                                    (longs-of arena off) (ints-of arena (range (count rows)))]))
      (->GpuGroup h (mapv first rows) dim :ivf (vec devices)))))

(defn search-group-batch
  "All queries in one call over all devices -> vector of result vectors.  :ivf groups take :num-probes, :hnsw groups :ef."
  [grp queries k & {:keys [num-probes ef] :or {num-probes 4 ef 50}}]
  (with-open [arena (Arena/ofConfined)]
    (let [nq (count queries)
          q (floats-of arena (vec queries) (:dim grp))
          ids (.allocate arena (* 4 nq k) 4)
          ds (.allocate arena (* 4 nq k) 4)
          ivf? (= :ivf (:kind grp))]
      (check (.invokeWithArguments ^MethodHandle (if ivf? @h-givf @h-ghnsw)
                                   [(:handle grp) q (int nq) (int k) (int (if ivf? num-probes (max ef k))) ids ds]))
      (mapv #(results grp ids ds % k) (range nq)))))

(defn close-group! [grp]
  (check (.invokeWithArguments ^MethodHandle @h-gdestroy [(:handle grp)])))

;; ===== first-class index next to the reference's own records (src/hnsw/api/unified.clj:30-95) =====

(def ^:private mode->probes {:turbo 1 :fast 2 :balanced 4 :accurate 8 :precise 12})   ; ivf_flat.clj:243-247

(extend-type GpuIndex
  proto/ANNIndex
  (search-knn* [this query k mode]
    (if (= :ivf (:kind this))
      (search-ivf this query k :num-probes (mode->probes mode 4))
      (search-knn this query k)))                          ; ef = (max k 50) whatever the mode, as graph.clj:304
  (index-info* [this] {:type (if (= :ivf (:kind this)) "GPU IVF-FLAT (MI355X)" "GPU HNSW (MI355X)")
                       :vectors (count (:ids this)) :dim (:dim this)})
  (index-type* [this] (if (= :ivf (:kind this)) :gpu-ivf-flat :gpu-hnsw))
  proto/BatchSearchIndex
  (search-batch* [this queries k mode]
    (if (= :ivf (:kind this))
      (search-ivf-batch this queries k :num-probes (mode->probes mode 4))
      (search-batch this queries k)))
  proto/FilterableIndex
  (search-knn-filtered* [this query k filter-fn mode]
    (if (= :ivf (:kind this))
      (proto/default-filtered-search this query k filter-fn mode)   ; the reference's post-filter (protocol.clj:97-102); search-ivf-filtered filters in the list scan
      (search-knn-filtered this query k filter-fn)))
  proto/PersistableIndex
  (save-index* [this filepath] (save this filepath)))
