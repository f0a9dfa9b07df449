/* JNI alternative to the Panama binding in clj/src/hnsw/gpu.clj: a mechanical wrapper over the C ABI
 * (include/hnswgpu.h) for JVMs older than 22.  UNVERIFIED: there is no jni.h in this image, so this
 * file is not part of the build (compile with: gcc -shared -fPIC -I$JAVA_HOME/include
 * -I$JAVA_HOME/include/linux -I../../include hnswgpu_jni.c -L../../hnsw-clj_amd -lhnswgpu -o libhnswgpu_jni.so).
 * Java side: package hnsw.gpu; class Native { static native long create(float[] base, long n, int dim,
 * int metric, int device); static native int hnswBuild(long h, int M, int efc, long seed); static native
 * int hnswSearch(long h, float[] q, int nq, int k, int ef, int[] ids, float[] dist); ... } */
#include <jni.h>

#include "hnswgpu.h"

static void throw_last(JNIEnv *env) {
    jclass ex = (*env)->FindClass(env, "java/lang/RuntimeException");
    (*env)->ThrowNew(env, ex, hnswgpu_last_error());
}
/* a null array argument: IllegalArgumentException instead of a crashed JVM */
static jint throw_iae(JNIEnv *env, const char *msg) {
    jclass ex = (*env)->FindClass(env, "java/lang/IllegalArgumentException");
    if (ex) (*env)->ThrowNew(env, ex, msg);
    return HNSWGPU_EINVAL;
}

JNIEXPORT jlong JNICALL Java_hnsw_gpu_Native_create(JNIEnv *env, jclass c, jfloatArray base, jlong n, jint dim,
                                                    jint metric, jint device) {
    hnswgpu_index *idx = NULL;
    jfloat *p = (*env)->GetPrimitiveArrayCritical(env, base, NULL);
    int rc = hnswgpu_create(p, n, dim, metric, device, &idx); /* copies to HBM before returning */
    (*env)->ReleasePrimitiveArrayCritical(env, base, p, JNI_ABORT);
    if (rc != 0) throw_last(env);
    return (jlong)(intptr_t)idx;
}

JNIEXPORT void JNICALL Java_hnsw_gpu_Native_destroy(JNIEnv *env, jclass c, jlong h) {
    hnswgpu_destroy((hnswgpu_index *)(intptr_t)h);
}

JNIEXPORT jint JNICALL Java_hnsw_gpu_Native_hnswBuild(JNIEnv *env, jclass c, jlong h, jint M, jint efc, jlong seed) {
    int rc = hnswgpu_hnsw_build((hnswgpu_index *)(intptr_t)h, M, efc, seed);
    if (rc != 0) throw_last(env);
    return rc;
}

/* build options: include/hnswgpu.h HNSWGPU_BUILD_* (1 sequential, 2 heuristic, 4 symmetric, 8 extend) */
JNIEXPORT jint JNICALL Java_hnsw_gpu_Native_hnswBuildEx(JNIEnv *env, jclass c, jlong h, jint M, jint efc, jlong seed, jint flags) {
    int rc = hnswgpu_hnsw_build_ex((hnswgpu_index *)(intptr_t)h, M, efc, seed, flags);
    if (rc != 0) throw_last(env);
    return rc;
}

JNIEXPORT jint JNICALL Java_hnsw_gpu_Native_hnswSearch(JNIEnv *env, jclass c, jlong h, jfloatArray q, jint nq, jint k,
                                                       jint ef, jintArray ids, jfloatArray dist) {
    jfloat *pq = (*env)->GetFloatArrayElements(env, q, NULL);
    jint *pi = (*env)->GetIntArrayElements(env, ids, NULL);
    jfloat *pd = (*env)->GetFloatArrayElements(env, dist, NULL);
    int rc = hnswgpu_hnsw_search((hnswgpu_index *)(intptr_t)h, pq, nq, k, ef, (int32_t *)pi, pd, NULL);
    (*env)->ReleaseFloatArrayElements(env, q, pq, JNI_ABORT);
    (*env)->ReleaseIntArrayElements(env, ids, pi, 0);
    (*env)->ReleaseFloatArrayElements(env, dist, pd, 0);
    if (rc != 0) throw_last(env);
    return rc;
}

JNIEXPORT jint JNICALL Java_hnsw_gpu_Native_ivfBuild(JNIEnv *env, jclass c, jlong h, jint nlist, jint iters, jlong seed) {
    int rc = hnswgpu_ivf_build((hnswgpu_index *)(intptr_t)h, nlist, iters, seed);
    if (rc != 0) throw_last(env);
    return rc;
}

JNIEXPORT jint JNICALL Java_hnsw_gpu_Native_ivfSearch(JNIEnv *env, jclass c, jlong h, jfloatArray q, jint nq, jint k,
                                                      jint nprobe, jintArray ids, jfloatArray dist) {
    jfloat *pq = (*env)->GetFloatArrayElements(env, q, NULL);
    jint *pi = (*env)->GetIntArrayElements(env, ids, NULL);
    jfloat *pd = (*env)->GetFloatArrayElements(env, dist, NULL);
    int rc = hnswgpu_ivf_search((hnswgpu_index *)(intptr_t)h, pq, nq, k, nprobe, (int32_t *)pi, pd, NULL);
    (*env)->ReleaseFloatArrayElements(env, q, pq, JNI_ABORT);
    (*env)->ReleaseIntArrayElements(env, ids, pi, 0);
    (*env)->ReleaseFloatArrayElements(env, dist, pd, 0);
    if (rc != 0) throw_last(env);
    return rc;
}

/* ---- a forest: several HNSW sub-graphs on one handle (include/hnswgpu.h: hnswgpu_hnsw_build_parts / hnswgpu_hnsw_search_parts) ---- */
JNIEXPORT jint JNICALL Java_hnsw_gpu_Native_hnswBuildParts(JNIEnv *env, jclass c, jlong h, jlongArray partOff, jint M, jint efc,
                                                           jlong seed, jint flags) {
    if (!partOff) return throw_iae(env, "hnswBuildParts: null array");
    jsize len = (*env)->GetArrayLength(env, partOff);
    if (len < 2) return throw_iae(env, "hnswBuildParts: partOff holds nparts + 1 offsets");
    jlong *po = (*env)->GetLongArrayElements(env, partOff, NULL);
    if (!po) return HNSWGPU_ENOMEM; /* OutOfMemoryError is pending */
    int rc = hnswgpu_hnsw_build_parts((hnswgpu_index *)(intptr_t)h, (int32_t)(len - 1), (const int64_t *)po, M, efc, seed, flags);
    (*env)->ReleaseLongArrayElements(env, partOff, po, JNI_ABORT);
    if (rc != 0) throw_last(env);
    return rc;
}

/* probes: nq x nprobe part ids (-1 = skip), or null = every part in order (nprobe is then ignored) */
JNIEXPORT jint JNICALL Java_hnsw_gpu_Native_hnswSearchParts(JNIEnv *env, jclass c, jlong h, jfloatArray q, jint nq, jint kPart,
                                                            jint ef, jintArray probes, jint nprobe, jint k, jintArray ids,
                                                            jfloatArray dist) {
    if (!q || !ids || !dist) return throw_iae(env, "hnswSearchParts: null array");
    if (probes && (jlong)(*env)->GetArrayLength(env, probes) < (jlong)nq * nprobe) return throw_iae(env, "hnswSearchParts: probes is shorter than nq x nprobe");
    jfloat *pq = (*env)->GetFloatArrayElements(env, q, NULL);
    jint *pp = probes ? (*env)->GetIntArrayElements(env, probes, NULL) : NULL;
    jint *pi = (*env)->GetIntArrayElements(env, ids, NULL);
    jfloat *pd = (*env)->GetFloatArrayElements(env, dist, NULL);
    int rc = (pq && pi && pd && (pp || !probes))
                 ? hnswgpu_hnsw_search_parts((hnswgpu_index *)(intptr_t)h, pq, nq, kPart, ef, (const int32_t *)pp, nprobe, k, (int32_t *)pi, pd, NULL)
                 : HNSWGPU_ENOMEM;
    if (pq) (*env)->ReleaseFloatArrayElements(env, q, pq, JNI_ABORT);
    if (pp) (*env)->ReleaseIntArrayElements(env, probes, pp, JNI_ABORT);
    if (pi) (*env)->ReleaseIntArrayElements(env, ids, pi, 0);
    if (pd) (*env)->ReleaseFloatArrayElements(env, dist, pd, 0);
    if (rc != 0 && rc != HNSWGPU_ENOMEM) throw_last(env);
    return rc;
}

/* ---- INTEGRATION.md section 5 / the simd-optimized seams / persistence: the same mechanical shape ---- */

JNIEXPORT jint JNICALL Java_hnsw_gpu_Native_setGraph(JNIEnv *env, jclass c, jlong h, jintArray levels, jintArray l0, jint M0,
                                                     jlongArray upOff, jintArray upAdj, jint M, jint entry, jint maxLevel) {
    if (!levels || !l0 || !upOff || !upAdj) return throw_iae(env, "setGraph: null array");
    jint *pl = (*env)->GetIntArrayElements(env, levels, NULL), *p0 = (*env)->GetIntArrayElements(env, l0, NULL);
    jlong *po = (*env)->GetLongArrayElements(env, upOff, NULL);
    jint *pu = (*env)->GetIntArrayElements(env, upAdj, NULL);
    if (!pl || !p0 || !po || !pu) { /* OutOfMemoryError is pending: release what was pinned and return */
        if (pl) (*env)->ReleaseIntArrayElements(env, levels, pl, JNI_ABORT);
        if (p0) (*env)->ReleaseIntArrayElements(env, l0, p0, JNI_ABORT);
        if (po) (*env)->ReleaseLongArrayElements(env, upOff, po, JNI_ABORT);
        if (pu) (*env)->ReleaseIntArrayElements(env, upAdj, pu, JNI_ABORT);
        return HNSWGPU_ENOMEM;
    }
    int rc = hnswgpu_set_graph((hnswgpu_index *)(intptr_t)h, (const int32_t *)pl, (const int32_t *)p0, M0, (const int64_t *)po,
                               (const int32_t *)pu, M, entry, maxLevel); /* validates and copies before returning */
    (*env)->ReleaseIntArrayElements(env, levels, pl, JNI_ABORT);
    (*env)->ReleaseIntArrayElements(env, l0, p0, JNI_ABORT);
    (*env)->ReleaseLongArrayElements(env, upOff, po, JNI_ABORT);
    (*env)->ReleaseIntArrayElements(env, upAdj, pu, JNI_ABORT);
    if (rc != 0) throw_last(env);
    return rc;
}

JNIEXPORT jint JNICALL Java_hnsw_gpu_Native_setIvf(JNIEnv *env, jclass c, jlong h, jfloatArray centroids, jint nlist,
                                                   jlongArray listOff, jintArray listIds) {
    if (!centroids || !listOff || !listIds) return throw_iae(env, "setIvf: null array");
    jfloat *pc = (*env)->GetFloatArrayElements(env, centroids, NULL);
    jlong *po = (*env)->GetLongArrayElements(env, listOff, NULL);
    jint *pi = (*env)->GetIntArrayElements(env, listIds, NULL);
    if (!pc || !po || !pi) {
        if (pc) (*env)->ReleaseFloatArrayElements(env, centroids, pc, JNI_ABORT);
        if (po) (*env)->ReleaseLongArrayElements(env, listOff, po, JNI_ABORT);
        if (pi) (*env)->ReleaseIntArrayElements(env, listIds, pi, JNI_ABORT);
        return HNSWGPU_ENOMEM;
    }
    int rc = hnswgpu_set_ivf((hnswgpu_index *)(intptr_t)h, pc, nlist, (const int64_t *)po, (const int32_t *)pi);
    (*env)->ReleaseFloatArrayElements(env, centroids, pc, JNI_ABORT);
    (*env)->ReleaseLongArrayElements(env, listOff, po, JNI_ABORT);
    (*env)->ReleaseIntArrayElements(env, listIds, pi, JNI_ABORT);
    if (rc != 0) throw_last(env);
    return rc;
}

JNIEXPORT jint JNICALL Java_hnsw_gpu_Native_batchDistances(JNIEnv *env, jclass c, jlong h, jfloatArray q, jintArray ids,
                                                           jint m, jfloatArray out) {
    if (!q || !out) return throw_iae(env, "batchDistances: null array");
    jfloat *pq = (*env)->GetFloatArrayElements(env, q, NULL);
    jint *pi = ids ? (*env)->GetIntArrayElements(env, ids, NULL) : NULL;
    jfloat *po = (*env)->GetFloatArrayElements(env, out, NULL);
    if (!pq || !po || (ids && !pi)) {
        if (pq) (*env)->ReleaseFloatArrayElements(env, q, pq, JNI_ABORT);
        if (pi) (*env)->ReleaseIntArrayElements(env, ids, pi, JNI_ABORT);
        if (po) (*env)->ReleaseFloatArrayElements(env, out, po, JNI_ABORT);
        return HNSWGPU_ENOMEM;
    }
    int rc = hnswgpu_batch_distances((hnswgpu_index *)(intptr_t)h, pq, (const int32_t *)pi, m, po);
    (*env)->ReleaseFloatArrayElements(env, q, pq, JNI_ABORT);
    if (pi) (*env)->ReleaseIntArrayElements(env, ids, pi, JNI_ABORT);
    (*env)->ReleaseFloatArrayElements(env, out, po, 0);
    if (rc != 0) throw_last(env);
    return rc;
}

JNIEXPORT jint JNICALL Java_hnsw_gpu_Native_save(JNIEnv *env, jclass c, jlong h, jstring path) {
    if (!path) return throw_iae(env, "save: null path");
    const char *p = (*env)->GetStringUTFChars(env, path, NULL);
    if (!p) return HNSWGPU_ENOMEM; /* OutOfMemoryError is pending */
    int rc = hnswgpu_save((hnswgpu_index *)(intptr_t)h, p);
    (*env)->ReleaseStringUTFChars(env, path, p);
    if (rc != 0) throw_last(env);
    return rc;
}

JNIEXPORT jlong JNICALL Java_hnsw_gpu_Native_load(JNIEnv *env, jclass c, jstring path, jint device) {
    hnswgpu_index *idx = NULL;
    if (!path) {
        throw_iae(env, "load: null path");
        return 0;
    }
    const char *p = (*env)->GetStringUTFChars(env, path, NULL);
    if (!p) return 0; /* OutOfMemoryError is pending */
    int rc = hnswgpu_load(p, device, &idx);
    (*env)->ReleaseStringUTFChars(env, path, p);
    if (rc != 0) throw_last(env);
    return (jlong)(intptr_t)idx;
}

/* ---- filtered search (FilterableIndex/search-knn-filtered*, src/hnsw/api/protocol.clj:34-41,97-102): `allow` is the call's
 * mask, (n + 31) / 32 ints, row i passes iff bit (i & 31) of allow[i >> 5] is set ---- */
JNIEXPORT jint JNICALL Java_hnsw_gpu_Native_exactKnnFiltered(JNIEnv *env, jclass c, jlong h, jfloatArray q, jint nq, jint k,
                                                             jintArray allow, jintArray ids, jfloatArray dist) {
    if (!q || !allow || !ids || !dist) return throw_iae(env, "exactKnnFiltered: null array");
    jfloat *pq = (*env)->GetFloatArrayElements(env, q, NULL);
    jint *pa = (*env)->GetIntArrayElements(env, allow, NULL);
    jint *pi = (*env)->GetIntArrayElements(env, ids, NULL);
    jfloat *pd = (*env)->GetFloatArrayElements(env, dist, NULL);
    int rc = (pq && pa && pi && pd)
                 ? hnswgpu_exact_knn_filtered((hnswgpu_index *)(intptr_t)h, pq, nq, k, (const uint32_t *)pa, (int32_t *)pi, pd)
                 : HNSWGPU_ENOMEM; /* OutOfMemoryError is pending */
    if (pq) (*env)->ReleaseFloatArrayElements(env, q, pq, JNI_ABORT);
    if (pa) (*env)->ReleaseIntArrayElements(env, allow, pa, JNI_ABORT);
    if (pi) (*env)->ReleaseIntArrayElements(env, ids, pi, 0);
    if (pd) (*env)->ReleaseFloatArrayElements(env, dist, pd, 0);
    if (rc != 0 && rc != HNSWGPU_ENOMEM) throw_last(env);
    return rc;
}

JNIEXPORT jint JNICALL Java_hnsw_gpu_Native_hnswSearchFiltered(JNIEnv *env, jclass c, jlong h, jfloatArray q, jint nq, jint k,
                                                               jint ef, jintArray allow, jintArray ids, jfloatArray dist) {
    if (!q || !allow || !ids || !dist) return throw_iae(env, "hnswSearchFiltered: null array");
    jfloat *pq = (*env)->GetFloatArrayElements(env, q, NULL);
    jint *pa = (*env)->GetIntArrayElements(env, allow, NULL);
    jint *pi = (*env)->GetIntArrayElements(env, ids, NULL);
    jfloat *pd = (*env)->GetFloatArrayElements(env, dist, NULL);
    int rc = (pq && pa && pi && pd) ? hnswgpu_hnsw_search_filtered((hnswgpu_index *)(intptr_t)h, pq, nq, k, ef, (const uint32_t *)pa,
                                                                   (int32_t *)pi, pd, NULL)
                                    : HNSWGPU_ENOMEM; /* OutOfMemoryError is pending */
    if (pq) (*env)->ReleaseFloatArrayElements(env, q, pq, JNI_ABORT);
    if (pa) (*env)->ReleaseIntArrayElements(env, allow, pa, JNI_ABORT);
    if (pi) (*env)->ReleaseIntArrayElements(env, ids, pi, 0);
    if (pd) (*env)->ReleaseFloatArrayElements(env, dist, pd, 0);
    if (rc != 0 && rc != HNSWGPU_ENOMEM) throw_last(env);
    return rc;
}

/* one mask per query: `allow` holds nq rows of (n + 31) / 32 ints, row q is query q's mask (hnswgpu_*_filtered_each) */
JNIEXPORT jint JNICALL Java_hnsw_gpu_Native_exactKnnFilteredEach(JNIEnv *env, jclass c, jlong h, jfloatArray q, jint nq, jint k,
                                                                 jintArray allow, jintArray ids, jfloatArray dist) {
    if (!q || !allow || !ids || !dist) return throw_iae(env, "exactKnnFilteredEach: null array");
    jfloat *pq = (*env)->GetFloatArrayElements(env, q, NULL);
    jint *pa = (*env)->GetIntArrayElements(env, allow, NULL);
    jint *pi = (*env)->GetIntArrayElements(env, ids, NULL);
    jfloat *pd = (*env)->GetFloatArrayElements(env, dist, NULL);
    int rc = (pq && pa && pi && pd)
                 ? hnswgpu_exact_knn_filtered_each((hnswgpu_index *)(intptr_t)h, pq, nq, k, (const uint32_t *)pa, (int32_t *)pi, pd)
                 : HNSWGPU_ENOMEM; /* OutOfMemoryError is pending */
    if (pq) (*env)->ReleaseFloatArrayElements(env, q, pq, JNI_ABORT);
    if (pa) (*env)->ReleaseIntArrayElements(env, allow, pa, JNI_ABORT);
    if (pi) (*env)->ReleaseIntArrayElements(env, ids, pi, 0);
    if (pd) (*env)->ReleaseFloatArrayElements(env, dist, pd, 0);
    if (rc != 0 && rc != HNSWGPU_ENOMEM) throw_last(env);
    return rc;
}

JNIEXPORT jint JNICALL Java_hnsw_gpu_Native_hnswSearchFilteredEach(JNIEnv *env, jclass c, jlong h, jfloatArray q, jint nq, jint k,
                                                                   jint ef, jintArray allow, jintArray ids, jfloatArray dist) {
    if (!q || !allow || !ids || !dist) return throw_iae(env, "hnswSearchFilteredEach: null array");
    jfloat *pq = (*env)->GetFloatArrayElements(env, q, NULL);
    jint *pa = (*env)->GetIntArrayElements(env, allow, NULL);
    jint *pi = (*env)->GetIntArrayElements(env, ids, NULL);
    jfloat *pd = (*env)->GetFloatArrayElements(env, dist, NULL);
    int rc = (pq && pa && pi && pd) ? hnswgpu_hnsw_search_filtered_each((hnswgpu_index *)(intptr_t)h, pq, nq, k, ef, (const uint32_t *)pa,
                                                                        (int32_t *)pi, pd, NULL)
                                    : HNSWGPU_ENOMEM; /* OutOfMemoryError is pending */
    if (pq) (*env)->ReleaseFloatArrayElements(env, q, pq, JNI_ABORT);
    if (pa) (*env)->ReleaseIntArrayElements(env, allow, pa, JNI_ABORT);
    if (pi) (*env)->ReleaseIntArrayElements(env, ids, pi, 0);
    if (pd) (*env)->ReleaseFloatArrayElements(env, dist, pd, 0);
    if (rc != 0 && rc != HNSWGPU_ENOMEM) throw_last(env);
    return rc;
}

/* the allow-mask through the IVF list scan: the k nearest passing rows of the probed lists (probes are not reported here) */
JNIEXPORT jint JNICALL Java_hnsw_gpu_Native_ivfSearchFiltered(JNIEnv *env, jclass c, jlong h, jfloatArray q, jint nq, jint k,
                                                              jint nprobe, jintArray allow, jintArray ids, jfloatArray dist) {
    if (!q || !allow || !ids || !dist) return throw_iae(env, "ivfSearchFiltered: null array");
    jfloat *pq = (*env)->GetFloatArrayElements(env, q, NULL);
    jint *pa = (*env)->GetIntArrayElements(env, allow, NULL);
    jint *pi = (*env)->GetIntArrayElements(env, ids, NULL);
    jfloat *pd = (*env)->GetFloatArrayElements(env, dist, NULL);
    int rc = (pq && pa && pi && pd) ? hnswgpu_ivf_search_filtered((hnswgpu_index *)(intptr_t)h, pq, nq, k, nprobe, (const uint32_t *)pa,
                                                                  (int32_t *)pi, pd, NULL)
                                    : HNSWGPU_ENOMEM; /* OutOfMemoryError is pending */
    if (pq) (*env)->ReleaseFloatArrayElements(env, q, pq, JNI_ABORT);
    if (pa) (*env)->ReleaseIntArrayElements(env, allow, pa, JNI_ABORT);
    if (pi) (*env)->ReleaseIntArrayElements(env, ids, pi, 0);
    if (pd) (*env)->ReleaseFloatArrayElements(env, dist, pd, 0);
    if (rc != 0 && rc != HNSWGPU_ENOMEM) throw_last(env);
    return rc;
}

/* ... with one mask per query: `allow` holds nq rows of (n + 31) / 32 ints, row q is query q's mask (hnswgpu_ivf_search_filtered_each) */
JNIEXPORT jint JNICALL Java_hnsw_gpu_Native_ivfSearchFilteredEach(JNIEnv *env, jclass c, jlong h, jfloatArray q, jint nq, jint k,
                                                                  jint nprobe, jintArray allow, jintArray ids, jfloatArray dist) {
    if (!q || !allow || !ids || !dist) return throw_iae(env, "ivfSearchFilteredEach: null array");
    jfloat *pq = (*env)->GetFloatArrayElements(env, q, NULL);
    jint *pa = (*env)->GetIntArrayElements(env, allow, NULL);
    jint *pi = (*env)->GetIntArrayElements(env, ids, NULL);
    jfloat *pd = (*env)->GetFloatArrayElements(env, dist, NULL);
    int rc = (pq && pa && pi && pd) ? hnswgpu_ivf_search_filtered_each((hnswgpu_index *)(intptr_t)h, pq, nq, k, nprobe, (const uint32_t *)pa,
                                                                       (int32_t *)pi, pd, NULL)
                                    : HNSWGPU_ENOMEM; /* OutOfMemoryError is pending */
    if (pq) (*env)->ReleaseFloatArrayElements(env, q, pq, JNI_ABORT);
    if (pa) (*env)->ReleaseIntArrayElements(env, allow, pa, JNI_ABORT);
    if (pi) (*env)->ReleaseIntArrayElements(env, ids, pi, 0);
    if (pd) (*env)->ReleaseFloatArrayElements(env, dist, pd, 0);
    if (rc != 0 && rc != HNSWGPU_ENOMEM) throw_last(env);
    return rc;
}

/* the allow-mask through the hybrid LSH bucket scan: every probed bucket keeps its nearest passing rows (hnswgpu_lsh_search_filtered) */
JNIEXPORT jint JNICALL Java_hnsw_gpu_Native_lshSearchFiltered(JNIEnv *env, jclass c, jlong h, jfloatArray q, jint nq, jint k,
                                                              jint probes, jint radius, jint take_main, jint take_flip, jintArray allow,
                                                              jintArray ids, jfloatArray dist) {
    if (!q || !allow || !ids || !dist) return throw_iae(env, "lshSearchFiltered: null array");
    jfloat *pq = (*env)->GetFloatArrayElements(env, q, NULL);
    jint *pa = (*env)->GetIntArrayElements(env, allow, NULL);
    jint *pi = (*env)->GetIntArrayElements(env, ids, NULL);
    jfloat *pd = (*env)->GetFloatArrayElements(env, dist, NULL);
    int rc = (pq && pa && pi && pd) ? hnswgpu_lsh_search_filtered((hnswgpu_index *)(intptr_t)h, pq, nq, k, probes, radius, take_main, take_flip,
                                                                  (const uint32_t *)pa, (int32_t *)pi, pd)
                                    : HNSWGPU_ENOMEM; /* OutOfMemoryError is pending */
    if (pq) (*env)->ReleaseFloatArrayElements(env, q, pq, JNI_ABORT);
    if (pa) (*env)->ReleaseIntArrayElements(env, allow, pa, JNI_ABORT);
    if (pi) (*env)->ReleaseIntArrayElements(env, ids, pi, 0);
    if (pd) (*env)->ReleaseFloatArrayElements(env, dist, pd, 0);
    if (rc != 0 && rc != HNSWGPU_ENOMEM) throw_last(env);
    return rc;
}

/* ... with one mask per query: `allow` holds nq rows of (n + 31) / 32 ints, row q is query q's mask (hnswgpu_lsh_search_filtered_each) */
JNIEXPORT jint JNICALL Java_hnsw_gpu_Native_lshSearchFilteredEach(JNIEnv *env, jclass c, jlong h, jfloatArray q, jint nq, jint k,
                                                                  jint probes, jint radius, jint take_main, jint take_flip,
                                                                  jintArray allow, jintArray ids, jfloatArray dist) {
    if (!q || !allow || !ids || !dist) return throw_iae(env, "lshSearchFilteredEach: null array");
    jfloat *pq = (*env)->GetFloatArrayElements(env, q, NULL);
    jint *pa = (*env)->GetIntArrayElements(env, allow, NULL);
    jint *pi = (*env)->GetIntArrayElements(env, ids, NULL);
    jfloat *pd = (*env)->GetFloatArrayElements(env, dist, NULL);
    int rc = (pq && pa && pi && pd) ? hnswgpu_lsh_search_filtered_each((hnswgpu_index *)(intptr_t)h, pq, nq, k, probes, radius, take_main,
                                                                       take_flip, (const uint32_t *)pa, (int32_t *)pi, pd)
                                    : HNSWGPU_ENOMEM; /* OutOfMemoryError is pending */
    if (pq) (*env)->ReleaseFloatArrayElements(env, q, pq, JNI_ABORT);
    if (pa) (*env)->ReleaseIntArrayElements(env, allow, pa, JNI_ABORT);
    if (pi) (*env)->ReleaseIntArrayElements(env, ids, pi, 0);
    if (pd) (*env)->ReleaseFloatArrayElements(env, dist, pd, 0);
    if (rc != 0 && rc != HNSWGPU_ENOMEM) throw_last(env);
    return rc;
}

/* rows leave a live hybrid LSH index (hnswgpu_lsh_remove): `rows` holds m row ids in any order, repeats count once; the kept rows
 * are renumbered densely in their old order.  Returns the rows the handle holds afterwards, or the negative error code (the
 * exception is pending).  Unverified like the rest of this file: no JVM where the library is built and tested. */
JNIEXPORT jlong JNICALL Java_hnsw_gpu_Native_lshRemove(JNIEnv *env, jclass c, jlong h, jintArray rows, jlong m) {
    if (!rows) return throw_iae(env, "lshRemove: null array");
    if (m < 0 || m > (jlong)(*env)->GetArrayLength(env, rows)) return throw_iae(env, "lshRemove: m outside the array");
    jint *pr = (*env)->GetIntArrayElements(env, rows, NULL);
    int64_t n_after = -1;
    int rc = pr ? hnswgpu_lsh_remove((hnswgpu_index *)(intptr_t)h, (const int32_t *)pr, (int64_t)m, &n_after)
                : HNSWGPU_ENOMEM; /* OutOfMemoryError is pending */
    if (pr) (*env)->ReleaseIntArrayElements(env, rows, pr, JNI_ABORT);
    if (rc != 0 && rc != HNSWGPU_ENOMEM) throw_last(env);
    return rc != 0 ? (jlong)rc : (jlong)n_after;
}

/* rows of a live hybrid LSH index take new values (hnswgpu_lsh_update): `ids` holds m row ids in any order, none named twice; `rows`
 * holds m x dim floats, row ids[i] takes rows[i]; n, the ids and the planes stay.  Returns 0, or the negative error code (the
 * exception is pending).  Unverified like the rest of this file: no JVM where the library is built and tested. */
JNIEXPORT jint JNICALL Java_hnsw_gpu_Native_lshUpdate(JNIEnv *env, jclass c, jlong h, jintArray ids, jfloatArray rows, jlong m, jint dim) {
    if (!ids || !rows) return throw_iae(env, "lshUpdate: null array");
    if (m < 0 || m > (jlong)(*env)->GetArrayLength(env, ids)) return throw_iae(env, "lshUpdate: m outside the id array");
    if (dim < 1 || m > (jlong)(*env)->GetArrayLength(env, rows) / dim) return throw_iae(env, "lshUpdate: fewer than m x dim floats");
    jint *pi = (*env)->GetIntArrayElements(env, ids, NULL);
    jfloat *pr = pi ? (*env)->GetFloatArrayElements(env, rows, NULL) : NULL;
    int rc = pi && pr ? hnswgpu_lsh_update((hnswgpu_index *)(intptr_t)h, (const int32_t *)pi, (const float *)pr, (int64_t)m)
                      : HNSWGPU_ENOMEM; /* OutOfMemoryError is pending */
    if (pr) (*env)->ReleaseFloatArrayElements(env, rows, pr, JNI_ABORT);
    if (pi) (*env)->ReleaseIntArrayElements(env, ids, pi, JNI_ABORT);
    if (rc != 0 && rc != HNSWGPU_ENOMEM) throw_last(env);
    return rc;
}

/* rows leave a live IVF-FLAT index (hnswgpu_ivf_remove): `rows` holds m row ids in any order, repeats count once; the kept rows are
 * renumbered densely in their old order, every list keeps its kept members in their order.  Returns the rows the handle holds
 * afterwards, or the negative error code (the exception is pending).  Unverified like the rest of this file: no JVM where the
 * library is built and tested. */
JNIEXPORT jlong JNICALL Java_hnsw_gpu_Native_ivfRemove(JNIEnv *env, jclass c, jlong h, jintArray rows, jlong m) {
    if (!rows) return throw_iae(env, "ivfRemove: null array");
    if (m < 0 || m > (jlong)(*env)->GetArrayLength(env, rows)) return throw_iae(env, "ivfRemove: m outside the array");
    jint *pr = (*env)->GetIntArrayElements(env, rows, NULL);
    int64_t n_after = -1;
    int rc = pr ? hnswgpu_ivf_remove((hnswgpu_index *)(intptr_t)h, (const int32_t *)pr, (int64_t)m, &n_after)
                : HNSWGPU_ENOMEM; /* OutOfMemoryError is pending */
    if (pr) (*env)->ReleaseIntArrayElements(env, rows, pr, JNI_ABORT);
    if (rc != 0 && rc != HNSWGPU_ENOMEM) throw_last(env);
    return rc != 0 ? (jlong)rc : (jlong)n_after;
}

/* rows of a live IVF-FLAT index take new values (hnswgpu_ivf_update): `ids` holds m row ids in any order, none named twice; `rows`
 * holds m x dim floats, row ids[i] takes rows[i]; n, the ids and the centroids stay.  Returns 0, or the negative error code (the
 * exception is pending).  Unverified like the rest of this file: no JVM where the library is built and tested. */
JNIEXPORT jint JNICALL Java_hnsw_gpu_Native_ivfUpdate(JNIEnv *env, jclass c, jlong h, jintArray ids, jfloatArray rows, jlong m, jint dim) {
    if (!ids || !rows) return throw_iae(env, "ivfUpdate: null array");
    if (m < 0 || m > (jlong)(*env)->GetArrayLength(env, ids)) return throw_iae(env, "ivfUpdate: m outside the id array");
    if (dim < 1 || m > (jlong)(*env)->GetArrayLength(env, rows) / dim) return throw_iae(env, "ivfUpdate: fewer than m x dim floats");
    jint *pi = (*env)->GetIntArrayElements(env, ids, NULL);
    jfloat *pr = pi ? (*env)->GetFloatArrayElements(env, rows, NULL) : NULL;
    int rc = pi && pr ? hnswgpu_ivf_update((hnswgpu_index *)(intptr_t)h, (const int32_t *)pi, (const float *)pr, (int64_t)m)
                      : HNSWGPU_ENOMEM; /* OutOfMemoryError is pending */
    if (pr) (*env)->ReleaseFloatArrayElements(env, rows, pr, JNI_ABORT);
    if (pi) (*env)->ReleaseIntArrayElements(env, ids, pi, JNI_ABORT);
    if (rc != 0 && rc != HNSWGPU_ENOMEM) throw_last(env);
    return rc;
}

/* rows leave a live HNSW graph (hnswgpu_hnsw_remove): `rows` holds m row ids in any order, repeats count once; the kept rows are
 * renumbered densely in their old order, a neighbour list that loses a member is selected again from the old graph.  Returns the
 * rows the handle holds afterwards, or the negative error code (the exception is pending).  Unverified like the rest of this
 * file: no JVM where the library is built and tested. */
JNIEXPORT jlong JNICALL Java_hnsw_gpu_Native_hnswRemove(JNIEnv *env, jclass c, jlong h, jintArray rows, jlong m) {
    if (!rows) return throw_iae(env, "hnswRemove: null array");
    if (m < 0 || m > (jlong)(*env)->GetArrayLength(env, rows)) return throw_iae(env, "hnswRemove: m outside the array");
    jint *pr = (*env)->GetIntArrayElements(env, rows, NULL);
    int64_t n_after = -1;
    int rc = pr ? hnswgpu_hnsw_remove((hnswgpu_index *)(intptr_t)h, (const int32_t *)pr, (int64_t)m, &n_after)
                : HNSWGPU_ENOMEM; /* OutOfMemoryError is pending */
    if (pr) (*env)->ReleaseIntArrayElements(env, rows, pr, JNI_ABORT);
    if (rc != 0 && rc != HNSWGPU_ENOMEM) throw_last(env);
    return rc != 0 ? (jlong)rc : (jlong)n_after;
}

/* rows of a live HNSW graph take new values (hnswgpu_hnsw_update): `ids` holds m row ids in any order, none named twice; `rows`
 * holds m x dim floats, row ids[i] takes rows[i]; n, the ids and every row's level stay: the rows are unlinked as rows that leave
 * are and inserted again, ascending, as hnswgpu_hnsw_add inserts rows.  Returns 0, or the negative error code (the exception is
 * pending).  Unverified like the rest of this file: no JVM where the library is built and tested. */
JNIEXPORT jint JNICALL Java_hnsw_gpu_Native_hnswUpdate(JNIEnv *env, jclass c, jlong h, jintArray ids, jfloatArray rows, jlong m, jint dim,
                                                       jint efConstruction) {
    if (!ids || !rows) return throw_iae(env, "hnswUpdate: null array");
    if (m < 0 || m > (jlong)(*env)->GetArrayLength(env, ids)) return throw_iae(env, "hnswUpdate: m outside the id array");
    if (dim < 1 || m > (jlong)(*env)->GetArrayLength(env, rows) / dim) return throw_iae(env, "hnswUpdate: fewer than m x dim floats");
    jint *pi = (*env)->GetIntArrayElements(env, ids, NULL);
    jfloat *pr = pi ? (*env)->GetFloatArrayElements(env, rows, NULL) : NULL;
    int rc = pi && pr ? hnswgpu_hnsw_update((hnswgpu_index *)(intptr_t)h, (const int32_t *)pi, (const float *)pr, (int64_t)m,
                                            (int32_t)efConstruction)
                      : HNSWGPU_ENOMEM; /* OutOfMemoryError is pending */
    if (pr) (*env)->ReleaseFloatArrayElements(env, rows, pr, JNI_ABORT);
    if (pi) (*env)->ReleaseIntArrayElements(env, ids, pi, JNI_ABORT);
    if (rc != 0 && rc != HNSWGPU_ENOMEM) throw_last(env);
    return rc;
}
