"""heuristic_select_kernel (build_kernels.hpp) on each of its three code paths, through the sequential heuristic build
against the oracle's restatement (oracle.c: orc_hnsw_build_ex), edge for edge:

  A  the taken rows stay in registers, the next candidate's row is fetched ahead     rows of up to 4 chunks (dim <= 1024)
  B  the taken rows stay in registers, no fetch ahead                                6 chunks (dim 1025 .. 1536)
  C  every candidate fetches the taken rows again                                    8 / 12 chunks (dim > 1536), a task that
                                                                                     wants more than 32 links (layer 0, M >= 17),
                                                                                     or BUILD_KEEP_ROWS = 0

600 rows in 10 clusters whose centres are rows themselves (their lists fill to 2M and overflow: hnsw_build_model.py), 20
duplicated pairs (runs of equal distances must reach the selection in id order), ef_construction 48.  The host test
asserts that every case overflows more than 100 lists and that M = 16 makes lists of more than 24 links -- selections that
fill register slots on all four waves."""
import pytest

import hnsw_build_model as H

pytestmark = pytest.mark.gpu

PATH_OF = {(40, 16): "A, all 32 register slots", (40, 20): "C at layer 0 (m = 40), A above", (300, 8): "A, 2 chunks",
           (700, 8): "A, 3 chunks", (1000, 8): "A, 4 chunks, ragged last chunk", (1100, 8): "B", (1536, 8): "B, full last chunk",
           (1700, 8): "C, 8 chunks", (2500, 6): "C, 12 chunks"}


@pytest.fixture(scope="module")
def eng(native_lib):
    from hnsw_clj_amd import engine

    assert engine.device_count() >= 1, "no GPU visible"
    return engine


def _build(eng, base, metric, M, extend):
    with eng.Index(base, metric) as idx:
        idx.hnsw_build(M, H.PATHS["efc"], H.PATHS["seed"], sequential=True, heuristic=True, extend=extend)
        return idx.get_graph()


def _oracle_graph(O, base, metric, M, extend):
    f = O.BUILD_HEURISTIC | (O.BUILD_EXTEND if extend else 0)
    og, cnt = O.hnsw_build_ex(base, O.METRICS[metric], M, H.PATHS["efc"], H.PATHS["seed"], f, mode=O.MODE_DEV, want_counters=True)
    assert cnt[3] > 100, "the data set must overflow lists: %s" % cnt
    return og


@pytest.mark.parametrize("metric", ["cosine", "l2"])
@pytest.mark.parametrize("dim,M", H.PATH_CASES)
def test_selection_paths_equal_the_oracle(eng, oracle, dim, M, metric):
    base = H.paths_data(oracle, dim)
    g = _build(eng, base, metric, M, False)
    H.same_graph(g, _oracle_graph(oracle, base, metric, M, False), "dim %d M %d %s (%s)" % (dim, M, metric, PATH_OF[(dim, M)]))


@pytest.mark.parametrize("metric", ["cosine", "l2"])
@pytest.mark.parametrize("dim,M", H.PATH_EXTEND)
def test_selection_paths_with_extend_equal_the_oracle(eng, oracle, dim, M, metric):
    """extend-candidates? fills the new node's list with the discarded candidates in their order: every list of 2M links."""
    base = H.paths_data(oracle, dim)
    g = _build(eng, base, metric, M, True)
    H.same_graph(g, _oracle_graph(oracle, base, metric, M, True), "dim %d M %d %s, extend (%s)" % (dim, M, metric, PATH_OF[(dim, M)]))


@pytest.mark.parametrize("metric", ["cosine", "l2"])
def test_reloading_the_taken_rows_gives_the_same_graph(eng, oracle, tune, metric):
    """BUILD_KEEP_ROWS = 0 sends rows of one chunk down path C: the graph equals the oracle's and the register path's."""
    dim, M = 40, 16
    base = H.paths_data(oracle, dim)
    kept = _build(eng, base, metric, M, False)
    tune.set("BUILD_KEEP_ROWS", 0)
    reloaded = _build(eng, base, metric, M, False)
    H.same_graph(reloaded, _oracle_graph(oracle, base, metric, M, False), "dim 40 M 16 %s, BUILD_KEEP_ROWS 0" % metric)
    H.same_graph(reloaded, kept, "dim 40 M 16 %s, BUILD_KEEP_ROWS 0 against 1" % metric)
