"""Calls of ONE handle on different streams, back to back: hg::Call (csrc/engine.hpp) orders the handle's shared scratch buffers
(s_ord, s_dist, s_tile, s_pairs, ...) across streams, so every call must return the bits it returns when it runs alone.

The index -- 2,000 x 128, cosine, 16 IVF lists, an HNSW graph of M 8 -- makes exact_knn, ivf_search, rerank and hnsw_search share
those buffers and is small enough for the oracle.  64 queries: the results of six calls (four *_dev entry points on torch's
current stream, the host ivf_search and exact_knn on the handle's own stream), one call at a time with a synchronise in between,
are the expectation; the same calls are then issued with no synchronise at all, alternating between two torch.cuda.Stream()
objects and the default stream, a host call after every second device call, twenty times with the stream assignment rotated.
A host ivf_search of four queries rides along among the host calls: it is the one call that opens its scope on a slot stream.

The error case: hnswgpu_ivf_home_bounds with a row range past the index returns HNSWGPU_EINVAL after its scope has opened and
before anything is enqueued; the scope's destructor then closes it, and the next call, on another stream, must still be right.
The three HNSWGPU_ELIMIT checks inside ivf_search_plan are not reachable on an index of this size: the routing kernel's LDS bound
holds for every nprobe <= 1024 that check_ivf_args lets through (40 bytes x 1024 < 48 KB), and the two work-list bounds (2^31
items) need more than 2^31 (query, list) pairs per 32, which 16 lists and an int32 query count cannot make.  No fault is injected
and no HIP error provoked."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, DIM, NQ, K, NPROBE, EF, NCAND, REPS = 2000, 128, 64, 10, 4, 64, 40, 20


@pytest.fixture(scope="module")
def setup(native_lib, oracle):
    import torch

    from hnsw_clj_amd import datagen, engine

    assert engine.device_count() >= 1, "no GPU visible"
    base = datagen.generate_dataset(N, DIM)
    Q = datagen.generate_dataset(NQ, DIM, seed=43)
    idx = engine.Index(base, "cosine", 0)
    idx.ivf_build(16, 3, 42)
    idx.hnsw_build(8, 100, 42)
    dev = torch.device("cuda", 0)
    Qd = torch.from_numpy(Q).to(dev)
    cand = torch.from_numpy(np.random.default_rng(7).integers(0, N, (NQ, NCAND)).astype(np.int32)).to(dev)
    torch.cuda.synchronize()
    yield idx, base, Q, Qd, cand
    idx.close()


def _out(torch, nq=NQ):
    dev = torch.device("cuda", 0)
    return torch.empty((nq, K), dtype=torch.int32, device=dev), torch.empty((nq, K), dtype=torch.float32, device=dev)


def _same(torch, got, want, what):
    gi, gd = (torch.as_tensor(x).cpu() for x in got)
    wi, wd = (torch.as_tensor(x).cpu() for x in want)
    assert torch.equal(gi, wi), what + ": ids"
    assert torch.equal(gd.view(torch.int32), wd.view(torch.int32)), what + ": distance bits"


def test_calls_on_alternating_streams_return_the_bits_of_calls_alone(setup, oracle):
    import torch

    idx, base, Q, Qd, cand = setup
    dev_calls = [
        ("exact_knn_dev", lambda o: idx.exact_knn_dev(Qd, K, out=o)),
        ("ivf_search_dev", lambda o: idx.ivf_search_dev(Qd, K, NPROBE, out=o)),
        ("rerank_dev", lambda o: idx.rerank_dev(Qd, cand, K, out=o)),
        ("hnsw_search_dev", lambda o: idx.hnsw_search_dev(Qd, K, EF, out=o)),
    ]
    host_calls = [
        ("ivf_search", lambda: idx.ivf_search(Q, K, NPROBE)),
        ("exact_knn", lambda: idx.exact_knn(Q, K)),
        ("ivf_search, 4 queries (slot stream)", lambda: idx.ivf_search(Q[:4], K, NPROBE)),
    ]
    # one call at a time
    want_dev, want_host = [], []
    for _, call in dev_calls:
        o = _out(torch)
        call(o)
        torch.cuda.synchronize()
        want_dev.append(o)
    for _, call in host_calls:
        want_host.append(call())
        torch.cuda.synchronize()
    oi, _, _ = oracle.exact_knn(base, Q, K, metric=oracle.COSINE, mode=oracle.MODE_MFMA)  # 64 queries: the MFMA tile order
    assert torch.equal(want_dev[0][0].cpu(), torch.from_numpy(np.ascontiguousarray(oi, np.int32))), "exact_knn_dev alone: ids differ from the oracle"
    assert np.array_equal(want_host[1][0], oi), "exact_knn alone: ids differ from the oracle"

    # back to back, no synchronise: results kept apart per repetition, compared at the end
    streams = [torch.cuda.Stream(), torch.cuda.Stream(), torch.cuda.default_stream()]
    got_dev = [[_out(torch) for _ in dev_calls] for _ in range(REPS)]
    got_host = []
    torch.cuda.synchronize()
    for r in range(REPS):
        for j, (_, call) in enumerate(dev_calls):
            with torch.cuda.stream(streams[(j + r) % 3]):
                call(got_dev[r][j])
            if j % 2 == 1:
                h = (2 * r + j // 2) % len(host_calls)
                got_host.append((r, h, host_calls[h][1]()))
        if r % 5 == 2:  # an argument error behind an opened scope; the next repetition starts on another stream
            with pytest.raises(Exception, match="row range"):
                idx.ivf_home_bounds(Q[:1], 0, N + 1)
    torch.cuda.synchronize()
    for r in range(REPS):
        for j, (name, _) in enumerate(dev_calls):
            _same(torch, got_dev[r][j], want_dev[j], "repetition %d, %s on stream %d" % (r, name, (j + r) % 3))
    for r, h, got in got_host:
        _same(torch, got, want_host[h], "repetition %d, host %s" % (r, host_calls[h][0]))
