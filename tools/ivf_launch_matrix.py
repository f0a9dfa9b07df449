"""Developer tool: which kernels does an IVF search launch, configuration by configuration?

Results can stay equal while a search silently takes another path; this runs a fixed list of searches that together reach
every kernel of the IVF search path and, from a kernel trace, compares two builds of the library launch by launch.

  run (GPU):     HNSWGPU_LIBRARY=<libhnswgpu.so> rocprofv3 --kernel-trace --output-format csv -d <dir> -- \
                     python3 tools/ivf_launch_matrix.py
  compare:       python3 tools/ivf_launch_matrix.py --compare <dir of build A> <dir of build B>  > table

Every search is bracketed by two marker kernels (a torch fill of an int16 and of an int8 tensor, which nothing else here
launches) and announced on stdout; --compare cuts the trace at the markers and requires, per search, the same ordered list
of (kernel name with template arguments, grid, workgroup, LDS bytes).  It also checks that build A's trace holds every
kernel of KERNELS.  Seeded data (bench.ivf_dataset), no files read.
"""
import csv
import glob
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# every kernel the search path can launch
KERNELS = ["ivf_route_kernel", "ivf_route_dist_kernel", "ivf_route_mfma16_kernel", "ivf_route_tail_kernel",
           "ivf_route_tail_wave_kernel", "ivf_bucket_fill_kernel", "probe_pairs_kernel", "ivf_query_prep_kernel",
           "ivf_worklist_kernel", "pair_order_kernel", "stream_bounds_kernel", "ivf_home_kernel", "ivf_home_select_kernel",
           "ivf_home_select_wave_kernel", "ivf_heavy_kernel", "ivf_mid_kernel", "ivf_finish_kernel",
           "ivf_finish_heavy_kernel", "scan_kernel", "select_topk_kernel", "merge_topk_kernel", "ivf_hist_kernel",
           "ivf_plan_kernel", "ivf_scatter_kernel", "l2_group_kernel", "tile_scan_kernel", "ivf_decode_kernel"]
N, NLIST, NPROBE, K = 1_000_000, 1024, 32, 10


def searches():
    """(handle, label, batch, k, given probes?) in the order they run; a handle is (label, metric, rejection mode, IVF_HALF)."""
    default = [1, 4, 8, 32, 256, 1024, 4096, 8192]       # 8192 x 32 probes: 256 pairs per list
    yield ("cosine", "cosine", None, 1), [(b, K, False) for b in default] + [(32, 100, False), (32, K, True)]
    yield ("l2", "l2", None, 1), [(b, K, False) for b in (1, 32, 256, 1024, 4096)]
    # without int8 rows: fused GEMV, GEMV in list order, group kernel, tile scan
    yield ("cosine_mode0", "cosine", 0, 1), [(b, K, False) for b in (1, 32, 64, 1024)]
    yield ("l2_mode0", "l2", 0, 1), [(b, K, False) for b in (32, 1024)]
    # without half-precision rows: the bounds pass's wide epilogue without deferring; the tile scan from 48 pairs per list
    yield ("cosine_nohalf", "cosine", None, 0), [(b, K, False) for b in (32, 256, 1024, 4096)]


def run():
    import numpy as np
    import torch

    import bench
    from hnsw_clj_amd import engine

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    x, Qa = bench.ivf_dataset(dev, N, NLIST, 8192)
    begin = torch.empty(8, dtype=torch.int16, device=dev)      # (empty: creating them launches no fill)
    end = torch.empty(8, dtype=torch.int8, device=dev)
    lists = None
    for (hname, metric, mode, half), todo in searches():
        engine.set_tuning("IVF_HALF", half)
        idx = engine.Index(x, metric, 0)
        if mode is not None:
            idx.set_rejection_test(mode)
        if lists is None:
            idx.ivf_build(NLIST, 3, 42)
            lists = idx.get_ivf()
        else:
            idx.set_ivf(*lists)          # the same lists on every handle
        for i, (nq, k, given) in enumerate(todo):
            label = "%s nq=%d k=%d%s%s" % (hname, nq, k, " given-probes" if given else "",
                                           " (first search of the handle)" if i == 0 else "")
            Q = Qa[:nq].contiguous()
            Qh = Q.cpu().numpy()
            probes = np.tile(np.arange(NPROBE, dtype=np.int32) * 7 % NLIST, (nq, 1)) if given else None
            torch.cuda.synchronize()
            print("== search: " + label, flush=True)
            begin.fill_(1)
            torch.cuda.synchronize()
            if given:
                idx.ivf_search_lists(Qh, k, probes)
            elif nq <= 8:
                idx.ivf_search(Qh, k, NPROBE)      # host entry point: the combiner and the mapped-memory slot
            else:
                idx.ivf_search_dev(Q, k, NPROBE)
            torch.cuda.synchronize()
            end.fill_(1)
            torch.cuda.synchronize()
        idx.close()
    engine.set_tuning("IVF_HALF", None)
    print("done", flush=True)


def read_trace(d):
    """The searches of one trace: [[(kernel, grid, workgroup, lds), ...], ...]"""
    files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    assert files, "no kernel trace under " + d
    rows = []
    for f in files:
        rows += list(csv.DictReader(open(f)))

    def num(r, *names):
        for n in names:
            if n in r:
                return int(r[n])
        xs = [int(r[n + s]) for n in names for s in ("_X", "_Y", "_Z") if n + s in r]
        assert xs, "column missing: %s in %s" % (names, sorted(r))
        return xs[0] * xs[1] * xs[2]

    rows.sort(key=lambda r: (int(r.get("Dispatch_Id", 0)), int(r["Start_Timestamp"])))   # the order of enqueueing
    out, cur = [], None
    for r in rows:
        name = r["Kernel_Name"]
        if "FillFunctor<short>" in name:
            cur = []
        elif "FillFunctor<signed char>" in name:
            assert cur is not None, "end marker without a begin marker"
            out.append(cur)
            cur = None
        elif cur is not None:
            cur.append((name, num(r, "Grid_Size"), num(r, "Workgroup_Size"), num(r, "LDS_Block_Size", "LDS_Block_Size_v")))
    return out


def compare(da, db):
    a, b = read_trace(da), read_trace(db)
    labels = ["%s nq=%d k=%d%s%s" % (h[0], nq, k, " given-probes" if g else "", " (first search of the handle)" if i == 0 else "")
              for h, todo in searches() for i, (nq, k, g) in enumerate(todo)]
    assert len(a) == len(labels) and len(b) == len(labels), "searches in the traces: %d / %d, expected %d" % (len(a), len(b), len(labels))
    bad = 0
    for lab, sa, sb in zip(labels, a, b):
        same = sa == sb
        bad += not same
        print("%-62s %3d launches  %s" % (lab, len(sa), "equal" if same else "DIFFERENT (%d launches in B)" % len(sb)))
        if not same:
            for i in range(max(len(sa), len(sb))):
                ea, eb = (sa[i] if i < len(sa) else None), (sb[i] if i < len(sb) else None)
                if ea != eb:
                    print("    #%d  A: %s\n        B: %s" % (i, ea, eb))
    seen = {}    # kernel name without template arguments -> {full name: grids in workgroups}
    for srch in a:
        for name, grid, wg, lds in srch:
            base = name.split("(")[0].split("<")[0].split()[-1].split("::")[-1]
            seen.setdefault(base, {}).setdefault(name.split("(")[0], set()).add(grid // max(wg, 1))
    missing = [kname for kname in KERNELS if kname not in seen]
    print("\nkernels of the search path missing from build A's trace: %s" % (", ".join(missing) or "none"))
    for base in ("ivf_worklist_kernel", "stream_bounds_kernel", "scan_kernel"):
        print("%s as launched (grids in workgroups):" % base)
        for full, grids in sorted(seen.get(base, {}).items()):
            print("    %s  %s" % (full, sorted(grids) if base == "ivf_worklist_kernel" else ""))
    print("\n%d searches, %d different" % (len(labels), bad))
    return 1 if bad or missing else 0


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    run()
