"""Developer tool: which kernels does an HNSW search launch, configuration by configuration?

Results can stay equal while a launch silently takes another kernel, another grid or another list size; this runs a fixed list of
searches that together reach every shape of the three traversal kernels (hnsw.hip: hnsw_launch_plan) and, from a kernel trace,
compares two builds of the library launch by launch.

  run (GPU):     HNSWGPU_LIBRARY=<libhnswgpu.so> rocprofv3 --kernel-trace --output-format csv -d <dir> -- \
                     python3 tools/hnsw_launch_matrix.py
  compare:       python3 tools/hnsw_launch_matrix.py --compare <dir of build A> <dir of build B>  > table

Every search is bracketed by two marker kernels (a torch fill of an int16 and of an int8 tensor, which nothing else here
launches) and announced on stdout; --compare cuts the trace at the markers and requires, per search, the same ordered list
of (kernel name with template arguments, grid, workgroup, LDS bytes).  It also checks that build A's trace holds the three
traversal kernels in every shape of SHAPES.  Seeded data (datagen.generate_dataset), no files read.
"""
import csv
import glob
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# every shape the plan can name: kernel -> the template arguments behind (NCH, rows in flight, L2)
SHAPES = {"hnsw_search_kernel": [(nw, vg, "false") for nw in ("1", "2", "4") for vg in ("false", "true")] + [("4", "false", "true")],
          "hnsw_wave_kernel": [("false",), ("true",)],
          "hnsw_solo_kernel": [("true",), ("false",)]}      # (the solo kernel's fourth argument is L2 itself: both metrics' kinds)
K = 10
WIDE = {"HNSW_WAVE": 0}        # the single-workgroup kernel where the default rule takes the wave kernel
HBM = {"VIS_GLOBAL": 1}


def handles():
    """(name, metric, dim, rows) and its steps in the order they run.  A step: ("build",), ("mode", m) or
    ("search", queries, ef, tuning keys of this search)."""
    main = []
    for mode, sizes in ((2, (300, 1100, 2100)), (0, (300, 800, 1600))):     # 4, 2 and 1 waves per query, with / without the test
        main.append(("mode", mode))
        for t in (WIDE, dict(WIDE, **HBM)):
            main += [("search", nq, 50, t) for nq in sizes]
    main.append(("mode", 2))
    main += [("search", nq, 50, {"SOLO": 0}) for nq in (1, 20)]              # the round-2 helper kernel
    main += [("search", nq, 50, {}) for nq in (1, 128)]                      # ... by the default rule below ef 96
    main += [("search", 20, 50, {"SOLO": 0, "PF_EVAL": 0}), ("search", 1, 50, {"PREFETCH": 0}), ("search", 1, 200, {"PREFETCH": 0})]
    main += [("search", nq, ef, {}) for ef in (96, 200, 640) for nq in (1, 20, 128)]     # one query over several CUs
    main += [("search", 1, 50, {"SOLO": 2}), ("search", 20, 200, {"SOLO_SLOTS": 9, "SOLO_CHASE": 0, "PF_HINTS": 3})]
    main += [("search", 129, 50, {}), ("search", 129, 200, {}), ("search", 256, 640, {})]  # no helpers; the wave kernel from ef 640
    main += [("search", 2100, 50, {}), ("search", 2100, 50, HBM)]           # ... and above 2048 queries
    main += [("search", 130, 50, dict(t, HNSW_WAVE=2)) for t in ({}, HBM)]   # ... and forced
    main += [("search", 2100, ef, WIDE) for ef in (1600, 3200)]             # fewer than 13 waves per CU: 2, then 4 waves per query
    main += [("search", 300, 50, {"HNSW_NW": nw}) for nw in (1, 2, 4)]
    main += [("search", 130, 10, {}), ("search", 600, 10, {}), ("search", 600, 10, HBM)]   # 300 duplicated rows: the repeat pass
    yield ("cosine136", "cosine", 136, 12000), [("build",)] + main
    # rejection modes on one handle: mode 1 measures on its first large launch, the launch after it reads the verdict
    yield ("cosine136_modes", "cosine", 136, 12000), [("build",), ("mode", 1)] + [("search", 1300, 48, {})] * 3 + \
        [("search", 300, 48, {}), ("mode", 0), ("search", 1300, 48, {}), ("mode", 2), ("search", 1300, 48, {})]
    for name, metric, dim, rows in (("l2_768", "l2", 768, 6000), ("dot1536", "dot", 1536, 4000)):
        steps = [("build",)]
        for mode in (2, 0):
            steps.append(("mode", mode))
            steps += [("search", 1, 50, {}), ("search", 1, 200, {}), ("search", 300, 50, WIDE), ("search", 300, 50, {"HNSW_WAVE": 2}),
                      ("search", 2100, 50, {})]
        yield (name, metric, dim, rows), steps


def labels():
    out = []
    for (hname, _, _, _), steps in handles():
        mode = 1
        for s in steps:
            if s[0] == "mode":
                mode = s[1]
            elif s[0] == "build":
                out.append("%s hnsw_build" % hname)
            else:
                out.append("%s mode=%d nq=%d ef=%d %s" % (hname, mode, s[1], s[2], " ".join("%s=%d" % kv for kv in sorted(s[3].items()))))
    return out


def run():
    import numpy as np
    import torch

    from hnsw_clj_amd import datagen, engine

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    begin = torch.empty(8, dtype=torch.int16, device=dev)      # (empty: creating them launches no fill)
    end = torch.empty(8, dtype=torch.int8, device=dev)
    names = iter(labels())

    def bracket(fn):
        torch.cuda.synchronize()
        print("== search: " + next(names), flush=True)
        begin.fill_(1)
        torch.cuda.synchronize()
        fn()
        torch.cuda.synchronize()
        end.fill_(1)
        torch.cuda.synchronize()

    for (hname, metric, dim, rows), steps in handles():
        base = datagen.generate_dataset(rows, dim, "clustered", seed=61).astype(np.float32)
        base[7000 % rows:7000 % rows + 300] = base[23]              # 300 copies of one row: ties beyond the ghost slots
        Q = np.concatenate([datagen.generate_dataset(2099, dim, "clustered", seed=62).astype(np.float32), base[23:24]])
        idx = engine.Index(base, metric, 0)
        for s in steps:
            if s[0] == "mode":
                idx.set_rejection_test(s[1])
            elif s[0] == "build":
                bracket(lambda: idx.hnsw_build(16, 80, 42))        # its searches come through the same launch function
            else:
                _, nq, ef, tuning = s
                for key, v in tuning.items():
                    engine.set_tuning(key, v)
                q = Q[-nq:] if ef == 10 else Q[:nq]                 # (the last query is the duplicated row)
                bracket(lambda: idx.hnsw_search(q, K, ef))          # host entry point: the combiner, the mapped-memory slot up to 256 queries
                for key in tuning:
                    engine.set_tuning(key, None)
        idx.close()
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
    labs = labels()
    assert len(a) == len(labs) and len(b) == len(labs), "searches in the traces: %d / %d, expected %d" % (len(a), len(b), len(labs))
    bad = 0
    for lab, sa, sb in zip(labs, a, b):
        same = sa == sb
        bad += not same
        print("%-78s %4d launches  %s" % (lab, len(sa), "equal" if same else "DIFFERENT (%d launches in B)" % len(sb)))
        if not same:
            for i in range(max(len(sa), len(sb))):
                ea, eb = (sa[i] if i < len(sa) else None), (sb[i] if i < len(sb) else None)
                if ea != eb:
                    print("    #%d  A: %s\n        B: %s" % (i, ea, eb))
    seen = {}    # kernel name without template arguments -> {template arguments: {(grid in workgroups, workgroup, LDS bytes)}}
    for lab, srch in zip(labs, a):
        if lab.endswith("hnsw_build"):
            continue
        for name, grid, wg, lds in srch:
            m = re.search(r"(hnsw_\w+_kernel)<([^>]*)>", name)
            if m:
                targs = tuple(t.strip() for t in m.group(2).split(","))
                seen.setdefault(m.group(1), {}).setdefault(targs, set()).add((grid // max(wg, 1), wg, lds))
    missing = []
    for kname, shapes in SHAPES.items():
        width = len(shapes[0])       # template arguments behind (NCH, rows in flight, L2); a defaulted last one reads "false"
        tails = {(t[3:] + ("false",))[:width] for t in seen.get(kname, {})}
        missing += ["%s<..., %s>" % (kname, ", ".join(s)) for s in shapes if s not in tails]
    print("\nshapes of the traversal kernels missing from build A's trace: %s" % (", ".join(missing) or "none"))
    for kname in SHAPES:
        print("%s as launched by the searches: instantiation, then (workgroups, workgroup size, LDS bytes)" % kname)
        for targs, shapes in sorted(seen.get(kname, {}).items()):
            print("    <%s>  %s" % (", ".join(targs), " ".join("(%d, %d, %d)" % s for s in sorted(shapes))))
    print("\n%d searches, %d different" % (len(labs), bad))
    return 1 if bad or missing else 0


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    run()
