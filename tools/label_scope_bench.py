"""Label-scoped graphs from one snapshot (jg_builder_keep_labels / jg_builder_finish_labels) at RMAT scale.

Labels are `edge index mod 4`, the scope is one label.  Measured on the GPU, one JSON line out:
  (a) jg_builder_finish_labels on a label-keeping ids builder (whole call: host clock around the call, which
      ends synchronised, and its build_ms; the select alone: HIP events, against its byte model as a share
      of 8 TB/s) against the route without it: filter on the host, then jg_graph_build from the filtered
      host arrays (H2D copy included).  Both graphs must give identical PageRank.
  (b) --rows: the chunked rows snapshot (tools/edgestore_bench.py's store and feeding) with and without
      keep_labels, alternating in one process: wall time of add_rows + finish.
  (c) device memory a builder holds once every chunk is in, with and without labels (free device memory
      before and after, the library's block cache trimmed first).
Usage: python tools/label_scope_bench.py [--scale 20] [--reps 5] [--chunks 8] [--rows]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

HBM_PEAK_GBS = 8000.0


def device_free_bytes():
    """hipMemGetInfo of the current device, through the HIP runtime libjanusgpu itself is linked against."""
    import ctypes
    hip = ctypes.CDLL("libamdhip64.so")
    free, total = ctypes.c_size_t(0), ctypes.c_size_t(0)
    if hip.hipDeviceSynchronize() != 0 or hip.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) != 0:
        raise RuntimeError("hipMemGetInfo failed")
    return int(free.value)


def median(xs):
    return float(np.median(np.asarray(xs, np.float64)))


def spread(xs):
    return [round(float(min(xs)), 3), round(float(max(xs)), 3)]


def ids_builder(ctx, vid, chunks, labeled):
    """(builder, device bytes it holds) after every chunk went in."""
    ctx.trim()
    before = device_free_bytes()
    b = ctx.builder()
    if labeled:
        b.keep_labels()
    b.add_vertices(vid)
    for s, t, lab in chunks:
        b.add_edges(s, t, label=lab if labeled else None)
    ctx.trim()
    return b, before - device_free_bytes()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--edgefactor", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--chunks", type=int, default=8)
    ap.add_argument("--rows", action="store_true", help="also time the rows snapshot with and without keep_labels")
    args = ap.parse_args()
    import janusgraph_amd as jg
    from oracle import oracle as o  # input generator only: the RMAT edge list

    n, m = 1 << args.scale, args.edgefactor << args.scale
    seed = 0x5EED + args.scale
    vid = (np.arange(n, dtype=np.int64) + 1) << 8
    step = (m + args.chunks - 1) // args.chunks
    chunks = []
    for e0 in range(0, m, step):
        s, t = o.rmat_edges(args.scale, args.edgefactor, seed, e0, min(step, m - e0))
        chunks.append((vid[s], vid[t], (np.arange(e0, e0 + len(s), dtype=np.int64) % 4)))
    scope = [1]
    flags = jg.ADJ_IN
    ctx = jg.Context((0,))

    # (c) what each builder holds on the device
    plain, plain_bytes = ids_builder(ctx, vid, chunks, False)
    plain.close()
    b, labeled_bytes = ids_builder(ctx, vid, chunks, True)

    # (a) the scoped finish, repeated on the one builder (warm-up first)
    whole, build_ms, select_ms = [], [], []
    st = None
    for rep in range(args.reps + 1):
        t0 = time.perf_counter()
        g = b.finish_labels(scope, flags)
        t1 = time.perf_counter()
        st = ctx.stats()
        if rep:
            whole.append((t1 - t0) * 1e3)
            build_ms.append(st["build_ms"])
            select_ms.append(st["kernel_ms_total"])
        if rep < args.reps:
            g.close()
    scoped = g
    kept = scoped.info()["num_edges"] + scoped.info()["ghost_edges"]

    # the route without it: filter on the host, then jg_graph_build from the host arrays
    filt, direct, direct_build_ms = [], [], []
    for rep in range(args.reps + 1):
        t0 = time.perf_counter()
        keep = [lab == scope[0] for _, _, lab in chunks]
        fs = np.concatenate([s[k] for (s, _, _), k in zip(chunks, keep)])
        ft = np.concatenate([t[k] for (_, t, _), k in zip(chunks, keep)])
        t1 = time.perf_counter()
        g2 = ctx.build(vid, fs, ft, flags=flags)
        t2 = time.perf_counter()
        if rep:
            filt.append((t1 - t0) * 1e3)
            direct.append((t2 - t1) * 1e3)
            direct_build_ms.append(ctx.stats()["build_ms"])
        if rep < args.reps:
            g2.close()
    assert len(fs) == kept, "the select kept another number of edges than the host filter"
    r1, _ = scoped.pagerank(0.85, n, 5)
    r2, _ = g2.pagerank(0.85, n, 5)
    assert np.array_equal(r1, r2), "PageRank differs between the scoped and the host-filtered graph"
    scoped.close()
    g2.close()
    b.close()

    sel = median(select_ms)
    alg = st["algorithmic_bytes"]
    line = {
        "workload": f"label_scope_rmat{args.scale}_ef{args.edgefactor}", "edges": int(m), "kept": int(kept),
        "reps": args.reps, "chunks": len(chunks),
        "finish_labels_wall_ms": round(median(whole), 3), "finish_labels_wall_ms_range": spread(whole),
        "finish_labels_build_ms": round(median(build_ms), 3),
        "select_ms": round(sel, 4), "select_ms_range": spread(select_ms), "select_launches": int(st["kernel_launches"]),
        "select_roofline": {"bound": "hbm", "bytes": alg, "achieved": round(alg / (sel * 1e-3) / 1e9, 1),
                            "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(alg / (sel * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)},
        "host_filter_ms": round(median(filt), 3), "graph_build_wall_ms": round(median(direct), 3),
        "graph_build_wall_ms_range": spread(direct), "graph_build_build_ms": round(median(direct_build_ms), 3),
        "ratio_build_over_finish_labels": round(median(direct) / median(whole), 3),
        "ratio_filter_and_build_over_finish_labels": round((median(filt) + median(direct)) / median(whole), 3),
        "builder_device_bytes": {"plain": int(plain_bytes), "labeled": int(labeled_bytes),
                                 "model_plain": 16 * m + 8 * n, "model_labeled": 24 * m + 8 * n},
        "pagerank_identical": True,
    }

    if args.rows:
        from edgestore_bench import write_edgestore
        rvid, rs, rt, keys, roff, data, off, vpos = write_edgestore(args.scale, args.edgefactor, seed)
        rows = {}
        for k in (1, args.chunks):
            bounds = np.linspace(0, len(keys), k + 1).astype(np.int64)
            pieces = []
            for lo, hi in zip(bounds[:-1], bounds[1:]):
                e0, e1 = int(roff[lo]), int(roff[hi])
                b0, b1 = int(off[e0]), int(off[e1])
                pieces.append((keys[lo:hi], roff[lo:hi + 1] - e0, data[b0:b1], off[e0:e1 + 1] - b0, vpos[e0:e1]))
            wall = {False: [], True: []}
            ranks = {}
            for rep in range(args.reps + 1):
                for labeled in (False, True):  # alternating
                    rb = ctx.builder()
                    if labeled:
                        rb.keep_labels()
                    rb.set_schema()
                    t0 = time.perf_counter()
                    for p in pieces:
                        rb.add_rows(*p)
                    gk = rb.finish(flags)
                    t1 = time.perf_counter()
                    if rep:
                        wall[labeled].append((t1 - t0) * 1e3)
                    else:
                        ranks[labeled] = gk.pagerank(0.85, len(rvid), 5)[0]
                    gk.close()
                    rb.close()
            assert np.array_equal(ranks[False], ranks[True]), "keep_labels changed the rows snapshot"
            rows[f"chunks_{k}"] = {"plain_ms": round(median(wall[False]), 2), "plain_ms_range": spread(wall[False]),
                                   "keep_labels_ms": round(median(wall[True]), 2),
                                   "keep_labels_ms_range": spread(wall[True])}
        line["rows_snapshot"] = rows
    print(json.dumps(line), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
