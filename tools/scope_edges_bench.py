"""What numbering a label scope's edges costs (jg_builder_keep_scope_ordinals; DESIGN.md §5, "Edge ordinals in
label scopes").

Input: an RMAT edge list with 4 random labels through a label-keeping ids builder.  Timed on the GPU, alternating
the variants inside one process, one JSON line out: jg_builder_finish_labels of one label and of all labels
  plain      without the opt-in (what the select did before the opt-in existed);
  positions  with it and JG_ADJ_EDGE_INDEX: the scatter also writes each kept edge's position (8 B);
  rows3      (--rows) a rows builder with keep_relations and set_weight_key_f64 (tools/edgestore_bench.py's store,
             one label, a Double on every edge): positions, relation ids and doubles, 8 + 16 + 16 B per kept edge.
Per case: the select's HIP-event time (kernel_ms_total: count, scan, scatter), its byte model and the share of
8 TB/s that is, and the whole call's build_ms (with JG_ADJ_EDGE_INDEX the CSR build carries the ordinals as well,
so build_ms is not the select's cost).
--plain-only runs the plain cases alone and needs nothing newer than jg_builder_finish_labels: the same script on
an older checkout, in alternating processes, gives the spread to judge `plain` by.
Usage: python tools/scope_edges_bench.py [--scale 20] [--reps 7] [--rows] [--plain-only] [--tag NAME]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

HBM_PEAK_GBS = 8000.0


def summary(runs):
    """runs: [(select_ms, build_ms, algorithmic_bytes, launches, kept)] of one case."""
    sel = np.array([r[0] for r in runs])
    med = float(np.median(sel))
    alg = runs[-1][2]
    return {"kept": int(runs[-1][4]), "select_ms": round(med, 4),
            "select_ms_range": [round(float(sel.min()), 4), round(float(sel.max()), 4)],
            "build_ms": round(float(np.median([r[1] for r in runs])), 3), "launches": int(runs[-1][3]),
            "bytes": alg, "GBs": round(alg / (med * 1e-3) / 1e9, 1),
            "frac_of_peak": round(alg / (med * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--edgefactor", type=int, default=16)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rows", action="store_true")
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--tag", default="")
    args = ap.parse_args()
    import janusgraph_amd as jg
    from janusgraph_amd import _lib
    from oracle import oracle as o  # input generator only: the RMAT edge list

    n = 1 << args.scale
    seed = 0x5EED + args.scale
    s, t = o.rmat_edges(args.scale, args.edgefactor, seed)
    m = len(s)
    vid = (np.arange(n, dtype=np.int64) + 1) << 8
    lab = np.random.default_rng(seed).integers(0, 4, m).astype(np.int64)
    ctx = jg.Context((0,))
    flags = jg.ADJ_IN
    scopes = {"one_label": [1], "all_labels": [0, 1, 2, 3]}

    def ids_builder(numbered):
        b = ctx.builder()
        b.keep_labels()
        if numbered:
            b.keep_scope_ordinals()
        b.add_vertices(vid)
        b.add_edges(vid[s], vid[t], label=lab)
        return b

    variants = {"plain": (ids_builder(False), flags)}
    if not args.plain_only:
        variants["positions"] = (ids_builder(True), flags | _lib.ADJ_EDGE_INDEX)
    if args.rows and not args.plain_only:
        from edgestore_bench import F64_KEY, write_edgestore
        from oracle import edgecodec as ec
        rvid, rs_, rt_, keys, roff, data, off, vpos, rel_list = write_edgestore(args.scale, args.edgefactor, seed, True)
        rb = ctx.builder()
        rb.set_schema()
        rb.keep_labels()
        rb.keep_relations()
        rb.keep_scope_ordinals()
        rb.set_weight_key_f64(F64_KEY, [F64_KEY], [_lib.PROP_DOUBLE])
        bounds = np.linspace(0, len(keys), 9).astype(np.int64)
        for lo, hi in zip(bounds[:-1], bounds[1:]):
            e0, e1 = int(roff[lo]), int(roff[hi])
            b0, b1 = int(off[e0]), int(off[e1])
            rb.add_rows(keys[lo:hi], roff[lo:hi + 1] - e0, data[b0:b1], off[e0:e1 + 1] - b0, vpos[e0:e1])
        variants["rows3"] = (rb, flags | _lib.ADJ_EDGE_INDEX)
        row_label = [ec.schema_id(3, "user_edge")]  # the store's one label: every edge is kept

    runs = {}
    for rep in range(args.reps + 1):  # the first repetition warms up
        for case, scope in scopes.items():
            for name, (b, f) in variants.items():  # alternating
                if name == "rows3":
                    if case != "all_labels":
                        continue
                    scope_ids = row_label
                else:
                    scope_ids = scope
                g = b.finish_labels(scope_ids, f)
                st = ctx.stats()
                info = g.info()
                kept = info["num_edges"] + info["ghost_edges"]
                if rep == 0 and name != "plain":
                    pos = g.scope_positions()
                    want = np.flatnonzero(np.isin(lab, scope_ids)) if name == "positions" else np.arange(kept)
                    assert np.array_equal(pos, want), f"{name}/{case}: positions differ from the host filter"
                    if name == "rows3":
                        assert kept == len(rel_list), "the rows scope did not keep the store's one label"
                        at = np.linspace(0, kept - 1, 4096).astype(np.int64)
                        assert np.array_equal(g.edge_relations(at), rel_list[at]), "relation ids differ"
                g.close()
                if rep:
                    runs.setdefault(f"{name}/{case}", []).append(
                        (st["kernel_ms_total"], st["build_ms"], st["algorithmic_bytes"], st["kernel_launches"], kept))
    for b, _ in variants.values():
        b.close()
    line = {"workload": f"scope_edges_rmat{args.scale}_ef{args.edgefactor}", "tag": args.tag, "edges": int(m),
            "reps": args.reps, "cases": {k: summary(v) for k, v in runs.items()}}
    print(json.dumps(line), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
