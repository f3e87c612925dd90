"""sPCR graph pruning for a whole panel on MI355X: KmerEngine.pcr_prune_panel (shk_pcr_prune_panel) beside its neighbours
in the stage chain, pcr_extend_panel before it and thread_reads_panel after it, on the same panel in the same process.

    python3 tools/pcr_prune_panel_bench.py --out profiles/pcr_prune_panel.json
    python3 tools/pcr_prune_panel_bench.py --sizes 1,16 --skip-big       (a part of it)

Panels (k 21, warm context): those of tools/pcr_extend_panel_bench.py — G = 1, 16, 64, 256 amplicon genes on a 1 Mb
synthetic genome at 30×, and the five off-target pairs on the 30 Mb genome at 10× whose genes run to their node budget.
Per panel: `prune_ms_lds` / `prune_ms_global` = whole-call wall-clock ms of pcr_prune_panel through the Python wrapper
(it ends in a device synchronise) with the genes that fit pruned in LDS (the default) and with every gene in global
memory (SHK_PRUNE_LDS_NODES=0), `repeats` samples taken alternating after an untimed call of each: min, median, max;
`device_ms_*` = the call's own event time around its launch, same samples; `extend_ms` = pcr_extend_panel on the same
primer sets; `thread_ms` = thread_reads_panel of the pruned graphs over a device-resident batch of the reads, each gene
over the reads filter_reads_panel lists for its primer k-mers.  The two forms' answers are compared, not assumed."""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [HERE, os.path.join(HERE, "tools")]

import pcr_extend_panel_bench as xb  # noqa: E402  (the panels are its panels)

K = xb.K


def stats(xs):
    return {"n": len(xs), "min": round(min(xs), 3), "median": round(statistics.median(xs), 3), "max": round(max(xs), 3)}


def timed(f):
    t0 = time.perf_counter()
    out = f()
    return (time.perf_counter() - t0) * 1e3, out


def canonical(kmers):
    out = []
    for x in kmers.tolist():
        r, y = 0, x
        for _ in range(K):
            r = (r << 2) | (3 - (y & 3))
            y >>= 2
        out.append(min(x, r))
    return out


def same(a, b):
    fields = ("node_keep", "node_index", "edge_src", "edge_tgt", "edge_counts", "edge_index", "coverage_ratio")
    return len(a) == len(b) and all(all(getattr(x, f).tobytes() == getattr(y, f).tobytes() for f in fields) and
                                    (x.median, x.tip_rounds, x.tips_removed, x.unreachable_removed) ==
                                    (y.median, y.tip_rounds, y.tips_removed, y.unreachable_removed) for x, y in zip(a, b))


def measure(sa, eng, prim, params, batch, repeats, extend_repeats):
    db, do = batch
    ng = len(prim) // 2
    graphs = eng.pcr_extend_panel(prim, params)  # (warm)
    extend = [timed(lambda: eng.pcr_extend_panel(prim, params))[0] for _ in range(extend_repeats)]

    def prune(lds_nodes):
        if lds_nodes is None:
            os.environ.pop("SHK_PRUNE_LDS_NODES", None)
        else:
            os.environ["SHK_PRUNE_LDS_NODES"] = str(lds_nodes)
        try:
            out = eng.pcr_prune_panel(graphs)
        finally:
            os.environ.pop("SHK_PRUNE_LDS_NODES", None)
        return out, eng.last_prune_device_ms

    in_lds, _ = prune(None)
    in_global, _ = prune(0)
    wall = {"lds": [], "global": []}
    dev = {"lds": [], "global": []}
    for _ in range(repeats):
        for form, arg in (("lds", None), ("global", 0)):
            ms, (_, dms) = timed(lambda: prune(arg))
            wall[form].append(ms)
            dev[form].append(dms)
    lists = eng.filter_reads_panel(db, do, [canonical(prim[2 * g][0]) + canonical(prim[2 * g + 1][0]) for g in range(ng)], device=True)
    eng.thread_reads_panel(in_lds, db, do, lists, device=True)  # (warm)
    thread = [timed(lambda: eng.thread_reads_panel(in_lds, db, do, lists, device=True))[0] for _ in range(repeats)]
    fits = sum(1 for g in graphs if 0 < len(g.node_sub_kmers) <= 2560 and
               24 * len(g.node_sub_kmers) + 8 + 8 * len(g.edge_src) + 8 * ((len(g.edge_src) + 31) // 32) <= 79 << 10)
    return {"genes": ng, "nodes_in": sum(len(g.node_sub_kmers) for g in graphs), "edges_in": sum(len(g.edge_src) for g in graphs),
            "nodes_out": sum(len(g.node_sub_kmers) for g in in_lds), "edges_out": sum(len(g.edge_src) for g in in_lds),
            "largest_gene_nodes": max(len(g.node_sub_kmers) for g in graphs), "genes_in_lds_by_default": fits,
            "tip_rounds_max": max(g.tip_rounds for g in in_lds), "tips_removed": sum(g.tips_removed for g in in_lds),
            "unreachable_removed": sum(g.unreachable_removed for g in in_lds), "forms_agree": same(in_lds, in_global),
            "listed_reads": sum(len(x) for x in lists), "extend_ms": stats(extend), "prune_ms_lds": stats(wall["lds"]),
            "prune_ms_global": stats(wall["global"]), "device_ms_lds": stats(dev["lds"]), "device_ms_global": stats(dev["global"]),
            "thread_ms": stats(thread)}


def read_batch(sa, eng, genome, n_reads):
    import torch
    db = torch.empty(n_reads * 150, dtype=torch.uint8, device="cuda:0")
    do = torch.empty(n_reads + 1, dtype=torch.int64, device="cuda:0")
    eng.synth_reads_device(sa.SynthSpec(genome_len=genome), 0, n_reads, db.data_ptr(), do.data_ptr())
    eng.sync()
    return db, do


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--sizes", default="1,16,64,256", help="genes per amplicon panel ('' = none)")
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--extend-repeats", type=int, default=2)
    ap.add_argument("--skip-big", action="store_true")
    a = ap.parse_args()
    import sharkmer_amd as sa
    sizes = [int(x) for x in a.sizes.split(",") if x]
    res = {"k": K, "repeats": a.repeats, "amplicons_1Mb_30x": {}}
    if sizes:
        genome, reads = 1_000_000, 200_000
        eng = xb.build_engine(sa, genome, reads)
        params = dict(min_count=2, table_min_count=2, sweep=True, max_num_nodes=sa.pcr_node_budget(reads * 150))
        prim = xb.amplicon_panel(sa, eng, genome, max(sizes))
        batch = read_batch(sa, eng, genome, reads)
        for g in sizes:
            res["amplicons_1Mb_30x"][str(g)] = measure(sa, eng, prim[:2 * g], params, batch, a.repeats, a.extend_repeats)
            print(g, json.dumps(res["amplicons_1Mb_30x"][str(g)]), flush=True)
        del batch
        eng.close()
    if not a.skip_big:
        genome, reads = 30_000_000, 2_000_000
        eng = xb.build_engine(sa, genome, reads)
        params = dict(min_count=2, table_min_count=1, sweep=False, max_num_nodes=sa.pcr_node_budget(reads * 150))
        prim = xb.offtarget_panel(sa, eng, genome)
        batch = read_batch(sa, eng, genome, 1_000_000)
        res["offtarget_30Mb_10x"] = measure(sa, eng, prim, params, batch, a.repeats, a.extend_repeats)
        print("30Mb", json.dumps(res["offtarget_30Mb_10x"]), flush=True)
        del batch
        eng.close()
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
