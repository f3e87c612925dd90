"""sPCR's last stage for a whole panel on MI355X: KmerEngine.pcr_products_panel (shk_pcr_products_panel) at the end of the
stage chain, its two halves apart — pcr_paths_panel (host) and pcr_dedup_panel (K_DEDUP) — and the dedup's host route
beside its device route in the same build and process, which is what sets the default of SHK_DEDUP_DEVICE_PAIRS.

    python3 tools/pcr_products_panel_bench.py --out profiles/pcr_products_panel.json
    python3 tools/pcr_products_panel_bench.py --sizes 1,16 --loads 100x500        (a part of it)

Panels (k 21, warm context): those of tools/pcr_extend_panel_bench.py — G amplicon genes on a 1 Mb synthetic genome at
30×, pushed through primer_kmers → extend → prune → filter → thread → products; with --big the five off-target pairs on
the 30 Mb genome.  Synthetic dedup loads the real panels do not reach: one gene of N records of L bases, `distant`
(independent random sequences: every pair far beyond t = 10) or `related` (one sequence with 15 random edits each: pairs
about 30 apart, so that an alignment has to run a third of the way before it can give up).

Per row: `*_ms_device` / `*_ms_host` = whole-call wall-clock ms through the Python wrapper with SHK_DEDUP_DEVICE_PAIRS=0 /
=2^62, `repeats` samples taken alternating after an untimed call of each: min, median, max; `device_ms` = the call's own
event time around K_DEDUP; `paths_ms` = pcr_paths_panel alone.  The two routes' answers are compared, not assumed."""
import argparse
import json
import os
import random
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [HERE, os.path.join(HERE, "tools")]

K = 21
ROUTES = (("device", "0"), ("host", str(2 ** 62)))


def stats(xs):
    return {"n": len(xs), "min": round(min(xs), 3), "median": round(statistics.median(xs), 3), "max": round(max(xs), 3)}


def timed(f):
    t0 = time.perf_counter()
    out = f()
    return (time.perf_counter() - t0) * 1e3, out


def on_route(value, f):
    os.environ["SHK_DEDUP_DEVICE_PAIRS"] = value
    try:
        return f()
    finally:
        os.environ.pop("SHK_DEDUP_DEVICE_PAIRS", None)


def alternate(call, repeats):
    """call() on either route by turns → ({route: wall ms samples}, {route: last answer})."""
    wall, last = {r: [] for r, _ in ROUTES}, {}
    for r, v in ROUTES:
        on_route(v, call)  # (untimed)
    for _ in range(repeats):
        for r, v in ROUTES:
            ms, out = timed(lambda: on_route(v, call))
            wall[r].append(ms)
            last[r] = out
    return wall, last


def dedup_load(eng, n, length, kind, repeats, t=10):
    rng = random.Random(n * 10007 + length)
    seq = lambda m: "".join(rng.choice("ACGT") for _ in range(m))
    if kind == "distant":
        records = [seq(length) for _ in range(n)]
    else:
        base = list(seq(length))
        records = []
        for _ in range(n):
            s = list(base)
            for _ in range(15):
                s[rng.randrange(length)] = rng.choice("ACGT")
            records.append("".join(s))
    scores = [float(rng.randrange(1000)) for _ in range(n)]
    dev_ms = []

    def call():
        out = eng.pcr_dedup_panel([records], [scores], t)
        dev_ms.append(eng.last_dedup["device_ms"])
        return out[0].kept.tolist(), dict(eng.last_dedup)

    wall, last = alternate(call, repeats)
    return {"records": n, "bases": length, "kind": kind, "t": t, "pairs": n * (n - 1) // 2, "kept": len(last["device"][0]),
            "routes_agree": last["device"][0] == last["host"][0], "pairs_device": last["device"][1]["pairs_device"],
            "dedup_ms_device": stats(wall["device"]), "dedup_ms_host": stats(wall["host"]), "device_ms": stats([x for x in dev_ms if x > 0])}


def canonical(kmers):
    out = []
    for x in kmers.tolist():
        r, y = 0, x
        for _ in range(K):
            r = (r << 2) | (3 - (y & 3))
            y >>= 2
        out.append(min(x, r))
    return out


def panel(sa, eng, prim, params, batch, repeats):
    db, do = batch
    ng = len(prim) // 2
    graphs = eng.pcr_prune_panel(eng.pcr_extend_panel(prim, params))
    lists = eng.filter_reads_panel(db, do, [canonical(prim[2 * g][0]) + canonical(prim[2 * g + 1][0]) for g in range(ng)], device=True)
    anns = eng.thread_reads_panel(graphs, db, do, lists, device=True)
    anns = [a if len(l) else None for a, l in zip(anns, lists)]
    paths = [timed(lambda: sa.pcr_paths_panel(K, graphs, anns))[0] for _ in range(repeats + 1)][1:]
    records = sa.pcr_paths_panel(K, graphs, anns)
    dev_ms = []

    def call():
        out = eng.pcr_products_panel(graphs, anns)
        dev_ms.append(eng.last_products_device_ms)
        return [(p.sequences, p.score.tobytes()) for p in out]

    wall, last = alternate(call, repeats)
    seqs, scs = [r.sequences for r in records], [r.score for r in records]
    dwall, dlast = alternate(lambda: [x.kept.tolist() for x in eng.pcr_dedup_panel(seqs, scs, 10)], repeats)
    return {"genes": ng, "nodes": sum(len(g.node_sub_kmers) for g in graphs), "edges": sum(len(g.edge_src) for g in graphs),
            "threaded_genes": sum(a is not None for a in anns), "paths_found": sum(r.paths_found for r in records),
            "records": sum(r.generated for r in records), "states_explored": sum(r.states_explored for r in records),
            "largest_gene_records": max([r.generated for r in records] or [0]),
            "pairs": sum(r.generated * (r.generated - 1) // 2 for r in records), "products": sum(len(x[0]) for x in last["device"]),
            "routes_agree": last["device"] == last["host"] and dlast["device"] == dlast["host"], "paths_ms": stats(paths),
            "products_ms_device": stats(wall["device"]), "products_ms_host": stats(wall["host"]),
            "dedup_ms_device": stats(dwall["device"]), "dedup_ms_host": stats(dwall["host"]), "device_ms": stats([x for x in dev_ms if x > 0] or [0.0])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--sizes", default="1,16,64,256", help="genes per amplicon panel ('' = none)")
    ap.add_argument("--loads", default="100x500,400x500,800x500,100x2500,400x2500,800x2500", help="synthetic dedup loads, records x bases")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--related-max", type=int, default=50_000_000, help="`related` loads only up to this many pairs x bases")
    ap.add_argument("--big", action="store_true", help="also the off-target panel on the 30 Mb genome")
    a = ap.parse_args()
    import sharkmer_amd as sa
    import pcr_extend_panel_bench as xb  # (the panels are its panels)
    import pcr_prune_panel_bench as pb
    res = {"k": K, "repeats": a.repeats, "dedup_loads": [], "amplicons_1Mb_30x": {}}
    with sa.KmerEngine(K, 1, 100) as eng:
        for load in [x for x in a.loads.split(",") if x]:
            n, length = (int(x) for x in load.split("x"))
            for kind in ("distant", "related"):
                if kind == "related" and n * (n - 1) // 2 * length > a.related_max:  # (the host route's seconds, not the device's)
                    continue
                res["dedup_loads"].append(dedup_load(eng, n, length, kind, a.repeats))
                print(json.dumps(res["dedup_loads"][-1]), flush=True)
        res["dedup_loads"].append(dedup_load(eng, 6, 1800, "related", a.repeats))  # a handful of records: where the device loses
        print(json.dumps(res["dedup_loads"][-1]), flush=True)
    sizes = [int(x) for x in a.sizes.split(",") if x]
    if sizes:
        genome, reads = 1_000_000, 200_000
        eng = xb.build_engine(sa, genome, reads)
        params = dict(min_count=2, table_min_count=2, sweep=True, max_num_nodes=sa.pcr_node_budget(reads * 150))
        prim = xb.amplicon_panel(sa, eng, genome, max(sizes))
        batch = pb.read_batch(sa, eng, genome, reads)
        for g in sizes:
            res["amplicons_1Mb_30x"][str(g)] = panel(sa, eng, prim[:2 * g], params, batch, a.repeats)
            print(g, json.dumps(res["amplicons_1Mb_30x"][str(g)]), flush=True)
        del batch
        eng.close()
    if a.big:
        genome, reads = 30_000_000, 2_000_000
        eng = xb.build_engine(sa, genome, reads)
        params = dict(min_count=2, table_min_count=1, sweep=False, max_num_nodes=sa.pcr_node_budget(reads * 150))
        prim = xb.offtarget_panel(sa, eng, genome)
        batch = pb.read_batch(sa, eng, genome, 1_000_000)
        res["offtarget_30Mb_10x"] = panel(sa, eng, prim, params, batch, a.repeats)
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
