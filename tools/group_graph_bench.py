"""sPCR graph extension on a multi-device context (SHK_FLAG_GROUP_GRAPH) against the plain context on the same card.

    python3 tools/group_graph_bench.py --out profiles/group_graph.json

The 10-gene amplicon panel and the table of tools/pcr_extend_panel_bench.py (k 21, a 1 Mb synthetic genome at 30×,
error-free 150 bp reads, primer pairs 300-1800 bases apart) and one shk_pcr_extend_panel call on three contexts that hold
the same reads: a plain one, device ids [0, 0] with the flag, [0] * 8 with the flag.  On one card the sharded route makes
the same probes into the same HBM; what differs is the share directory (its upload rides in the call's one copy; the
narrow kernel's descriptor read goes to LDS) and one settle and stream synchronise per share and fetch.

Per context: wall-clock ms around the call (it ends in a device synchronise), `samples` of them taken alternating between
the three in one process after two untimed calls each: median, min, max.  extend_ms / extend_launches: device time and
timed launches in the SHK_K_EXTEND slot of one call on a second set of contexts created with FLAG_TIMING, so that the
event records are not in the wall-clock figures; host_ms = the median wall-clock minus that device time — what the host
side of the call costs, the per-share settles among it.  Distinct cards cannot be measured by this tool on a one-card box:
the remote-probe latency over xGMI and the visibility of peers' writes are unmeasured."""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [HERE, os.path.join(HERE, "tools")]
K, GENOME, READS, GENES = 21, 1_000_000, 200_000, 10
CONTEXTS = (("plain", None), ("group_2", [0, 0]), ("group_8", [0] * 8))


def build(sa, bases, offsets, device_ids, flags):
    if device_ids is None:
        eng = sa.KmerEngine(K, 1, 100, capacity_hint=GENOME, flags=flags)
    else:
        eng = sa.KmerEngine(K, 1, 100, capacity_hint=GENOME, flags=flags | sa.FLAG_GROUP_GRAPH, device_ids=device_ids)
    eng.ingest_reads(bases, offsets)
    eng.finalize()
    return eng


def same(a, b):
    return len(a) == len(b) and all((x.node_sub_kmers.tolist(), x.edge_src.tolist(), x.edge_tgt.tolist(), x.edge_counts.tolist(), x.steps_run) ==
                                    (y.node_sub_kmers.tolist(), y.edge_src.tolist(), y.edge_tgt.tolist(), y.edge_counts.tolist(), y.steps_run)
                                    for x, y in zip(a, b))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--samples", type=int, default=5)
    a = ap.parse_args()
    import sharkmer_amd as sa
    from pcr_extend_panel_bench import amplicon_panel
    bases, offsets = sa.synth_reads(sa.SynthSpec(genome_len=GENOME), 0, READS)
    params = dict(min_count=2, table_min_count=2, sweep=True, max_num_nodes=sa.pcr_node_budget(READS * 150))
    res = {"k": K, "genome": GENOME, "reads": READS, "genes": GENES, "samples": a.samples, "contexts": {}}
    engines = {name: build(sa, bases, offsets, ids, 0) for name, ids in CONTEXTS}
    prim = amplicon_panel(sa, engines["plain"], GENOME, GENES)
    got = {}
    for name, eng in engines.items():  # warm: code objects, scratch
        for _ in range(2):
            got[name] = eng.pcr_extend_panel(prim, params)
    wall = {name: [] for name in engines}
    for _ in range(a.samples):
        for name, eng in engines.items():
            t0 = time.perf_counter()
            eng.pcr_extend_panel(prim, params)
            wall[name].append((time.perf_counter() - t0) * 1e3)
    for eng in engines.values():
        eng.close()
    res["found_path"] = sum(g.found_path for g in got["plain"])
    res["nodes"] = [len(g.node_sub_kmers) for g in got["plain"]]
    for name, ids in CONTEXTS:
        eng = build(sa, bases, offsets, ids, sa.FLAG_TIMING)
        eng.pcr_extend_panel(prim, params)
        eng.sync()
        eng.reset_timings()
        eng.pcr_extend_panel(prim, params)
        eng.sync()
        t = eng.timings()
        eng.close()
        ms, n = t.get("extend", (0.0, 0))
        xs = wall[name]
        res["contexts"][name] = {"device_ids": ids, "equals_plain": same(got[name], got["plain"]),
                                 "wall_ms": {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3),
                                             "samples": [round(x, 3) for x in xs]},
                                 "extend_ms": round(ms, 3), "extend_launches": n, "host_ms": round(statistics.median(xs) - ms, 3),
                                 "other_timed_launches": {k: v[1] for k, v in t.items() if k != "extend"}}
    base = res["contexts"]["plain"]["wall_ms"]["median"]
    for name in res["contexts"]:
        res["contexts"][name]["wall_over_plain"] = round(res["contexts"][name]["wall_ms"]["median"] / base, 3)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
