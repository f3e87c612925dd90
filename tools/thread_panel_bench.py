"""sPCR's read threading for a whole panel on MI355X: KmerEngine.thread_reads_panel (shk_thread_reads_panel_device) against
the route a caller had before it — per gene, gather_reads + thread_reads(device=True) — both fed by the same
filter_reads_panel answer over the same device-resident batch, in the same process.

    python3 tools/thread_panel_bench.py --out profiles/thread_panel.json

Panel: the 10 genes of tools/filter_panel_bench.py at k 21 (gene 0's amplicon is the 18S sequence of
tests/golden/pcr_18s_padded.txt and its graph the one pcr_extend builds; genes 1–9 are 400-base amplicons whose graph is
the chain of their windows).  Batches: 10^5 and 10^6 synthetic 150-base reads of which --share (default 0.1, a tenth)
are cut from the amplicons, both strands.  The panel filter runs once per batch and is not timed.  Wall-clock per
route on a warm context (one call of each made before, so scratch is allocated); --repeats rounds (default 7) of the two
routes in turn, every sample kept and the median named.  The two routes' answers are compared before anything is timed."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]

import numpy as np  # noqa: E402

import sharkmer_amd as sa  # noqa: E402
import filter_panel_bench as fp  # noqa: E402

K = fp.K
FIELDS = ("support_total", "support_unambiguous", "links", "link_counts", "read_edges")


def enc(s: bytes) -> int:
    v = 0
    for ch in s:
        v = (v << 2) | b"ACGT".index(ch)
    return v


def chain_graph(amp: bytes):
    """The chain of an amplicon's windows: node i = its i-th (k−1)-mer, edge i = its i-th k-mer."""
    n = len(amp) - K + 1
    sub = np.array([enc(amp[i:i + K - 1]) for i in range(n + 1)], dtype=np.uint64)
    return sub, np.arange(n, dtype=np.uint32), np.arange(1, n + 1, dtype=np.uint32)


def timed_alternating(calls: dict, repeats: int) -> dict:
    """Every route once to warm, then `repeats` rounds of every route in turn, so that what else the machine does meets
    both alike.  Each call returns with its answer on the host, so the host clock covers the device's work."""
    for call in calls.values():
        call()
    out = {name: [] for name in calls}
    for _ in range(repeats):
        for name, call in calls.items():
            t0 = time.perf_counter()
            call()
            out[name].append(round((time.perf_counter() - t0) * 1e3, 3))
    return {name: {"samples_ms": x, "median_ms": statistics.median(x)} for name, x in out.items()}


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--share", type=float, default=0.1)
    ap.add_argument("--sizes", default="100000,1000000")
    a = ap.parse_args()
    seq, g18 = fp.graph_18s()
    amps = fp.amplicons(seq)
    graphs = [(g18.node_sub_kmers, g18.edge_src, g18.edge_tgt)] + [chain_graph(x[:400]) for x in amps[1:]]
    res = {"k": K, "genes": fp.N_GENES, "amplicon_share": a.share, "graph_edges": [int(len(x[1])) for x in graphs],
           "sampling": f"wall-clock ms per route, warm context, {a.repeats} rounds of the two routes in turn, all samples kept, median "
                       "named; both routes start from the panel filter's lists on the host and the batch on the device, and return "
                       "with every gene's annotation on the host",
           "batches": []}
    with sa.KmerEngine(K, 1, 100) as eng:
        genes = fp.panel(eng, amps)
        for n in [int(x) for x in a.sizes.split(",")]:
            bases, offsets, n_amp = fp.batch(amps, n, a.share)
            db = torch.from_numpy(bases).to(eng._tdev)
            do = torch.from_numpy(offsets.astype(np.int64)).to(eng._tdev)
            torch.cuda.synchronize()
            lists = eng.filter_reads_panel(db, do, genes, device=True)

            def panel_call():
                return eng.thread_reads_panel(graphs, db, do, lists, device=True)

            def per_gene():
                out = []
                for graph, ids in zip(graphs, lists):
                    gb, go = eng.gather_reads(db, do, ids)
                    out.append(eng.thread_reads(graph, gb, go, device=True))
                return out

            # the routes agree before anything is timed
            for x, y in zip(panel_call(), per_gene()):
                assert all(np.array_equal(getattr(x, f), getattr(y, f)) for f in FIELDS), "the panel call and the per-gene calls disagree"
            row = {"reads": n, "amplicon_reads": n_amp, "bases": int(len(bases)), "listed_reads": [int(len(x)) for x in lists],
                   "mapped_reads": [int((x.read_edges > 0).sum()) for x in panel_call()]}
            row.update(timed_alternating({"thread_reads_panel": panel_call, "gather_thread_x%d" % fp.N_GENES: per_gene}, a.repeats))
            res["batches"].append(row)
            print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
