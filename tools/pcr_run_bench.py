"""sPCR for a whole panel on MI355X: KmerEngine.pcr_run (shk_pcr_run) against the route a caller had
before it — the six stage calls chained in Python (primer_kmers, pcr_extend_panel, pcr_prune_panel,
filter_reads_retained, thread_reads_retained, pcr_products_panel), the code of
tests/test_gpu_pcr_products_panel.py::test_18s_pipeline_yields_the_amplicon generalised to a panel.

    python3 tools/pcr_run_bench.py --out profiles/pcr_run.json

The 10 amplicons and the batches of tools/filter_panel_bench.py at 10^5 and 10^6 reads (k 21, 2 % of the reads cut from
the amplicons), counted on a context that retains them; gene g's primers are 24 bases of its amplicon and the
reverse complement of 24 others, each taken 100 bases inside from an end.  The two routes are measured
ALTERNATING, one untimed call of each first, --repeats samples each (at least 5), every sample kept, median and range
named.  Their answers are compared before anything is timed.  The chain runs the same stage calls, which shk_pcr_run
does not change: timing it on this library is timing what a caller could do before."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]

import numpy as np  # noqa: E402

import sharkmer_amd as sa  # noqa: E402
from filter_panel_bench import COMP, K, amplicons, batch  # noqa: E402
from retained_reads_bench import alternating  # noqa: E402


def panel_genes(amps):
    """Primers 100 bases inside each amplicon: the batches cut their reads from inside the amplicon only, so its first and
    last bases are covered by a few reads and its middle by all of them — a ratio high_coverage_ratio would take for a
    repeat (graph.rs:495) if the walk started at the very end."""
    genes = []
    for i, a in enumerate(amps):
        genes.append(sa.PcrGene("18s" if i == 0 else f"amp{i}", a[100:124].decode(), a[-124:-100][::-1].translate(COMP).decode(),
                                max_length=2500))
    return genes


def canonical(eng, kmers):
    k = np.asarray(kmers, dtype=np.uint64)
    r = np.zeros_like(k)
    x = k.copy()
    for _ in range(K):
        r = (r << np.uint64(2)) | (np.uint64(3) - (x & np.uint64(3)))
        x >>= np.uint64(2)
    return np.unique(np.minimum(k, r))


def chain(eng, genes, budget):
    """The six calls over retained reads → per gene the product sequences (None without both primer sets)."""
    prim = eng.primer_kmers([sa.Primer(s, g.trim, g.mismatches, g.min_count, g.max_primer_kmers) for g in genes
                             for s in (g.forward_seq, g.reverse_seq)])
    alive = [i for i in range(len(genes)) if len(prim[2 * i][0]) and len(prim[2 * i + 1][0])]
    out = [None] * len(genes)
    if not alive:
        return out
    graphs = eng.pcr_extend_panel([prim[2 * i + d] for i in alive for d in (0, 1)],
                                  [dict(min_count=genes[i].min_count, table_min_count=2, high_coverage_ratio=genes[i].high_coverage_ratio,
                                        max_num_nodes=budget) for i in alive])
    for i in alive:
        out[i] = []
    found = [(i, g) for i, g in zip(alive, graphs) if g.found_path]
    if not found:
        return out
    pruned = eng.pcr_prune_panel([g for _, g in found], tip_coverage_fraction=[genes[i].tip_coverage_fraction for i, _ in found])
    lists = eng.filter_reads_retained([canonical(eng, np.concatenate([prim[2 * i][0], prim[2 * i + 1][0]])) for i, _ in found])
    anns = eng.thread_reads_retained(pruned, lists)
    anns = [a if len(l) else None for a, l in zip(anns, lists)]
    gs = [genes[i] for i, _ in found]
    prods = eng.pcr_products_panel(pruned, anns, min_length=[g.min_length for g in gs], max_length=[g.max_length for g in gs],
                                   dedup_edit_threshold=[g.dedup_edit_threshold for g in gs])
    for (i, _), p in zip(found, prods):
        out[i] = p.sequences
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--share", type=float, default=0.02)
    ap.add_argument("--sizes", default="100000,1000000")
    a = ap.parse_args()
    repeats = max(a.repeats, 5)
    seq = open(os.path.join(ROOT, "tests", "golden", "pcr_18s_padded.txt")).read().strip()
    amps = amplicons(seq)
    genes = panel_genes(amps)
    res = {"k": K, "genes": len(genes), "amplicon_share": a.share,
           "sampling": f"wall-clock ms per call, warm context, the two routes alternating, {repeats} samples each, all kept; median and "
                       "range named; every call returns with the products on the host",
           "batches": []}
    for n in [int(x) for x in a.sizes.split(",")]:
        bases, offsets, n_amp = batch(amps, n, a.share)
        with sa.KmerEngine(K, 1, 100) as eng:
            eng.retain_reads(True)
            eng.ingest_reads(bases, offsets)
            eng.finalize()
            budget = sa.pcr_node_budget(eng.counters()["n_bases_ingested"])
            driver = lambda: eng.pcr_run(genes, reads="retained", max_num_nodes=budget)  # noqa: E731
            got, want = driver(), chain(eng, genes, budget)
            for o, w in zip(got, want):  # the routes agree before anything is timed
                assert o.products.sequences == (w or []), f"pcr_run and the chain disagree on {o.gene_name}"
            row = {"reads": n, "amplicon_reads": n_amp, "bases": int(len(bases)), "node_budget": budget,
                   "status": [o.status for o in got], "products": [len(o.products.sequences) for o in got],
                   "reads_matched": [o.n_reads_matched for o in got], "threaded": [int(o.threaded) for o in got]}
            t = alternating({"pcr_run": driver, "six_call_chain": lambda: chain(eng, genes, budget)}, repeats)
            for name, v in t.items():
                v["range_ms"] = [min(v["samples_ms"]), max(v["samples_ms"])]
            row.update(t)
            res["batches"].append(row)
            print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
