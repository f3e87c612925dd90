"""The sPCR depth sweep on MI355X: a panel at every cumulative chunk from ONE count, against single runs.

    python3 tools/pcr_depths_bench.py --out profiles/pcr_depths.json

tools/pcr_run_bench.py's 10-gene panel and batch (k 21, 2 % of the reads cut from the amplicons), counted with 10 chunks.
Measured ALTERNATING, one untimed call of each first, --repeats samples each (at least 5), every sample kept, median and
range named:
  (i)   pcr_run(reads=None) and primer_kmers, one call each: what one point of a sweep costs without the depth calls
        (beside the recount it needs); their kernels are instruction for instruction the parent commit's;
  (ii)  pcr_run_depths at the 10 depths;
  (iii) primer_kmers_depths at the 10 depths: the fused scan, one pass over the table;
  (iv)  ten one-depth calls of (iii): a lane-bounded scan per depth, ten passes.
Ratios are to 10 x (i).  The fused scan is kept only if (iii) beats (iv) beyond the samples' spread.  The sweep's last
depth is compared with pcr_run before anything is timed."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]

import sharkmer_amd as sa  # noqa: E402
from filter_panel_bench import K, amplicons, batch  # noqa: E402
from pcr_run_bench import panel_genes  # noqa: E402
from retained_reads_bench import alternating  # noqa: E402

CHUNKS = 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--share", type=float, default=0.02)
    ap.add_argument("--sizes", default="100000,1000000")
    a = ap.parse_args()
    repeats = max(a.repeats, 5)
    seq = open(os.path.join(ROOT, "tests", "golden", "pcr_18s_padded.txt")).read().strip()
    genes = panel_genes(amplicons(seq))
    primers = [sa.Primer(s, g.trim, g.mismatches, g.min_count, g.max_primer_kmers) for g in genes for s in (g.forward_seq, g.reverse_seq)]
    depths = list(range(1, CHUNKS + 1))
    res = {"k": K, "genes": len(genes), "chunks": CHUNKS, "depths": depths, "amplicon_share": a.share,
           "sampling": f"wall-clock ms per call, warm context, the five calls alternating, {repeats} samples each, all kept; median "
                       "and range named; every call returns with its results on the host",
           "batches": []}
    for n in [int(x) for x in a.sizes.split(",")]:
        bases, offsets, n_amp = batch(amplicons(seq), n, a.share)
        with sa.KmerEngine(K, CHUNKS, 100) as eng:
            eng.ingest_reads(bases, offsets)
            eng.finalize()
            cnt = eng.counters()
            budget = sa.pcr_node_budget(cnt["n_bases_ingested"])
            calls = {
                "pcr_run": lambda: eng.pcr_run(genes, max_num_nodes=budget),
                "primer_kmers": lambda: eng.primer_kmers(primers),
                "pcr_run_depths": lambda: eng.pcr_run_depths(genes, depths, max_num_nodes=budget),
                "primer_kmers_depths": lambda: eng.primer_kmers_depths(primers, depths),
                "primer_kmers_one_depth_x10": lambda: [eng.primer_kmers_depths(primers, [d]) for d in depths],
            }
            sweep, single = calls["pcr_run_depths"](), calls["pcr_run"]()
            for o, w in zip(sweep[-1], single):  # the last depth is the merged table
                assert (o.status, o.products.sequences) == (w.status, w.products.sequences), f"the sweep and pcr_run disagree on {o.gene_name}"
            fused, apart = calls["primer_kmers_depths"](), calls["primer_kmers_one_depth_x10"]()
            for blk, (one,) in zip(fused, apart):
                assert all((x[0] == y[0]).all() and (x[1] == y[1]).all() for x, y in zip(blk, one)), "fused and per-depth scans disagree"
            row = {"reads": n, "amplicon_reads": n_amp, "bases": int(len(bases)), "table_capacity": cnt["table_capacity"],
                   "unique_kmers": cnt["n_unique_kmers"], "node_budget": budget,
                   "genes_succeeding_per_depth": [sum(o.status == sa.PCR_SUCCESS for o in blk) for blk in sweep]}
            t = alternating(calls, repeats)
            for v in t.values():
                v["range_ms"] = [min(v["samples_ms"]), max(v["samples_ms"])]
            row.update(t)
            D = len(depths)
            row["ratios"] = {
                "pcr_run_depths / (10 x pcr_run)": round(t["pcr_run_depths"]["median_ms"] / (D * t["pcr_run"]["median_ms"]), 3),
                "primer_kmers_depths / (10 x primer_kmers)": round(t["primer_kmers_depths"]["median_ms"] / (D * t["primer_kmers"]["median_ms"]), 3),
                "ten one-depth scans / (10 x primer_kmers)": round(t["primer_kmers_one_depth_x10"]["median_ms"] / (D * t["primer_kmers"]["median_ms"]), 3),
                "primer_kmers_depths / ten one-depth scans": round(t["primer_kmers_depths"]["median_ms"] / t["primer_kmers_one_depth_x10"]["median_ms"], 3),
            }
            f, s = t["primer_kmers_depths"]["range_ms"], t["primer_kmers_one_depth_x10"]["range_ms"]
            row["fused_beats_per_depth_beyond_spread"] = bool(f[1] < s[0])
            res["batches"].append(row)
            print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
