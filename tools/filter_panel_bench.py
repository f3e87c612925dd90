"""sPCR's read filter for a whole panel on MI355X: KmerEngine.filter_reads_panel (shk_filter_reads_panel) — host form and
device form, with the lookup set in LDS and in global memory — against the route a caller had before, one
shk_filter_reads call per gene over the same batch; and, for one gene, the chain filter → gather_reads →
thread_reads(device=True), in which the reads never leave the device.

    python3 tools/filter_panel_bench.py --out profiles/filter_panel.json

Panel: 10 genes of 60 k-mers each at k 21, cut from ten amplicons of 400 bases; gene 0's amplicon is the 18S sequence of
tests/golden/pcr_18s_padded.txt, whose pcr_extend graph is what the chain threads through.  Batches: 10^5 and 10^6
synthetic 150-base reads of which --share (default 0.02) are cut from the amplicons (both strands), the rest from a
30 Mb synthetic genome.  Wall-clock per call on a warm context (one call made before, so scratch is allocated);
--repeats calls each (default 5), every sample kept and the median named.  The answers of the routes are compared
before anything is timed."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

import numpy as np  # noqa: E402

import sharkmer_amd as sa  # noqa: E402

K = 21
N_GENES = 10
COMP = bytes.maketrans(b"ACGTN", b"TGCAN")


def graph_18s():
    seq = open(os.path.join(ROOT, "tests", "golden", "pcr_18s_padded.txt")).read().strip()
    bases = np.frombuffer(seq.encode() * 10, dtype=np.uint8).copy()
    offsets = np.arange(11, dtype=np.uint64) * np.uint64(len(seq))
    with sa.KmerEngine(K, 1, 100) as eng:
        eng.ingest_reads(bases, offsets)
        eng.finalize()
        fwd, rev = eng.primer_pair_kmers("AACCTGGTTGATCCTGCCAGT", "TGATCCTTCTGCAGGTTCACCTAC", trim=15, mismatches=2, min_count=3)
        return seq, eng.pcr_extend(fwd, rev, min_count=5, table_min_count=1, sweep=False, max_num_nodes=500_000)


def amplicons(seq):
    rng = np.random.default_rng(5)
    amps = [seq.encode()]
    for _ in range(N_GENES - 1):
        amps.append(bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=400)))
    return amps


def panel(eng, amps):
    """Per gene the canonical k-mers of the first and the last 50 windows of its amplicon's first 400 bases, 60 of them."""
    genes = []
    for a in amps:
        a = a[:400]
        kmers = np.concatenate([eng.kmers_from_ascii(a[:K + 49]), eng.kmers_from_ascii(a[-(K + 49):])])
        genes.append(np.unique(kmers)[:60])
    return genes


def batch(amps, n_reads, share):
    rng = np.random.default_rng(11)
    bases, offsets = sa.synth_reads(sa.SynthSpec(genome_len=30_000_000, sub_per_64k=300, n_per_64k=30), 0, n_reads)
    bases = bases.copy().reshape(n_reads, 150)
    amp = np.flatnonzero(rng.random(n_reads) < share)
    fw = [np.frombuffer(a, dtype=np.uint8) for a in amps]
    rv = [np.frombuffer(a[::-1].translate(COMP), dtype=np.uint8) for a in amps]
    for j, r in enumerate(amp.tolist()):
        s = (rv if j & 1 else fw)[j % len(amps)]
        at = int(rng.integers(0, len(s) - 150 + 1))
        bases[r] = s[at:at + 150]
    return bases.reshape(-1), offsets, len(amp)


def timed(call, repeats):
    call()  # warm
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        call()
        out.append(round((time.perf_counter() - t0) * 1e3, 3))
    return {"samples_ms": out, "median_ms": statistics.median(out)}


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--share", type=float, default=0.02)
    ap.add_argument("--sizes", default="100000,1000000")
    a = ap.parse_args()
    seq, g = graph_18s()
    amps = amplicons(seq)
    res = {"k": K, "genes": N_GENES, "amplicon_share": a.share, "graph": {"nodes": len(g.node_sub_kmers), "edges": len(g.edge_src)},
           "sampling": f"wall-clock ms per call, warm context, {a.repeats} calls each, all samples kept, median named; every call "
                       "returns with its answer on the host (the chain: with the annotation on the host)",
           "batches": []}
    with sa.KmerEngine(K, 1, 100) as eng:
        genes = panel(eng, amps)
        res["panel_kmers"] = int(sum(len(x) for x in genes))
        for n in [int(x) for x in a.sizes.split(",")]:
            bases, offsets, n_amp = batch(amps, n, a.share)
            db = torch.from_numpy(bases).to(eng._tdev)
            do = torch.from_numpy(offsets.astype(np.int64)).to(eng._tdev)
            torch.cuda.synchronize()
            # the routes agree before anything is timed
            want = [np.flatnonzero(eng.filter_reads(bases, offsets, x)).astype(np.uint64) for x in genes]
            for knob in ("0", None):
                os.environ.pop("SHK_FILTER_LDS_KEYS", None)
                if knob is not None:
                    os.environ["SHK_FILTER_LDS_KEYS"] = knob
                for got in (eng.filter_reads_panel(bases, offsets, genes), eng.filter_reads_panel(db, do, genes, device=True)):
                    assert all(np.array_equal(x, y) for x, y in zip(got, want)), "the panel call and the single calls disagree"
            row = {"reads": n, "amplicon_reads": n_amp, "bases": int(len(bases)), "matches": int(sum(len(x) for x in want)),
                   "matches_gene0": int(len(want[0]))}
            for name, knob in (("lds", None), ("global", "0")):
                os.environ.pop("SHK_FILTER_LDS_KEYS", None)
                if knob is not None:
                    os.environ["SHK_FILTER_LDS_KEYS"] = knob
                row["panel_host_" + name] = timed(lambda: eng.filter_reads_panel(bases, offsets, genes), a.repeats)
                row["panel_device_" + name] = timed(lambda: eng.filter_reads_panel(db, do, genes, device=True), a.repeats)
            os.environ.pop("SHK_FILTER_LDS_KEYS", None)
            row["single_calls_x%d" % N_GENES] = timed(lambda: [eng.filter_reads(bases, offsets, x) for x in genes], a.repeats)

            def chain():
                ids = eng.filter_reads_panel(db, do, genes[:1], device=True)[0]
                gb, go = eng.gather_reads(db, do, ids)
                return eng.thread_reads(g, gb, go, device=True)

            row["chain_filter_gather_thread_gene0"] = timed(chain, a.repeats)
            row["chain_mapped_reads"] = int((chain().read_edges > 0).sum())
            res["batches"].append(row)
            print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
