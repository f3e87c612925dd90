"""sPCR read threading on MI355X: KmerEngine.thread_reads (shk_thread_reads) with the lookup set in LDS and in global
memory, and, on the same build and batch, shk_kmers_from_reads alone — the only device route to threading the
library had before, and a lower bound for it: that route copies every k-mer back and leaves lookup, run finding and
annotation to the host, none of which is counted here.

    python3 tools/thread_reads_bench.py --out profiles/thread_reads.json

Graph: pcr_extend on tests/golden/pcr_18s_padded.txt ×10 at k 21.  Batches: 10^5 and 10^6 synthetic 150-base reads of
which --share (default 0.1) are cut from the 18S sequence (both strands, every tenth with a substitution), the rest
from a 30 Mb synthetic genome.  Host buffers in, host arrays out; wall-clock per call on a warm context (one call made
before, so scratch is allocated); --repeats calls each (default 5), every sample kept and the median named."""
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


def batch(seq, n_reads, share):
    rng = np.random.default_rng(11)
    bases, offsets = sa.synth_reads(sa.SynthSpec(genome_len=30_000_000, sub_per_64k=300, n_per_64k=30), 0, n_reads)
    bases = bases.copy().reshape(n_reads, 150)
    amp = np.flatnonzero(rng.random(n_reads) < share)
    s = np.frombuffer(seq.encode(), dtype=np.uint8)
    rcs = np.frombuffer(seq.encode()[::-1].translate(COMP), dtype=np.uint8)
    at = rng.integers(0, len(seq) - 150 + 1, size=len(amp))
    for j, (r, a) in enumerate(zip(amp.tolist(), at.tolist())):
        row = (rcs if j & 1 else s)[a:a + 150].copy()
        if j % 10 == 0:
            row[75] = b"ACGT"[(b"ACGT".index(bytes([row[75]])) + 1) % 4] if row[75] in b"ACGT" else row[75]
        bases[r] = row
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
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--share", type=float, default=0.1)
    ap.add_argument("--sizes", default="100000,1000000")
    a = ap.parse_args()
    seq, g = graph_18s()
    res = {"k": K, "graph": {"nodes": len(g.node_sub_kmers), "edges": len(g.edge_src)}, "amplicon_share": a.share,
           "sampling": f"wall-clock ms per call, host buffers in and out, warm context, {a.repeats} calls each, all samples kept, median named",
           "batches": []}
    with sa.KmerEngine(K, 1, 100) as eng:
        for n in [int(x) for x in a.sizes.split(",")]:
            bases, offsets, n_amp = batch(seq, n, a.share)
            row = {"reads": n, "amplicon_reads": n_amp, "bases": int(len(bases))}
            for name, edges in (("lds", "1000000"), ("global", "0")):
                os.environ["SHK_THREAD_LDS_EDGES"] = edges
                row["thread_reads_" + name] = timed(lambda: eng.thread_reads(g, bases, offsets), a.repeats)
            os.environ.pop("SHK_THREAD_LDS_EDGES")
            ann = eng.thread_reads(g, bases, offsets)
            row["mapped_reads"] = int((ann.read_edges > 0).sum())
            row["edges_supported"] = int((ann.support_total > 0).sum())
            # the C call itself into preallocated arrays (KmerEngine.kmers_from_reads would add a Python slice per read)
            room = int(np.maximum(np.diff(offsets.astype(np.int64)) - K + 1, 0).sum())
            kmers, n_k, bad = np.empty(room, dtype=np.uint64), np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint8)
            row["kmers_from_reads_only"] = timed(lambda: eng._check(eng._L.shk_kmers_from_reads(
                eng._h, bases.ctypes.data, offsets.ctypes.data, n, kmers.ctypes.data, room, n_k.ctypes.data, bad.ctypes.data)),
                a.repeats)
            row["kmers_copied_back"] = room
            res["batches"].append(row)
            print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
