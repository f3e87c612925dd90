"""sPCR graph extension on MI355X: shk_pcr_extend against the route the library offered before it — the same
breadth-first fetch with one KmerEngine.lookup call per level — and against shk_neighborhood alone.

    python3 tools/pcr_extend_bench.py --out profiles/pcr_extend.json
    rocprofv3 --kernel-trace --stats -d OUT -- python3 tools/pcr_extend_bench.py --case 18s

Cases: 18s = the reference's integration case (tests/golden/pcr_18s_padded.txt ×10, k 21, a chain about 1800 levels
deep); synth = a 30 Mb synthetic genome at 10× (2 M error-free 150 bp reads, k 21) with five primer pairs cut 300-900
bases apart.  Every figure is one wall-clock call on a warm context (the call made once before, so that scratch is
allocated), in ms.  per_level_lookup: `fetch_ms` is the whole host loop (numpy candidate generation, the call, the
visited set), `lookup_ms` the part spent inside KmerEngine.lookup — the floor of that route whatever drives it.  The
replay that would follow it is not timed (pcr_extend's own replay is included in pcr_extend_ms)."""
import argparse
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402

import sharkmer_amd as sa  # noqa: E402

K = 21
MASK = np.uint64((1 << (2 * (K - 1))) - 1)


def rc_str(s):
    return s[::-1].translate(str.maketrans("ACGTN", "TGCAN"))


def per_level_lookup(eng, nodes, dirs, min_count):
    """The neighbourhood of the seeds, one lookup call per level → (k-mers found, levels, ms inside lookup)."""
    ent = set()
    for n, d in zip(nodes, dirs):
        ent.update((int(n) << 1) | b for b in (0, 1) if d >> b & 1)
    level = np.array(sorted(ent), dtype=np.uint64)
    seen, found, levels, t_lookup = set(level.tolist()), set(), 0, 0.0
    b4 = np.arange(4, dtype=np.uint64)
    while len(level):
        node, d = level >> np.uint64(1), level & np.uint64(1)
        fwd = (node[:, None] << np.uint64(2)) | b4[None, :]
        rev = (b4[None, :] << np.uint64(2 * (K - 1))) | node[:, None]
        x = np.where(d[:, None] == 0, fwd, rev).reshape(-1)
        t0 = time.perf_counter()
        c = eng.lookup(x, canonical=True)
        t_lookup += time.perf_counter() - t0
        ok = c >= min_count
        xs, ds = x[ok], np.repeat(d, 4)[ok]
        found.update(xs.tolist())
        succ = (np.where(ds == 0, xs & MASK, xs >> np.uint64(2)) << np.uint64(1)) | ds
        nxt = [s for s in np.unique(succ).tolist() if s not in seen]
        seen.update(nxt)
        level = np.array(nxt, dtype=np.uint64)
        levels += 1
    return len(found), levels, t_lookup * 1e3


def measure(eng, fwd, rev, min_count, budget):
    def once():
        t0 = time.perf_counter()
        g = eng.pcr_extend(fwd, rev, min_count=min_count, table_min_count=1, sweep=False, max_num_nodes=budget)
        t1 = time.perf_counter()
        seeds = g.node_sub_kmers[g.node_flags != 0]
        sd = g.node_flags[g.node_flags != 0]
        t2 = time.perf_counter()
        nb = eng.neighborhood(seeds, sd, min_count, cap=1 << 20, fringe_cap=1 << 18)
        t3 = time.perf_counter()
        nf, lv, tl = per_level_lookup(eng, seeds, sd, min_count)
        t4 = time.perf_counter()
        return {"pcr_extend_ms": round((t1 - t0) * 1e3, 3), "nodes": len(g.node_sub_kmers), "edges": len(g.edge_src),
                "found_path": g.found_path, "neighborhood_ms": round((t3 - t2) * 1e3, 3), "neighborhood_kmers": len(nb[0]),
                "levels": nb[4], "complete": len(nb[2]) == 0,
                "per_level_lookup": {"fetch_ms": round((t4 - t3) * 1e3, 3), "lookup_ms": round(tl, 3), "levels": lv,
                                     "kmers": nf}}
    once()  # warm: scratch allocated, code objects loaded
    return once()


def case_18s():
    seq = open(os.path.join(ROOT, "tests", "golden", "pcr_18s_padded.txt")).read().strip()
    bases = np.frombuffer(seq.encode() * 10, dtype=np.uint8).copy()
    offsets = np.arange(11, dtype=np.uint64) * np.uint64(len(seq))
    with sa.KmerEngine(K, 1, 100) as eng:
        eng.ingest_reads(bases, offsets)
        eng.finalize()
        fwd, rev = eng.primer_pair_kmers("AACCTGGTTGATCCTGCCAGT", "TGATCCTTCTGCAGGTTCACCTAC", min_count=3)
        return measure(eng, fwd, rev, 5, 500_000)


def case_synth(genome=30_000_000, reads=2_000_000, pairs=5):
    import torch
    spec = sa.SynthSpec(genome_len=genome)
    out = []
    with sa.KmerEngine(K, 1, 100, capacity_hint=genome) as eng:
        batch = 1_000_000
        db = torch.empty(batch * 150, dtype=torch.uint8, device="cuda:0")
        do = torch.empty(batch + 1, dtype=torch.int64, device="cuda:0")
        for first in range(0, reads, batch):
            eng.synth_reads_device(spec, first, batch, db.data_ptr(), do.data_ptr())
            eng.sync()
            eng.ingest_reads_device(db.data_ptr(), do.data_ptr(), batch, batch * 150)
        eng.finalize()
        del db, do
        long_, _ = sa.synth_reads(sa.SynthSpec(genome_len=genome, read_len=1000), 0, pairs)
        rng = random.Random(3)
        for r in range(pairs):
            s = long_[r * 1000:(r + 1) * 1000].tobytes().decode()
            a, d = rng.randrange(0, 60), rng.randrange(300, 900)
            fwd, rev = eng.primer_pair_kmers(s[a:a + 24], rc_str(s[a + d:a + d + 24]), min_count=2)
            m = measure(eng, fwd, rev, 2, sa.pcr_node_budget(reads * 150))
            m["primer_distance"] = d
            out.append(m)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=("18s", "synth", "both"), default="both")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    res = {"k": K}
    if a.case in ("18s", "both"):
        res["18s"] = case_18s()
    if a.case in ("synth", "both"):
        res["synth_30Mb_10x"] = case_synth()
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
