"""Primer seed discovery on MI355X: shk_primer_kmers (one pass, every primer direction and mismatch level) against
one single-oligo shk_find_oligos pass (the bandwidth floor) and against today's route (shk_find_oligos per direction
and level with host-listed variants, refused above 3000 oligos).

    python3 tools/primer_kmers_bench.py --table config2 --repeats 20 --out profiles/primer_kmers_config2.json
    python3 tools/primer_kmers_bench.py --table large  --repeats 10 --out profiles/primer_kmers_large.json

Tables: config2 = BASELINE configs[1] (1 M synthetic 150 bp reads of a 3 Mb genome, k 21); large = 20× that
(20 M reads of a 60 Mb genome).  Panels: the README's seven pairs (tests/golden/primer_panel_cnidaria.tsv) at
mismatches 2 and 3, and 100 directions cut from the genome.  Kernel times: HIP events around every launch
(SHK_FLAG_TIMING, slot "lookup"); call times: wall clock around the whole call after warm-up (host planning, the
launch, the copies back and the host selection).  Kernel times from rocprofv3 come from a separate run:
    rocprofv3 --kernel-trace --stats -d OUT -- python3 tools/primer_kmers_bench.py --table config2 --repeats 5
"""
import argparse
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import sharkmer_amd as sa  # noqa: E402
import primer_ref as ref  # noqa: E402

L_READ = 150
HBM_PEAK = 8.0e12


def readme_panel(**params):
    out = []
    for line in open(os.path.join(ROOT, "tests", "golden", "primer_panel_cnidaria.tsv")):
        if line.startswith("#") or not line.strip():
            continue
        name, fwd, rev = line.split()
        out += [(name + " fwd", sa.Primer(fwd, **params)), (name + " rev", sa.Primer(rev, **params))]
    return out


def genome_panel(spec, n, seed=11):
    rng = random.Random(seed)
    bases, offsets = sa.synth_reads(spec, 0, 400)
    out = []
    codes = {"A": "RWM", "C": "YSM", "G": "RSK", "T": "YWK"}
    while len(out) < n:
        r = rng.randrange(400)
        s = bases[r * L_READ:(r + 1) * L_READ].tobytes().decode()
        at = rng.randrange(0, L_READ - 24)
        p = list(s[at:at + rng.randint(17, 24)])
        for _ in range(rng.choice((0, 1, 2))):
            i = rng.randrange(len(p))
            p[i] = rng.choice(codes[p[i]]) if p[i] in codes else p[i]
        out.append((f"g{len(out)}", sa.Primer("".join(p))))
    return out


def build_table(name):
    genome, reads = (3_000_000, 1_000_000) if name == "config2" else (60_000_000, 20_000_000)
    spec = sa.SynthSpec(genome_len=genome, read_len=L_READ)
    eng = sa.KmerEngine(21, 1, 100, capacity_hint=genome, flags=sa.FLAG_TIMING)
    batch = 2_000_000 if reads > 2_000_000 else reads
    db = torch.empty(batch * L_READ, dtype=torch.uint8, device="cuda:0")
    do = torch.empty(batch + 1, dtype=torch.int64, device="cuda:0")
    for first in range(0, reads, batch):
        eng.synth_reads_device(spec, first, batch, db.data_ptr(), do.data_ptr())
        eng.sync()
        eng.ingest_reads_device(db.data_ptr(), do.data_ptr(), batch, batch * L_READ)
    eng.finalize()
    del db, do
    return eng, spec


def timed(eng, fn, repeats, warmup=2):
    for _ in range(warmup):
        fn()
    call, kern = [], []
    for _ in range(repeats):
        eng.reset_timings()
        t0 = time.perf_counter()
        fn()
        call.append((time.perf_counter() - t0) * 1e3)
        ms, launches = eng.timings().get("lookup", (0.0, 1))
        kern.append(ms / max(launches, 1))  # per table pass (find_oligos' binding makes two: count, then fetch)
    return call, kern


def summary(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4),
            "n": len(xs)}


def old_route(eng, panel, k, repeats):
    """Per direction and level: the variants listed on the host and one shk_find_oligos pass (≤ 3000 oligos)."""
    total, refused, passes = 0.0, [], 0
    for name, p in panel:
        P = ref.trim_primer(p.seq, p.trim, k)
        for m, lvl in enumerate(ref.levels_encoded(P, p.mismatches)):
            if len(lvl) > 3000:
                refused.append(f"{name} level {m}: {len(lvl)} oligos")
                continue
            call, _ = timed(eng, lambda: eng.find_oligos(lvl, len(P), p.min_count), max(1, repeats // 4), warmup=1)
            total += statistics.median(call)
            passes += 1
    return {"passes": passes, "sum_of_median_call_ms": round(total, 3), "refused": refused}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--table", choices=("config2", "large"), default="config2")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--no-old-route", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    t0 = time.perf_counter()
    eng, spec = build_table(a.table)
    cnt = eng.counters()
    slots = int(cnt["table_capacity"])
    table_bytes = slots * (8 + 4 * 1)
    res = {"table": a.table, "k": 21, "lanes": 1, "n_unique_kmers": int(cnt["n_unique_kmers"]), "slots": slots,
           "table_bytes": table_bytes, "build_s": round(time.perf_counter() - t0, 1),
           "device": torch.cuda.get_device_name(0)}
    # the floor: one single-oligo find_oligos pass
    one = np.array([ref.string_to_oligo("ACGTACGTACGTACG")], dtype=np.uint64)
    call, kern = timed(eng, lambda: eng.find_oligos(one, 15, 2), a.repeats)
    res["find_oligos_single"] = {"call_ms_two_passes": summary(call), "kernel_ms_per_pass": summary(kern),
                                 "hbm_fraction": round(table_bytes / (statistics.median(kern) * 1e-3) / HBM_PEAK, 3)}
    res_floor, res_call = kern, call
    panels = [("readme14_m2", readme_panel(mismatches=2)), ("readme14_m3", readme_panel(mismatches=3)),
              ("genome100_m2", genome_panel(spec, 100))]
    res["panels"] = {}
    for pname, panel in panels:
        primers = [p for _, p in panel]
        out = eng.primer_kmers(primers)
        call, kern = timed(eng, lambda: eng.primer_kmers(primers), a.repeats)
        km = statistics.median(kern)
        r = {"directions": len(primers), "call_ms": summary(call), "kernel_ms_per_pass": summary(kern),
             "host_side_ms_median": round(statistics.median(call) - km, 4),
             "table_bytes_per_kernel_s_TBps": round(table_bytes / (km * 1e-3) / 1e12, 3),
             "hbm_fraction": round(table_bytes / (km * 1e-3) / HBM_PEAK, 3),
             "kernel_over_single_find_oligos": round(km / statistics.median(res_floor), 3),
             "call_over_single_find_oligos_call": round(statistics.median(call) / (statistics.median(res_call) / 2), 3),
             "kmers_found": int(sum(len(o[0]) for o in out)),
             "hits_before_cap": int(sum(int(o[3].sum()) for o in out))}
        if not a.no_old_route:
            r["old_route"] = old_route(eng, panel, 21, a.repeats)
        res["panels"][pname] = r
    eng.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
