"""sPCR graph extension for a whole panel on MI355X: shk_pcr_extend_panel against the per-gene loop over shk_pcr_extend.

    python3 tools/pcr_extend_panel_bench.py --out profiles/pcr_extend_panel.json [--baseline-root DIR]
    python3 tools/pcr_extend_panel_bench.py --sizes 1,16 --repeats 9,5 --skip-big       (a part of it)

Panels (k 21, warm context): G = 1, 16, 64, 256 genes on a 1 Mb synthetic genome at 30× (error-free 150 bp reads), primer
pairs cut 300-1800 bases apart and found without mismatches, so that every graph is its amplicon — chains of the 18S shape,
under the sweep; and the five pairs of profiles/pcr_extend.json on the 30 Mb genome at 10×, where off-target seeds run
every gene to its node budget and wide levels occur.

Per panel: `loop` = one shk_pcr_extend call per gene; `panel` = one shk_pcr_extend_panel call, at SHK_PCR_PANEL_THREADS 1
and 8.  --baseline-root: a built checkout of the commit to compare against — the loop is then ALSO run in a child process
on that tree's library (`loop_baseline`), in the same session.  Every figure is wall-clock ms around a call that ends in a
device synchronise, `repeats` samples taken alternating loop / panel(1) / panel(8) after untimed calls of each:
min, median, max.  rounds / launches come from the library's SHK_PCR_PANEL_TRACE line, extend_ms / extend_launches
(SHK_K_EXTEND device time and timed launches) from a second context created with FLAG_TIMING, so that the event records
are not in the wall-clock figures."""
import argparse
import json
import os
import random
import re
import statistics
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 21
SIZES = (1, 16, 64, 256)


def rc_str(s):
    return s[::-1].translate(str.maketrans("ACGTN", "TGCAN"))


def stats(xs):
    return {"n": len(xs), "min": round(min(xs), 3), "median": round(statistics.median(xs), 3), "max": round(max(xs), 3)}


def build_engine(sa, genome, reads, flags=0):
    import torch
    spec = sa.SynthSpec(genome_len=genome)
    eng = sa.KmerEngine(K, 1, 100, capacity_hint=genome, flags=flags)
    batch = min(reads, 1_000_000)
    db = torch.empty(batch * 150, dtype=torch.uint8, device="cuda:0")
    do = torch.empty(batch + 1, dtype=torch.int64, device="cuda:0")
    for first in range(0, reads, batch):
        n = min(batch, reads - first)
        eng.synth_reads_device(spec, first, n, db.data_ptr(), do.data_ptr())
        eng.sync()
        eng.ingest_reads_device(db.data_ptr(), do.data_ptr(), n, n * 150)
    eng.finalize()
    del db, do
    return eng


def amplicon_panel(sa, eng, genome, n_genes):
    """n_genes primer pairs 300-1800 bases apart, each from its own error-free 2000-base stretch → primer_kmers' result."""
    long_, _ = sa.synth_reads(sa.SynthSpec(genome_len=genome, read_len=2000), 0, n_genes)
    rng = random.Random(14)
    primers = []
    for r in range(n_genes):
        s = long_[r * 2000:(r + 1) * 2000].tobytes().decode()
        a, d = rng.randrange(0, 150), rng.randrange(300, 1800)
        primers += [sa.Primer(s[a:a + 24], mismatches=0, min_count=2), sa.Primer(rc_str(s[a + d:a + d + 24]), mismatches=0, min_count=2)]
    return eng.primer_kmers(primers)


def offtarget_panel(sa, eng, genome, pairs=5):
    long_, _ = sa.synth_reads(sa.SynthSpec(genome_len=genome, read_len=1000), 0, pairs)
    rng = random.Random(3)
    primers = []
    for r in range(pairs):
        s = long_[r * 1000:(r + 1) * 1000].tobytes().decode()
        a, d = rng.randrange(0, 60), rng.randrange(300, 900)
        primers += [sa.Primer(s[a:a + 24], min_count=2), sa.Primer(rc_str(s[a + d:a + d + 24]), min_count=2)]
    return eng.primer_kmers(primers)


def run_loop(eng, prim, params):
    return [eng.pcr_extend(prim[2 * g], prim[2 * g + 1], **params) for g in range(len(prim) // 2)]


def traced_panel(eng, prim, params):
    """One panel call with the library's trace line read back → (rounds, launches)."""
    sys.stderr.flush()
    with tempfile.TemporaryFile() as tmp:
        keep = os.dup(2)
        os.dup2(tmp.fileno(), 2)
        os.environ["SHK_PCR_PANEL_TRACE"] = "1"
        try:
            eng.pcr_extend_panel(prim, params)
        finally:
            del os.environ["SHK_PCR_PANEL_TRACE"]
            os.dup2(keep, 2)
            os.close(keep)
        tmp.seek(0)
        m = re.search(rb"rounds (\d+) launches (\d+)", tmp.read())
    return (int(m.group(1)), int(m.group(2))) if m else (None, None)


def measure(eng, teng, prim, params, repeats, with_panel, time_loop_kernels=True):
    def timed(f):
        t0 = time.perf_counter()
        out = f()
        return (time.perf_counter() - t0) * 1e3, out

    def panel(threads):
        os.environ["SHK_PCR_PANEL_THREADS"] = str(threads)
        try:
            return eng.pcr_extend_panel(prim, params)
        finally:
            del os.environ["SHK_PCR_PANEL_THREADS"]

    res = {"genes": len(prim) // 2}
    # warm: code objects loaded, the loop's scratch allocated (it is sized per gene: a few genes warm it for all) …
    run_loop(eng, prim[:2 * min(len(prim) // 2, 4)], params)
    got = {}
    if with_panel:  # … and the panel's, which is sized by the whole panel
        for t in (1, 8):
            got[t] = panel(t)
    loop, p1, p8 = [], [], []
    for i in range(repeats):
        ms, want = timed(lambda: run_loop(eng, prim, params))
        loop.append(ms)
        if with_panel:
            p1.append(timed(lambda: panel(1))[0])
            p8.append(timed(lambda: panel(8))[0])
    res["nodes"] = [len(g.node_sub_kmers) for g in want][:16]
    res["steps_run"] = [g.steps_run for g in want][:16]
    res["found_path"] = sum(g.found_path for g in want)
    if with_panel:
        res["panel_equals_loop"] = all(len(x) == len(want) and all(
            (a.node_sub_kmers.tolist(), a.edge_src.tolist(), a.edge_counts.tolist(), a.steps_run) ==
            (b.node_sub_kmers.tolist(), b.edge_src.tolist(), b.edge_counts.tolist(), b.steps_run) for a, b in zip(x, want))
            for x in got.values())
    res["loop_ms"] = stats(loop)
    if with_panel:
        res["panel_ms_threads_1"], res["panel_ms_threads_8"] = stats(p1), stats(p8)
        res["rounds"], res["launches"] = traced_panel(eng, prim, params)
        teng.pcr_extend_panel(prim, params)
        teng.sync()
        teng.reset_timings()
        teng.pcr_extend_panel(prim, params)
        teng.sync()
        ms, n = teng.timings().get("extend", (0.0, 0))
        res["panel_extend_ms"], res["panel_extend_launches"] = round(ms, 3), n
        if time_loop_kernels:
            teng.reset_timings()
            run_loop(teng, prim, params)
            teng.sync()
            ms, n = teng.timings().get("extend", (0.0, 0))
            res["loop_extend_ms"], res["loop_extend_launches"] = round(ms, 3), n
    return res


def run(root, repeats, big_repeats, with_panel, sizes, skip_big):
    sys.path[:0] = [root]
    import sharkmer_amd as sa
    from sharkmer_amd.engine import FLAG_TIMING
    res = {"k": K, "root": os.path.basename(os.path.abspath(root)), "amplicons_1Mb_30x": {}}
    if sizes:
        genome, reads = 1_000_000, 200_000
        eng = build_engine(sa, genome, reads)
        teng = build_engine(sa, genome, reads, FLAG_TIMING) if with_panel else None
        params = dict(min_count=2, table_min_count=2, sweep=True, max_num_nodes=sa.pcr_node_budget(reads * 150))
        prim = amplicon_panel(sa, eng, genome, max(sizes))
        for g, n in zip(sizes, repeats):
            res["amplicons_1Mb_30x"][str(g)] = measure(eng, teng, prim[:2 * g], params, n, with_panel, time_loop_kernels=g < 256)
            print(g, json.dumps(res["amplicons_1Mb_30x"][str(g)]), flush=True)
        eng.close()
        if teng:
            teng.close()
    if not skip_big:
        genome, reads = 30_000_000, 2_000_000
        eng = build_engine(sa, genome, reads)
        teng = build_engine(sa, genome, reads, FLAG_TIMING) if with_panel else None
        params = dict(min_count=2, table_min_count=1, sweep=False, max_num_nodes=sa.pcr_node_budget(reads * 150))
        prim = offtarget_panel(sa, eng, genome)
        res["offtarget_30Mb_10x"] = measure(eng, teng, prim, params, big_repeats, with_panel)
        print("30Mb", json.dumps(res["offtarget_30Mb_10x"]), flush=True)
        eng.close()
        if teng:
            teng.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--sizes", default="1,16,64,256", help="genes per amplicon panel ('' = none)")
    ap.add_argument("--repeats", default="9,5,3,3", help="samples per size (the loop over 256 genes takes over a minute)")
    ap.add_argument("--big-repeats", type=int, default=3)
    ap.add_argument("--skip-big", action="store_true")
    ap.add_argument("--baseline-root", default="", help="a built checkout of the commit to compare the loop against")
    ap.add_argument("--loop-only-root", default="", help=argparse.SUPPRESS)  # the child's mode: the loop on that tree
    a = ap.parse_args()
    sizes = [int(x) for x in a.sizes.split(",") if x]
    repeats = [int(x) for x in a.repeats.split(",") if x][:len(sizes)]
    if len(repeats) != len(sizes):
        ap.error("--repeats takes one figure per size")
    if a.loop_only_root:
        print("RESULT " + json.dumps(run(a.loop_only_root, repeats, a.big_repeats, False, sizes, a.skip_big)))
        return
    res = run(HERE, repeats, a.big_repeats, True, sizes, a.skip_big)
    if a.baseline_root:
        cmd = [sys.executable, os.path.abspath(__file__), "--loop-only-root", a.baseline_root, "--sizes", a.sizes, "--repeats",
               a.repeats, "--big-repeats", str(a.big_repeats)] + (["--skip-big"] if a.skip_big else [])
        out = subprocess.run(cmd, stdout=subprocess.PIPE, check=True, timeout=1100).stdout.decode()
        base = json.loads([ln for ln in out.splitlines() if ln.startswith("RESULT ")][-1][7:])
        for g, m in base["amplicons_1Mb_30x"].items():
            res["amplicons_1Mb_30x"][g]["loop_baseline_ms"] = m["loop_ms"]
        if "offtarget_30Mb_10x" in base:
            res["offtarget_30Mb_10x"]["loop_baseline_ms"] = base["offtarget_30Mb_10x"]["loop_ms"]
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
