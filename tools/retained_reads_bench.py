"""Retained reads on MI355X: what keeping a job's reads in HBM costs at ingest, and what sPCR's read pass gains when it
walks them where they lie (shk_retain_reads, shk_filter_reads_panel_retained, shk_thread_reads_panel_retained;
DESIGN.md §17).

    python3 tools/retained_reads_bench.py --out profiles/retained_reads.json

k 21, 10^5 and 10^6 synthetic 150-base reads, the 10-gene panel and the batches of tools/filter_panel_bench.py (gene 0's
amplicon is the 18S sequence, threaded through its pcr_extend graph; the other genes thread through the chain graphs of
their amplicons).  Per batch size, each pair measured ALTERNATING, one untimed call of each first, --repeats samples
each (default 5, at least 5), every sample kept and the median named:
    count_job_*          a config-2-like counting job — reset, the batch ingested from HBM, finalize — on a context
                         without retention and on one with it: the difference is k_retain's launch per batch; `store`
                         says what the retained reads add in device memory
    filter_device / filter_retained      filter_reads_panel(device=True) over the resident ASCII batch against
                                         filter_reads_retained over the store
    thread_device / thread_retained      thread_reads_panel(device=True) against thread_reads_retained, the filter's lists
    filter_host / thread_host            the host-batch forms, which pay the upload of the batch
    kernel_only          the four walks' launches alone, timed with HIP events inside the library (SHK_FLAG_TIMING): what the
                         calls above add around them is the copy of the offsets back to the host (8 bytes per read), their
                         check, the set's upload and the answer's way back
The routes' answers are compared before anything is timed.  --bench-parent / --bench-this take bench.py result lines
(files of JSON lines, one file per session) of the parent commit and of this one, run alternating within a session, into
the same file."""
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
from filter_panel_bench import K, amplicons, batch, graph_18s, panel  # noqa: E402


def chain_graph(amp: bytes):
    """The path graph of an amplicon: a node per (k−1)-mer in order, an edge per k-mer (repeats are not merged)."""
    code = {65: 0, 67: 1, 71: 2, 84: 3}
    n = len(amp) - (K - 1) + 1
    sub = np.zeros(n, dtype=np.uint64)
    for i in range(n):
        v = 0
        for ch in amp[i:i + K - 1]:
            v = (v << 2) | code[ch]
        sub[i] = v
    return sub, np.arange(n - 1, dtype=np.uint32), np.arange(1, n, dtype=np.uint32)


def alternating(calls: dict, repeats: int) -> dict:
    """One untimed call of each, then `repeats` rounds in which every call runs once, in turn → samples and medians (ms)."""
    for call in calls.values():
        call()
    out = {name: [] for name in calls}
    for _ in range(repeats):
        for name, call in calls.items():
            t0 = time.perf_counter()
            call()
            out[name].append(round((time.perf_counter() - t0) * 1e3, 3))
    return {name: {"samples_ms": s, "median_ms": statistics.median(s)} for name, s in out.items()}


def same(a, b) -> bool:
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def same_anns(a, b) -> bool:
    names = ("support_total", "support_unambiguous", "links", "link_counts", "read_edges")
    return len(a) == len(b) and all(np.array_equal(getattr(x, n), getattr(y, n)) for x, y in zip(a, b) for n in names)


def bench_lines(path):
    rows = []
    for line in open(path):
        line = line.strip()
        if line.startswith("{"):
            r = json.loads(line)
            rows.append({k: r[k] for k in ("metric", "value", "unit", "ms_per_step", "gbases_per_s") if k in r} or r)
    return rows


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--share", type=float, default=0.02)
    ap.add_argument("--sizes", default="100000,1000000")
    ap.add_argument("--bench-parent", nargs="*", default=[], help="bench.py result lines of the parent commit, a file per session")
    ap.add_argument("--bench-this", nargs="*", default=[], help="… of this commit, the same sessions in the same order")
    a = ap.parse_args()
    a.repeats = max(a.repeats, 5)
    seq, g = graph_18s()
    amps = amplicons(seq)
    graphs = [(g.node_sub_kmers, g.edge_src, g.edge_tgt)] + [chain_graph(x) for x in amps[1:]]
    res = {"k": K, "genes": len(amps), "amplicon_share": a.share, "graph_edges": [int(len(x[1])) for x in graphs],
           "sampling": f"wall-clock ms per call, the two routes of a pair alternating, one untimed call of each first, {a.repeats} samples "
                       "each, all kept, median named; every call returns with its answer on the host",
           "batches": []}
    if a.bench_parent and len(a.bench_parent) == len(a.bench_this):
        res["bench_py_default_path"] = {"what": "bench.py --gpus 1 --steps 100 --warmup 50 result lines, parent commit and this commit alternating "
                                                "within a session (retention off: the default path); every session kept",
                                        "sessions": [{"parent": bench_lines(p), "this": bench_lines(t)}
                                                     for p, t in zip(a.bench_parent, a.bench_this)]}
        for ses in res["bench_py_default_path"]["sessions"]:
            ses["parent_slowest"] = min(r["value"] for r in ses["parent"])
            ses["this_median"] = statistics.median(r["value"] for r in ses["this"])
    with sa.KmerEngine(K, 1, 100) as plain, sa.KmerEngine(K, 1, 100) as eng:
        eng.retain_reads()
        genes = panel(eng, amps)
        for n in [int(x) for x in a.sizes.split(",")]:
            bases, offsets, n_amp = batch(amps, n, a.share)
            db = torch.from_numpy(bases).to(eng._tdev)
            do = torch.from_numpy(offsets.astype(np.int64)).to(eng._tdev)
            torch.cuda.synchronize()

            def job(e):
                e.reset()
                e.ingest_reads_device(db.data_ptr(), do.data_ptr(), n, len(bases))
                e.finalize()

            row = {"reads": n, "amplicon_reads": n_amp, "bases": int(len(bases))}
            row.update({"count_job_" + name: v for name, v in alternating({"plain": lambda: job(plain), "retaining": lambda: job(eng)},
                                                                          a.repeats).items()})
            assert np.array_equal(plain.histograms(), eng.histograms()), "retention changed the histogram"
            info = eng.retained_info()
            assert (info["reads"], info["bases"]) == (n, len(bases))
            row["store"] = dict(info, bytes_per_base=round(info["device_bytes"] / len(bases), 4))
            # the routes agree before anything is timed
            lists = eng.filter_reads_retained(genes)
            assert same(lists, eng.filter_reads_panel(db, do, genes, device=True)) and same(lists, eng.filter_reads_panel(bases, offsets, genes))
            anns = eng.thread_reads_retained(graphs, lists)
            assert same_anns(anns, eng.thread_reads_panel(graphs, db, do, lists, device=True))
            assert same_anns(anns, eng.thread_reads_panel(graphs, bases, offsets, lists))
            rb, ro = eng.retained_reads(0, 1000)
            assert np.array_equal(rb, bases[:len(rb)]) and np.array_equal(ro, offsets[:1001])
            row["matches"] = int(sum(len(x) for x in lists))
            row["mapped_reads"] = int(sum(int((x.read_edges > 0).sum()) for x in anns))
            row.update(alternating({"filter_device": lambda: eng.filter_reads_panel(db, do, genes, device=True),
                                    "filter_retained": lambda: eng.filter_reads_retained(genes)}, a.repeats))
            row.update(alternating({"thread_device": lambda: eng.thread_reads_panel(graphs, db, do, lists, device=True),
                                    "thread_retained": lambda: eng.thread_reads_retained(graphs, lists)}, a.repeats))
            row.update(alternating({"filter_host": lambda: eng.filter_reads_panel(bases, offsets, genes),
                                    "thread_host": lambda: eng.thread_reads_panel(graphs, bases, offsets, lists)}, a.repeats))
            # the walks alone: HIP events around the launch inside the library (SHK_FLAG_TIMING), on a context of their own
            with sa.KmerEngine(K, 1, 100, flags=sa.FLAG_TIMING) as teng:
                teng.retain_reads()
                teng.ingest_reads_device(db.data_ptr(), do.data_ptr(), n, len(bases))

                def kernel_ms(call):
                    call()
                    out = []
                    for _ in range(a.repeats):
                        teng.reset_timings()
                        call()
                        teng.sync()
                        ms, launches = teng.timings()["lookup"]
                        assert launches == 1
                        out.append(round(ms, 4))
                    return {"samples_ms": out, "median_ms": statistics.median(out)}

                row["kernel_only"] = {"filter_device": kernel_ms(lambda: teng.filter_reads_panel(db, do, genes, device=True)),
                                      "filter_retained": kernel_ms(lambda: teng.filter_reads_retained(genes)),
                                      "thread_device": kernel_ms(lambda: teng.thread_reads_panel(graphs, db, do, lists, device=True)),
                                      "thread_retained": kernel_ms(lambda: teng.thread_reads_retained(graphs, lists))}
            res["batches"].append(row)
            print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
