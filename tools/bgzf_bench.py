#!/usr/bin/env python
"""bgzip'd FASTQ, file → histograms, over the four routes that read every member:
  sequential    run_files(gzip_all_members=True): one thread, a member after the other — the yardstick
  host          run_files(bgzf="host"): BGZF members in batches on the reader's threads
  device        run_files(bgzf="device"): K_INFLATE, one wave per member; the text comes back to the host parser
  device_parse  run_files(bgzf="device", parse="device"): K_INFLATE, then CRC-32 and the FASTQ framing on the device
                (K_FASTQ); the text stays in device memory

Writes N synthetic reads of L bases as FASTQ, bgzips the text itself (level 6, 65280-byte members) once, outside the
timed part, checks that the four routes write the same histograms, then times them alternately: SAMPLES samples each
after one warm-up, median and range in Gbases/s.  For the device route also the kernel's own time and members per
second (hipEvents, shk_bgzf_device_totals) and the bytes moved each way; for the device_parse route the bytes moved
each way per run and the CRC-32 and framing kernels' time (shk_fastq_device_totals), and that it never gave up.
Beside the protocol (--alone N, default 10): each batched route N times in a row on its own, and the device_parse
route over batch budgets from 8 MiB to one batch for the whole file.

  python tools/bgzf_bench.py [--reads 1000000] [--length 150] [--samples 5] [--out profiles/bgzf_device_parse.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import struct
import sys
import tempfile
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sharkmer_amd as sa  # noqa: E402


def bgzf_member(payload: bytes, level: int = 6) -> bytes:
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9)
    body = c.compress(payload) + c.flush()
    head = struct.pack("<4BI2BH2BHH", 0x1F, 0x8B, 8, 4, 0, 0, 0xFF, 6, 66, 67, 2, len(body) + 25)
    return head + body + struct.pack("<II", zlib.crc32(payload), len(payload))


def write_inputs(path: str, n_reads: int, length: int, seed: int = 1):
    """A genome-like source (so that k-mers repeat), reads with substitutions and a few N's; returns (members, text bytes)."""
    rng = np.random.default_rng(seed)
    genome = rng.integers(0, 4, size=2_000_000, dtype=np.uint8)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    qual = np.frombuffer(bytes(range(35, 75)), dtype=np.uint8)
    n_members = n_text = 0
    pending = bytearray()
    with open(path, "wb") as f:
        for first in range(0, n_reads, 20000):
            m = min(20000, n_reads - first)
            starts = rng.integers(0, len(genome) - length, size=m)
            idx = starts[:, None] + np.arange(length)[None, :]
            codes = genome[idx]
            sub = rng.random((m, length)) < 0.01
            codes = np.where(sub, rng.integers(0, 4, size=(m, length), dtype=np.uint8), codes)
            seqs = acgt[codes]
            seqs[rng.random((m, length)) < 0.0005] = ord("N")
            quals = qual[rng.integers(0, len(qual), size=(m, length))]
            parts = []
            for i in range(m):
                parts.append(b"@SRR0000001.%d %d/1\n" % (first + i + 1, first + i + 1))
                parts.append(seqs[i].tobytes())
                parts.append(b"\n+\n")
                parts.append(quals[i].tobytes())
                parts.append(b"\n")
            pending += b"".join(parts)
            while len(pending) >= 65280:
                f.write(bgzf_member(bytes(pending[:65280])))
                del pending[:65280]
                n_members += 1
                n_text += 65280
        if pending:
            f.write(bgzf_member(bytes(pending)))
            n_members += 1
            n_text += len(pending)
        f.write(bgzf_member(b""))
        n_members += 1
    return n_members, n_text


def usable_cpus() -> int:
    """What the reader sizes its pools by: the affinity mask, or the container's CPU quota where that is smaller."""
    n = len(os.sched_getaffinity(0))
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = min(n, max(1, int(quota) // int(period)))
    except (OSError, ValueError):
        pass
    return n


def device_totals(L):
    v = [C.c_uint64(0) for _ in range(4)]
    L.shk_bgzf_device_totals(*[C.byref(x) for x in v])
    return [int(x.value) for x in v]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--length", type=int, default=150)
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--alone", type=int, default=10, help="runs in a row of each batched route on its own, after the protocol (0: none, and no batch sweep)")
    ap.add_argument("--k", type=int, default=21)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bgzf_device_parse.json"))
    a = ap.parse_args()
    L = sa.engine.load_library()
    routes = {"sequential": dict(gzip_all_members=True), "host": dict(bgzf="host"), "device": dict(bgzf="device"),
              "device_parse": dict(bgzf="device", parse="device")}
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "reads.fastq.gz")
        t0 = time.time()
        n_members, n_text = write_inputs(path, a.reads, a.length)
        print(f"wrote {a.reads} reads, {n_members} members, {os.path.getsize(path) / 1e6:.1f} MB of {n_text / 1e6:.1f} MB text in {time.time() - t0:.0f} s",
              flush=True)

        def run(route):
            out = os.path.join(tmp, route)
            os.makedirs(out, exist_ok=True)
            t = time.perf_counter()
            st = sa.run_files([path], k=a.k, chunks=2, sample="b", outdir=out, histo_max=1000, **routes[route])
            dt = time.perf_counter() - t
            st.pop("peak_memory_bytes", None)  # (the process's high-water mark: not a result)
            return dt, st, open(os.path.join(out, "b.histo"), "rb").read()

        # one warm-up each, and the histograms equal across the routes before anything is timed
        warm = {r: run(r) for r in routes}
        for r in routes:
            assert warm[r][2] == warm["sequential"][2] and warm[r][1] == warm["sequential"][1], f"{r}: not the sequential route's histograms"
        n_bases = warm["sequential"][1]["n_bases_read"]
        assert warm["sequential"][1]["n_reads_read"] == a.reads
        times = {r: [] for r in routes}
        assert sa.fastq_device_totals()["give_ups"] == 0, "the device_parse route gave up in its warm-up: that run was the device route's"
        dev0, fq0 = device_totals(L), sa.fastq_device_totals()
        for _ in range(a.samples):
            for r in routes:   # (alternating: drift of the machine lands on all of them alike)
                times[r].append(run(r)[0])
                print(f"  {r:10s} {n_bases / times[r][-1] / 1e9:.3f} Gbases/s", flush=True)
        dev1, fq1 = device_totals(L), sa.fastq_device_totals()
        # beside the protocol: each batched route on its own, --alone runs in a row (no other route in between) …
        alone = {}
        for r in ("host", "device", "device_parse"):
            run(r)
            alone[r] = [run(r)[0] for _ in range(a.alone)]
            print(f"  {r:12s} alone: median {statistics.median(alone[r]) * 1e3:.1f} ms", flush=True)
        # … and the device_parse route over batch budgets (SHK_BGZF_BATCH_KB; unset: the default of 128 MiB)
        sweep = {}
        for kb in (8192, 16384, 32768, 65536, 0, 1048576) if a.alone else ():
            if kb:
                os.environ["SHK_BGZF_BATCH_KB"] = str(kb)
            else:
                os.environ.pop("SHK_BGZF_BATCH_KB", None)
            run("device_parse")
            f0 = sa.fastq_device_totals()
            sweep[str(kb) if kb else "default"] = {"seconds": [run("device_parse")[0] for _ in range(5)],
                                                   "batches_per_run": (sa.fastq_device_totals()["batches"] - f0["batches"]) // 5}
        os.environ.pop("SHK_BGZF_BATCH_KB", None)
        assert sa.fastq_device_totals()["give_ups"] == 0
    members, kernel_ns, up, down = [b - a_ for a_, b in zip(dev0, dev1)]
    res = {"workload": {"reads": a.reads, "read_length": a.length, "k": a.k, "members": n_members, "text_bytes": n_text,
                        "bases": n_bases, "level": 6, "member_payload": 65280, "cpus": usable_cpus()},
           "routes": {}}
    for r in routes:
        g = sorted(n_bases / t / 1e9 for t in times[r])
        res["routes"][r] = {"gbases_per_s_median": statistics.median(g), "gbases_per_s_min": g[0], "gbases_per_s_max": g[-1],
                            "seconds": times[r]}
    res["device_kernel"] = {"members": members, "kernel_seconds": kernel_ns / 1e9,
                            "members_per_second": members / (kernel_ns / 1e9) if kernel_ns else None,
                            "text_gbytes_per_second": n_text * a.samples / kernel_ns if kernel_ns else None,
                            "bytes_up_per_run": up // max(a.samples, 1), "bytes_down_per_run": down // max(a.samples, 1)}
    fq = {f: fq1[f] - fq0[f] for f in fq1}
    assert fq["give_ups"] == 0 and fq["records"] == a.reads * a.samples, fq   # every record of every run framed on the device
    n = max(a.samples, 1)
    res["device_parse"] = {"batches_per_run": fq["batches"] // n, "records_per_run": fq["records"] // n, "give_ups": fq["give_ups"],
                           "bytes_up_per_run": fq["bytes_up"] // n, "bytes_down_per_run": fq["bytes_down"] // n,
                           "crc_and_framing_kernel_seconds_per_run": fq["kernel_ns"] / 1e9 / n}
    res["alone"] = {r: {"seconds": t, "seconds_median": statistics.median(t), "gbases_per_s_median": n_bases / statistics.median(t) / 1e9}
                    for r, t in alone.items() if t}
    res["device_parse_batch_kb_sweep"] = {kb: dict(v, seconds_median=statistics.median(v["seconds"])) for kb, v in sweep.items()}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res["routes"], indent=1))
    print(json.dumps(res["device_kernel"], indent=1))
    print(json.dumps(res["device_parse"], indent=1))


if __name__ == "__main__":
    main()
