"""The BGZF batch planner (bgzf_plan_batch, bgzf_jobs_inside, bgzf_batch_budget in sharkmer_amd/csrc/shk_inflate.cpp) under
AddressSanitizer and UBSan: the stand-alone program of tests/native/fastq_text_driver.cpp (runtimes linked statically,
nothing preloaded) plans every clean file of tests/bgzf_cases.py batch after batch under budgets of 1 KiB, 3 KiB, 64 KiB and
0, and what it prints is held against the members this file reads off the bytes itself: BSIZE from the header's BC
subfield, ISIZE from the trailer (CPU only)."""
import os
import struct
import subprocess

import pytest

import bgzf_cases as bc

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "sharkmer_amd", "csrc")
BUDGETS = (1 << 10, 3 << 10, 64 << 10, 0)


@pytest.fixture(scope="module")
def driver():
    r = subprocess.run(["make", "-C", CSRC, "fastq_text_driver"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return os.path.join(CSRC, "fastq_text_driver")


def members(data: bytes, n: int) -> list:
    """(offset, size, isize) of the first n members of a file of bgzf_cases' writer (18-byte headers)."""
    ms, at = [], 0
    for _ in range(n):
        size = struct.unpack_from("<H", data, at + 16)[0] + 1
        ms.append((at, size, struct.unpack_from("<I", data, at + size - 4)[0]))
        at += size
    return ms


def plan(driver, tmp_path, data: bytes) -> dict:
    """budget → (batches, where it stopped or None at the file's end); a batch: (n, out_bytes, begin, end, first, last)."""
    path = os.path.join(tmp_path, "file.gz")
    open(path, "wb").write(data)
    r = subprocess.run([driver, "plan", path] + [str(b) for b in BUDGETS], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    out, cur = {}, None
    for line in r.stdout.splitlines():
        w = line.split()
        if w[0] == "budget":
            cur = int(w[1])
            out[cur] = [[], "open"]
        elif w[0] == "batch":
            v = [int(x) for x in w[1:]]
            out[cur][0].append((v[0], v[1], v[2], v[3], tuple(v[4:8]), tuple(v[8:12])))
        else:
            assert out[cur][1] == "open"
            out[cur][1] = int(w[1]) if w[0] == "stop" else None
    assert sorted(out) == sorted(BUDGETS) and all(v[1] != "open" for v in out.values())
    return out


def check_batches(ms: list, batches: list, budget: int, what):
    """The batches tile ms in order; the jobs are the members' bodies and the running ISIZE sum; the budget holds."""
    k = 0
    for n, out_bytes, begin, end, first, last in batches:
        assert n >= 1 and k + n <= len(ms), what
        mine = ms[k:k + n]
        assert begin == mine[0][0] and end == mine[-1][0] + mine[-1][1], what
        assert out_bytes == sum(m[2] for m in mine), what
        assert out_bytes <= budget or n == 1, (what, n, out_bytes)
        # a batch ends where the next member would not fit (or where the members do)
        assert k + n == len(ms) or out_bytes + ms[k + n][2] > budget, what
        for job, i in ((first, 0), (last, n - 1)):
            off, size, isize = mine[i]
            assert job == (off - begin + 18, sum(m[2] for m in mine[:i]), size - 26, isize), (what, i)
        k += n
    assert k == len(ms), what


def test_batches_tile_every_clean_file(driver, tmp_path):
    n_batches = 0
    for name, (data, n_members, _env, _text) in bc.clean_cases().items():
        ms = members(data, n_members)
        assert ms[-1][0] + ms[-1][1] == len(data), name
        for budget, (batches, stop) in plan(driver, tmp_path, data).items():
            assert stop is None, (name, budget)
            check_batches(ms, batches, budget, (name, budget))
            n_batches += len(batches)
    assert n_batches > 1000


def test_planning_stops_at_the_first_member_that_is_not_batchable(driver, tmp_path):
    ms = bc.bgzf(bc.SMALL, 3000)
    damaged = bc.damaged_cases()
    big = ms[9][:-4] + struct.pack("<I", 65537)
    cases = {"plain gzip member": damaged["plain_gzip_in_the_middle@10"], "cut by the file's end": damaged["cut_in_body@9"],
             "cut inside the trailer": damaged["cut_in_trailer@18"], "ISIZE 65537": (b"".join(ms[:9] + [big] + ms[10:]), 9),
             "plain gzip member first": (bc.plain_gzip_member(bc.SMALL), 0)}
    for name, (data, at) in cases.items():
        good = members(data, at)
        stop_at = good[-1][0] + good[-1][1] if good else 0
        for budget, (batches, stop) in plan(driver, tmp_path, data).items():
            assert stop == stop_at, (name, budget)
            check_batches(good, batches, budget, (name, budget))


def test_jobs_inside_is_overflow_safe(driver):
    r = subprocess.run([driver, "inside"], capture_output=True, text=True)
    assert r.returncode == 0 and "inside ok" in r.stdout, r.stdout + r.stderr
    assert "runtime error" not in r.stderr


def test_the_batch_budget_hook(driver):
    def budget(default, kb=None):
        env = {k: v for k, v in os.environ.items() if k != "SHK_BGZF_BATCH_KB"}
        if kb is not None:
            env["SHK_BGZF_BATCH_KB"] = kb
        return int(subprocess.run([driver, "budget", str(default)], capture_output=True, text=True, env=env, check=True).stdout)

    assert budget(64 << 20) == 64 << 20 and budget(128 << 20) == 128 << 20
    assert budget(64 << 20, "3") == 3 << 10 and budget(1, "6000") == 6000 << 10
    assert budget(64 << 20, "0") == 1 << 10 and budget(64 << 20, "junk") == 1 << 10   # (KiB, at least 1)
