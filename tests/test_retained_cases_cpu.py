"""The retained reads without a GPU: the five entry points are declared, bound and exported; the cases of
tests/retained_cases.py hold what they say — checked against the oracle and the reference model alone, so that a case
cannot silently stop exercising what it is there for; and the store's loader and decode, compiled for the host, run
clean under AddressSanitizer and UBSan as a stand-alone program (tests/native/retain_driver.cpp; nothing is preloaded
and no sanitized code is loaded into the interpreter)."""
import ctypes
import os
import re
import subprocess

import pytest

import panel_cases as pc
import retained_cases as rc
import thread_panel_cases as tp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sharkmer_amd", "csrc")
T = rc.T
NEW = ["shk_retain_reads", "shk_retained_info", "shk_retained_export", "shk_filter_reads_panel_retained", "shk_thread_reads_panel_retained"]


# ---- the boundary ------------------------------------------------------------------------------------------------------------------
def test_the_five_entry_points_are_declared_bound_and_exported():
    import __graft_entry__ as g
    g.build()
    from sharkmer_amd.engine import ABI_SYMBOLS, lib_path
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "shk.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(shk_[a-z_0-9]+)\s*\(", src))
    L = ctypes.CDLL(lib_path())
    for name in NEW:
        assert name in declared, name
        assert name in ABI_SYMBOLS, name
        assert hasattr(L, name), name
    L.shk_abi_version.restype = ctypes.c_int
    assert L.shk_abi_version() == 2
    assert "#define SHK_N_KERNELS 16" in src and "#define SHK_ABI_VERSION 2" in src


# ---- the substituted cases -----------------------------------------------------------------------------------------------------------
def test_filter_cases_are_all_there_and_two_have_reads_substituted(orc):
    original, cases = pc.crafted_cases(orc), rc.filter_cases(orc)
    assert len(cases) == len(original) == 14
    changed = {}
    for o, c in zip(original, cases):
        assert (c.name, c.k, c.genes, len(c.reads)) == (o.name, o.k, o.genes, len(o.reads))
        assert all(rc.valid(r) for r in c.reads), c.name
        n = rc.substitute(o.reads)[1]
        assert [i for i, (a, b) in enumerate(zip(o.reads, c.reads)) if a != b] == [i for i, r in enumerate(o.reads) if not rc.valid(r)]
        if n:
            changed[c.name] = n
        # an empty read matches nothing, like the invalid one it stands for: the expected rows do not move
        assert pc.expected(orc, c) == pc.expected(orc, o), c.name
    assert len(changed) == 2 and changed["k=2"] == 1
    (other,) = [name for name in changed if name != "k=2"]
    assert other.startswith("k=21: an invalid byte") and changed[other] == 7


def test_thread_panels_are_all_there_with_the_stated_substitutions():
    panels = rc.thread_panels()
    originals = [tp.crafted_panel(), tp.lists_panel(), tp.many_panel()]
    assert [(len(o.reads), rc.substitute(o.reads)[1]) for o in originals] == [(46, 4), (10, 1), (155, 12)]
    assert len(panels) == 7 + len(tp.sweep_groups()) == 19
    for p in panels:
        assert all(rc.valid(r) for r in p.reads), p.name
    for o, p in zip(originals, panels):
        assert (p.name, p.lists, len(p.reads)) == (o.name, o.lists, len(o.reads))
        # … and supports nothing: every count of the model stays, gene by gene
        for a, b, g in zip(tp.expected(o), tp.expected(p), p.graphs):
            assert tp.rows(a, len(g.edges)) == tp.rows(b, len(g.edges)), p.name
    assert any(p.mate is not None for p in panels)
    for p in panels[:3]:
        rev, twice = rc.list_variants(p)[1:]
        assert [ids[::-1] for ids in rev.lists] == p.lists and all(len(t) == 2 * len(ids) for t, ids in zip(twice.lists, p.lists))


def test_splits_put_a_case_behind_every_kind_of_start_bit():
    reads = [b"ACGT", b"", b"AAC"]
    got = rc.splits(reads)
    assert [name for name, _, _ in got] == list(rc.SPLITS) and len(got) == 2 + len(rc.FILLERS)
    for (name, batches, n_front), f in zip(got[2:], rc.FILLERS):
        flat = rc.flat(batches)
        assert flat[n_front:] == reads and sum(len(r) for r in flat[:n_front]) == f, name
        assert all(rc.valid(r) for r in flat) and len(batches) >= 2
    assert got[0][1] == [reads] and got[1][1] == [[r] for r in reads]
    assert sorted(set(f % 64 for f in rc.FILLERS)) == [0, 1, 63] and any(f > 64 for f in rc.FILLERS) and any(f > 128 for f in rc.FILLERS)


# ---- the alignment cases ---------------------------------------------------------------------------------------------------------------
def test_alignment_cases_hold_what_they_claim(orc):
    cases = rc.alignment_cases(orc)
    assert sorted(set(c.k for c in cases)) == [3, 21, 31] and len(cases) == 3 * len(rc.FILLERS)
    assert sorted(set(c.filler for c in cases)) == sorted(rc.FILLERS)
    for c in cases:
        k, reads, at = c.k, rc.flat(c.batches), c.at
        rows = rc.align_expected(orc, c)
        assert all(rc.valid(r) for r in reads), c.name
        start = [0]
        for r in reads:
            start.append(start[-1] + len(r))
        # the fillers in front, in batches of their own; the first target starts at bit `filler`
        assert start[at["n_at_edge"]] == c.filler and sum(len(b) for b in c.batches[:-3]) == at["n_at_edge"], c.name
        # an N at bit 63 of a word and at bit 0 of the next
        S = reads[at["n_at_edge"]]
        n_bits = [c.filler + i for i, ch in enumerate(S) if ch == ord("N")]
        assert len(n_bits) == 2 and n_bits[0] % 64 == 63 and n_bits[1] == n_bits[0] + 1, (c.name, n_bits)
        behind = pc.hit_positions(orc, c.genes[6], S, k)  # the window just behind the two N hits, and the read's last
        assert {n_bits[1] + 1 - c.filler, len(S) - k} <= set(behind) and (k == 3 or len(behind) == 2), c.name
        assert at["n_at_edge"] in rows[6]
        # the target lengths: 0, k − 1, k, k + 1 bases; 64 bases; 64 windows; 2·64 + 1 windows
        want_len = {"empty_middle": 0, "len_k-1": k - 1, "len_k": k, "len_k+1": k + 1, "len_64": 64, "64_windows": 64 + k - 1, "R": 2 * T + k}
        for name, n in want_len.items():
            assert len(reads[at[name]]) == n, (c.name, name)
        assert at["len_k"] in rows[0] and at["len_k+1"] in rows[0] and at["len_k-1"] not in rows[0], c.name
        # the only hit at window 0, 63, 64, the last, and one that straddles two steps
        ws = sorted(int(name.split("_")[-1]) for name in at if name.startswith("only_hit_"))
        sw = rc.straddler(k)
        assert ws == sorted([0, T - 1, T, 2 * T, sw]) and sw // T != (sw + k - 1) // T and sw != T - 1, c.name
        for w in ws:
            r = reads[at[f"only_hit_{w}"]]
            assert len(r) - k + 1 == 2 * T + 1 and pc.hit_positions(orc, c.genes[0], r, k) == [w], (c.name, w)
            assert sum(1 for p in range(len(r) - k + 1) if b"N" not in r[p:p + k]) == 1
            assert at[f"only_hit_{w}"] in rows[0]
        assert at["no_hit"] not in rows[0] and len(reads[at["no_hit"]]) == 2 * T + k, c.name
        if k >= 21:  # a random read holds each of its windows once: gene 1 + j is window hits[j] of R alone
            for j, w in enumerate([0, T - 1, T, 2 * T, sw]):
                assert pc.hit_positions(orc, c.genes[1 + j], reads[at["R"]], k) == [w], (c.name, w)
                assert at["R"] in rows[1 + j] and at["R_rc"] in rows[1 + j]
        # a target that ends at the store's last word edge with nothing behind it: an empty read is last, one is in the middle
        assert at["empty_last"] == len(reads) - 1 and reads[-1] == b"" and c.batches[-1] == [b""] and c.batches[-2] == [reads[-2]]
        assert start[-1] % 64 == 0 and start[-1] == start[at["ends_at_edge"] + 1] and len(reads[at["ends_at_edge"]]) >= 64
        end = reads[at["ends_at_edge"]]
        assert pc.hit_positions(orc, c.genes[0], end, k)[-1:] == [len(end) - k] and at["ends_at_edge"] in rows[0], c.name
        assert 0 < at["empty_middle"] < len(reads) - 1 and rows[7] == [] and c.genes[7] == []
        assert not any(at["empty_middle"] in r or at["empty_last"] in r for r in rows)


def test_big_valid_batch_gives_every_wave_several_reads(orc):
    k, genes, reads, rows = rc.big_valid_batch(orc)
    assert len(reads) == pc.STRIDE_READS >= 4 * 8192 and all(rc.valid(r) for r in reads[:2000])
    assert len(set(reads)) == 9 and sum(len(r) for r in rows) > len(reads) // 2 and rows[1] == []
    # the rows are the oracle's: a sample of the reads, gene by gene
    sample = pc.expected(orc, pc.Case("sample", k, genes, reads[:300], []))
    assert sample == [[i for i in r if i < 300] for r in rows]


# ---- the loader and the decode under the sanitizers -----------------------------------------------------------------------------------
def test_retain_driver_clean_under_asan_ubsan():
    probe = subprocess.run(["g++", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    if not (os.path.isabs(probe) and os.path.exists(probe)):
        pytest.skip("no asan runtime in this toolchain")
    subprocess.check_call(["make", "-C", CSRC, "retain_driver"], stdout=subprocess.DEVNULL)
    env = dict(os.environ)
    env["ASAN_OPTIONS"] = "halt_on_error=1:abort_on_error=0:detect_leaks=1"
    env["UBSAN_OPTIONS"] = "halt_on_error=1:print_stacktrace=1"
    r = subprocess.run([os.path.join(CSRC, "retain_driver")], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    m = re.fullmatch(r"ok (\d+) (\d+)\n", r.stdout)
    assert m and int(m.group(1)) > 10_000 and int(m.group(2)) > 1_000_000, r.stdout
