"""GPU tests of sPCR's graph extension on a MULTI-DEVICE context made with SHK_FLAG_GROUP_GRAPH: the neighbourhood kernels
probe the share that owns each key through the share directory (k_nb_narrow_panel<true>, k_nb_wide<true>), and
shk_neighborhood[_panel], shk_pcr_extend[_panel], shk_pcr_run, shk_run_files_pcr and shk_count --group-graph answer what
one context holding the union of the shares answers.  The box has one card, so device ids repeat ([0, 0], [0] * 4,
[0] * 8): every share is a context of its own with its own arrays, stream and growth, on the same HBM.

Tables go in through `insert` (tests/nb_cases.py) or as reads; neighbourhoods are compared with tests/pcr_ref.py over the
merged inserts, panels and runs with a plain context on the same reads, array for array.  Each test has at most one
multi-device context open at a time."""
import ctypes
import gzip
import os
import random
import subprocess

import numpy as np
import pytest
import yaml

import sharkmer_amd as sa
import nb_cases
import pcr_panel_cases as pc
import pcr_ref as ref
import pcr_run_cases as cases
from lane_model import LaneModel
from sharkmer_amd.engine import lib_path
from test_gpu_nb_edges import Walk
from test_gpu_pcr_extend import assert_neighborhood
from test_gpu_pcr_extend_panel import same_graph
from test_gpu_pcr_run import same_outcomes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
EXE = os.path.join(ROOT, "sharkmer_amd", "csrc", "shk_count")
FILES = [os.path.join(G, "reads_main.fastq.gz"), os.path.join(G, "reads_part2.fastq")]
REFUSAL = "needs the whole table on one device: this is a multi-device context (n_devices > 1)"


@pytest.fixture(scope="module")
def key_owner():
    L = ctypes.CDLL(lib_path())
    L.shk_key_owner.restype = ctypes.c_uint32
    L.shk_key_owner.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint64]
    return L.shk_key_owner


def group_for(case, n_devices, hint=0, flags=0):
    eng = sa.KmerEngine(case.k, case.chunks, 10, capacity_hint=hint, flags=sa.FLAG_GROUP_GRAPH | flags, device_ids=[0] * n_devices)
    for lane, keys, counts in case.inserts:
        eng.insert(keys, counts, chunk_id=lane)
    return eng


_tables = {}


def case_and_table(name):
    """A crafted case and its merged table, built once for the three device counts."""
    if name not in _tables:
        case = nb_cases.CASES[name]()
        _tables[name] = (case, nb_cases.merged_table(case.inserts))
    return _tables[name]


# ---- 1. the hand-over sizes, neighbours on different shares at every step -----------------------------------------------

@pytest.mark.parametrize("n_devices", [2, 4, 8])
@pytest.mark.parametrize("name", ["flat1023", "flat1024", "flat1025", "zigzag", "rising"])
def test_hand_over_sizes_across_shares(name, n_devices, key_owner):
    """The cuts of test_gpu_nb_edges.py::test_levels_at_the_hand_over_sizes on tables split over 2, 4 and 8 shares: chains
    of random k-mers, so a k-mer's successor lives on another share more often than not; levels of 1023 to 1025 entries take
    the sharded narrow kernel, the wider ones (flat1025, zigzag, rising's last) the sharded wide one."""
    case, table = case_and_table(name)
    owners = {key_owner(case.k, 8, x) for x in table}
    assert owners == set(range(8)), owners  # keys on every share at D = 8 (and so at 2 and 4: their owners are prefixes)
    with group_for(case, n_devices) as eng:
        w = Walk(eng, case, table)
        assert w.sizes == case.sizes
        whole = w.check()
        assert whole[4] == len(case.sizes) and not whole[2] and len(whole[0]) == len(table)
        for f in (1023, 1024, 1025):
            w.check(fringe_cap=f)
        L = case.hand_over or 3
        for m in (L - 1, L, L + 1):
            w.check(max_levels=m)
            w.check(max_levels=m, fringe_cap=1024)
        for cap in (w.ksz[L], w.ksz[L] - 1, w.ksz[L + 1], w.ksz[L + 1] - 1):
            cut = w.check(cap=cap)
            assert cut[4] == (L + 1 if cap == w.ksz[L + 1] else L if cap >= w.ksz[L] else L - 1)
        assert w.resume(max_levels=2) == (len(case.sizes) + 1) // 2


# ---- 2. thresholds met only over lanes ----------------------------------------------------------------------------------

def test_threshold_met_only_over_lanes():
    """The sharded probe sums a share's lanes with saturation: nb_cases.lanes() on two shares."""
    lanes = nb_cases.lanes()
    table = nb_cases.merged_table(lanes[0].inserts)
    with group_for(lanes[0], 2) as eng:
        for case in lanes:
            w = Walk(eng, case, table)
            assert w.sizes == case.sizes, case.name
            whole = w.check()
            assert len(whole[0]) == sum(case.sizes[1:]) and not whole[2], case.name
            if case.min_count == nb_cases.U32_MAX:
                assert whole[1] == [nb_cases.U32_MAX] * 2
            if case.min_count == nb_cases.U32_MAX - 1:
                assert sorted(whole[1]) == [nb_cases.U32_MAX - 1, nb_cases.U32_MAX, nb_cases.U32_MAX]
            w.check(max_levels=2)
            w.check(cap=1)


# ---- 3. shares of different size: one share grows under the graph -------------------------------------------------------

def revcomp_np(x, k):
    y = np.zeros_like(x)
    for _ in range(k):
        y = (y << np.uint64(2)) | (np.uint64(3) - (x & np.uint64(3)))
        x = x >> np.uint64(2)
    return y


def test_one_share_grows_under_the_graph(key_owner):
    """A chain of 2000 k-mers over all four shares, then 200 000 more keys that shk_key_owner gives to share 1 alone: that
    share grows (other arrays, other log_pages) and the others do not, so the second call answers right only from a
    directory built anew.  (A share starts with at least 2^21 slots whatever the hint, which 200 000 keys spread over it
    never fill: the keys are taken from one sixteenth of share 1 — owner 16 of 64, sixteen of its pages, 131 072 slots —
    so that they cannot fit where they land and the share has to grow.)"""
    k, D = 15, 4
    rng = random.Random(1504)
    heads, kmers, counts, _, _ = nb_cases._chains(rng, k, [2001], ())
    chain = nb_cases.Case(k, 1, [(0, [nb_cases.canonical(x, k) for x in kmers], counts)], heads, [1], [], 1, "chain")
    assert {key_owner(k, D, x) for x in chain.inserts[0][1]} == set(range(D))
    # candidates: the key mix undone on values whose top six bits are 16 (one multiplication by the inverse mod 2^30)
    low = np.random.default_rng(1505).integers(0, 1 << (2 * k - 6), size=450_000, dtype=np.uint64)
    inv = np.uint64(pow(0xC2B2AE35, -1, 1 << (2 * k)))
    with np.errstate(over="ignore"):
        raw = ((np.uint64(16 << (2 * k - 6)) | low) * inv) & np.uint64((1 << (2 * k)) - 1)
    canon = np.unique(raw[raw <= revcomp_np(raw, k)])
    bulk = canon[:200_000]
    assert len(bulk) == 200_000
    assert all(key_owner(k, 64, x) == 16 and key_owner(k, D, x) == 1 for x in bulk.tolist())
    more = (0, bulk.tolist(), [1 + (i % 5) for i in range(len(bulk))])
    small, union = nb_cases.merged_table(chain.inserts), nb_cases.merged_table(chain.inserts + [more])
    a = dict(cap=4096, fringe_cap=4096)
    with group_for(chain, D, hint=1) as eng:
        before = eng.counters()["n_grows"]
        w = Walk(eng, chain, small)
        first = w.check(**a)
        assert len(first[0]) >= 1900 and not first[2]
        eng.insert(more[1], more[2], chunk_id=0)
        assert eng.counters()["n_grows"] > before and eng.counters()["n_grows"] > 0
        w2 = Walk(eng, chain, union)
        second = w2.check(**a)
        assert len(second[0]) >= len(first[0]) and set(first[0]) <= set(second[0])
        w2.check(max_levels=1000, **a)
        assert eng.lookup(bulk[:64], canonical=True).tolist() == more[2][:64]


# ---- 4. in the middle of a job -------------------------------------------------------------------------------------------

def node_of(bases, at, k):
    x = 0
    for c in bases[at:at + k - 1].tobytes():
        x = (x << 2) | b"ACGT".index(c)
    return x


def test_in_the_middle_of_a_job(orc):
    """ingest, neighbourhood, ingest, finalize, neighbourhood, reset, neighbourhood on two shares — every answer the merged
    view's of the lane model at that moment (which refuses a multi-device context only by the flagless rule)."""
    k, chunks, histo_max = 15, 2, 50
    bases, offsets = sa.synth_reads(sa.SynthSpec(genome_len=3000, read_len=100, sub_per_64k=0, n_per_64k=0, seed_genome=77), 0, 2400)
    cut = 1300  # (the second call starts inside a 1000-read block: lanes by the running index)
    seeds = [node_of(bases, int(offsets[i]), k) for i in (0, 5, 1700)]
    dirs = [3, 1, 2]
    args = dict(min_count=2, max_levels=40, cap=1 << 13, fringe_cap=1 << 13)
    model = LaneModel(orc, k, chunks, histo_max, multi_device=False)
    with sa.KmerEngine(k, chunks, histo_max, flags=sa.FLAG_GROUP_GRAPH, device_ids=[0, 0]) as eng:
        def compare(what):
            want = model.neighborhood(seeds, dirs, **args)
            assert_neighborhood(eng.neighborhood(seeds, dirs, **args), want, what)
            return want

        eng.ingest_reads(bases, offsets[:cut + 1])
        model.ingest_reads(bases, offsets[:cut + 1])
        one = compare("after the first ingest")
        eng.ingest_reads(bases, offsets[cut:])
        model.ingest_reads(bases, offsets[cut:])
        eng.finalize()
        model.finalize()
        assert np.array_equal(eng.histograms(), model.columns())
        two = compare("after finalize")
        assert len(one[0]) > 100 and len(two[0]) >= len(one[0]) and two[1] != one[1]
        assert np.array_equal(eng.histograms(), model.columns())
        eng.reset()
        model.reset()
        none = compare("after reset")
        assert none[0] == [] and none[4] == 1


# ---- 5, 6. a panel and a whole run: the plain context's arrays -------------------------------------------------------------

@pytest.fixture(scope="module")
def plain(orc):
    """The mixed panel's reads on a one-device context: its primer sets, graphs, launch counts and runs, computed once."""
    p = pc.mixed_panel(orc)
    genes = cases.mixed_genes(orc)
    n = len(p.offsets) - 1
    with sa.KmerEngine(p.k, 1, 100, flags=sa.FLAG_TIMING) as e:
        e.ingest_reads(p.bases, p.offsets)
        e.finalize()
        prim = e.primer_kmers([sa.Primer(s, **pc.PRIMER) for g in p.genes for s in (g.forward, g.reverse)])
        params = [g.params for g in p.genes]
        e.reset_timings()
        graphs = e.pcr_extend_panel(prim, params)
        alone = [e.pcr_extend(prim[2 * i], prim[2 * i + 1], **params[i]) for i in range(len(p.genes))]
        launches = e.timings()["extend"][1]
        runs = dict(none=e.pcr_run(genes, max_num_nodes=pc.MIXED_BUDGET),
                    host=e.pcr_run(genes, reads=(p.bases, p.offsets), max_num_nodes=pc.MIXED_BUDGET),
                    paired=e.pcr_run(genes, reads=(p.bases, p.offsets), paired=True, max_num_nodes=pc.MIXED_BUDGET))
    assert sum(g.found_path for g in graphs) >= 3 and n == pc.MIXED_READS
    return dict(p=p, genes=genes, prim=prim, params=params, graphs=graphs, alone=alone, launches=launches, runs=runs)


@pytest.mark.parametrize("n_devices", [2, 4])
def test_panel_equals_the_plain_context(plain, n_devices):
    p, prim, params = plain["p"], plain["prim"], plain["params"]
    with sa.KmerEngine(p.k, 1, 100, flags=sa.FLAG_GROUP_GRAPH | sa.FLAG_TIMING, device_ids=[0] * n_devices) as eng:
        eng.ingest_reads(p.bases, p.offsets)
        eng.finalize()
        mine = eng.primer_kmers([sa.Primer(s, **pc.PRIMER) for g in p.genes for s in (g.forward, g.reverse)])
        for a, b in zip(mine, prim):
            assert list(a[0]) == list(b[0]) and list(a[1]) == list(b[1])
        eng.reset_timings()
        graphs = eng.pcr_extend_panel(prim, params)
        alone = [eng.pcr_extend(prim[2 * i], prim[2 * i + 1], **params[i]) for i in range(len(p.genes))]
        launches = eng.timings()["extend"][1]
    assert len(graphs) == len(plain["graphs"])
    for i, g in enumerate(p.genes):
        assert same_graph(graphs[i], plain["graphs"][i]), g.name
        assert same_graph(alone[i], plain["alone"][i]), g.name
    # the k_nb_* launches (seed, narrow, wide, pack) of the same calls: not one more per share or per level
    assert launches == plain["launches"]


def test_pcr_run_equals_the_plain_context(plain):
    p, genes = plain["p"], plain["genes"]
    with sa.KmerEngine(p.k, 1, 100, flags=sa.FLAG_GROUP_GRAPH, device_ids=[0, 0]) as eng:
        eng.ingest_reads(p.bases, p.offsets)
        eng.finalize()
        got = dict(none=eng.pcr_run(genes, max_num_nodes=pc.MIXED_BUDGET),
                   host=eng.pcr_run(genes, reads=(p.bases, p.offsets), max_num_nodes=pc.MIXED_BUDGET),
                   paired=eng.pcr_run(genes, reads=(p.bases, p.offsets), paired=True, max_num_nodes=pc.MIXED_BUDGET))
        with pytest.raises(sa.ShkError) as err:
            eng.pcr_run(genes[:2], reads="retained")
        assert err.value.code == -11 and "reads are not retained" in err.value.msg
    for mode, want in plain["runs"].items():
        assert len(got[mode]) == len(want) == len(genes)
        same_outcomes(got[mode], want, mode)
        for x, y in zip(got[mode], want):
            assert (x.failure_reason, x.products.paths_found, x.products.generated) == (y.failure_reason, y.products.paths_found, y.products.generated)
    assert any(o.threaded for o in got["host"]) and any(o.threaded for o in got["paired"])
    assert {o.status for o in got["none"]} == {0, 1, 3, 4, 5}


# ---- 7. what the flag does not change --------------------------------------------------------------------------------------

def test_refusals_stay(plain):
    p, genes, prim = plain["p"], plain["genes"], plain["prim"]
    case, table = case_and_table("rising")
    # a flagged one-device context is an unflagged one
    with sa.KmerEngine(case.k, case.chunks, 10, flags=sa.FLAG_GROUP_GRAPH) as one:
        for lane, keys, counts in case.inserts:
            one.insert(keys, counts, chunk_id=lane)
        Walk(one, case, table).check()
    with sa.KmerEngine(p.k, 1, 100, flags=sa.FLAG_GROUP_GRAPH) as one:
        one.ingest_reads(p.bases, p.offsets)
        one.finalize()
        same_outcomes(one.pcr_run(genes, max_num_nodes=pc.MIXED_BUDGET), plain["runs"]["none"], "flagged one-device context")
        with pytest.raises(sa.ShkError) as err:
            one.pcr_run(genes[:2], reads="retained")
        assert err.value.code == -11 and "reads are not retained" in err.value.msg
    # a flagged owner share (the multi-process form) still refuses
    with sa.KmerEngine(p.k, 1, 100, flags=sa.FLAG_GROUP_GRAPH, n_owners=2, owner_id=1) as share:
        share.ingest_reads(p.bases, p.offsets)
        share.finalize()
        for call in (lambda: share.neighborhood([1], [1], 1), lambda: share.pcr_extend_panel(prim[:4], [dict(max_num_nodes=1000)] * 2),
                     lambda: share.pcr_extend(prim[0], prim[1], max_num_nodes=1000), lambda: share.pcr_run(genes[:2])):
            with pytest.raises(sa.ShkError) as err:
                call()
            assert err.value.code == -11 and "this context is an owner share (n_owners > 1)" in err.value.msg
    # and a multi-device context without the flag refuses as it did, text and code
    with sa.KmerEngine(p.k, 1, 100, device_ids=[0, 0]) as multi:
        multi.ingest_reads(p.bases, p.offsets)
        multi.finalize()
        for name, call in (("shk_neighborhood", lambda: multi.neighborhood([1], [1], 1)),
                           ("shk_neighborhood_panel", lambda: multi.neighborhood_panel([([1], [1], 1, 8, 8)])),
                           ("shk_pcr_extend", lambda: multi.pcr_extend(prim[0], prim[1], max_num_nodes=1000)),
                           ("shk_pcr_extend_panel", lambda: multi.pcr_extend_panel(prim[:4], [dict(max_num_nodes=1000)] * 2)),
                           ("shk_pcr_extend_panel", lambda: multi.pcr_run(genes[:2]))):
            with pytest.raises(sa.ShkError) as err:
                call()
            assert err.value.code == -11 and err.value.msg == name + " " + REFUSAL, err.value.msg


# ---- 8. the command line and run_files -------------------------------------------------------------------------------------

# two primer pairs cut from the genome the golden reads were drawn from (306 and 406 bases apart), one that is not there
SPECS = ["forward=GAAAAGGGTCGTTGAATAGTCATC,reverse=CACCCAACTTGTTGTTCGCCAGCA,name=a",
         "forward=TAAGCACTGGCGTCCTAGGGGTAA,reverse=TATTAAGGACCGTGCGAATGGTAG,name=b",
         f"forward={pc.ABSENT},reverse=TATTAAGGACCGTGCGAATGGTAG,name=absent"]


def run_cli(outdir, extra):
    cmd = [EXE, "-k", "21", "-s", "g", "-o", str(outdir), "--chunks", "3", "--histo-max", "50"]
    for s in SPECS:
        cmd += ["--pcr-primers", s]
    return subprocess.run(cmd + extra + FILES, capture_output=True, text=True)


def test_cli_over_two_shares_writes_the_one_device_files(tmp_path):
    one, two, three, py = (tmp_path / d for d in ("one", "two", "three", "py"))
    for d in (one, two, three, py):
        d.mkdir()
    r = run_cli(one, [])
    assert r.returncode == 0, r.stderr
    r = run_cli(two, ["--devices", "0,0", "--group-graph"])
    assert r.returncode == 0, r.stderr
    names = sorted(f.name for f in one.iterdir())
    assert names == sorted(f.name for f in two.iterdir()) and "g_a.fasta" in names and "g_b.fasta" in names and "g_absent.fasta" not in names
    for f in names:
        if f.endswith(".fasta") or f.endswith(".histo"):
            assert (one / f).read_bytes() == (two / f).read_bytes(), f
    assert (two / "g.histo").read_bytes() == open(os.path.join(G, "golden_k21_c3.histo"), "rb").read()
    ya, yb = yaml.safe_load((one / "g.stats.yaml").read_text()), yaml.safe_load((two / "g.stats.yaml").read_text())
    assert ya["pcr_results"] == yb["pcr_results"] and [x["status"] for x in yb["pcr_results"]] == ["success", "success", "fail"]
    for y in (ya, yb):
        y.pop("command"), y.pop("peak_memory_bytes")
    assert ya == yb
    text = lambda d: [l for l in (d / "g.stats.yaml").read_text().split("\n") if not l.startswith(("command:", "peak_memory_bytes:"))]
    assert text(one) == text(two)
    with gzip.open(FILES[0], "rt") as f:  # the amplicon lies in the reads' genome: its two ends are in some read
        reads = f.read()
    seq = "".join((two / "g_a.fasta").read_text().split("\n")[1:])
    assert len(seq) == 306 and seq[:40] in reads and seq[-40:] in reads
    # --read-threading: refused before a read is read, nothing written
    r = run_cli(three, ["--devices", "0,0", "--group-graph", "--read-threading"])
    assert r.returncode != 0 and "a multi-device context keeps no reads: --read-threading needs one device" in r.stderr
    assert not list(three.iterdir())
    # without --group-graph: the refusal as it was
    r = run_cli(three, ["--devices", "0,0"])
    assert r.returncode != 0 and "shk_pcr_extend_panel " + REFUSAL in r.stderr and not list(three.iterdir())
    # run_files: the same files through Python
    sa.run_files(FILES, k=21, chunks=3, sample="g", outdir=str(py), histo_max=50, device_ids=[0, 0], group_graph=True, pcr_primers=SPECS)
    for f in names:
        if f.endswith(".fasta") or f.endswith(".histo"):
            assert (py / f).read_bytes() == (one / f).read_bytes(), f
    with pytest.raises(sa.ShkError) as err:
        sa.run_files(FILES, k=21, chunks=3, sample="g", outdir=str(three), histo_max=50, device_ids=[0, 0], group_graph=True,
                     read_threading=True, pcr_primers=SPECS)
    assert err.value.code == -11 and "keeps no reads" in err.value.msg
