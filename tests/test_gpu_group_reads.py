"""GPU tests of retained reads and sPCR's read pass on a MULTI-DEVICE context made with SHK_FLAG_GROUP_READS (DESIGN.md
§22): every share keeps the runs of reads the exchange rounds deal it, walks its own store (k_retain, k_retained_export,
k_filter_panel_retained, k_thread_panel_retained as they are) and the host stitches the answers by the run directory.

The box has one card, so device ids repeat ([0, 0], [0] * 4).  Every answer is compared with a one-device context with
retention fed the same calls, and where tests/ has a model (panel_cases, retained_cases, thread_panel_cases) with that
too.  SHK_GROUP_ROUND_KB=1: a round deals at most 1 KiB per share, so a few dozen reads span several rounds."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest
import yaml

import sharkmer_amd as sa
import panel_cases as pc
import pcr_panel_cases as ppc
import pcr_run_cases as cases
import retained_cases as rc
from sharkmer_amd.engine import _ThreadPanelOut
from test_gpu_pcr_run import same_outcomes
from test_gpu_retained_reads import got_rows, retained, want_rows
from test_gpu_thread_reads import graph_arrays

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
EXE = os.path.join(ROOT, "sharkmer_amd", "csrc", "shk_count")
FILES = [os.path.join(G, "reads_main.fastq.gz"), os.path.join(G, "reads_part2.fastq")]
BOTH = sa.FLAG_GROUP_GRAPH | sa.FLAG_GROUP_READS
NOT_HERE = "not available on a multi-device context"


@pytest.fixture(autouse=True)
def _small_rounds(monkeypatch):
    monkeypatch.setenv("SHK_GROUP_ROUND_KB", "1")


def group(k, n_devices, chunks=1, hint=None, flags=BOTH):
    eng = sa.KmerEngine(k, chunks, 100, flags=flags, device_ids=[0] * n_devices)
    eng.retain_reads(**({} if hint is None else dict(capacity_bases=hint)))
    return eng


def plain(k, chunks=1):
    eng = sa.KmerEngine(k, chunks, 100)
    eng.retain_reads()
    return eng


class Twin:
    """A one-device context and a flagged group given the same calls."""

    def __init__(self, k, n_devices, chunks=1, hint=None):
        self.one, self.grp = plain(k, chunks), group(k, n_devices, chunks, hint)

    def close(self):
        self.one.close()
        self.grp.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def both(self, f):
        return f(self.one), f(self.grp)

    def ingest(self, reads, lane=None):
        for e in (self.one, self.grp):
            b, o = e._pack(reads)
            e.ingest_reads(b, o) if lane is None else e.ingest_batch(lane, b, o)

    def same_store(self, reads=None):
        a, b = self.both(retained)
        assert a == b and (reads is None or a == list(reads))
        ia, ib = self.both(lambda e: e.retained_info())
        assert (ia["reads"], ia["bases"]) == (ib["reads"], ib["bases"])
        return a


def canon(kmer: bytes) -> int:
    import thread_cases as tc
    return min(tc.enc(kmer.decode()), tc.enc(pc.rc_bytes(kmer).decode()))


def rand_reads(rng, n, lo=80, hi=300):
    return [bytes(rng.choice(b"ACGT") for _ in range(rng.randint(lo, hi))) for _ in range(n)]


# ---- 1. the store: round trip, ordinals, growth, reset, the switch ----------------------------------------------------------

@pytest.mark.parametrize("n_devices", [2, 4])
def test_round_trip_over_every_range_and_call_kind(n_devices):
    rng = random.Random(11 + n_devices)
    reads = rand_reads(rng, 40)
    reads[3], reads[17], reads[18] = b"", b"ACGTN", b"N" * 70  # an empty read, reads shorter than k
    with Twin(21, n_devices, chunks=3, hint=64) as t:  # (a hint of 64 bases: every call grows some store)
        t.ingest(reads[:2])                # fewer reads than shares (of four)
        t.same_store(reads[:2])
        t.ingest(reads[2:3])               # a batch of one read: the other shares' runs are empty
        t.grp.set_read_index(5000), t.one.set_read_index(5000)  # moves the striping, not the ordinals
        t.ingest(reads[3:20])
        t.ingest(reads[20:29], lane=2)     # an explicit lane between two striped calls
        t.ingest(reads[29:])
        t.same_store(reads)
        n = len(reads)
        for first in range(n + 1):         # every range start, lengths 0, 1, 2, a few rounds' worth and the rest
            for cnt in {0, 1, 2, 9, n - first}:
                if first + cnt <= n:
                    assert retained(t.grp, first, cnt) == reads[first:first + cnt], (first, cnt)
        with pytest.raises(sa.ShkError) as err:
            t.grp.retained_reads(n - 1, 2)
        assert err.value.code == -2 and f"outside the {n} retained reads" in err.value.msg
        # bases_cap one short: the need, nothing written
        need = sum(len(r) for r in reads[5:31])
        out, off, nb = np.full(need, 99, dtype=np.uint8), np.zeros(27, dtype=np.uint64), C.c_uint64(0)
        call = lambda cap: t.grp._L.shk_retained_export(t.grp._h, 5, 26, out.ctypes.data, cap, off.ctypes.data, C.byref(nb))  # noqa: E731
        assert call(need - 1) == -2 and nb.value == need and (out == 99).all()
        assert call(need) == 0 and bytes(out) == b"".join(reads[5:31]) and off[-1] == need
        # the counts are the one-device context's too
        for e in (t.one, t.grp):
            e.finalize()
        assert np.array_equal(t.one.histograms(), t.grp.histograms())
        # reset: empty, retention still on; then again
        t.one.reset(), t.grp.reset()
        assert t.same_store([]) == [] and t.grp.retained_info()["device_bytes"] > 0
        t.ingest(reads[7:19])
        t.same_store(reads[7:19])
        with pytest.raises(sa.ShkError) as err:
            t.grp.retain_reads()
        assert err.value.code == -11 and "retained already" in err.value.msg
        # off: the stores are gone; on again needs an empty context
        t.grp.retain_reads(False)
        assert t.grp.retained_info() == {"reads": 0, "bases": 0, "device_bytes": 0}
        with pytest.raises(sa.ShkError) as err:
            t.grp.retained_reads()
        assert err.value.code == -11 and "reads are not retained" in err.value.msg
        with pytest.raises(sa.ShkError) as err:
            t.grp.retain_reads()
        assert err.value.code == -11 and "holds reads already" in err.value.msg
        t.grp.reset()
        t.grp.retain_reads()
        b, o = t.grp._pack(reads[:5])
        t.grp.ingest_reads(b, o)
        assert retained(t.grp) == reads[:5]


@pytest.mark.parametrize("n_devices", [2, 4])
def test_store_ends_at_every_kind_of_bit(n_devices):
    """retained_cases.splits: fillers that end a store at bit 63 / 64 / 65 of a word, one read per batch, one batch."""
    reads = [b"ACGTACGTTGCA" * 9, b"", b"AAC", b"GATTACA" * 20]
    with Twin(21, n_devices) as t:
        for name, batches, n_front in rc.splits(reads):
            t.one.reset(), t.grp.reset()
            for b in batches:
                t.ingest(b)
            assert t.same_store(rc.flat(batches))[n_front:] == reads, name


# ---- 2. the filter ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_devices", [2, 4])
def test_filter_equals_the_one_device_answer(orc, n_devices):
    engines = {}
    try:
        for case in rc.filter_cases(orc):
            if case.k not in engines:
                engines[case.k] = Twin(case.k, n_devices)
            t = engines[case.k]
            for name, batches, n_front in rc.splits(case.reads)[::3]:
                t.one.reset(), t.grp.reset()
                for b in batches:
                    t.ingest(b)
                want = pc.expected(orc, pc.Case(case.name, case.k, case.genes, rc.flat(batches), []))
                a, b = t.both(lambda e: [r.tolist() for r in e.filter_reads_retained(case.genes)])
                assert a == want and b == want, (case.name, name)
    finally:
        for t in engines.values():
            t.close()


def test_filter_matches_alternate_between_shares_and_match_cap():
    k = 21
    rng = random.Random(5)
    hit = bytes(rng.choice(b"ACGT") for _ in range(150))
    key = [canon(hit[40:40 + k])]
    reads = [hit if i % 2 == 0 else bytes(rng.choice(b"ACGT") for _ in range(150)) for i in range(48)]
    with Twin(k, 2) as t:
        t.ingest(reads)  # runs of 6 reads (1 KiB rounds): the matches, every other read, change share every 6 reads
        genes = [key, [], key]
        a, b = t.both(lambda e: [r.tolist() for r in e.filter_reads_retained(genes)])
        assert a == b == [list(range(0, 48, 2)), [], list(range(0, 48, 2))]
        need = 48
        pk = np.asarray(key + key, dtype=np.uint64)
        goff = np.asarray([0, 1, 1, 2], dtype=np.uint64)
        for cap in (need - 1, need):
            moff, out, n = np.full(4, 99, dtype=np.uint64), np.full(need, 99, dtype=np.uint64), C.c_uint64(0)
            rcode = t.grp._L.shk_filter_reads_panel_retained(t.grp._h, pk.ctypes.data, goff.ctypes.data, 3, moff.ctypes.data, out.ctypes.data, cap,
                                                             C.byref(n))
            assert (rcode, n.value, moff.tolist()) == (-2 if cap < need else 0, need, [0, 24, 24, 48]), cap
            if cap < need:
                assert f"{need} matches do not fit match_cap {cap}" in t.grp._L.shk_last_error(t.grp._h).decode() and (out == 99).all()
        assert out.tolist() == a[0] + a[2]


# ---- 3. the threading -------------------------------------------------------------------------------------------------------

def thread_twin(t, p, batches, n_front):
    t.one.reset(), t.grp.reset()
    for b in batches:
        t.ingest(b)
    graphs = [graph_arrays(g) for g in p.graphs]
    lists = [[n_front + i for i in ids] for ids in p.lists]
    n = n_front + len(p.reads)
    ri = None if p.read_index is None else [0] * n_front + list(p.read_index)
    mt = None if p.mate is None else [0] * n_front + list(p.mate)
    return t.both(lambda e: got_rows(e.thread_reads_retained(graphs, lists, ri, mt)))


@pytest.mark.parametrize("n_devices", [2, 4])
def test_thread_panels_equal_the_one_device_answer(n_devices):
    """retained_cases.thread_panels with their reversed and doubled lists: genes without reads, genes without edges, branch
    links, paired panels — the model's rows (thread_panel_cases.expected) from both contexts."""
    engines = {}
    seen_links = seen_pairs = 0
    try:
        for p0 in rc.thread_panels():
            if p0.k not in engines:
                engines[p0.k] = Twin(p0.k, n_devices)
            t = engines[p0.k]
            for p in rc.list_variants(p0):
                want = want_rows(p)
                for name, batches, n_front in rc.splits(p.reads)[::(2 if p is p0 else 5)]:
                    one, grp = thread_twin(t, p, batches, n_front)
                    assert one == want and grp == want, (p.name, name)
                seen_links += sum(len(w[2]) for w in want)
                seen_pairs += sum(w[5] for w in want)
    finally:
        for t in engines.values():
            t.close()
    assert seen_links > 0 and seen_pairs > 0


def test_thread_shuffled_lists_shared_links_caps_and_pairs_across_shares():
    import thread_cases as tc
    import thread_ref as ref
    k = 21
    rng = random.Random(9)
    # a fork: a → b → {c, d}: node b is a branch node, reads over a-b-c and a-b-d give links (ab, bc) and (ab, bd)
    stem, left, right = (bytes(rng.choice(b"ACGT") for _ in range(n)) for n in (60, 60, 60))
    path = lambda tail: (stem + tail).decode()  # noqa: E731
    nodes, edges, index = [], [], {}
    for s in (path(left), path(right)):
        prev = None
        for i in range(len(s) - k + 2):
            sub = tc.enc(s[i:i + k - 1])
            if sub not in index:
                index[sub] = len(nodes)
                nodes.append(sub)
            if prev is not None and (prev, index[sub]) not in edges:
                edges.append((prev, index[sub]))
            prev = index[sub]
    g = ref.Graph(nodes, edges)
    lone = ref.Graph(nodes[:5], [])  # a gene with no edges
    cut = lambda s, a, n: s[a:a + n].encode()  # noqa: E731
    # 15 reads of 125 bases → runs of 7 reads (odd) under 1 KiB rounds: pair (6, 7) is cut across the two shares
    reads = [cut(path(left if i % 2 else right), 0, 120) + b"ACGTA" for i in range(15)]
    graphs = [graph_arrays(x) for x in (g, g, lone, g)]
    order = list(range(15))
    rng.shuffle(order)
    lists = [order + order[:4], list(range(15))[::-1], [1, 2], []]  # shuffled with repeats, reversed, (no edges), no reads
    ri, mt = list(range(15)), [1 + (i & 1) for i in range(15)]
    with Twin(k, 2) as t:
        t.ingest(reads)
        pieces = [retained(t.grp, 0, 7), retained(t.grp, 7, 8)]
        assert pieces[0] + pieces[1] == reads
        one, grp = t.both(lambda e: got_rows(e.thread_reads_retained(graphs, lists, ri, mt)))
        assert grp == one
        links, counts = one[1][2], one[1][3]
        assert len(links) == 2 and sum(counts) == 15 and min(counts) >= 7  # each link arises on both shares: the sum
        assert one[0][5] == one[1][5] == 7 and one[3][5] == 0                # 7 whole pairs, (6, 7) among them
        assert sum(one[2][0]) == 0 and one[3][4] == []
        # pairs by the caller's arrays only for reads 6 and 7: the one pair whose mates lie on two shares
        m2 = [m if i in (6, 7) else 0 for i, m in enumerate(mt)]
        one2, grp2 = t.both(lambda e: got_rows(e.thread_reads_retained(graphs, lists, ri, m2)))
        assert grp2 == one2 and one2[0][5] == 1
        # link_cap one short: the need, the offsets complete
        n_links = sum(len(w[2]) for w in one)
        sub = np.concatenate([x[0] for x in graphs])
        es, et = (np.concatenate([x[i] for x in graphs]) for i in (1, 2))
        noff = np.concatenate([[0], np.cumsum([len(x[0]) for x in graphs])]).astype(np.uint64)
        eoff = np.concatenate([[0], np.cumsum([len(x[1]) for x in graphs])]).astype(np.uint64)
        lr = np.concatenate([np.asarray(x, dtype=np.uint64) for x in lists])
        loff = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.uint64)
        offs = np.concatenate([[0], np.cumsum([len(w[2]) for w in one])]).tolist()
        for cap in (n_links - 1, n_links):
            tot, una = np.zeros(len(es), dtype=np.uint32), np.zeros(len(es), dtype=np.uint32)
            li, lo, lc = (np.zeros(n_links, dtype=np.uint32) for _ in range(3))
            koff, re, npl = np.zeros(len(graphs) + 1, dtype=np.uint64), np.zeros(len(lr), dtype=np.uint32), np.zeros(len(graphs), dtype=np.uint64)
            out = _ThreadPanelOut(tot.ctypes.data, una.ctypes.data, koff.ctypes.data, li.ctypes.data, lo.ctypes.data, lc.ctypes.data, cap, 0,
                                  re.ctypes.data, npl.ctypes.data)
            rcode = t.grp._L.shk_thread_reads_panel_retained(t.grp._h, sub.ctypes.data, noff.ctypes.data, es.ctypes.data, et.ctypes.data, eoff.ctypes.data,
                                                             len(graphs), loff.ctypes.data, lr.ctypes.data, None, None, C.byref(out))
            assert (rcode, int(out.n_links), koff.tolist()) == (-2 if cap < n_links else 0, n_links, offs), cap
            if cap < n_links:
                assert f"{n_links} branch links do not fit link_cap {cap}" in t.grp._L.shk_last_error(t.grp._h).decode()
        assert tot.tolist() == [x for w in one for x in w[0]] and lc.tolist() == [x for w in one for x in w[3]]
        bad = lists[:1] + [[15]] + lists[2:]
        with pytest.raises(sa.ShkError) as err:
            t.grp.thread_reads_retained(graphs, bad)
        assert err.value.code == -2 and "is outside the 15 reads" in err.value.msg


# ---- 4. pcr_run -------------------------------------------------------------------------------------------------------------

def test_pcr_run_over_retained_reads_equals_the_plain_context(orc):
    p = ppc.mixed_panel(orc)
    genes = cases.mixed_genes(orc)
    runs = []
    for eng in (plain(p.k), group(p.k, 2), group(p.k, 4)):
        with eng:
            eng.ingest_reads(p.bases, p.offsets)
            eng.finalize()
            runs.append(dict(retained=eng.pcr_run(genes, reads="retained", max_num_nodes=ppc.MIXED_BUDGET),
                             paired=eng.pcr_run(genes, reads="retained", paired=True, max_num_nodes=ppc.MIXED_BUDGET)))
    want = runs[0]
    for got in runs[1:]:
        for mode in want:
            assert len(got[mode]) == len(want[mode]) == len(genes)
            same_outcomes(got[mode], want[mode], mode)
            for x, y in zip(got[mode], want[mode]):
                assert (x.failure_reason, x.products.paths_found, x.products.generated) == (y.failure_reason, y.products.paths_found, y.products.generated)
    assert any(o.threaded for o in want["retained"]) and any(o.threaded for o in want["paired"])


# ---- 5. a random sweep of call sequences ------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", range(12))
def test_random_call_sequences(seed, monkeypatch):
    rng = random.Random(1000 + seed)
    monkeypatch.setenv("SHK_GROUP_ROUND_KB", str(rng.choice([1, 2, 5])))
    k = 21
    motif = bytes(rng.choice(b"ACGT") for _ in range(40))
    genes = [[canon(motif[i:i + k])] for i in (0, 10)]
    held = []
    with Twin(k, rng.choice([2, 4]), chunks=2, hint=rng.choice([None, 64])) as t:
        for step in range(8):
            what = rng.random()
            if what < 0.15:
                t.one.reset(), t.grp.reset()
                held = []
            else:
                reads = rand_reads(rng, rng.choice([1, 2, 3, 9, 25]), 0, 260)
                reads = [r[:30] + motif + r[30:] if rng.random() < 0.4 else r for r in reads]
                t.ingest(reads, lane=rng.choice([None, None, 0, 1]))
                held += reads
            assert t.same_store(held) == held, (seed, step)
            a, b = t.both(lambda e: [r.tolist() for r in e.filter_reads_retained(genes)])
            assert a == b, (seed, step)
            if held:
                first = rng.randrange(len(held))
                cnt = rng.randint(0, len(held) - first)
                assert retained(t.grp, first, cnt) == held[first:first + cnt]
        for e in (t.one, t.grp):
            if held:
                e.finalize()
        if held:
            assert np.array_equal(t.one.histograms(), t.grp.histograms())


# ---- 6. what the flag does not change ---------------------------------------------------------------------------------------

def test_refusals_stay(orc):
    reads = rand_reads(random.Random(2), 6)
    with sa.KmerEngine(21, 1, 100, device_ids=[0, 0]) as multi:  # no flag: the five calls and the switch refuse as they did
        for call in (lambda: multi.retain_reads(), lambda: multi.retained_info(), lambda: multi.retained_reads(),
                     lambda: multi.filter_reads_retained([[1]]), lambda: multi.thread_reads_retained([], [])):
            with pytest.raises(sa.ShkError) as err:
                call()
            assert err.value.code == -11 and NOT_HERE in err.value.msg
    p = ppc.mixed_panel(orc)
    genes = cases.mixed_genes(orc)
    with sa.KmerEngine(p.k, 1, 100, flags=sa.FLAG_GROUP_GRAPH, device_ids=[0, 0]) as graph_only:
        graph_only.ingest_reads(p.bases, p.offsets)
        graph_only.finalize()
        with pytest.raises(sa.ShkError) as err:
            graph_only.pcr_run(genes[:2], reads="retained")
        assert err.value.code == -11 and "reads are not retained" in err.value.msg
        with pytest.raises(sa.ShkError) as err:
            graph_only.retain_reads()
        assert err.value.code == -11 and NOT_HERE in err.value.msg
    # a flagged one-device context is an unflagged one; so is a flagged owner share
    for kw in (dict(), dict(n_owners=2, owner_id=1)):
        with sa.KmerEngine(21, 1, 100, flags=BOTH, **kw) as one, sa.KmerEngine(21, 1, 100, **kw) as ref:
            for e in (one, ref):
                e.retain_reads()
                e.ingest_reads(*e._pack(reads))
            assert retained(one) == retained(ref) == reads
            assert one.retained_info()["reads"] == ref.retained_info()["reads"] == 6


# ---- 7. the command line and run_files --------------------------------------------------------------------------------------

SPECS = ["forward=GAAAAGGGTCGTTGAATAGTCATC,reverse=CACCCAACTTGTTGTTCGCCAGCA,name=a",
         "forward=TAAGCACTGGCGTCCTAGGGGTAA,reverse=TATTAAGGACCGTGCGAATGGTAG,name=b",
         f"forward={ppc.ABSENT},reverse=TATTAAGGACCGTGCGAATGGTAG,name=absent"]


def run_cli(outdir, extra):
    cmd = [EXE, "-k", "21", "-s", "g", "-o", str(outdir), "--chunks", "3", "--histo-max", "50"]
    for s in SPECS:
        cmd += ["--pcr-primers", s]
    return subprocess.run(cmd + extra + FILES, capture_output=True, text=True)


def test_cli_and_run_files_thread_reads_over_two_shares(tmp_path, monkeypatch):
    monkeypatch.setenv("SHK_GROUP_ROUND_KB", "64")
    one, two, three, py = (tmp_path / d for d in ("one", "two", "three", "py"))
    for d in (one, two, three, py):
        d.mkdir()
    r = run_cli(one, ["--read-threading"])
    assert r.returncode == 0, r.stderr
    r = run_cli(two, ["--devices", "0,0", "--group-graph", "--group-reads", "--read-threading"])
    assert r.returncode == 0, r.stderr
    names = sorted(f.name for f in one.iterdir())
    assert names == sorted(f.name for f in two.iterdir()) and "g_a.fasta" in names and "g_b.fasta" in names
    sa.run_files(FILES, k=21, chunks=3, sample="g", outdir=str(py), histo_max=50, device_ids=[0, 0], group_graph=True, group_reads=True,
                 read_threading=True, pcr_primers=SPECS)
    for f in names:
        if f.endswith(".fasta") or f.endswith(".histo"):
            assert (one / f).read_bytes() == (two / f).read_bytes() == (py / f).read_bytes(), f
    ya, yb, yc = (yaml.safe_load((d / "g.stats.yaml").read_text()) for d in (one, two, py))
    assert ya["pcr_results"] == yb["pcr_results"] == yc["pcr_results"] and [x["status"] for x in yb["pcr_results"]] == ["success", "success", "fail"]
    # without --group-reads: today's refusal, nothing written
    r = run_cli(three, ["--devices", "0,0", "--group-graph", "--read-threading"])
    assert r.returncode != 0 and "a multi-device context keeps no reads: --read-threading needs one device" in r.stderr
    assert not list(three.iterdir())
    r = run_cli(three, ["--devices", "0,0", "--group-reads", "--read-threading"])  # the graph refusal stays first
    assert r.returncode != 0 and "needs the whole table on one device" in r.stderr and not list(three.iterdir())
