"""GPU tests of sPCR's read threading for a whole panel in one call: shk_thread_reads_panel / _device (k_thread_panel)
against tests/thread_ref.py per gene over that gene's listed reads in list order (thread_panel_cases.expected).
Everything is integers and compared for equality, order included: support_total, support_unambiguous, the links, their
counts, read_edges per list position and n_paired_links.  Every check runs both forms, host buffers and device buffers."""
import ctypes as C

import numpy as np
import pytest

import sharkmer_amd as sa
from sharkmer_amd.engine import THREAD_TILE, _ThreadPanelOut
import thread_cases as tc
import thread_panel_cases as tp
import thread_ref as ref
from test_gpu_thread_reads import case_18s, graph_arrays

pytestmark = pytest.mark.gpu

T = THREAD_TILE
_run = {}
_want = {}


@pytest.fixture(autouse=True)
def trace(monkeypatch, capfd):
    """With SHK_TRACE set a launch says on stderr how it was cut: genes, jobs, blocks, genes in LDS / in global memory."""
    monkeypatch.setenv("SHK_TRACE", "1")
    for name in ("SHK_THREAD_PANEL_BLOCKS", "SHK_THREAD_PANEL_JOB", "SHK_THREAD_LDS_EDGES"):
        monkeypatch.delenv(name, raising=False)
    _run.update(capfd=capfd)


def launches():
    """The launches since the last look → [(genes, jobs, blocks, in_lds, in_global)]."""
    out = []
    for x in _run["capfd"].readouterr().err.splitlines():
        if "thread_reads_panel:" in x:
            w = x.split("thread_reads_panel:")[1].replace(",", "").split()
            assert w[1::2][:3] == ["genes", "jobs", "blocks"] and x.endswith("genes in global memory"), x
            out.append((int(w[0]), int(w[2]), int(w[4]), int(w[6]), int(w[10])))
    return out


def to_device(bases, offsets):
    import torch
    db = torch.from_numpy(np.ascontiguousarray(bases).copy()).to("cuda:0")
    do = torch.from_numpy(np.ascontiguousarray(offsets).astype(np.int64)).to("cuda:0")
    torch.cuda.synchronize()
    return db, do


def got_rows(anns):
    return [(a.support_total.tolist(), a.support_unambiguous.tolist(), a.links.tolist(), a.link_counts.tolist(), a.read_edges.tolist(),
             a.n_paired_links) for a in anns]


def want_rows(p):
    if p.name not in _want:  # the model's answer: computed once per panel
        _want[p.name] = [tp.rows(a, len(g.edges)) for a, g in zip(tp.expected(p), p.graphs)]
    return _want[p.name]


def run(eng, p, device=False):
    bases, offsets = eng._pack(p.reads)
    if device:
        bases, offsets = to_device(bases, offsets)
    return got_rows(eng.thread_reads_panel([graph_arrays(g) for g in p.graphs], bases, offsets, p.lists, p.read_index, p.mate, device=device))


def check(eng, p, what=None):
    """Both forms against the model → the launches' trace lines."""
    want = want_rows(p)
    launches()
    for device in (False, True):
        got = run(eng, p, device)
        for g, (a, b) in enumerate(zip(got, want)):
            assert a == b, (p.name, what, "device" if device else "host", "gene", g)
        assert len(got) == len(want)
    return launches()


# ---- 1. thread_cases as one panel; a gene change inside a workgroup ----------------------------------------------------------

def test_crafted_cases_as_one_panel():
    p = tp.crafted_panel()
    with sa.KmerEngine(3, 1, 100) as eng:
        assert len(check(eng, p)) == 2
        check(eng, tp.reverse(p))
        check(eng, p._replace(name=p.name + " (paired)", read_index=list(range(len(p.reads))), mate=[1 + (i & 1) for i in range(len(p.reads))]))


@pytest.mark.parametrize("blocks", ["1", "2", None])
@pytest.mark.parametrize("job", ["1", "3", None])
def test_gene_change_inside_a_workgroup(monkeypatch, blocks, job):
    if blocks:
        monkeypatch.setenv("SHK_THREAD_PANEL_BLOCKS", blocks)
    if job:
        monkeypatch.setenv("SHK_THREAD_PANEL_JOB", job)
    with sa.KmerEngine(3, 1, 100) as eng:
        for p in (tp.crafted_panel(), tp.many_panel()):
            with_edges = sum(1 for g, ids in zip(p.graphs, p.lists) if g.edges and ids)
            for genes, jobs, n_blocks, in_lds, in_global in check(eng, p, (blocks, job)):
                assert genes == len(p.graphs) and in_lds + in_global == sum(1 for g in p.graphs if g.edges)
                if blocks:  # more genes than blocks and more jobs than blocks: every workgroup changes gene
                    assert n_blocks == int(blocks) and with_edges > n_blocks and jobs > n_blocks
                if job == "1":
                    assert jobs == sum(len(ids) for g, ids in zip(p.graphs, p.lists) if g.edges)
                assert jobs >= with_edges


# ---- 2. nothing leaks from one gene to the next ---------------------------------------------------------------------------------

@pytest.mark.parametrize("where", ["lds", "global"])
def test_no_leak_between_twin_genes(monkeypatch, where):
    monkeypatch.setenv("SHK_THREAD_PANEL_BLOCKS", "1")
    monkeypatch.setenv("SHK_THREAD_LDS_EDGES", "0" if where == "global" else "2048")
    with sa.KmerEngine(3, 1, 100) as eng:
        for swap in (False, True):
            p = tp.twin_panel(swap)
            for line in check(eng, p, where):
                assert line[2] == 1 and line[3:] == ((2, 0) if where == "lds" else (0, 2))
            a, b = want_rows(p)
            assert a[0] != b[0]  # the twins' supports differ, as test_thread_panel_cases_cpu.py shows from the model


# ---- 3. the 18S chain at k = 21: LDS → global → LDS on one workgroup; steps ----------------------------------------------------

def chain_panel():
    """Three genes: a short chain cut from the 18S sequence, the 18S graph of pcr_extend (> 1700 edges), another short
    chain; reads of T−1, T, T+1 and 2T+1 windows on the big graph listed next to short reads of the small ones — the
    longest read of the batch belongs to the middle gene only."""
    k = 21
    seq, g, a, lookup = case_18s()
    cut = lambda n_kmers, at=a: seq[at:at + n_kmers + k - 1].encode()  # noqa: E731

    def chain(at, n_edges):
        subs = [tc.enc(seq[at + i:at + i + k - 1]) for i in range(n_edges + 1)]
        return ref.Graph(subs, [(i, i + 1) for i in range(n_edges)])

    small1, small2 = chain(a, 40), chain(a + 100, 30)
    reads = [cut(n, at) for n in (T - 1, T, T + 1, 2 * T + 1) for at in (a, a + 7)]
    reads.append(cut(2 * T + 1)[:-1] + b"X")
    reads.append(cut(2 * T + 1)[:T + 30] + b"N" + cut(2 * T + 1)[T + 31:])
    n_long = len(reads)
    reads += [cut(1, a + i) for i in range(0, 40, 3)] + [cut(5, a + 100 + i) for i in range(0, 25, 4)] + [tc.rc_bytes(cut(10, a + 20))]
    short = list(range(n_long, len(reads)))
    lists = [short, list(range(n_long)) + short[::2], short[::-1]]
    return tp.Panel("18S chain between two small chains", k, [small1, g, small2], reads, lists)


def test_lds_global_lds_on_one_workgroup_and_steps(monkeypatch):
    p = chain_panel()
    n_big = len(p.graphs[1].edges)
    assert len(p.graphs[0].edges) < 100 < n_big <= 2048 and len(p.graphs[2].edges) < 100
    want = want_rows(p)
    assert want[1][4][:8] == [T - 1, T - 1, T, T, T + 1, T + 1, 2 * T + 1, 2 * T + 1] and want[1][4][8] == 0
    assert sum(want[0][4]) > 10 and sum(want[2][4]) > 10
    monkeypatch.setenv("SHK_THREAD_PANEL_BLOCKS", "1")
    with sa.KmerEngine(21, 1, 100) as eng:
        for knob, split in (("100", (2, 1)), ("0", (0, 3)), (None, (3, 0))):
            if knob is None:
                monkeypatch.delenv("SHK_THREAD_LDS_EDGES")
            else:
                monkeypatch.setenv("SHK_THREAD_LDS_EDGES", knob)
            lines = check(eng, p, knob)
            assert len(lines) == 2
            for line in lines:
                assert line[2] == 1 and line[3:] == split, (knob, line)
        # default blocks too: the per-read scratch stride comes from the batch's longest read, whichever gene lists it
        monkeypatch.delenv("SHK_THREAD_PANEL_BLOCKS")
        check(eng, p, "default blocks")


# ---- 4. lists ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("job", ["3", None])
def test_lists(monkeypatch, job):
    if job:
        monkeypatch.setenv("SHK_THREAD_PANEL_JOB", job)
    with sa.KmerEngine(3, 1, 100) as eng:
        p = tp.lists_panel()
        for line in check(eng, p, job):
            if job:  # 3 | 3 | 3 | (no edges) | 3 3 1 | 1 reads
                assert line[1] == 1 + 0 + 1 + 0 + 3 + 1
        check(eng, tp.shared_read_panel())
        # n_genes == 0 and n_seqs == 0: all zero, no launch
        bases, offsets = eng._pack(p.reads)
        assert eng.thread_reads_panel([], bases, offsets, []) == []
        assert eng.thread_reads_panel([], *to_device(bases, offsets), [], device=True) == []
        empty = tp.Panel("no reads", 3, [tc.linear_graph(), tc.branch_graph()], [], [[], []])
        assert check(eng, empty) == []
        for rows, g in zip(want_rows(empty), empty.graphs):
            assert rows[0] == [0] * len(g.edges) and rows[4] == []


# ---- 5. paired ------------------------------------------------------------------------------------------------------------------------

def test_paired():
    p = tp.paired_panel()
    with sa.KmerEngine(3, 1, 100) as eng:
        check(eng, p)
        assert [r[5] for r in want_rows(p)] == [1, 0]
        unpaired = p._replace(name="paired without mates", read_index=None, mate=None)
        check(eng, unpaired)
        assert [r[5] for r in run(eng, unpaired)] == [0, 0]


# ---- 6. against the existing route: filter → gather → thread_reads per gene --------------------------------------------------------

def test_against_filter_gather_thread_per_gene():
    k = 21
    seq = case_18s()[0]
    spec = sa.SynthSpec(genome_len=20_000, sub_per_64k=300, n_per_64k=60)
    other, oo = sa.synth_reads(spec, 0, 3000)
    reads = []
    for i in range(3000):
        if i % 10 == 0:  # a tenth of the batch lies on the 18S sequence, both strands, some with an N or an X
            at = (i * 37) % (len(seq) - 150)
            r = bytearray(seq[at:at + 150].encode())
            if i % 70 == 0:
                r[20 + i % 100] = ord("N")
            if i % 110 == 0:
                r[149] = ord("X")
            reads.append(tc.rc_bytes(bytes(r)) if i % 20 else bytes(r))
        else:
            reads.append(bytes(other[int(oo[i]):int(oo[i + 1])]))
    # three genes cut from the sequence's windows: a chain graph each, its primer set a k-mer every 40 bases of the window
    graphs, genes = [], []
    for at, n_edges in ((len(seq) // 8, 500), (len(seq) // 8 + 300, 450), (len(seq) * 5 // 8, 300)):
        subs = [tc.enc(seq[at + i:at + i + k - 1]) for i in range(n_edges + 1)]
        graphs.append(ref.Graph(subs, [(i, i + 1) for i in range(n_edges)]))
        genes.append(np.array([ref.kmers_from_ascii(seq[at + i:at + i + k].encode(), k)[0][0] for i in range(0, n_edges, 40)], dtype=np.uint64))
    with sa.KmerEngine(k, 1, 100) as eng:
        db, do = to_device(*eng._pack(reads))
        lists = eng.filter_reads_panel(db, do, genes, device=True)
        assert all(20 < len(x) < 300 for x in lists) and set(lists[0].tolist()) & set(lists[1].tolist())
        got = eng.thread_reads_panel([graph_arrays(g) for g in graphs], db, do, lists, device=True)
        p = tp.Panel("filtered 18S", k, graphs, reads, [x.tolist() for x in lists])
        assert got_rows(got) == want_rows(p)
        for g, ids in enumerate(lists):
            gb, go = eng.gather_reads(db, do, ids)
            one = eng.thread_reads(graph_arrays(graphs[g]), gb, go, device=True)
            assert got_rows([one]) == got_rows([got[g]]), g
            assert one.read_edges.sum() > 1000


# ---- 7. the random sweep ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("blocks", ["1", None])
def test_random_sweep(monkeypatch, blocks):
    """The 40 seeds of thread_cases.SWEEP_SEEDS grouped by k into 12 panels of 2, 3 and 5 graphs (none left out:
    test_thread_panel_cases_cpu.py), paired and unpaired."""
    if blocks:
        monkeypatch.setenv("SHK_THREAD_PANEL_BLOCKS", blocks)
    engines = {}
    try:
        for seeds in tp.sweep_groups():
            p = tp.sweep_panel(seeds)
            if p.k not in engines:
                engines[p.k] = sa.KmerEngine(p.k, 1, 100)
            check(engines[p.k], p, blocks)
            check(engines[p.k], p._replace(name=p.name + " unpaired", read_index=None, mate=None), blocks)
    finally:
        for e in engines.values():
            e.close()


# ---- 8. link_cap and argument errors ------------------------------------------------------------------------------------------------------

def cat(parts, dtype):
    off = np.zeros(len(parts) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(x) for x in parts])
    return np.concatenate([np.asarray(x, dtype=dtype) for x in parts] + [np.zeros(0, dtype=dtype)]), off


class Raw:
    """The arrays of one raw shk_thread_reads_panel call over a Panel, any of them replaceable."""

    def __init__(self, eng, p, link_cap=64):
        self.eng = eng
        ga = [graph_arrays(g) for g in p.graphs]
        self.sub, self.noff = cat([x[0] for x in ga], np.uint64)
        self.es, self.eoff = cat([x[1] for x in ga], np.uint32)
        self.et, _ = cat([x[2] for x in ga], np.uint32)
        self.lr, self.loff = cat(p.lists, np.uint64)
        self.bases, self.offsets = eng._pack(p.reads)
        self.n_genes, self.n_seqs = len(p.graphs), len(p.reads)
        self.ri = self.mt = None
        self.tot, self.una = (np.full(len(self.es) + 1, 77, dtype=np.uint32) for _ in range(2))
        self.koff = np.full(self.n_genes + 1, 77, dtype=np.uint64)
        self.li, self.lo, self.lc = (np.zeros(max(link_cap, 1), dtype=np.uint32) for _ in range(3))
        self.re = np.zeros(len(self.lr) + 1, dtype=np.uint32)
        self.npl = np.zeros(self.n_genes + 1, dtype=np.uint64)
        self.link_cap = link_cap

    def call(self):
        ptr = lambda x: None if x is None else x.ctypes.data  # noqa: E731
        self.out = _ThreadPanelOut(ptr(self.tot), ptr(self.una), ptr(self.koff), ptr(self.li), ptr(self.lo), ptr(self.lc), self.link_cap, 0,
                                   ptr(self.re), ptr(self.npl))
        rc = self.eng._L.shk_thread_reads_panel(self.eng._h, ptr(self.sub), ptr(self.noff), ptr(self.es), ptr(self.et), ptr(self.eoff),
                                                self.n_genes, ptr(self.bases), ptr(self.offsets), self.n_seqs, ptr(self.loff), ptr(self.lr),
                                                ptr(self.ri), ptr(self.mt), C.byref(self.out))
        return rc, self.eng._L.shk_last_error(self.eng._h).decode()


def link_panel():
    """Gene 0: AA → AC → {CC, CA}, crossed by (0, 1) and (0, 2); gene 1: the branch graph, crossed by (0, 1) twice."""
    g0 = tc.graph_of(["AA", "AC", "CC", "CA"], [(0, 1), (1, 2), (1, 3)])
    return tp.Panel("links", 3, [g0, tc.branch_graph()], [b"AACC", b"AACA", b"AACG"], [[0, 1], [2, 2]])


def test_link_cap():
    p = link_panel()
    want = want_rows(p)
    need = sum(len(r[2]) for r in want)
    assert need == 3
    with sa.KmerEngine(3, 1, 100) as eng:
        for cap in (need - 1, need):
            r = Raw(eng, p, cap)
            rc, msg = r.call()
            assert (rc, r.out.n_links) == (-2 if cap < need else 0, need), cap
            if cap < need:
                assert f"{need} branch links do not fit link_cap {cap}" in msg
            assert r.koff.tolist() == [0, 2, 3]                                    # link_offsets complete either way
            assert r.tot[:-1].tolist() == want[0][0] + want[1][0] and r.una[:-1].tolist() == want[0][1] + want[1][1]
            assert r.re[:-1].tolist() == want[0][4] + want[1][4]
        assert np.stack([r.li, r.lo], axis=1).tolist() == want[0][2] + want[1][2]  # edge indices local to the gene
        assert r.lc.tolist() == want[0][3] + want[1][3]
        check(eng, p)


def test_argument_errors():
    p = tp.twin_panel()
    with sa.KmerEngine(3, 1, 100) as eng:

        def refused(change, text):
            r = Raw(eng, p)
            change(r)
            rc, msg = r.call()
            assert rc == -2 and text in msg, (text, rc, msg)
            assert launches() == []          # refused before the device was touched
            assert len(check(eng, p)) == 2   # and the context is still usable

        def setv(name, value):
            return lambda r: setattr(r, name, value)

        def seti(name, at, value):
            def f(r):
                getattr(r, name)[at] = value
            return f

        launches()
        # the graph errors of thread_plan, with the gene named
        refused(seti("es", 3, 3), "gene 1: edge 1: endpoint (3, 2) outside the 3 nodes")
        refused(seti("et", 0, 9), "gene 0: edge 0: endpoint (0, 9) outside the 3 nodes")
        refused(seti("sub", 4, 16), "gene 1: node 1: sub_kmer is not a 2-mer")
        refused(setv("tot", None), "gene 0: shk_thread_reads: a graph array or a support array is missing")
        # the offsets
        refused(seti("noff", 1, 7), "gene 1: node_offsets must be non-decreasing")
        refused(seti("eoff", 1, 5), "gene 1: edge_offsets must be non-decreasing")
        refused(seti("loff", 1, 7), "gene 1: list_offsets must be non-decreasing")
        refused(seti("offsets", 2, 3), "offsets must be non-decreasing")
        # the lists
        refused(seti("lr", 3, 6), "gene 1: list_reads[3] = 6 is outside the 6 reads")
        # the limits
        refused(setv("n_genes", 4097), "n_genes 4097 is above the limit of 4096")
        refused(seti("eoff", 2, 1 << 32), "a panel of 4294967296 edges")
        # the mates
        refused(setv("ri", np.arange(6, dtype=np.uint64)), "read_index and mate go together")
        refused(setv("mt", np.ones(6, dtype=np.uint8)), "read_index and mate go together")

        def bad_mate(r):
            r.ri, r.mt = np.arange(6, dtype=np.uint64), np.array([1, 2, 0, 3, 1, 2], dtype=np.uint8)
        refused(bad_mate, "mate[3] = 3: 0 unpaired, 1 R1, 2 R2")
        # the Python side: as ShkError
        with pytest.raises(sa.ShkError) as e:
            eng.thread_reads_panel([graph_arrays(g) for g in p.graphs], *eng._pack(p.reads), [[0], [9]])
        assert e.value.code == -2 and "gene 1: list_reads[1] = 9" in e.value.msg
        assert len(check(eng, p)) == 2


def test_link_slots_above_2_31_are_refused():
    """Three genes, each a star with 2^15 edges into one node and 2^15 out of it: 2^30 (in, out) pairs per gene, and the
    third takes the panel past 2^31 link slots.  Refused on the host: no counter is allocated."""
    n = 1 << 15
    star = (np.zeros(2 * n + 1, dtype=np.uint64), np.concatenate([np.arange(1, n + 1), np.zeros(n)]).astype(np.uint32),
            np.concatenate([np.zeros(n), np.arange(n + 1, 2 * n + 1)]).astype(np.uint32))
    p = tp.twin_panel()
    with sa.KmerEngine(3, 1, 100) as eng:
        launches()
        with pytest.raises(sa.ShkError) as e:
            eng.thread_reads_panel([star, star, star], *eng._pack([b"AAA"]), [[0], [0], [0]])
        assert e.value.code == -2 and "gene 2: the panel's branch nodes have more than 2^31" in e.value.msg
        assert launches() == []
        assert len(check(eng, p)) == 2


def test_k_below_2_is_refused():
    with sa.KmerEngine(1, 1, 100) as eng:
        with pytest.raises(sa.ShkError) as e:
            eng.thread_reads_panel([(np.zeros(1, dtype=np.uint64), np.zeros(1, dtype=np.uint32), np.zeros(1, dtype=np.uint32))],
                                   *eng._pack([b"ACGT"]), [[0]])
        assert e.value.code == -2 and "gene 0:" in e.value.msg and "k >= 2" in e.value.msg


# ---- 9. contexts --------------------------------------------------------------------------------------------------------------------------

def test_table_untouched_mid_job():
    spec = sa.SynthSpec(genome_len=20_000, sub_per_64k=300, n_per_64k=60)
    b1, o1 = sa.synth_reads(spec, 0, 3000)
    b2, o2 = sa.synth_reads(spec, 3000, 3000)
    p = tp.sweep_panel(tp.sweep_groups()[0])

    def job(with_call):
        with sa.KmerEngine(p.k, 3, 100) as eng:
            eng.ingest_reads(b1, o1)
            if with_call:
                assert len(check(eng, p)) == 2
            eng.ingest_reads(b2, o2)
            eng.finalize()
            return eng.histograms(), eng.counters()

    h0, c0 = job(False)
    h1, c1 = job(True)
    assert np.array_equal(h0, h1)
    for name in ("n_reads_ingested", "n_bases_read", "n_bases_ingested", "n_kmers_ingested", "n_unique_kmers", "n_hashed_kmers",
                 "n_singleton_kmers"):
        assert c0[name] == c1[name], name


def test_owner_share_and_multi_device():
    p = tp.sweep_panel(tp.sweep_groups()[1])
    with sa.KmerEngine(p.k, 1, 100, n_owners=2, owner_id=1) as eng:
        assert len(check(eng, p, "owner share")) == 2
    with sa.KmerEngine(p.k, 1, 100, device_ids=[0, 0]) as eng:
        assert len(check(eng, p, "multi-device")) == 2
