"""GPU tests of the retained reads: shk_retain_reads (k_retain), shk_retained_info, shk_retained_export
(k_retained_export) and the two read-side calls over the store, shk_filter_reads_panel_retained and
shk_thread_reads_panel_retained (the plane walks of k_filter_panel_retained / k_thread_panel_retained).

Everything is integers and lists, compared for equality.  The expected value is the reference's semantics as the
project states them — the oracle's KmerCounts.filter_matches per gene and read, tests/thread_ref.py per gene
(tests/retained_cases.py) — and the host-batch panel calls on the same reads as a cross-check; never the retained
calls alone."""
import ctypes as C
import os

import numpy as np
import pytest

import sharkmer_amd as sa
from sharkmer_amd.engine import _ThreadPanelOut
import panel_cases as pc
import retained_cases as rc
import thread_panel_cases as tp
from test_gpu_thread_reads import graph_arrays

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROUTES = ("reads", "batch", "packed", "reads_device", "packed_device")
_keep = []  # device tensors of queued ingests: alive until the test is over


@pytest.fixture(autouse=True)
def _clean(monkeypatch):
    for name in ("SHK_FILTER_LDS_KEYS", "SHK_FILTER_CANDIDATES", "SHK_THREAD_LDS_EDGES", "SHK_THREAD_PANEL_JOB", "SHK_THREAD_PANEL_BLOCKS",
                 "SHK_SUB_KB"):
        monkeypatch.delenv(name, raising=False)
    yield
    _keep.clear()


def ingest(eng, reads, route="reads", lane=0):
    import torch
    bases, offsets = eng._pack(reads)
    if route == "reads":
        eng.ingest_reads(bases, offsets)
    elif route == "batch":
        eng.ingest_batch(lane, bases, offsets)
    elif route == "packed":
        eng.ingest_packed(sa.pack_reads(bases, offsets))
    elif route == "reads_device":
        db = torch.from_numpy(np.concatenate([bases, np.zeros(16, dtype=np.uint8)])).to("cuda:0")
        do = torch.from_numpy(offsets.astype(np.int64)).to("cuda:0")
        torch.cuda.synchronize()
        _keep.extend([db, do])
        eng.ingest_reads_device(db.data_ptr(), do.data_ptr(), len(reads), len(bases))
    elif route == "packed_device":
        pk = sa.pack_reads(bases, offsets)
        dp = torch.from_numpy(np.concatenate([pk.packed, np.zeros(16, dtype=np.uint8)])).to("cuda:0")
        dm = torch.from_numpy(np.concatenate([pk.nmask, np.zeros(2, dtype=np.uint32)]).view(np.int32)).to("cuda:0")
        do = torch.from_numpy(offsets.astype(np.int64)).to("cuda:0")
        torch.cuda.synchronize()
        _keep.extend([dp, dm, do])
        eng.ingest_packed_device(dp.data_ptr(), dm.data_ptr(), do.data_ptr(), len(reads), len(bases))
    else:
        raise AssertionError(route)


def retained(eng, first=0, n=None):
    bases, offsets = eng.retained_reads(first, n)
    assert bases.dtype == np.uint8 and offsets.dtype == np.uint64 and offsets[0] == 0 and offsets[-1] == len(bases)
    return [bytes(bases[int(a):int(b)]) for a, b in zip(offsets[:-1], offsets[1:])]


def fresh(k, chunks=1, **kw):
    eng = sa.KmerEngine(k, chunks, 100, **kw)
    eng.retain_reads()
    return eng


def assert_holds(eng, reads):
    assert retained(eng) == list(reads)
    assert eng.retained_info()["reads"] == len(reads) and eng.retained_info()["bases"] == sum(len(r) for r in reads)


# ---- 1. the round trip ---------------------------------------------------------------------------------------------------------------
READS = [b"ACGTN" * 30, b"", b"N", pc.rand_seq(5, 149), b"", pc.rand_seq(6, 64), pc.rand_seq(7, 65), b"TTNNA", pc.rand_seq(8, 1000), b"G" * 63,
         pc.put(pc.rand_seq(9, 200), 63, b"N"), b"C"]


@pytest.mark.parametrize("route", ROUTES)
def test_round_trip_by_route(route):
    with fresh(21, 3) as eng:
        ingest(eng, READS, route, lane=2)           # one call
        assert_holds(eng, READS)
        eng.reset()
        for i, r in enumerate(READS):               # one read per call
            ingest(eng, [r], route, lane=i % 3)
        assert_holds(eng, READS)
        for _, batches, _ in rc.splits(READS)[2:]:  # behind every filler pattern
            eng.reset()
            for b in batches:
                ingest(eng, b, route, lane=1)
            assert_holds(eng, rc.flat(batches))
        assert eng.retained_info()["device_bytes"] > 0


def test_round_trip_of_sliced_and_sub_launched_batches(monkeypatch):
    """One host call cut into several slices (SHK_SLICE_KB), as ASCII and packed on the host, and a batch that SHK_SUB_KB
    cuts into several counting launches: one append each, every read as it went in."""
    spec = sa.SynthSpec(genome_len=30_000, sub_per_64k=300, n_per_64k=200)
    bases, offsets = sa.synth_reads(spec, 0, 3000)
    reads = [bytes(bases[int(a):int(b)]) for a, b in zip(offsets[:-1], offsets[1:])]
    reads[7], reads[1500] = b"", reads[1500][:77]
    for host_pack in ("0", "1"):
        monkeypatch.setenv("SHK_SLICE_KB", "64")
        monkeypatch.setenv("SHK_HOST_PACK", host_pack)
        with fresh(21, 3) as eng:
            ingest(eng, reads, "reads")
            assert_holds(eng, reads)
    monkeypatch.delenv("SHK_SLICE_KB")
    monkeypatch.delenv("SHK_HOST_PACK")
    monkeypatch.setenv("SHK_SUB_KB", "64")
    with fresh(21, 3) as eng, sa.KmerEngine(21, 3, 100) as plain:
        ingest(eng, reads, "reads_device")
        ingest(plain, reads, "reads_device")
        assert_holds(eng, reads)
        eng.finalize(), plain.finalize()
        assert np.array_equal(eng.histograms(), plain.histograms())


def test_export_ranges_and_capacity():
    with fresh(21) as eng:
        ingest(eng, READS[:5])
        ingest(eng, READS[5:])
        assert retained(eng, 3, 4) == READS[3:7] and retained(eng, len(READS), 0) == [] and retained(eng, 0, 0) == []
        assert retained(eng, 11, 1) == [READS[11]] and retained(eng, 1, 2) == [b"", b"N"]
        need = sum(len(r) for r in READS[3:9])
        out, off, n = np.full(need, 7, dtype=np.uint8), np.full(7, 7, dtype=np.uint64), C.c_uint64(0)
        call = lambda first, cnt, cap: eng._L.shk_retained_export(eng._h, first, cnt, out.ctypes.data, cap, off.ctypes.data, C.byref(n))  # noqa: E731
        assert call(3, 6, need - 1) == -2 and n.value == need and (out == 7).all()
        assert f"{need} bases do not fit bases_cap {need - 1}" in eng._L.shk_last_error(eng._h).decode()
        assert call(3, 6, need) == 0 and n.value == need and bytes(out) == b"".join(READS[3:9])
        assert off.tolist() == np.concatenate([[0], np.cumsum([len(r) for r in READS[3:9]])]).tolist()
        assert call(len(READS) - 1, 2, need) == -2 and "outside the 12 retained reads" in eng._L.shk_last_error(eng._h).decode()


# ---- 2. retention changes nothing else -------------------------------------------------------------------------------------------------
def test_counting_is_the_same_with_and_without_retention():
    spec = sa.SynthSpec(genome_len=20_000, sub_per_64k=300, n_per_64k=60)
    b1, o1 = sa.synth_reads(spec, 0, 2500)
    b2, o2 = sa.synth_reads(spec, 2500, 1500)

    def job(retain):
        with sa.KmerEngine(21, 3, 100) as eng:
            if retain:
                eng.retain_reads(capacity_bases=1000)
            eng.ingest_reads(b1, o1)
            eng.ingest_reads(b2, o2)
            eng.finalize()
            n = eng.retained_info()
            assert (n["reads"], n["bases"]) == ((4000, 4000 * 150) if retain else (0, 0))
            kmers, counts = eng.export_table()[:2]
            order = np.argsort(kmers, kind="stable")  # (the table's order is the slots': compared as a sorted list)
            return eng.histograms(), eng.counters(), (kmers[order], counts[order])

    h0, c0, t0 = job(False)
    h1, c1, t1 = job(True)
    assert np.array_equal(h0, h1) and c0 == c1
    for a, b in zip(t0, t1):
        assert np.array_equal(a, b)


# ---- 3. the filter -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(params=["lds", "global"])
def filter_set(request, monkeypatch, capfd):
    """Where the panel's set lies (SHK_FILTER_LDS_KEYS forced to 0, or the default) → a check of the passes' trace lines."""
    if request.param == "global":
        monkeypatch.setenv("SHK_FILTER_LDS_KEYS", "0")
    monkeypatch.setenv("SHK_TRACE", "1")
    where = " in " + ("global memory" if request.param == "global" else "LDS") + ","

    def passes():
        lines = [x for x in capfd.readouterr().err.splitlines() if "filter_panel:" in x]
        for x in lines:
            assert where in x, x
        return [(int(x.split("room ")[1].split(",")[0]), x.endswith(", retained reads")) for x in lines]
    return passes


def filter_both(eng, batches, genes, passes):
    """The reads ingested batch by batch → (filter_reads_retained's rows, the host-batch call's over the same reads)."""
    eng.reset()
    for b in batches:
        ingest(eng, b)
    passes()
    got = eng.filter_reads_retained(genes)
    seen = passes()
    assert all(r.dtype == np.uint64 for r in got) and all(ret for _, ret in seen)
    host = eng.filter_reads_panel(*eng._pack(rc.flat(batches)), genes)
    assert not any(ret for _, ret in passes())
    return [r.tolist() for r in got], [r.tolist() for r in host]


def test_filter_crafted_cases_under_every_split(orc, filter_set):
    engines = {}
    try:
        for case in rc.filter_cases(orc):
            eng = engines.setdefault(case.k, fresh(case.k))
            for name, batches, n_front in rc.splits(case.reads):
                want = pc.expected(orc, pc.Case(case.name, case.k, case.genes, rc.flat(batches), []))
                if n_front == 0:
                    assert want == pc.expected(orc, case)
                got, host = filter_both(eng, batches, case.genes, filter_set)
                assert got == want, (case.name, name)
                assert host == want, (case.name, name)
    finally:
        for e in engines.values():
            e.close()


def test_filter_alignment_cases(orc, filter_set):
    engines = {k: fresh(k) for k in rc.KS}
    try:
        for case in rc.alignment_cases(orc):
            want = rc.align_expected(orc, case)
            got, host = filter_both(engines[case.k], case.batches, case.genes, filter_set)
            assert got == want, case.name
            assert host == want, case.name
            assert retained(engines[case.k]) == rc.flat(case.batches), case.name
    finally:
        for e in engines.values():
            e.close()


def test_filter_big_batch_overflow_and_match_cap(orc, filter_set, monkeypatch):
    k, genes, reads, rows = rc.big_valid_batch(orc)
    need = sum(len(r) for r in rows)
    with fresh(k) as eng:
        ingest(eng, reads[:15_000])
        ingest(eng, reads[15_000:])
        filter_set()
        got = eng.filter_reads_retained(genes)
        assert [r.tolist() for r in got] == rows
        assert filter_set() == [(1 << 20, True)]
        # the record list overflows: counted, rerun with room for exactly that
        monkeypatch.setenv("SHK_FILTER_CANDIDATES", "4")
        assert [r.tolist() for r in eng.filter_reads_retained(genes)] == rows
        assert filter_set() == [(4, True), (need, True)]
        monkeypatch.delenv("SHK_FILTER_CANDIDATES")
        # match_cap one short: the need, the offsets complete, nothing written
        pk = np.concatenate([np.asarray(g, dtype=np.uint64) for g in genes])
        goff = np.concatenate([[0], np.cumsum([len(g) for g in genes])]).astype(np.uint64)
        offs = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).tolist()
        for cap in (need - 1, need):
            moff, out, n = np.full(len(genes) + 1, 99, dtype=np.uint64), np.full(need, 99, dtype=np.uint64), C.c_uint64(0)
            rcode = eng._L.shk_filter_reads_panel_retained(eng._h, pk.ctypes.data, goff.ctypes.data, len(genes), moff.ctypes.data, out.ctypes.data,
                                                           cap, C.byref(n))
            assert (rcode, n.value, moff.tolist()) == (-2 if cap < need else 0, need, offs), cap
            if cap < need:
                assert f"{need} matches do not fit match_cap {cap}" in eng._L.shk_last_error(eng._h).decode() and (out == 99).all()
        assert out.tolist() == [i for r in rows for i in r]


# ---- 4. the threading --------------------------------------------------------------------------------------------------------------------
def got_rows(anns):
    return [(a.support_total.tolist(), a.support_unambiguous.tolist(), a.links.tolist(), a.link_counts.tolist(), a.read_edges.tolist(),
             a.n_paired_links) for a in anns]


_want = {}


def want_rows(p):
    if p.name not in _want:  # the model's answer: once per panel
        _want[p.name] = [tp.rows(a, len(g.edges)) for a, g in zip(tp.expected(p), p.graphs)]
    return _want[p.name]


def thread_both(eng, p, batches, n_front):
    """Panel p with its reads behind n_front filler reads → (thread_reads_retained's rows, the host-batch call's)."""
    eng.reset()
    for b in batches:
        ingest(eng, b)
    graphs = [graph_arrays(g) for g in p.graphs]
    lists = [[n_front + i for i in ids] for ids in p.lists]
    n = n_front + len(p.reads)
    ri = None if p.read_index is None else [0] * n_front + list(p.read_index)
    mt = None if p.mate is None else [0] * n_front + list(p.mate)
    got = eng.thread_reads_retained(graphs, lists, ri, mt)
    host = eng.thread_reads_panel(graphs, *eng._pack(rc.flat(batches)), lists, ri, mt)
    return got_rows(got), got_rows(host)


@pytest.mark.parametrize("where", ["lds", "global"])
def test_thread_panels_under_every_split(monkeypatch, capfd, where):
    monkeypatch.setenv("SHK_THREAD_LDS_EDGES", "0" if where == "global" else "2048")
    monkeypatch.setenv("SHK_TRACE", "1")
    engines = {}
    try:
        for p0 in rc.thread_panels():
            eng = engines.setdefault(p0.k, fresh(p0.k))
            for p in rc.list_variants(p0):
                want = want_rows(p)
                for name, batches, n_front in rc.splits(p.reads)[::(1 if p is p0 else 4)]:
                    capfd.readouterr()
                    got, host = thread_both(eng, p, batches, n_front)
                    lines = [x for x in capfd.readouterr().err.splitlines() if "thread_reads_panel:" in x]
                    assert got == want, (p.name, name)
                    assert host == want, (p.name, name)
                    with_edges = sum(1 for g in p.graphs if g.edges)
                    if with_edges and any(ids for g, ids in zip(p.graphs, p.lists) if g.edges):
                        assert len(lines) == 2 and lines[0].endswith(", retained reads") and not lines[1].endswith("retained reads")
                        assert (f"{with_edges} genes in LDS, 0 genes" if where == "lds" else f"0 genes in LDS, {with_edges} genes") in lines[0]
    finally:
        for e in engines.values():
            e.close()


def test_thread_long_reads_across_word_edges():
    """Reads of T − 1, T, T + 1 and 2T + 1 windows threaded along a chain graph at k = 21, 31 behind every filler pattern:
    every step's planes come from two words at a shift."""
    import thread_cases as tc
    import thread_ref as ref
    for k in (21, 31):
        seq = pc.rand_seq(90 + k, 400).decode()
        subs = [tc.enc(seq[i:i + k - 1]) for i in range(300)]
        g = ref.Graph(subs, [(i, i + 1) for i in range(299)])
        cut = lambda n_win, at: seq[at:at + n_win + k - 1].encode()  # noqa: E731
        reads = [cut(n, at) for n in (rc.T - 1, rc.T, rc.T + 1, 2 * rc.T + 1) for at in (0, 9)]
        reads += [pc.put(cut(2 * rc.T + 1, 3), 70, b"N"), b"", pc.rc_bytes(cut(rc.T + 5, 20)), cut(1, 100), cut(1, 100)[:-1]]
        p = tp.Panel(f"chain k={k}", k, [g, g], reads, [list(range(len(reads))), list(range(len(reads)))[::-2]])
        want = want_rows(p)
        assert sum(want[0][4]) > 8 * rc.T
        with fresh(k) as eng:
            for name, batches, n_front in rc.splits(reads):
                got, host = thread_both(eng, p, batches, n_front)
                assert got == want, (k, name)
                assert host == want, (k, name)


def test_thread_link_cap_and_list_errors():
    p = rc.thread_panels()[0]
    want = want_rows(p)
    n_links = sum(len(w[2]) for w in want)
    assert n_links > 1
    with fresh(p.k) as eng:
        ingest(eng, p.reads)
        graphs = [graph_arrays(g) for g in p.graphs]
        sub = np.concatenate([g[0] for g in graphs])
        es, et = (np.concatenate([g[i] for g in graphs]) for i in (1, 2))
        noff = np.concatenate([[0], np.cumsum([len(g[0]) for g in graphs])]).astype(np.uint64)
        eoff = np.concatenate([[0], np.cumsum([len(g[1]) for g in graphs])]).astype(np.uint64)
        lr = np.concatenate([np.asarray(x, dtype=np.uint64) for x in p.lists])
        loff = np.concatenate([[0], np.cumsum([len(x) for x in p.lists])]).astype(np.uint64)

        def call(lr=lr, link_cap=n_links):
            tot, una = np.zeros(len(es), dtype=np.uint32), np.zeros(len(es), dtype=np.uint32)
            li, lo, lc = (np.zeros(max(link_cap, 1), dtype=np.uint32) for _ in range(3))
            koff, re, npl = np.zeros(len(graphs) + 1, dtype=np.uint64), np.zeros(len(lr), dtype=np.uint32), np.zeros(len(graphs), dtype=np.uint64)
            out = _ThreadPanelOut(tot.ctypes.data, una.ctypes.data, koff.ctypes.data, li.ctypes.data, lo.ctypes.data, lc.ctypes.data, link_cap, 0,
                                  re.ctypes.data, npl.ctypes.data)
            rcode = eng._L.shk_thread_reads_panel_retained(eng._h, sub.ctypes.data, noff.ctypes.data, es.ctypes.data, et.ctypes.data,
                                                           eoff.ctypes.data, len(graphs), loff.ctypes.data, lr.ctypes.data, None, None, C.byref(out))
            return rcode, int(out.n_links), koff.tolist(), eng._L.shk_last_error(eng._h).decode()

        offs = np.concatenate([[0], np.cumsum([len(w[2]) for w in want])]).tolist()
        assert call()[:3] == (0, n_links, offs)
        rcode, n, koff, err = call(link_cap=n_links - 1)
        assert (rcode, n, koff) == (-2, n_links, offs) and f"{n_links} branch links do not fit link_cap {n_links - 1}" in err
        bad = lr.copy()
        bad[3] = len(p.reads)
        rcode, _, _, err = call(lr=bad)
        assert rcode == -2 and f"list_reads[3] = {len(p.reads)} is outside the {len(p.reads)} reads" in err


# ---- 5. the life cycle -------------------------------------------------------------------------------------------------------------------
def test_store_grows_from_a_small_hint(orc):
    k, genes, reads, rows = rc.big_valid_batch(orc)
    reads = reads[:2000]
    with sa.KmerEngine(k, 1, 100) as eng:
        eng.retain_reads(capacity_bases=64)
        sizes = []
        for i in range(20):
            ingest(eng, reads[100 * i:100 * (i + 1)])
            sizes.append(eng.retained_info()["device_bytes"])
        assert_holds(eng, reads)
        assert sizes == sorted(sizes) and 3 <= len(set(sizes)) < 15  # geometric: it grew, and not at every batch
        assert [r.tolist() for r in eng.filter_reads_retained(genes)] == [[i for i in r if i < 2000] for r in rows]


def test_reset_finalize_and_a_call_mid_job(orc):
    spec = sa.SynthSpec(genome_len=20_000, sub_per_64k=300, n_per_64k=60)
    b1, o1 = sa.synth_reads(spec, 0, 2000)
    b2, o2 = sa.synth_reads(spec, 2000, 1000)
    r1 = [bytes(b1[int(a):int(b)]) for a, b in zip(o1[:-1], o1[1:])]
    r2 = [bytes(b2[int(a):int(b)]) for a, b in zip(o2[:-1], o2[1:])]
    genes = [orc.kmers_from_ascii(r1[5][10:40], 21), orc.kmers_from_ascii(r2[7][10:40], 21)]
    want = lambda reads: pc.expected(orc, pc.Case("job", 21, genes, reads, []))  # noqa: E731
    with sa.KmerEngine(21, 3, 100) as plain:
        plain.ingest_reads(b1, o1)
        plain.ingest_reads(b2, o2)
        plain.finalize()
        h_plain = plain.histograms()
    with fresh(21, 3) as eng:
        eng.ingest_reads(b1, o1)
        mid = eng.filter_reads_retained(genes)              # mid-job: sees the first batch, leaves the table alone
        assert [r.tolist() for r in mid] == want(r1) and len(mid[0]) > 0
        eng.ingest_reads(b2, o2)
        eng.finalize()
        assert np.array_equal(eng.histograms(), h_plain)    # … and the histogram is exact
        assert [r.tolist() for r in eng.filter_reads_retained(genes)] == want(r1 + r2)
        eng.ingest_reads(b1[:1500], o1[:11])                # after finalize: goes on appending
        assert_holds(eng, r1 + r2 + r1[:10])
        kept = eng.retained_info()["device_bytes"]
        eng.reset()                                         # emptied, the allocation kept, retention still on
        assert eng.retained_info() == {"reads": 0, "bases": 0, "device_bytes": kept} and retained(eng) == []
        assert [r.tolist() for r in eng.filter_reads_retained(genes)] == [[], []]
        eng.ingest_reads(b2, o2)
        assert_holds(eng, r2)
        assert [r.tolist() for r in eng.filter_reads_retained(genes)] == want(r2)
        eng.retain_reads(False)                             # off: the store is gone
        assert eng.retained_info() == {"reads": 0, "bases": 0, "device_bytes": 0}


def test_states_that_are_refused():
    reads = [b"ACGTACGTACGTACGTACGTACGTAC", b"ACGTTGCATGCATGCATGCATGCA"]
    with sa.KmerEngine(21, 1, 100) as eng:
        for call in (lambda: eng.filter_reads_retained([[1]]), lambda: eng.thread_reads_retained([], []), lambda: eng.retained_reads()):
            with pytest.raises(sa.ShkError) as e:
                call()
            assert e.value.code == -11 and "reads are not retained" in str(e.value)
        assert eng.retained_info() == {"reads": 0, "bases": 0, "device_bytes": 0}
        ingest(eng, reads)
        with pytest.raises(sa.ShkError) as e:   # switching on after a read
            eng.retain_reads()
        assert e.value.code == -11 and "holds reads already" in str(e.value)
        eng.reset()
        eng.retain_reads()                      # after a reset: accepted
        ingest(eng, reads)
        assert_holds(eng, reads)
        # zero genes, zero lists: all-zero outputs
        assert eng.filter_reads_retained([]) == [] and eng.thread_reads_retained([], []) == []
    with fresh(21) as eng:                      # zero retained reads
        assert [r.tolist() for r in eng.filter_reads_retained([[1], [2]])] == [[], []] and retained(eng) == []
    with sa.KmerEngine(21, 1, 100, device_ids=[0, 0]) as eng:   # a multi-device context
        for call in (lambda: eng.retain_reads(), lambda: eng.retained_info(), lambda: eng.filter_reads_retained([[1]])):
            with pytest.raises(sa.ShkError) as e:
                call()
            assert e.value.code == -11 and "not available on a multi-device context" in str(e.value)


def test_owner_share_retains_whole_reads_and_an_exchange_round_nothing(orc):
    import torch
    reads = [pc.rand_seq(300 + i, 80 + i) for i in range(40)] + [b"", b"ACGNT"]
    genes = [orc.kmers_from_ascii(reads[3][5:40], 21)]
    want = pc.expected(orc, pc.Case("share", 21, genes, reads, []))
    assert want[0] == [3]
    with fresh(21, 1, n_owners=2, owner_id=1) as eng:   # one owner of two: the share's k-mers are half, its retained reads whole
        ingest(eng, reads)
        assert_holds(eng, reads)
        assert [r.tolist() for r in eng.filter_reads_retained(genes)] == want
    with fresh(21, 1, capacity_hint=4_200_000, n_owners=1, owner_id=0) as eng:  # the share of a world of one: a whole exchange round
        ingest(eng, reads)
        bases, offsets = sa.synth_reads(sa.SynthSpec(genome_len=50_000), 0, 2_000)
        d_b = torch.from_numpy(bases.copy()).cuda()
        d_o = torch.from_numpy(offsets.astype(np.int64)).cuda()
        torch.cuda.synchronize()
        rec, cur, lay = eng.xchg_scatter_begin_tensors(d_b.data_ptr(), d_o.data_ptr(), 2_000, len(bases))
        assert eng.xchg_scatter_end() == 0
        eng.xchg_absorb_tensors(rec, cur, lay)
        assert_holds(eng, reads)                # the round counted 2000 reads and retained none of them
        assert [r.tolist() for r in eng.filter_reads_retained(genes)] == want
        eng.finalize()
        assert eng.counters()["n_kmers_ingested"] == 2_000 * 130 + sum(max(len(r) - 20, 0) for r in reads[:40])


def test_an_invalid_byte_poisons_and_the_retained_calls_say_so():
    text = "Invalid character 'X' in sequence. Only ACGTN allowed."
    with fresh(21) as eng:
        ingest(eng, [b"ACGTACGTACGTACGTACGTACGTAC"])
        with pytest.raises(sa.ShkError) as e:
            ingest(eng, [b"ACGTACGTACGTACGTACGTAXGTAC", b"ACGT"])
            eng.sync()
        assert e.value.code == -1 and text in str(e.value)
        for call in (lambda: eng.filter_reads_retained([[1]]), lambda: eng.thread_reads_retained([], []), lambda: eng.retained_reads()):
            with pytest.raises(sa.ShkError) as e:
                call()
            assert e.value.code == -1 and text in str(e.value)
        eng.reset()                             # a reset clears the poison and empties the store
        ingest(eng, [b"ACGT"])
        assert_holds(eng, [b"ACGT"])


# ---- 6. the whole chain ------------------------------------------------------------------------------------------------------------------
def test_18s_chain_without_a_batch_argument():
    """primer_kmers → pcr_extend_panel → pcr_prune_panel → filter_reads_retained → thread_reads_retained →
    pcr_products_panel on the padded 18S ×10: the products of the same chain with the batch passed explicitly."""
    from test_gpu_pcr_products_panel import FWD_18S, REV_18S, canonical
    seq = open(os.path.join(G, "pcr_18s_padded.txt")).read().strip()
    bases = np.frombuffer(seq.encode() * 10, dtype=np.uint8).copy()
    offsets = np.arange(11, dtype=np.uint64) * np.uint64(len(seq))
    with fresh(21) as e:
        e.ingest_reads(bases[:3 * len(seq)], offsets[:4])
        e.ingest_reads(bases[3 * len(seq):], offsets[3:] - offsets[3])
        e.finalize()
        prim = e.primer_kmers([sa.Primer(s, trim=15, mismatches=2, min_count=3) for s in (FWD_18S, REV_18S)])
        pruned = e.pcr_prune_panel(e.pcr_extend_panel(prim, [dict(min_count=3, max_num_nodes=500_000)]))
        gene = [canonical(np.concatenate([prim[0][0], prim[1][0]]), 21)]
        lists = e.filter_reads_retained(gene)
        anns = e.thread_reads_retained(pruned, lists)
        (got,) = e.pcr_products_panel(pruned, anns, min_length=0, max_length=2500)
        lists2 = e.filter_reads_panel(bases, offsets, gene)
        anns2 = e.thread_reads_panel(pruned, bases, offsets, lists2)
        (want,) = e.pcr_products_panel(pruned, anns2, min_length=0, max_length=2500)
    assert [x.tolist() for x in lists] == [x.tolist() for x in lists2] == [list(range(10))]
    assert got_rows(anns) == got_rows(anns2) and anns[0].read_edges.sum() > 10 * 1700
    assert got.sequences == want.sequences and len(got.sequences) == 1 and len(got.sequences[0]) > 1700 and got.sequences[0] in seq
    assert np.array_equal(got.score_fields, want.score_fields) and np.array_equal(got.score, want.score) and got.retained == want.retained == 1
