"""GPU tests of the panel read filter: shk_filter_reads_panel / _device (k_filter_panel) and shk_gather_reads_device
(k_gather_reads) against the oracle's KmerCounts.filter_matches — PrimerReadFilter::matches — per gene and per read.
Everything is integers and compared for equality, order included.  Every test runs twice: with the lookup set in
global memory (SHK_FILTER_LDS_KEYS=0) and with the knob at its default, which keeps every panel of this file in LDS."""
import ctypes as C
import os

import numpy as np
import pytest

import sharkmer_amd as sa
import panel_cases as pc

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_run = {}


@pytest.fixture(params=["lds", "global"], autouse=True)
def variant(request, monkeypatch, capfd):
    """With SHK_TRACE set a pass says on stderr where its set lies and how much room its record list has; `launched`
    checks that it was where the variant puts it."""
    if request.param == "global":
        monkeypatch.setenv("SHK_FILTER_LDS_KEYS", "0")
    else:
        monkeypatch.delenv("SHK_FILTER_LDS_KEYS", raising=False)
    monkeypatch.delenv("SHK_FILTER_CANDIDATES", raising=False)
    monkeypatch.setenv("SHK_TRACE", "1")
    _run.update(capfd=capfd, where=" in " + ("global memory" if request.param == "global" else "LDS") + ",")
    return request.param


def launched(n=None):
    """The passes since the last look (n of them, if given), each with its set where the variant puts it → their rooms."""
    lines = [x for x in _run["capfd"].readouterr().err.splitlines() if "filter_panel:" in x]
    assert n is None or len(lines) == n, lines
    for x in lines:
        assert _run["where"] in x, x
    _run["blocks"] = [int(x.split(", ")[-1].split(" blocks")[0]) for x in lines]
    return [int(x.split("room ")[1].split(",")[0]) for x in lines]


def to_device(bases, offsets):
    import torch
    db = torch.from_numpy(np.ascontiguousarray(bases, dtype=np.uint8).copy()).to("cuda:0")
    do = torch.from_numpy(np.ascontiguousarray(offsets).astype(np.int64)).to("cuda:0")
    torch.cuda.synchronize()
    return db, do


def both_forms(eng, reads, genes):
    """The panel call through the host form and through the device form → the two answers as lists of lists."""
    bases, offsets = eng._pack(reads)
    host = eng.filter_reads_panel(bases, offsets, genes)
    db, do = to_device(bases, offsets)
    dev = eng.filter_reads_panel(db, do, genes, device=True)
    for rows in (host, dev):
        assert all(r.dtype == np.uint64 for r in rows)
    return [r.tolist() for r in host], [r.tolist() for r in dev]


# ---- 1. the crafted cases ---------------------------------------------------------------------------------------------------

def test_crafted_cases(orc):
    engines = {}
    try:
        for case in pc.crafted_cases(orc):
            if case.k not in engines:
                engines[case.k] = sa.KmerEngine(case.k, 1, 100)
            want = pc.expected(orc, case)
            launched()
            host, dev = both_forms(engines[case.k], case.reads, case.genes)
            assert len(launched()) >= 2, case.name  # at least a pass per form, each with its set where the variant puts it
            assert host == want, case.name
            assert dev == want, case.name
    finally:
        for e in engines.values():
            e.close()


# ---- 1b. many reads per wave: what a wave carries from one read to the next ------------------------------------------------------

def test_every_wave_walks_many_reads(orc):
    """The kernel's waves are persistent and stride over the batch; a wave's bitmap has to be all zero again after every
    read, matched, cancelled by an invalid byte or neither.  40000 reads of a few kinds in pseudo-random order: every
    wave of the grid gets at least four, and every kind follows every kind on some wave (the CPU test asserts that)."""
    k, genes, kinds, kind_genes, order = pc.stride_batch(orc)
    want = pc.stride_rows(orc)
    reads = [kinds[j] for j in order.tolist()]
    with sa.KmerEngine(k, 1, 100) as eng:
        launched()
        host, dev = both_forms(eng, reads, genes)
        launched()
        assert len(_run["blocks"]) >= 2 and all(4 * 16 * b <= len(reads) for b in _run["blocks"]), _run["blocks"]
        assert host == want
        assert dev == want


# ---- 2. the batch of test_filter_reads_matches_reference_semantics: one gene = shk_filter_reads, and a 12-gene panel ------

@pytest.mark.parametrize("k", [5, 21, 31])
def test_one_gene_equals_filter_reads_and_a_panel_cut_from_the_reads(orc, k):
    seqs, single, genes, rows = pc.big_batch(orc, k)
    assert all(len(r) > 0 for r in rows) and len(seqs) - len(set(i for r in rows for i in r)) >= 40
    with sa.KmerEngine(k, 1, 10) as eng:
        bases, offsets = eng._pack(seqs)
        flags = eng.filter_reads(bases, offsets, single)
        host, dev = both_forms(eng, seqs, [single])
        assert host == dev == [np.flatnonzero(flags).tolist()] and flags.sum() > 25 and (~flags).sum() >= 40
        host, dev = both_forms(eng, seqs, genes)
        assert host == rows
        assert dev == rows
        launched()


# ---- 3. the record list overflows: counted, rerun with the exact size ---------------------------------------------------------

def test_overflow_reruns_with_exact_room(orc, monkeypatch):
    seqs, single, genes, rows = pc.big_batch(orc, 21)
    need = sum(len(r) for r in rows)
    assert 4 < need <= len(seqs)  # (within the binding's first capacity: one pass per call, unless the record list overflows)
    with sa.KmerEngine(21, 1, 10) as eng:
        bases, offsets = eng._pack(seqs)
        launched()
        for room in ("4", str(need - 1), str(need)):
            monkeypatch.setenv("SHK_FILTER_CANDIDATES", room)
            got = eng.filter_reads_panel(bases, offsets, genes)
            assert [r.tolist() for r in got] == rows, room
            assert launched() == ([int(room), need] if int(room) < need else [need]), room


# ---- 4. match_cap ---------------------------------------------------------------------------------------------------------------

def panel_arrays(genes):
    genes = [np.ascontiguousarray(g, dtype=np.uint64) for g in genes]
    goff = np.concatenate([[0], np.cumsum([len(g) for g in genes])]).astype(np.uint64)
    return (np.concatenate(genes) if genes else np.zeros(0, dtype=np.uint64)), goff


def test_match_cap_one_short_then_retry(orc):
    case = [c for c in pc.crafted_cases(orc) if "a read in three genes" in c.name][0]
    want = pc.expected(orc, case)
    need = sum(len(r) for r in want)
    offs = np.concatenate([[0], np.cumsum([len(r) for r in want])]).tolist()
    pk, goff = panel_arrays(case.genes)
    with sa.KmerEngine(case.k, 1, 100) as eng:
        bases, offsets = eng._pack(case.reads)
        db, do = to_device(bases, offsets)
        forms = [(eng._L.shk_filter_reads_panel, (bases.ctypes.data, offsets.ctypes.data, len(case.reads))),
                 (eng._L.shk_filter_reads_panel_device, (db.data_ptr(), do.data_ptr(), len(case.reads), len(bases)))]
        for call, args in forms:
            for cap in (need - 1, 0, need):
                moff = np.full(len(case.genes) + 1, 99, dtype=np.uint64)
                reads = np.full(need, 99, dtype=np.uint64)
                n = C.c_uint64(0)
                rc = call(eng._h, *args, pk.ctypes.data, goff.ctypes.data, len(case.genes), moff.ctypes.data, reads.ctypes.data, cap, C.byref(n))
                assert (rc, n.value, moff.tolist()) == (-2 if cap < need else 0, need, offs), cap
                if cap < need:
                    assert f"{need} matches do not fit match_cap {cap}" in eng._L.shk_last_error(eng._h).decode()
                    assert (reads == 99).all()
            assert reads.tolist() == [i for r in want for i in r]


# ---- 5. argument errors --------------------------------------------------------------------------------------------------------

def test_argument_errors(orc):
    with sa.KmerEngine(5, 1, 100) as eng:
        L, h = eng._L, eng._h
        bases, offsets = eng._pack([b"ACGTACGT", b"ACGTA"])
        db, do = to_device(bases, offsets)
        pk, goff = np.array([1, 2, 3], dtype=np.uint64), np.array([0, 2, 3], dtype=np.uint64)
        moff, reads, n = np.zeros(4200, dtype=np.uint64), np.zeros(8, dtype=np.uint64), C.c_uint64(0)

        def host(bases=bases, offsets=offsets, pk=pk, goff=goff, n_genes=2, n_seqs=2):
            return L.shk_filter_reads_panel(h, bases.ctypes.data, offsets.ctypes.data, n_seqs, pk.ctypes.data, goff.ctypes.data, n_genes,
                                            moff.ctypes.data, reads.ctypes.data, 8, C.byref(n))

        def dev(do=do, n_bases=len(bases), pk=pk, goff=goff, n_genes=2):
            return L.shk_filter_reads_panel_device(h, db.data_ptr(), do.data_ptr(), 2, n_bases, pk.ctypes.data, goff.ctypes.data, n_genes,
                                                   moff.ctypes.data, reads.ctypes.data, 8, C.byref(n))

        def refused(rc, text):
            assert rc == -2 and text in L.shk_last_error(h).decode(), (rc, L.shk_last_error(h))

        assert host() == 0 and dev() == 0
        down = np.array([0, 3, 2], dtype=np.uint64)
        for call in (host, dev):
            refused(call(goff=down), "gene_offsets must be non-decreasing")
            refused(call(pk=np.array([1, 1 << 10, 3], dtype=np.uint64)), "primer k-mer 1024 does not fit 5 bases")
            refused(call(n_genes=4097, goff=np.zeros(4098, dtype=np.uint64)), "n_genes 4097 is above the limit of 4096")
            assert call(n_genes=4096, goff=np.zeros(4097, dtype=np.uint64)) == 0  # the limit itself: every gene empty
        refused(host(offsets=np.array([0, 8, 7], dtype=np.uint64)), "offsets must be non-decreasing")
        refused(dev(do=to_device(bases, [0, 8, 7])[1]), "offsets must be non-decreasing")
        refused(dev(n_bases=12), "offsets end at 13, beyond the 12 bases")
        # a read of 2^31 bases: refused on its offsets alone, before any base is touched
        long = np.array([0, 8, 8 + (1 << 31)], dtype=np.uint64)
        refused(host(offsets=long), "a read of 2147483648 bases: shk_filter_reads_panel takes reads below 2^31")
        refused(dev(do=to_device(bases, long)[1], n_bases=8 + (1 << 31)), "a read of 2147483648 bases: shk_filter_reads_panel takes reads below 2^31")
        # nothing to do: all zero, SHK_OK
        moff[:] = 7
        assert host(n_genes=0) == 0 and n.value == 0 and moff[0] == 0
        moff[:] = 7
        assert host(n_seqs=0) == 0 and n.value == 0 and moff[:3].tolist() == [0, 0, 0]
        assert eng.filter_reads_panel(bases, offsets, []) == []
        assert [r.tolist() for r in eng.filter_reads_panel(*eng._pack([]), [[1], [2]])] == [[], []]
        launched(2)  # the two calls that went through; nothing else reached the device


# ---- 6. the table is not touched -------------------------------------------------------------------------------------------------

def test_table_untouched_mid_job(orc):
    spec = sa.SynthSpec(genome_len=20_000, sub_per_64k=300, n_per_64k=60)
    b1, o1 = sa.synth_reads(spec, 0, 3000)
    b2, o2 = sa.synth_reads(spec, 3000, 3000)
    seqs, single, genes, rows = pc.big_batch(orc, 21)

    def job(with_call):
        with sa.KmerEngine(21, 3, 100) as eng:
            eng.ingest_reads(b1, o1)
            if with_call:
                host, dev = both_forms(eng, seqs, genes)
                assert host == rows and dev == rows
                own = eng.filter_reads_panel(b1, o1, genes)  # the job's own reads too
                assert len(own) == 12
            eng.ingest_reads(b2, o2)
            eng.finalize()
            return eng.histograms(), eng.counters()

    h0, c0 = job(False)
    h1, c1 = job(True)
    assert np.array_equal(h0, h1)
    for name in ("n_reads_ingested", "n_bases_read", "n_bases_ingested", "n_kmers_ingested", "n_unique_kmers", "n_hashed_kmers",
                 "n_singleton_kmers"):
        assert c0[name] == c1[name], name


def test_owner_share_and_multi_device(orc):
    case = [c for c in pc.crafted_cases(orc) if "a read in three genes" in c.name][0]
    want = pc.expected(orc, case)
    with sa.KmerEngine(case.k, 1, 100, n_owners=2, owner_id=1) as eng:
        assert both_forms(eng, case.reads, case.genes) == (want, want)
    with sa.KmerEngine(case.k, 1, 100, device_ids=[0, 0]) as eng:
        assert both_forms(eng, case.reads, case.genes) == (want, want)
        db, do = to_device(*eng._pack(case.reads))
        gb, go = eng.gather_reads(db, do, [3, 0])
        assert bytes(gb.cpu().numpy()) == case.reads[3] + case.reads[0]


# ---- 7. gather ---------------------------------------------------------------------------------------------------------------------

def test_gather_reads():
    reads = [b"ACGT" * 40, b"", b"N", pc.rand_seq(5, 149), b"", pc.rand_seq(6, 64), pc.rand_seq(7, 65), b"TTX", pc.rand_seq(8, 1000)]
    with sa.KmerEngine(21, 1, 100) as eng:
        bases, offsets = eng._pack(reads)
        db, do = to_device(bases, offsets)
        for ids in ([], [1], [1, 4, 1], [8, 0, 3], list(range(9)), [7, 7, 2, 8, 8, 1, 5, 6, 0, 3, 3], list(range(8, -1, -1)) * 40):
            gb, go = eng.gather_reads(db, do, ids)
            want = [reads[i] for i in ids]
            assert go.cpu().numpy().tolist() == np.concatenate([[0], np.cumsum([len(w) for w in want])]).astype(np.int64).tolist(), ids
            assert bytes(gb.cpu().numpy()) == b"".join(want), ids
            assert gb.device == db.device and go.device == db.device
        # cap one short: the need, and nothing written; an id out of range
        import torch
        ids = np.array([3, 0, 8], dtype=np.uint64)
        need = 149 + 160 + 1000
        out = torch.full((need,), 7, dtype=torch.uint8, device="cuda:0")
        oo = torch.full((4,), 7, dtype=torch.int64, device="cuda:0")
        n = C.c_uint64(0)
        call = lambda ids, cap: eng._L.shk_gather_reads_device(eng._h, db.data_ptr(), do.data_ptr(), len(reads), ids.ctypes.data, len(ids),  # noqa: E731
                                                               out.data_ptr(), cap, oo.data_ptr(), C.byref(n))
        assert call(ids, need - 1) == -2 and n.value == need
        assert f"{need} bases do not fit out_bases_cap {need - 1}" in eng._L.shk_last_error(eng._h).decode()
        assert (out.cpu() == 7).all() and (oo.cpu() == 7).all()
        assert call(np.array([3, 9], dtype=np.uint64), need) == -2
        assert "read_ids[1] = 9 is outside the 9 reads" in eng._L.shk_last_error(eng._h).decode()
        assert (out.cpu() == 7).all() and (oo.cpu() == 7).all()
        assert call(ids, need) == 0 and n.value == need
        assert bytes(out.cpu().numpy()) == reads[3] + reads[0] + reads[8] and oo.cpu().tolist() == [0, 149, 309, 1309]
        with pytest.raises(sa.ShkError) as e:
            eng.gather_reads(db, do, [0, 9])
        assert e.value.code == -2


# ---- 8. the chain: filter → gather → thread, the reads never leaving the device ----------------------------------------------------

def test_chain_filter_gather_thread_18s(orc):
    k = 21
    seq = open(os.path.join(G, "pcr_18s_padded.txt")).read().strip()
    b = np.frombuffer(seq.encode() * 10, dtype=np.uint8).copy()
    o = np.arange(11, dtype=np.uint64) * np.uint64(len(seq))
    with sa.KmerEngine(k, 1, 100) as eng:
        eng.ingest_reads(b, o)
        eng.finalize()
        fwd, rev = eng.primer_pair_kmers("AACCTGGTTGATCCTGCCAGT", "TGATCCTTCTGCAGGTTCACCTAC", trim=15, mismatches=2, min_count=3)
        pg = eng.pcr_extend(fwd, rev, min_count=5, table_min_count=1, sweep=False, max_num_nodes=500_000)
        assert pg.found_path and len(pg.edge_src) > 1700
        # 150-base reads at stride 50 over the sequence, both strands, some with an N or an X, between reads of elsewhere
        reads = []
        other, oo = sa.synth_reads(sa.SynthSpec(genome_len=20_000, sub_per_64k=300, n_per_64k=60), 0, 60)
        for i, at in enumerate(range(0, len(seq) - 150 + 1, 50)):
            r = bytearray(seq[at:at + 150].encode())
            if i % 7 == 0:
                r[20 + i % 100] = ord("N")
            if i % 11 == 0:
                r[149] = ord("X")
            reads.append(pc.rc_bytes(bytes(r)) if i & 1 else bytes(r))
            reads.append(bytes(other[int(oo[i % 60]):int(oo[i % 60 + 1])]))
        # the panel: the amplicon's gene is the primer k-mers and a k-mer every 200 bases (so that reads along it match)
        along = [orc.kmers_from_ascii(seq[p:p + k], k)[0] for p in range(0, len(seq) - k, 200)]
        gene = np.unique(np.concatenate([fwd[0], rev[0], np.array(along, dtype=np.uint64)]))
        decoy = np.array([orc.kmers_from_ascii(pc.rand_seq(9, k), k)[0]], dtype=np.uint64)
        bases, offsets = eng._pack(reads)
        db, do = to_device(bases, offsets)
        ids = eng.filter_reads_panel(db, do, [decoy, gene], device=True)[1]
        kc = orc.KmerCounts(k)
        for x in gene:
            kc.insert(int(x), 1)
        assert ids.tolist() == [i for i, r in enumerate(reads) if kc.filter_matches(r)] and 10 < len(ids) < len(reads) // 2
        gb, go = eng.gather_reads(db, do, ids)
        got = eng.thread_reads(pg, gb, go, device=True)
        want = eng.thread_reads(pg, *eng._pack([reads[int(i)] for i in ids]))
        assert want.read_edges.sum() > 200
        for name in ("support_total", "support_unambiguous", "links", "link_counts", "read_edges"):
            assert np.array_equal(getattr(got, name), getattr(want, name)), name
