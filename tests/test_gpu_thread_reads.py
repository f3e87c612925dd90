"""GPU tests of sPCR's read threading on the device: shk_thread_reads — the one-gene case of shk_thread_reads_panel, run by
k_thread_panel over the batch's reads in their order — against tests/thread_ref.py, the reference's thread_reads /
thread_reads_paired restated literally.  Everything is integers and compared for equality, order included: support_total,
support_unambiguous, the links, their counts, read_edges (and n_paired_links where mates are given).  Every test runs
twice: with the lookup set in LDS and in global memory (SHK_THREAD_LDS_EDGES).  The panel's cuts (SHK_THREAD_PANEL_JOB,
SHK_THREAD_PANEL_BLOCKS) apply to the single call too: section 6 runs it with job tails on both sides of a workgroup's 16
waves."""
import os

import numpy as np
import pytest

import sharkmer_amd as sa
from sharkmer_amd.engine import THREAD_TILE
import thread_cases as tc
import thread_ref as ref

pytestmark = pytest.mark.gpu

T = THREAD_TILE  # list elements one wave step of the read walk covers: a read's state crosses steps at multiples of it
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FWD_18S, REV_18S = "AACCTGGTTGATCCTGCCAGT", "TGATCCTTCTGCAGGTTCACCTAC"
_cache = {}


_run = {}


@pytest.fixture(params=["lds", "global"], autouse=True)
def variant(request, monkeypatch, capfd):
    """Graphs up to SHK_THREAD_LDS_EDGES edges keep their set in LDS (if it fits): 0 sends every graph to global memory,
    a large number every graph that fits to LDS (all of this file's do: the 18S graph is the largest).  With SHK_TRACE
    set a launch says on stderr how many genes' sets lie where (the single call is a panel of one gene); `launched` checks
    that the one set was where the test meant it to be."""
    monkeypatch.setenv("SHK_THREAD_LDS_EDGES", "0" if request.param == "global" else "1000000")
    monkeypatch.setenv("SHK_TRACE", "1")
    for name in ("SHK_THREAD_PANEL_BLOCKS", "SHK_THREAD_PANEL_JOB"):
        monkeypatch.delenv(name, raising=False)
    _run.update(capfd=capfd, where="1 genes, %d jobs, %d blocks, " + ("0 genes in LDS, 1 genes in global memory" if request.param == "global"
                                                                      else "1 genes in LDS, 0 genes in global memory"))
    return request.param


def launched(n):
    """The launches since the last look: n of them, each of one gene with its set where the variant puts it → [(jobs, blocks)]."""
    lines = [x for x in _run["capfd"].readouterr().err.splitlines() if "thread_reads_panel:" in x]
    assert len(lines) == n, lines
    cuts = []
    for x in lines:
        jobs, blocks = int(x.split(" genes, ")[1].split()[0]), int(x.split(" jobs, ")[1].split()[0])
        assert x.endswith(_run["where"] % (jobs, blocks)), x
        cuts.append((jobs, blocks))
    return cuts


def to_device(bases, offsets):
    import torch
    db = torch.from_numpy(np.ascontiguousarray(bases, dtype=np.uint8).copy()).to("cuda:0")
    do = torch.from_numpy(np.ascontiguousarray(offsets).astype(np.int64)).to("cuda:0")
    torch.cuda.synchronize()
    return db, do


def graph_arrays(g):
    return (np.array(g.sub_kmer, dtype=np.uint64), np.array([e[0] for e in g.edges], dtype=np.uint32),
            np.array([e[1] for e in g.edges], dtype=np.uint32))


def check(eng, g, reads, k, read_index=None, mate=None, what=None, want=None, device=False):
    """want: the model's answer where the caller keeps it (the same batch under several cuts); device: the device form."""
    bases, offsets = eng._pack(reads)
    if device:
        bases, offsets = to_device(bases, offsets)
    launched(0)
    got = eng.thread_reads(graph_arrays(g), bases, offsets, read_index, mate, device=device)
    _run["cuts"] = launched(1 if g.edges and reads else 0)
    if want is not None:
        pass
    elif mate is None:
        want = ref.thread_reads(g, reads, k)
    else:
        want = ref.thread_reads_paired(g, reads, read_index, mate, k)
    tot, una, links, counts, read_edges = ref.as_arrays(want, len(g.edges))
    assert got.read_edges.tolist() == read_edges, what
    assert got.support_total.tolist() == tot, what
    assert got.support_unambiguous.tolist() == una, what
    assert got.links.tolist() == links and got.link_counts.tolist() == counts, what
    assert got.n_paired_links == want.n_paired_links, what
    return want


# ---- 1. crafted cases at k = 3 -------------------------------------------------------------------------------------------

def test_crafted_k3():
    with sa.KmerEngine(3, 1, 100) as eng:
        for name, g, reads in tc.crafted_cases():
            check(eng, g, reads, 3, what=name)
            check(eng, g, reads, 3, list(range(len(reads))), [1 + (i & 1) for i in range(len(reads))], what=name + " (paired)")


# ---- 2. the 18S chain at k = 21: tile edges and end to end ---------------------------------------------------------------

def case_18s():
    """The graph of pcr_extend on the padded 18S ×10 (as test_gpu_pcr_extend.py builds it), the sequence, and the start
    of its longest stretch of consecutive windows that are edges of the graph."""
    if "18s" not in _cache:
        seq = open(os.path.join(G, "pcr_18s_padded.txt")).read().strip()
        b = np.frombuffer(seq.encode() * 10, dtype=np.uint8).copy()
        o = np.arange(11, dtype=np.uint64) * np.uint64(len(seq))
        with sa.KmerEngine(21, 1, 100) as eng:
            eng.ingest_reads(b, o)
            eng.finalize()
            fwd, rev = eng.primer_pair_kmers(FWD_18S, REV_18S, trim=15, mismatches=2, min_count=3)
            pg = eng.pcr_extend(fwd, rev, min_count=5, table_min_count=1, sweep=False, max_num_nodes=500_000)
        g = ref.Graph(pg.node_sub_kmers.tolist(), list(zip(pg.edge_src.tolist(), pg.edge_tgt.tolist())))
        assert pg.found_path and len(g.edges) > 1700
        lookup = ref.build_edge_lookup(g, 21)
        kmers, _ = ref.kmers_from_ascii(seq.encode(), 21)
        best, at = (0, 0), 0
        while at < len(kmers):
            end = at
            while end < len(kmers) and kmers[end] in lookup:
                end += 1
            best = max(best, (end - at, at))
            at = end + 1
        assert best[0] > 4 * T
        _cache["18s"] = (seq, g, best[1], lookup)
    return _cache["18s"]


def test_18s_tile_edges():
    k = 21
    seq, g, a, lookup = case_18s()
    cut = lambda n_kmers, at=a: seq[at:at + n_kmers + k - 1].encode()  # noqa: E731
    with sa.KmerEngine(k, 1, 100) as eng:
        # reads of T−1, T, T+1 and 2T+1 k-mers, at two places; one with an N, one with an invalid byte in its last step
        reads = [cut(n, at) for n in (T - 1, T, T + 1, 2 * T + 1) for at in (a, a + 7)]
        reads.append(cut(2 * T + 1)[:-1] + b"X")
        reads.append(cut(2 * T + 1)[:T + 30] + b"N" + cut(2 * T + 1)[T + 31:])
        want = check(eng, g, reads, k, what="plain chain")
        assert want.read_edges[:8] == [T - 1, T - 1, T, T, T + 1, T + 1, 2 * T + 1, 2 * T + 1] and want.read_edges[8] == 0
        # a branch node behind element 2T − 1: the one branch pair of a 2T+1 read is (2T − 1, 2T), the last step's first
        # element with its predecessor in the step before; the first step's edges must gain no support_unambiguous
        e_in = lookup[ref.kmers_from_ascii(cut(2 * T), k)[0][2 * T - 1]][0]
        gb = ref.Graph(g.sub_kmer + [0], g.edges + [(g.edges[e_in][1], len(g.sub_kmer))])
        want = check(eng, gb, [cut(2 * T + 1), cut(2 * T - 1), cut(T, a + T + 3)], k, what="branch pair in the last step")
        e_out = lookup[ref.kmers_from_ascii(cut(2 * T + 1), k)[0][2 * T]][0]
        assert want.branch_links.get((e_in, e_out)) == 2
        first = lookup[ref.kmers_from_ascii(cut(1), k)[0][0]][0]
        assert want.support_total[first] == 2 and want.support_unambiguous.get(first, 0) < 2
        # a two-candidate key at element T, the first element of the second step: a twin of that edge from a second node
        # with the same sub_kmer goes in FRONT of the edge list, so candidate 0 is the wrong one and only the edge carried
        # over from the first step picks the right one
        e_t = lookup[ref.kmers_from_ascii(cut(T + 1), k)[0][T]][0]
        s, t = g.edges[e_t]
        gm = ref.Graph(g.sub_kmer + [g.sub_kmer[s]], [(len(g.sub_kmer), t)] + g.edges)
        want = check(eng, gm, [cut(2 * T + 1), cut(T + 1, a + T), cut(3, a + T - 1)], k, what="two candidates at a step's first element")
        assert want.events.get("resolved_by_adjacency_not_first", 0) >= 2 and want.support_total[0] == 1


def reads_18s():
    if "reads" not in _cache:
        seq = case_18s()[0]
        reads = []
        for i, at in enumerate(range(0, len(seq) - 150 + 1, 50)):
            for strand in (0, 1):
                b = bytearray(seq[at:at + 150].encode())
                n = len(reads)
                if n % 10 == 0:
                    b[40 + n % 60] = b"ACGT"[("ACGT".index(chr(b[40 + n % 60])) + 1) % 4]
                if n % 7 == 0:
                    b[20 + n % 100] = ord("N")
                reads.append(tc.rc_bytes(bytes(b)) if strand else bytes(b))
        _cache["reads"] = reads
    return _cache["reads"]


@pytest.mark.parametrize("paired", [False, True])
def test_18s_end_to_end(paired):
    """150-base windows at stride 50 over the sequence, both strands, every tenth with a substitution, every seventh with
    an N; unpaired, and as alternating R1 / R2 with n_paired_links."""
    seq, g, a, lookup = case_18s()
    reads = reads_18s()
    with sa.KmerEngine(21, 1, 100) as eng:
        if paired:
            want = check(eng, g, reads, 21, list(range(len(reads))), [1 + (i & 1) for i in range(len(reads))])
            assert want.n_paired_links > 10
        else:
            want = check(eng, g, reads, 21)
        assert sum(want.read_edges) > 2000


# ---- 3. the random sweep ---------------------------------------------------------------------------------------------------

def test_random_sweep():
    engines = {}
    try:
        for seed in tc.SWEEP_SEEDS:
            k, g, reads, read_index, mate = tc.random_case(seed, T)
            if k not in engines:
                engines[k] = sa.KmerEngine(k, 1, 100)
            check(engines[k], g, reads, k, what=("unpaired", seed))
            check(engines[k], g, reads, k, read_index, mate, what=("paired", seed))
    finally:
        for e in engines.values():
            e.close()


# ---- 4. the table is not touched -------------------------------------------------------------------------------------------

def test_table_untouched_mid_job():
    spec = sa.SynthSpec(genome_len=20_000, sub_per_64k=300, n_per_64k=60)
    b1, o1 = sa.synth_reads(spec, 0, 3000)
    b2, o2 = sa.synth_reads(spec, 3000, 3000)
    k, g, reads, _, _ = tc.random_case(3)

    def job(with_call):
        with sa.KmerEngine(k, 3, 100) as eng:
            eng.ingest_reads(b1, o1)
            if with_call:
                check(eng, g, reads, k)
                got = eng.thread_reads(graph_arrays(g), b1, o1)  # the job's own reads too: a batch of 3000
                assert got.read_edges.shape == (3000,)
                launched(1)
            eng.ingest_reads(b2, o2)
            eng.finalize()
            return eng.histograms(), eng.counters()

    h0, c0 = job(False)
    h1, c1 = job(True)
    assert np.array_equal(h0, h1)
    for name in ("n_reads_ingested", "n_bases_read", "n_bases_ingested", "n_kmers_ingested", "n_unique_kmers", "n_hashed_kmers",
                 "n_singleton_kmers"):
        assert c0[name] == c1[name], name


def test_owner_share_and_multi_device_and_device_buffers():
    import torch
    k, g, reads, read_index, mate = tc.random_case(5)
    with sa.KmerEngine(k, 1, 100, n_owners=2, owner_id=1) as eng:
        check(eng, g, reads, k, read_index, mate, what="owner share")
    with sa.KmerEngine(k, 1, 100, device_ids=[0, 0]) as eng:
        check(eng, g, reads, k, read_index, mate, what="multi-device")
    with sa.KmerEngine(k, 1, 100) as eng:
        bases, offsets = eng._pack(reads)
        db = torch.from_numpy(bases.copy()).to("cuda:0")
        do = torch.from_numpy(offsets.astype(np.int64)).to("cuda:0")
        torch.cuda.synchronize()
        got = eng.thread_reads(graph_arrays(g), db, do, device=True)
        launched(1)
        tot, una, links, counts, read_edges = ref.as_arrays(ref.thread_reads(g, reads, k), len(g.edges))
        assert (got.support_total.tolist(), got.support_unambiguous.tolist(), got.links.tolist(), got.link_counts.tolist(),
                got.read_edges.tolist()) == (tot, una, links, counts, read_edges)


# ---- 5. argument errors ------------------------------------------------------------------------------------------------------

def test_argument_errors_and_link_cap():
    import ctypes as C
    from sharkmer_amd.engine import _ThreadOut
    g = tc.branch_graph()
    sub, es, et = graph_arrays(g)
    reads = [b"AACG", b"AACGG"]
    with sa.KmerEngine(3, 1, 100) as eng:
        bases, offsets = eng._pack(reads)
        bad = [
            dict(graph=(sub, np.array([0, 1, 4], dtype=np.uint32), et)),              # a source ≥ n_nodes
            dict(graph=(sub, es, np.array([1, 2, 4], dtype=np.uint32))),              # a target ≥ n_nodes
            dict(graph=(np.array([0, 1, 6, 16], dtype=np.uint64), es, et)),           # a sub_kmer above (1 << 2(k−1)) − 1
            dict(offsets=np.array([0, 5, 4], dtype=np.uint64)),                       # decreasing offsets
            dict(read_index=[0, 1]),                                                  # one of the two alone
            dict(mate=[1, 2]),
            dict(read_index=[0, 1], mate=[1, 3]),                                     # mate > 2
        ]
        for kw in bad:
            a = dict(graph=(sub, es, et), bases=bases, offsets=offsets)
            a.update(kw)
            with pytest.raises(sa.ShkError) as e:
                eng.thread_reads(**a)
            assert e.value.code == -2, kw
        # n_nodes / n_edges ≥ 2^32 (refused before any array is read)
        tot = np.zeros(4, dtype=np.uint32)
        out = _ThreadOut(tot.ctypes.data, tot.ctypes.data, None, None, None, 0, 0, None, 0)
        for nn, ne in ((1 << 32, 3), (4, 1 << 32)):
            rc = eng._L.shk_thread_reads(eng._h, sub.ctypes.data, nn, es.ctypes.data, et.ctypes.data, ne, bases.ctypes.data,
                                         offsets.ctypes.data, 2, None, None, C.byref(out))
            assert rc == -2
        # link_cap: AA → AC → {CC, CA}; the two reads cross the branch node AC by (0, 1) and (0, 2) — no room, room for
        # one, room for both
        sub, es, et = graph_arrays(tc.graph_of(["AA", "AC", "CC", "CA"], [(0, 1), (1, 2), (1, 3)]))
        bases, offsets = eng._pack([b"AACC", b"AACA"])
        li, lo, lc = (np.zeros(2, dtype=np.uint32) for _ in range(3))
        tot, una = np.zeros(3, dtype=np.uint32), np.zeros(3, dtype=np.uint32)
        for cap in (0, 1, 2):
            out = _ThreadOut(tot.ctypes.data, una.ctypes.data, li.ctypes.data, lo.ctypes.data, lc.ctypes.data, cap, 0, None, 0)
            rc = eng._L.shk_thread_reads(eng._h, sub.ctypes.data, 4, es.ctypes.data, et.ctypes.data, 3, bases.ctypes.data,
                                         offsets.ctypes.data, 2, None, None, C.byref(out))
            assert (rc, out.n_links) == (-2 if cap < 2 else 0, 2), cap
        assert (li.tolist(), lo.tolist(), lc.tolist()) == ([0, 0], [1, 2], [1, 1])
        assert tot.tolist() == [2, 1, 1] and una.tolist() == [0, 0, 0]
    with sa.KmerEngine(1, 1, 100) as eng:  # k < 2: a node would be a 0-mer
        with pytest.raises(sa.ShkError) as e:
            eng.thread_reads((np.zeros(1, dtype=np.uint64), np.zeros(1, dtype=np.uint32), np.zeros(1, dtype=np.uint32)),
                             *eng._pack([b"ACGT"]))
        assert e.value.code == -2 and "k >= 2" in e.value.msg


# ---- 6. the panel's cuts under the single call -------------------------------------------------------------------------------

TAIL_SIZES = (1, 15, 16, 17, 33)  # a job tail on both sides of the 16 waves of a workgroup; 33: two full slices and one read
_tails, _paired = {}, {}


def tail_batches():
    """Per crafted k = 3 case that has edges and reads, and per size: the case's reads taken round and round up to that
    many, and the model's answer — computed once, the same under every cut."""
    if not _tails:
        for name, g, reads in tc.crafted_cases():
            if g.edges and reads:
                for n in TAIL_SIZES:
                    batch = [reads[i % len(reads)] for i in range(n)]
                    _tails[name, n] = (g, batch, ref.thread_reads(g, batch, 3))
    return _tails


def paired_batch():
    """Mates 0 / 1 / 2 mixed over the branch graph; a read of fewer than k bases and an empty one as somebody's mate.  Pair
    p is reads 2p and 2p + 1: only pair 0 has an R1 and an R2 that both map."""
    if not _paired:
        g = tc.branch_graph()
        reads = [b"AACG", b"ACG", b"AA", b"AACGG", b"TTTT", b"AAC", b"AACG", tc.rc_bytes(b"AACG"), b"AAC", b"", b"ACG", b"AACG", b"AACGG"]
        mate = [1, 2, 1, 2, 1, 2, 0, 0, 1, 2, 2, 2, 0]
        read_index = list(range(len(reads)))
        want = ref.thread_reads_paired(g, reads, read_index, mate, 3)
        assert want.n_paired_links == 1 and want.read_edges[2] == 0 and sum(1 for x in want.read_edges if x) >= 8
        _paired["batch"] = (g, reads, read_index, mate, want)
    return _paired["batch"]


@pytest.mark.parametrize("blocks", ["1", "2", None])
@pytest.mark.parametrize("job", ["1", "5", None])
def test_job_tails_and_block_caps_under_the_single_call(monkeypatch, job, blocks):
    """SHK_THREAD_PANEL_JOB and SHK_THREAD_PANEL_BLOCKS cut the single call as they cut a panel: every batch of
    tail_batches and the paired batch (host and device form) under job sizes 1, 5 and the default 16 and 1, 2 and
    unbounded workgroups, against the model, every array."""
    if blocks:
        monkeypatch.setenv("SHK_THREAD_PANEL_BLOCKS", blocks)
    if job:
        monkeypatch.setenv("SHK_THREAD_PANEL_JOB", job)
    per_job = int(job or 16)
    with sa.KmerEngine(3, 1, 100) as eng:
        for (name, n), (g, batch, want) in tail_batches().items():
            check(eng, g, batch, 3, what=(name, n, job, blocks), want=want)
            ((n_jobs, n_blocks),) = _run["cuts"]
            assert n_jobs == (n + per_job - 1) // per_job and 1 <= n_blocks <= min(n_jobs, int(blocks or n_jobs))
        g, reads, read_index, mate, want = paired_batch()
        for device in (False, True):
            check(eng, g, reads, 3, read_index, mate, what=("paired", job, blocks, device), want=want, device=device)
