"""All four read walkers on ONE batch per k (tests/read_walk_cases.py): shk_filter_reads, shk_kmers_from_reads,
shk_filter_reads_panel (host and device form) and shk_thread_reads, the last two with the lookup set in LDS and in global
memory.  They share the byte decoding, the canonical key of a window, the probe of the lookup set and the key runs behind
it, so they are held to each other and to the oracle where those can go wrong: reads that end either side of the
64-window step, an N or an invalid byte either side of it, the only hit in window 63, 64 or the last.  Everything is
integers and compared for equality."""
import numpy as np
import pytest

import sharkmer_amd as sa
import read_walk_cases as rw
import thread_ref as ref

pytestmark = pytest.mark.gpu

SET_WHERE = {"lds": "LDS", "global": "global memory"}


def to_device(bases, offsets):
    import torch
    db = torch.from_numpy(np.ascontiguousarray(bases, dtype=np.uint8).copy()).to("cuda:0")
    do = torch.from_numpy(np.ascontiguousarray(offsets).astype(np.int64)).to("cuda:0")
    torch.cuda.synchronize()
    return db, do


def trace(capfd, what):
    return [x for x in capfd.readouterr().err.splitlines() if what in x]


@pytest.mark.parametrize("k", rw.KS)
def test_filter_reads_and_kmers_from_reads_against_the_oracle(orc, k):
    b = rw.batch(orc, k)
    with sa.KmerEngine(k, 1, 10) as eng:
        bases, offsets = eng._pack(b.reads)
        flags = eng.filter_reads(bases, offsets, b.set_kmers)
        got, bad = eng.kmers_from_reads(bases, offsets)
    assert flags.tolist() == rw.expected_matches(orc, b)
    want = rw.expected_kmers(orc, b)
    assert bad.tolist() == [w[1] for w in want]
    for i, (kmers, _) in enumerate(want):
        assert got[i].tolist() == kmers, b.names[i]


@pytest.mark.parametrize("where", ["lds", "global"])
@pytest.mark.parametrize("k", rw.KS)
def test_panel_of_one_gene_equals_filter_reads(orc, k, where, monkeypatch, capfd):
    if where == "global":
        monkeypatch.setenv("SHK_FILTER_LDS_KEYS", "0")
    else:
        monkeypatch.delenv("SHK_FILTER_LDS_KEYS", raising=False)
    monkeypatch.setenv("SHK_TRACE", "1")
    b = rw.batch(orc, k)
    with sa.KmerEngine(k, 1, 10) as eng:
        bases, offsets = eng._pack(b.reads)
        flags = eng.filter_reads(bases, offsets, b.set_kmers)
        trace(capfd, "filter_panel:")
        host = eng.filter_reads_panel(bases, offsets, [b.set_kmers])
        db, do = to_device(bases, offsets)
        dev = eng.filter_reads_panel(db, do, [b.set_kmers], device=True)
    lines = trace(capfd, "filter_panel:")
    assert len(lines) == 2 and all(" in " + SET_WHERE[where] + "," in x for x in lines), lines
    assert flags.tolist() == rw.expected_matches(orc, b)
    assert [r.tolist() for r in host] == [np.flatnonzero(flags).tolist()]
    assert [r.tolist() for r in dev] == [np.flatnonzero(flags).tolist()]


@pytest.mark.parametrize("where", ["lds", "global"])
@pytest.mark.parametrize("k", rw.KS)
def test_thread_reads_over_a_chain_cut_from_a_read(orc, k, where, monkeypatch, capfd):
    monkeypatch.setenv("SHK_THREAD_LDS_EDGES", "0" if where == "global" else "1000000")
    monkeypatch.setenv("SHK_TRACE", "1")
    b = rw.batch(orc, k)
    nodes, edges, edge_kmers, _ = rw.linear_graph(b)
    g = ref.Graph(nodes, edges)
    canon = sorted(set(orc.kmers_from_ascii(x, k)[0] for x in edge_kmers))
    graph = (np.array(nodes, dtype=np.uint64), np.array([e[0] for e in edges], dtype=np.uint32),
             np.array([e[1] for e in edges], dtype=np.uint32))
    with sa.KmerEngine(k, 1, 10) as eng:
        bases, offsets = eng._pack(b.reads)
        trace(capfd, "thread_reads_panel:")
        got = eng.thread_reads(graph, bases, offsets)
        lines = trace(capfd, "thread_reads_panel:")  # (the single call is the panel of one gene, and says so)
        flags = eng.filter_reads(bases, offsets, canon)
    assert len(lines) == 1 and " 1 genes, " in lines[0] and " 1 genes in " + SET_WHERE[where] in lines[0], lines
    tot, una, links, counts, read_edges = ref.as_arrays(ref.thread_reads(g, b.reads, k), len(edges))
    assert got.read_edges.tolist() == read_edges
    assert got.support_total.tolist() == tot
    assert got.support_unambiguous.tolist() == una
    assert got.links.tolist() == links and got.link_counts.tolist() == counts
    assert (got.read_edges > 0).tolist() == flags.tolist()
    assert flags.tolist() == rw.expected_matches(orc, b, canon)
