"""GPU tests of shk_pcr_prune_panel (K_PRUNE) against tests/prune_ref.py, the reference's remove_low_coverage_tips /
reachability_pruning / annotate_coverage_ratios restated literally: the crafted graphs of tests/prune_cases.py one gene
per call and all in one panel, with the genes in LDS and in global memory; real extension output handed on to
shk_thread_reads_panel; capacities, errors and states.  Everything is compared as arrays, doubles bit for bit."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import sharkmer_amd as sa
import pcr_panel_cases as pc
import prune_cases as pcs
import prune_ref as ref
from sharkmer_amd.engine import _PcrPruneOut, _PcrPruneParams

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FWD_18S, REV_18S = "AACCTGGTTGATCCTGCCAGT", "TGATCCTTCTGCAGGTTCACCTAC"
MODES = {"default": None, "global": "0", "lds": str(1 << 30)}  # SHK_PRUNE_LDS_NODES


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64).tolist()


def assert_pruned(got, arrays, want, what):
    """got: a PrunedGraph; arrays: the graph that went in; want: prune_ref.Pruned."""
    sub = arrays[0]
    assert got.node_keep.tolist() == want.node_keep, what
    assert got.node_index.tolist() == want.node_index, what
    assert got.node_flags.tolist() == want.node_flags, what
    assert got.node_sub_kmers.tolist() == [int(sub[v]) for v in want.node_index], what
    assert got.edge_index.tolist() == want.edge_index, what
    assert got.edge_src.tolist() == want.edge_src and got.edge_tgt.tolist() == want.edge_tgt, what
    assert got.edge_counts.tolist() == want.edge_counts, what
    assert bits(got.coverage_ratio) == bits(want.coverage_ratio), what
    assert bits([got.median]) == bits([want.median]), what
    assert (got.tip_rounds, got.tips_removed, got.unreachable_removed) == (want.tip_rounds, want.tips_removed, want.unreachable_removed), what


def trace_lines(capfd):
    """The calls since the last look → [(genes, in LDS, in global memory)]."""
    return [tuple(int(x) for x in m.groups())
            for m in re.finditer(r"pcr_prune_panel: (\d+) genes, (\d+) genes in LDS \(\d+ bytes\), (\d+) genes in global memory",
                                 capfd.readouterr().err)]


@pytest.fixture(scope="module")
def engines():
    """Contexts that hold nothing: the call needs no table.  One per k of the cases."""
    e = {k: sa.KmerEngine(k, 1, 100) for k in (3, pcs.K)}
    yield e
    for x in e.values():
        x.close()


@pytest.mark.parametrize("mode", list(MODES))
def test_cases_alone_and_in_one_panel(engines, mode, monkeypatch, capfd):
    monkeypatch.setenv("SHK_TRACE", "1")
    if MODES[mode] is None:
        monkeypatch.delenv("SHK_PRUNE_LDS_NODES", raising=False)
    else:
        monkeypatch.setenv("SHK_PRUNE_LDS_NODES", MODES[mode])
    for k, eng in engines.items():
        cases = [c for c in pcs.cases() if c.k == k]
        assert cases
        capfd.readouterr()
        for c in cases:
            got = eng.pcr_prune(c.arrays(), c.fraction, c.stages)
            assert_pruned(got, c.arrays(), c.expected(), (mode, c.name, "alone"))
        alone = trace_lines(capfd)
        got = eng.pcr_prune_panel([c.arrays() for c in cases], [c.fraction for c in cases], [c.stages for c in cases])
        assert len(got) == len(cases)
        for c, g in zip(cases, got):
            assert_pruned(g, c.arrays(), c.expected(), (mode, c.name, "panel"))
        (panel,) = trace_lines(capfd)
        n_real = sum(1 for c in cases if c.flags)
        assert panel[0] == len(cases) and panel[1] + panel[2] == n_real
        if mode == "global":
            assert panel[1] == 0 and all(a[1] == 0 for a in alone)
        if mode == "lds":  # whatever fits 79 KiB: the width and depth cases do not
            small = sum(1 for c in cases if c.flags and 24 * len(c.flags) + 8 + 8 * len(c.edges) + 8 * ((len(c.edges) + 31) // 32) <= 79 << 10)
            assert panel[1] == small and (k != pcs.K or 0 < small < n_real)


@pytest.mark.parametrize("mode", list(MODES))
def test_more_genes_than_workgroups(engines, mode, monkeypatch):
    if MODES[mode] is not None:
        monkeypatch.setenv("SHK_PRUNE_LDS_NODES", MODES[mode])
    eng = engines[pcs.K]
    genes = pcs.many_genes()
    got = eng.pcr_prune_panel([g.arrays() for g in genes])
    assert len(got) == len(genes)
    for c, g in zip(genes, got):
        assert_pruned(g, c.arrays(), c.expected(), (mode, c.name))
    if mode == "default":
        for c in genes:
            assert_pruned(eng.pcr_prune(c.arrays()), c.arrays(), c.expected(), (c.name, "alone"))


def graph_tuple(g):
    return (g.node_sub_kmers, g.node_flags, g.edge_src, g.edge_tgt, g.edge_counts)


def model_of(g, k, fraction=0.1):
    return ref.prune(g.node_flags.tolist(), g.edge_src.tolist(), g.edge_tgt.tolist(), g.edge_counts.tolist(), k, fraction, 3)


def ann_rows(a):
    return (a.support_total.tolist(), a.support_unambiguous.tolist(), a.links.tolist(), a.link_counts.tolist(), a.read_edges.tolist())


def chain(eng, graphs, k, bases, offsets, lists):
    """extend's graphs → pcr_prune_panel equals the model → thread_reads_panel on the PrunedGraphs equals thread_reads on
    the model-pruned graph, gene by gene → per gene (pruned annotation rows, the model's answer)."""
    pruned = eng.pcr_prune_panel(graphs)
    wants = [model_of(g, k) for g in graphs]
    for i, (g, p, w) in enumerate(zip(graphs, pruned, wants)):
        assert_pruned(p, graph_tuple(g), w, i)
    anns = eng.thread_reads_panel(pruned, bases, offsets, lists)
    for i, (g, w, ids) in enumerate(zip(graphs, wants, lists)):
        sub = np.concatenate([bases[int(offsets[r]):int(offsets[r + 1])] for r in ids])
        off = np.concatenate([[0], np.cumsum([int(offsets[r + 1] - offsets[r]) for r in ids])]).astype(np.uint64)
        model_graph = (g.node_sub_kmers[w.node_index] if w.node_index else np.zeros(0, np.uint64), np.array(w.edge_src, np.uint32),
                       np.array(w.edge_tgt, np.uint32))
        assert ann_rows(anns[i]) == ann_rows(eng.thread_reads(model_graph, sub, off)), i
    return pruned, wants, anns


def test_18s_chain(orc):
    """The padded 18S ×10 at k 21: a chain about 1800 levels deep through extension, pruning and threading."""
    seq = open(os.path.join(G, "pcr_18s_padded.txt")).read().strip()
    bases = np.frombuffer(seq.encode() * 10, dtype=np.uint8).copy()
    offsets = np.arange(11, dtype=np.uint64) * np.uint64(len(seq))
    params = [dict(min_count=3, table_min_count=1, sweep=True, max_num_nodes=500_000),
              dict(min_count=5, table_min_count=1, sweep=False, max_num_nodes=500_000)]
    with sa.KmerEngine(21, 1, 100) as eng:
        eng.ingest_reads(bases, offsets)
        eng.finalize()
        prim = eng.primer_kmers([sa.Primer(s, trim=15, mismatches=2, min_count=3) for s in (FWD_18S, REV_18S) * 2])
        graphs = eng.pcr_extend_panel(prim, params)
        assert all(g.found_path and len(g.node_sub_kmers) > 1700 for g in graphs)
        pruned, wants, anns = chain(eng, graphs, 21, bases, offsets, [list(range(10))] * 2)
    assert all(len(p.node_sub_kmers) > 1700 and p.median > 0 for p in pruned)
    assert all(int(a.support_total.sum()) > 0 for a in anns)


def test_mixed_panel_chain(orc):
    """The mixed panel of pcr_panel_cases.py; and the gap the call closes: for some gene, threading the pruned graph is
    not threading the unpruned one, even on the edges that survive."""
    p = pc.mixed_panel(orc)
    n = 300
    bases, offsets = p.bases[:int(p.offsets[n])], p.offsets[:n + 1]
    with sa.KmerEngine(p.k, 1, 100) as eng:
        eng.ingest_reads(p.bases, p.offsets)
        eng.finalize()
        prim = eng.primer_kmers([sa.Primer(s, **pc.PRIMER) for g in p.genes for s in (g.forward, g.reverse)])
        graphs = eng.pcr_extend_panel(prim, [g.params for g in p.genes])
        lists = [list(range(i % 3, n, 3)) if len(g.edge_src) else [0, 1] for i, g in enumerate(graphs)]
        pruned, wants, anns = chain(eng, graphs, p.k, bases, offsets, lists)
        unpruned = eng.thread_reads_panel(graphs, bases, offsets, lists)
    differ = []
    for i, (pg, a, u) in enumerate(zip(pruned, anns, unpruned)):
        keep = pg.edge_index
        new = {int(e): j for j, e in enumerate(keep)}
        links = [([new[int(x)], new[int(y)]], int(c)) for (x, y), c in zip(u.links, u.link_counts) if int(x) in new and int(y) in new]
        on_survivors = (u.support_total[keep].tolist(), u.support_unambiguous[keep].tolist(), [x[0] for x in links], [x[1] for x in links])
        if on_survivors != ann_rows(a)[:4]:
            differ.append(p.genes[i].name)
    # in this panel a gene stays whole or goes whole: on surviving edges nothing can differ (test_threaded_gene has a tip)
    assert not differ
    gone = [i for i, (x, y) in enumerate(zip(graphs, pruned)) if len(x.edge_src) and not len(y.edge_src)]
    assert {p.genes[i].name for i in gone} >= {"never found", "budget"}
    for i in gone:  # an off-target component that survived: reads were threaded through it, and now are not
        assert ann_rows(unpruned[i]) != ann_rows(anns[i])
        assert int(unpruned[i].support_total.sum()) > 0 and int(unpruned[i].read_edges.sum()) > 0
        assert anns[i].support_total.size == 0 and not anns[i].read_edges.any()


def test_threaded_gene():
    """A low tip off a real path, with the reads that made it: pruned and threaded, the branch links at the tip's root
    are gone and the reads through it are unambiguous — on edges that survive, not what the unpruned graph gives."""
    t = pcs.threaded_gene()
    c = t.case
    arrays = (t.sub_kmers,) + c.arrays()[1:]
    with sa.KmerEngine(c.k, 1, 100) as eng:
        bases, offsets = eng._pack(t.reads)
        ids = list(range(len(t.reads)))
        (pg,) = eng.pcr_prune_panel([arrays])
        assert_pruned(pg, arrays, c.expected(), c.name)
        (a,) = eng.thread_reads_panel([pg], bases, offsets, [ids])
        (u,) = eng.thread_reads_panel([arrays[:1] + arrays[2:4]], bases, offsets, [ids])
        want = c.expected()
        model_graph = (t.sub_kmers[want.node_index], np.array(want.edge_src, np.uint32), np.array(want.edge_tgt, np.uint32))
        assert ann_rows(a) == ann_rows(eng.thread_reads(model_graph, bases, offsets))
    keep = pg.edge_index
    assert len(u.links) > 0 and len(a.links) == 0
    assert u.support_total[keep].tolist() == a.support_total.tolist()
    assert u.support_unambiguous[keep].tolist() != a.support_unambiguous.tolist()


def raw_call(eng, graphs, fractions, stages, node_cap, edge_cap, noff=None, eoff=None, n_genes=None):
    """shk_pcr_prune_panel as C sees it → (rc, message, out offsets ×2, node_keep, counters ×3, median)."""
    ng = len(graphs) if n_genes is None else n_genes
    cat = lambda i, dt: np.concatenate([np.asarray(g[i], dtype=dt) for g in graphs]) if graphs else np.zeros(0, dt)
    sub, fl, es, et, ec = cat(0, np.uint64), cat(1, np.uint8), cat(2, np.uint32), cat(3, np.uint32), cat(4, np.uint32)
    if noff is None:
        noff = np.concatenate([[0], np.cumsum([len(g[1]) for g in graphs])]).astype(np.uint64)
    if eoff is None:
        eoff = np.concatenate([[0], np.cumsum([len(g[2]) for g in graphs])]).astype(np.uint64)
    prm = (_PcrPruneParams * max(len(fractions), 1))(*[_PcrPruneParams(f, s, 0) for f, s in zip(fractions, stages)])
    keep = np.full(max(len(sub), 1), 9, np.uint8)
    ono, oeo = np.full(max(ng, 0) + 1, 77, np.uint64), np.full(max(ng, 0) + 1, 77, np.uint64)
    osub, ofl, oni = np.zeros(max(node_cap, 1), np.uint64), np.zeros(max(node_cap, 1), np.uint8), np.zeros(max(node_cap, 1), np.uint32)
    oes, oet, oec, oei = (np.zeros(max(edge_cap, 1), np.uint32) for _ in range(4))
    ratio = np.zeros(max(edge_cap, 1), np.float64)
    med = np.full(max(ng, 1), -1.0, np.float64)
    rounds, tips, unreach = (np.full(max(ng, 1), 99, np.uint32) for _ in range(3))
    out = _PcrPruneOut(keep.ctypes.data, ono.ctypes.data, oeo.ctypes.data, osub.ctypes.data, ofl.ctypes.data, oni.ctypes.data, node_cap,
                       oes.ctypes.data, oet.ctypes.data, oec.ctypes.data, oei.ctypes.data, ratio.ctypes.data, edge_cap, med.ctypes.data,
                       rounds.ctypes.data, tips.ctypes.data, unreach.ctypes.data, 0.0)
    rc = eng._L.shk_pcr_prune_panel(eng._h, sub.ctypes.data, fl.ctypes.data, noff.ctypes.data, es.ctypes.data, et.ctypes.data, ec.ctypes.data,
                                    eoff.ctypes.data, ng, C.cast(prm, C.c_void_p), C.byref(out))
    return rc, eng._L.shk_last_error(eng._h).decode(), ono, oeo, keep, rounds, tips, unreach, med


PICK = ("tips of k-1", "no edges", "starts and ends", "cycle on the path")


def test_caps_report_the_need(engines):
    eng = engines[pcs.K]
    cases = [pcs.case(n) for n in PICK]
    wants = [c.expected() for c in cases]
    graphs = [c.arrays() for c in cases]
    fr, st = [c.fraction for c in cases], [c.stages for c in cases]
    n_off = [0] + np.cumsum([len(w.node_index) for w in wants]).tolist()
    e_off = [0] + np.cumsum([len(w.edge_index) for w in wants]).tolist()
    nn, ne = n_off[-1], e_off[-1]
    assert nn > 1 and ne > 1
    for node_cap, edge_cap in ((0, 0), (nn - 1, ne), (nn, ne - 1)):
        rc, msg, ono, oeo, keep, rounds, tips, unreach, med = raw_call(eng, graphs, fr, st, node_cap, edge_cap)
        assert rc == -2 and "does not fit" in msg, (node_cap, edge_cap)
        assert ono.tolist() == n_off and oeo.tolist() == e_off
        assert keep.tolist() == [x for w in wants for x in w.node_keep]
        assert (rounds.tolist(), tips.tolist(), unreach.tolist()) == ([w.tip_rounds for w in wants], [w.tips_removed for w in wants],
                                                                      [w.unreachable_removed for w in wants])
        assert bits(med) == bits([w.median for w in wants])
    rc, msg, ono, oeo, keep, *_ = raw_call(eng, graphs, fr, st, nn, ne)
    assert rc == 0 and ono.tolist() == n_off and oeo.tolist() == e_off
    # the wrapper's first guess too small for what the panel keeps: it retries once, at the need
    big = pcs.case("width 1025")
    assert len(big.flags) > 1000
    with sa.KmerEngine(pcs.K, 1, 100) as small:
        small.prune_first_cap = 1000
        twice = small.pcr_prune_panel([big.arrays()] * 2, stages=1)
        assert all(len(g.node_index) == len(big.flags) and g.unreachable_removed == 0 for g in twice)
        (one,) = small.pcr_prune_panel([big.arrays()])
        assert_pruned(one, big.arrays(), big.expected(), "retry")


def test_errors_name_the_gene(engines):
    eng = engines[pcs.K]
    good = [pcs.case(n).arrays() for n in ("late dead end", "self-loop", "cycle on the path")]
    fr, st = [0.1] * 3, [3] * 3

    def bad(graphs=good, fractions=fr, stages=st, **kw):
        rc, msg, *_ = raw_call(eng, graphs, fractions, stages, 1 << 12, 1 << 12, **kw)
        assert rc == -2, msg
        return msg

    g = [list(x) for x in good]
    g[1][2] = g[1][2].copy()
    g[1][2][0] = len(g[1][1])  # a source one past the gene's nodes
    assert "gene 1" in bad(g) and "endpoint" in bad(g)
    g = [list(x) for x in good]
    g[2][3] = g[2][3].copy()
    g[2][3][-1] = 0xFFFFFFFF
    assert "gene 2" in bad(g)
    g = [list(x) for x in good]
    g[0][1] = g[0][1].copy()
    g[0][1][1] = 4
    assert "gene 0" in bad(g) and "flags" in bad(g)
    n = [len(x[1]) for x in good]
    e = [len(x[2]) for x in good]
    assert "gene 1" in bad(noff=np.array([0, n[0] + n[1], n[0], sum(n)], np.uint64)) and "node_offsets" in bad(
        noff=np.array([0, n[0] + n[1], n[0], sum(n)], np.uint64))
    msg = bad(eoff=np.array([0, e[0], e[0] + e[1], e[0]], np.uint64))
    assert "gene 2" in msg and "edge_offsets" in msg
    msg = bad(fractions=[0.1, float("nan"), 0.1])
    assert "gene 1" in msg and "NaN" in msg
    msg = bad(stages=[3, 3, 4])
    assert "gene 2" in msg and "stages" in msg
    msg = bad(graphs=[], fractions=[], stages=[], n_genes=4097, noff=np.zeros(2, np.uint64), eoff=np.zeros(2, np.uint64))
    assert "4097" in msg
    msg = bad(graphs=[], fractions=[0.1], stages=[3], n_genes=1, noff=np.array([0, 1 << 32], np.uint64), eoff=np.zeros(2, np.uint64))
    assert "2^32" in msg and "gene 0" in msg
    msg = bad(graphs=[], fractions=[0.1], stages=[3], n_genes=1, noff=np.zeros(2, np.uint64), eoff=np.array([0, 1 << 32], np.uint64))
    assert "2^32" in msg
    # infinities are numbers: +inf removes every short tip, −inf leaves min_tip at 1.0
    c = pcs.case("fraction 1e12")
    for f in (float("inf"), float("-inf")):
        want = ref.prune(c.flags, *zip(*c.edges), c.k, f, c.stages)
        assert_pruned(eng.pcr_prune(c.arrays(), f, c.stages), c.arrays(), want, f)


def test_no_genes_and_states(orc):
    """n_genes == 0; the table and histograms are left alone; a two-device context and an owner share answer alike."""
    cases = [pcs.case(n) for n in ("tips of k-1", "starts and ends", "width 1023", "no edges")]
    graphs = [c.arrays() for c in cases]
    fr, st = [c.fraction for c in cases], [c.stages for c in cases]
    spec = sa.SynthSpec(genome_len=5000, sub_per_64k=300, n_per_64k=60)
    bases, offsets = sa.synth_reads(spec, 0, 400)
    with sa.KmerEngine(pcs.K, 1, 100) as eng:
        assert eng.pcr_prune_panel([]) == []
        rc, msg, ono, oeo, *_ = raw_call(eng, [], [], [], 0, 0)
        assert rc == 0 and ono.tolist() == [0] and oeo.tolist() == [0]
        eng.ingest_reads(bases, offsets)
        mid = eng.pcr_prune_panel(graphs, fr, st)  # between ingest and finalize
        eng.finalize()
        before = (eng.export_table(), eng.histograms().copy())
        plain = eng.pcr_prune_panel(graphs, fr, st)
        after = (eng.export_table(), eng.histograms())
        assert np.array_equal(before[0][0], after[0][0]) and np.array_equal(before[0][1], after[0][1]) and np.array_equal(before[1], after[1])
    for c, a, b in zip(cases, plain, mid):
        assert_pruned(a, c.arrays(), c.expected(), c.name)
        assert_pruned(b, c.arrays(), c.expected(), (c.name, "before finalize"))
    with sa.KmerEngine(pcs.K, 1, 100, device_ids=[0, 0]) as multi:
        for c, a in zip(cases, multi.pcr_prune_panel(graphs, fr, st)):
            assert_pruned(a, c.arrays(), c.expected(), (c.name, "two devices"))
    with sa.KmerEngine(pcs.K, 1, 100, n_owners=2, owner_id=1) as share:
        for c, a in zip(cases, share.pcr_prune_panel(graphs, fr, st)):
            assert_pruned(a, c.arrays(), c.expected(), (c.name, "owner share"))
