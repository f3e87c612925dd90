"""GPU tests of shk_pcr_extend_panel: every gene of a panel call against the same gene alone through shk_pcr_extend and
against tests/pcr_ref.py (the reference's create_seed_graph / extend_graph / threshold sweep restated literally), on the
18S case and the mixed panel of tests/pcr_panel_cases.py; the hand-over to shk_thread_reads_panel; capacities and errors.
Everything is compared as arrays, order included."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import sharkmer_amd as sa
import pcr_panel_cases as pc
import pcr_ref as ref
from sharkmer_amd.engine import _PcrExtendParams

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FWD_18S, REV_18S = "AACCTGGTTGATCCTGCCAGT", "TGATCCTTCTGCAGGTTCACCTAC"


def assert_graph(got, want, used, steps, what=None):
    g = want
    assert list(got.node_sub_kmers) == g.sub_kmer, what
    assert list(got.node_flags) == g.flags(), what
    assert list(got.edge_src) == [e[0] for e in g.edges], what
    assert list(got.edge_tgt) == [e[1] for e in g.edges], what
    assert list(got.edge_counts) == [e[2] for e in g.edges], what
    assert (got.found_path, got.threshold_used, got.steps_run) == (g.found_path, used, steps), what


def same_graph(a, b):
    return (all(np.array_equal(getattr(a, f), getattr(b, f)) for f in ("node_sub_kmers", "node_flags", "edge_src", "edge_tgt", "edge_counts"))
            and (a.found_path, a.threshold_used, a.steps_run) == (b.found_path, b.threshold_used, b.steps_run))


def test_18s_three_times(orc):
    """The padded 18S ×10 at k 21 as a panel of that gene three times: min_count 3 under the sweep, 5 and 5 without —
    chains about 1800 levels deep, side by side."""
    seq = open(os.path.join(G, "pcr_18s_padded.txt")).read().strip()
    bases = np.frombuffer(seq.encode() * 10, dtype=np.uint8).copy()
    offsets = np.arange(11, dtype=np.uint64) * np.uint64(len(seq))
    run = orc.run_batch(bases, offsets, 21, 1, 100)
    table = ref.table_dict(*run.merged().export())
    params = [dict(min_count=3, table_min_count=1, sweep=True, max_num_nodes=ref.DEFAULT_MAX_NUM_NODES),
              dict(min_count=5, table_min_count=1, sweep=False, max_num_nodes=ref.DEFAULT_MAX_NUM_NODES),
              dict(min_count=5, table_min_count=1, sweep=False, max_num_nodes=ref.DEFAULT_MAX_NUM_NODES)]
    with sa.KmerEngine(21, 1, 100) as eng:
        eng.ingest_reads(bases, offsets)
        eng.finalize()
        prim = eng.primer_kmers([sa.Primer(s, trim=15, mismatches=2, min_count=3) for s in (FWD_18S, REV_18S) * 3])
        got = eng.pcr_extend_panel(prim, params)
        alone = [eng.pcr_extend(prim[2 * g], prim[2 * g + 1], **params[g]) for g in range(3)]
    assert len(got) == 3
    for g in range(3):
        p = params[g]
        want, used, steps = ref.pcr_extend(prim[2 * g][:2], prim[2 * g + 1][:2], table, 21, p["min_count"], 1, 10.0,
                                           p["max_num_nodes"], p["sweep"])
        assert want.found_path and len(want.sub_kmer) > 1700
        assert_graph(got[g], want, used, steps, g)
        assert same_graph(got[g], alone[g]), g
    assert same_graph(got[1], got[2])


@pytest.fixture(scope="module")
def mixed(orc):
    p = pc.mixed_panel(orc)
    eng = sa.KmerEngine(p.k, 1, 100)
    eng.ingest_reads(p.bases, p.offsets)
    eng.finalize()
    prim = eng.primer_kmers([sa.Primer(s, **pc.PRIMER) for g in p.genes for s in (g.forward, g.reverse)])
    for a, b in zip(prim, p.sets):  # the library's primer sets are the model's: the panel keeps its properties
        assert list(a[0]) == list(b[0]) and list(a[1]) == list(b[1])
    yield p, eng, prim
    eng.close()


def test_mixed_panel(mixed, monkeypatch, capfd):
    """Every way a sweep can end, in one call; then the same call under every tuning variable: none changes an array.
    The library's SHK_PCR_PANEL_TRACE line says how many rounds and launches a call took: a small panel budget must
    have cut rounds into several launches, the default budget none."""
    p, eng, prim = mixed
    for v in ("SHK_PCR_FETCH_CAP", "SHK_PCR_PANEL_FETCH_CAP", "SHK_PCR_PANEL_THREADS"):
        monkeypatch.delenv(v, raising=False)
    params = [g.params for g in p.genes]
    got = eng.pcr_extend_panel(prim, params)
    assert len(got) == len(p.genes)
    for i, g in enumerate(p.genes):
        want, used, steps = p.expected[i]
        assert_graph(got[i], want, used, steps, g.name)
        assert same_graph(got[i], eng.pcr_extend(prim[2 * i], prim[2 * i + 1], **g.params)), g.name
    a, b = pc.gene_index(p, "twin a"), pc.gene_index(p, "twin b")
    assert same_graph(got[a], got[b])
    monkeypatch.setenv("SHK_PCR_PANEL_TRACE", "1")
    shape = {}
    for var, val in (("SHK_PCR_FETCH_CAP", "8"), ("SHK_PCR_PANEL_FETCH_CAP", "64"), ("SHK_PCR_PANEL_THREADS", "1"),
                     ("SHK_PCR_PANEL_THREADS", "4"), ("SHK_PCR_PANEL_THREADS", "0")):
        monkeypatch.setenv(var, val)
        capfd.readouterr()
        again = eng.pcr_extend_panel(prim, params)
        monkeypatch.delenv(var)
        assert len(again) == len(got) and all(same_graph(x, y) for x, y in zip(again, got)), (var, val)
        m = re.search(r"rounds (\d+) launches (\d+) threads (\d+)", capfd.readouterr().err)
        shape[var, val] = tuple(int(x) for x in m.groups())
    monkeypatch.delenv("SHK_PCR_PANEL_TRACE")
    rounds, launches, _ = shape["SHK_PCR_PANEL_FETCH_CAP", "64"]
    assert launches > rounds - 1, shape          # (the last round fetches nothing) some round went in several launches
    rounds, launches, threads = shape["SHK_PCR_PANEL_THREADS", "4"]
    assert launches == rounds - 1 and threads == 4, shape
    assert shape["SHK_PCR_PANEL_THREADS", "0"][2] == 1 and shape["SHK_PCR_PANEL_THREADS", "1"][2] == 1, shape  # clamped, not the default
    assert shape["SHK_PCR_FETCH_CAP", "8"][0] > 10 * rounds, shape  # a fetch every few nodes
    # the raw arrays of shk_primer_kmers go in unchanged, and one set of parameters can stand for all
    raw = (np.concatenate([x[0] for x in prim]), np.concatenate([x[1] for x in prim]),
           np.concatenate([[0], np.cumsum([len(x[0]) for x in prim])]).astype(np.uint64))
    std = p.genes[0].params
    one = eng.pcr_extend_panel(raw, std)
    for i, g in enumerate(p.genes):
        if g.params == std:
            assert same_graph(one[i], got[i]), g.name


def test_hand_over_to_thread_reads_panel(mixed):
    p, eng, prim = mixed
    graphs = eng.pcr_extend_panel(prim, [g.params for g in p.genes])
    n = 300
    bases, offsets = p.bases[:int(p.offsets[n])], p.offsets[:n + 1]
    lists = [list(range(i % 3, n, 3)) if len(g.edge_src) else [0, 1] for i, g in enumerate(graphs)]
    got = eng.thread_reads_panel(graphs, bases, offsets, lists)
    assert len(got) == len(graphs) and sum(int(a.support_total.sum()) > 0 for a in got) >= 6
    for i, (g, ids) in enumerate(zip(graphs, lists)):
        alone = eng.pcr_extend(prim[2 * i], prim[2 * i + 1], **p.genes[i].params)
        sub = np.concatenate([bases[int(offsets[r]):int(offsets[r + 1])] for r in ids])
        off = np.concatenate([[0], np.cumsum([int(offsets[r + 1] - offsets[r]) for r in ids])]).astype(np.uint64)
        want = eng.thread_reads(alone, sub, off)
        for f in ("support_total", "support_unambiguous", "links", "link_counts", "read_edges"):
            assert np.array_equal(getattr(got[i], f), getattr(want, f)), (p.genes[i].name, f)


def raw_call(eng, prim, params, node_cap, edge_cap):
    ng = len(prim) // 2
    pk = np.concatenate([np.asarray(x[0], dtype=np.uint64) for x in prim]) if prim else np.zeros(0, np.uint64)
    pcn = np.concatenate([np.asarray(x[1], dtype=np.uint32) for x in prim]) if prim else np.zeros(0, np.uint32)
    po = np.concatenate([[0], np.cumsum([len(x[0]) for x in prim])]).astype(np.uint64)
    prm = (_PcrExtendParams * max(ng, 1))(*[_PcrExtendParams(q["min_count"], q["table_min_count"], q["high_coverage_ratio"],
                                                              q["max_num_nodes"], 1 if q["sweep"] else 0, 0) for q in params])
    sub, flags = np.zeros(max(node_cap, 1), np.uint64), np.zeros(max(node_cap, 1), np.uint8)
    es, et, ec = (np.zeros(max(edge_cap, 1), np.uint32) for _ in range(3))
    noff, eoff = np.full(ng + 1, 77, np.uint64), np.full(ng + 1, 77, np.uint64)
    found, thr, steps = (np.zeros(max(ng, 1), np.uint32) for _ in range(3))
    rc = eng._L.shk_pcr_extend_panel(eng._h, pk.ctypes.data, pcn.ctypes.data, po.ctypes.data, ng, C.cast(prm, C.c_void_p),
                                     sub.ctypes.data, flags.ctypes.data, noff.ctypes.data, node_cap, es.ctypes.data, et.ctypes.data,
                                     ec.ctypes.data, eoff.ctypes.data, edge_cap, found.ctypes.data, thr.ctypes.data, steps.ctypes.data)
    return rc, noff, eoff, sub, es


def test_caps_report_the_need(mixed):
    p, eng, prim = mixed
    pick = [pc.gene_index(p, n) for n in ("first threshold", "no set at all", "second step")]
    pr = [prim[2 * i + d] for i in pick for d in (0, 1)]
    params = [p.genes[i].params for i in pick]
    sizes = [(len(p.expected[i][0].sub_kmer), len(p.expected[i][0].edges)) for i in pick]
    nn, ne = sum(s[0] for s in sizes), sum(s[1] for s in sizes)
    for node_cap, edge_cap in ((0, 0), (nn - 1, ne), (nn, ne - 1)):
        rc, noff, eoff, _, _ = raw_call(eng, pr, params, node_cap, edge_cap)
        assert rc == -2, (node_cap, edge_cap)
        assert list(noff) == [0] + list(np.cumsum([s[0] for s in sizes])) and list(eoff) == [0] + list(np.cumsum([s[1] for s in sizes]))
    rc, noff, eoff, sub, es = raw_call(eng, pr, params, nn, ne)
    assert rc == 0 and int(noff[-1]) == nn and int(eoff[-1]) == ne
    assert list(sub[:sizes[0][0]]) == p.expected[pick[0]][0].sub_kmer
    assert list(sub[nn - sizes[2][0]:nn]) == p.expected[pick[2]][0].sub_kmer
    big = pc.gene_index(p, "never found")  # more nodes than the wrapper's first guess holds: it retries once, at the need
    assert len(p.expected[big][0].sub_kmer) > 4096
    twice = eng.pcr_extend_panel([prim[2 * big], prim[2 * big + 1]] * 2, p.genes[big].params)
    assert len(twice) == 2 and all(list(g.node_sub_kmers) == p.expected[big][0].sub_kmer for g in twice)


def test_edge_cases(mixed):
    p, eng, prim = mixed
    before = (eng.export_table(), eng.histograms().copy())
    assert eng.pcr_extend_panel([], []) == []
    rc, noff, eoff, _, _ = raw_call(eng, [], [], 0, 0)
    assert rc == 0 and list(noff) == [0] and list(eoff) == [0]
    params = [g.params for g in p.genes]
    bad = [(x[0].copy(), x[1]) for x in prim]
    bad[2 * 3 + 1][0][0] = 1 << (2 * p.k)  # not a k-mer
    with pytest.raises(sa.ShkError) as e:
        eng.pcr_extend_panel(bad, params)
    assert e.value.code == -2 and "gene 3" in e.value.msg and "reverse" in e.value.msg and "forward" not in e.value.msg
    bad = [(x[0].copy(), x[1]) for x in prim]
    bad[2 * 4][0][0] = 1 << (2 * p.k)
    with pytest.raises(sa.ShkError) as e:
        eng.pcr_extend_panel(bad, params)
    assert e.value.code == -2 and "gene 4" in e.value.msg and "forward" in e.value.msg
    po = np.array([0, 1, 0, 1, 1], dtype=np.uint64)  # gene 0's reverse set ends before it starts
    with pytest.raises(sa.ShkError) as e:
        eng.pcr_extend_panel((np.zeros(1, np.uint64), np.ones(1, np.uint32), po), params[:2])
    assert e.value.code == -2 and "gene 0" in e.value.msg and "reverse" in e.value.msg and "primer_offsets" in e.value.msg
    off = np.zeros(2, np.uint64)
    rc = eng._L.shk_pcr_extend_panel(eng._h, None, None, None, 4097, None, None, None, off.ctypes.data, 0, None, None, None,
                                     off.ctypes.data, 0, None, None, None)
    assert rc == -2 and "4097" in eng._L.shk_last_error(eng._h).decode()
    after = (eng.export_table(), eng.histograms())
    assert np.array_equal(before[0][0], after[0][0]) and np.array_equal(before[0][1], after[0][1]) and np.array_equal(before[1], after[1])
    with sa.KmerEngine(p.k, 1, 100, device_ids=[0, 0]) as multi:
        multi.ingest_reads(p.bases, p.offsets)
        multi.finalize()
        with pytest.raises(sa.ShkError) as e:
            multi.pcr_extend_panel(prim[:4], [dict(max_num_nodes=1000)] * 2)
        assert e.value.code == -11 and "multi-device context" in e.value.msg
    with sa.KmerEngine(p.k, 1, 100, n_owners=2, owner_id=1) as share:
        share.ingest_reads(p.bases, p.offsets)
        share.finalize()
        with pytest.raises(sa.ShkError) as e:
            share.pcr_extend_panel(prim[:4], [dict(max_num_nodes=1000)] * 2)
        assert e.value.code == -11 and "owner share" in e.value.msg
