"""GPU tests of shk_pcr_dedup_panel (K_DEDUP) and shk_pcr_products_panel against tests/products_ref.py, the reference's
last stage restated literally: the dedup on the device and on the host route (kept lists AND every pair bit against the
full Levenshtein matrix), wave and workgroup boundaries, many genes, long records, the threshold where the routes part,
the greedy order, the truncation; the whole pipeline on the padded 18S down to the amplicon; a gene with reads; errors
and states.  Each record set's distances are computed once and shared."""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest

import sharkmer_amd as sa
import prune_cases as pcs
import products_cases as pc
import products_ref as ref
from sharkmer_amd.engine import _PcrDedupOut, ShkError
from test_products_ref_cpu import BOUNDARY_LENGTHS, _ann, _mutate, _params, _seq, assert_records

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FWD_18S, REV_18S = "AACCTGGTTGATCCTGCCAGT", "TGATCCTTCTGCAGGTTCACCTAC"
ROUTES = {"device": "0", "host": str(2 ** 62)}  # SHK_DEDUP_DEVICE_PAIRS
_dist = {}


def dist_of(name, seqs):
    if name not in _dist:
        _dist[name] = (list(seqs), ref.distance_matrix(seqs))
    assert _dist[name][0] == list(seqs)
    return _dist[name][1]


@pytest.fixture(scope="module")
def eng():
    with sa.KmerEngine(21, 1, 100) as e:  # holds nothing: the dedup needs no table
        yield e


def trace_lines(capfd):
    """The calls since the last look → [(genes, pairs on the device, on the host, by the prefilters)]."""
    return [tuple(int(x) for x in m.groups())
            for m in re.finditer(r"pcr_dedup_panel: (\d+) genes, (\d+) pairs on the device, (\d+) pairs on the host, (\d+) pairs decided by the prefilters",
                                 capfd.readouterr().err)]


def assert_dedup(got, seqs, scores, t, dist, what):
    """A DedupResult against the model: order, every pair bit, kept list, counters."""
    order = ref.sort_order(seqs, scores)
    assert got.order.tolist() == order, what
    if got.pair_bits is not None:
        assert got.pair_bits.tolist() == ref.pair_matrix(seqs, order, t, dist), what
    kept, retained = ref.sort_and_deduplicate(seqs, scores, t, dist)
    assert got.kept.tolist() == kept and (got.generated, got.retained) == (len(seqs), retained), what


def prefiltered(seqs, t):
    n = [len(s) for s in seqs]
    return sum(1 for i in range(len(n)) for j in range(i + 1, len(n)) if abs(n[i] - n[j]) > t or t >= max(n[i], n[j]))


def boundary_records():
    rng = random.Random(41)
    seqs = []
    for n in BOUNDARY_LENGTHS:
        s = _seq(rng, n)
        seqs += [s, _mutate(rng, s, 3), _mutate(rng, s, 12)]
    return seqs, [float(rng.randrange(4)) for _ in seqs]


@pytest.mark.parametrize("route", list(ROUTES))
def test_dedup_boundary_set_and_random_sets(eng, route, monkeypatch, capfd):
    monkeypatch.setenv("SHK_DEDUP_DEVICE_PAIRS", ROUTES[route])
    monkeypatch.setenv("SHK_TRACE", "1")
    seqs, scores = boundary_records()
    d = dist_of("boundary", seqs)
    n_pairs = len(seqs) * (len(seqs) - 1) // 2
    for t in (0, 1, 10, 31, 32, 2 ** 32 - 1):
        capfd.readouterr()
        (got,) = eng.pcr_dedup_panel([seqs], [scores], t, want_pairs=True)
        assert_dedup(got, seqs, scores, t, d, (route, t))
        (line,) = trace_lines(capfd)
        pre = prefiltered(seqs, t)
        on_device = route == "device" and t <= 31
        assert line == (1, n_pairs - pre if on_device else 0, 0 if on_device else n_pairs - pre, pre), (route, t)
        assert (eng.last_dedup["device_ms"] > 0) == on_device
    rng = random.Random(42)
    sets, thr = [], []
    for g in range(12):
        base = _seq(rng, rng.randrange(20, 200))
        sets.append([_mutate(rng, base, rng.randrange(0, 30)) if rng.random() < 0.8 else _seq(rng, rng.randrange(0, 200))
                     for _ in range(rng.randrange(0, 14))])
        thr.append(rng.choice((0, 1, 2, 5, 10, 20, 31)))
    scs = [[float(rng.randrange(3)) for _ in s] for s in sets]
    got = eng.pcr_dedup_panel(sets, scs, thr, want_pairs=True)
    for g in range(12):
        assert_dedup(got[g], sets[g], scs[g], thr[g], dist_of(f"random {g}", sets[g]), (route, "random", g))
    lazy = eng.pcr_dedup_panel(sets, scs, thr)  # without the bits the host route aligns only what the greedy pass asks for
    assert [x.kept.tolist() for x in lazy] == [x.kept.tolist() for x in got]


def test_dedup_wave_and_workgroup_boundaries(eng, monkeypatch):
    """47 records of 40 bases: 1081 pairs, 9 workgroups of 128 and a last wave of 57 lanes."""
    monkeypatch.setenv("SHK_DEDUP_DEVICE_PAIRS", "0")
    rng = random.Random(43)
    base = _seq(rng, 40)
    seqs = [_mutate(rng, base, rng.randrange(0, 9))[:40].ljust(40, "A") for _ in range(47)]
    scores = [float(i % 5) for i in range(47)]
    (got,) = eng.pcr_dedup_panel([seqs], [scores], 4, want_pairs=True)
    assert len(got.pair_bits) == 1081 and 0 < int(got.pair_bits.sum()) < 1081
    assert_dedup(got, seqs, scores, 4, dist_of("47", seqs), "47 records")
    assert eng.last_dedup["pairs_device"] == 1081


def test_dedup_many_genes(eng, monkeypatch):
    """70 genes of 0, 1, 2, .. records in one call equal 70 calls."""
    monkeypatch.setenv("SHK_DEDUP_DEVICE_PAIRS", "0")
    rng = random.Random(44)
    base = _seq(rng, 60)
    sets = [[_mutate(rng, base, rng.randrange(0, 12)) for _ in range(g)] for g in range(70)]
    scs = [[float(rng.randrange(4)) for _ in s] for s in sets]
    thr = [g % 7 for g in range(70)]
    panel = eng.pcr_dedup_panel(sets, scs, thr, want_pairs=True)
    for g in range(70):
        (one,) = eng.pcr_dedup_panel([sets[g]], [scs[g]], thr[g], want_pairs=True)
        assert (one.kept.tolist(), one.order.tolist(), one.pair_bits.tolist(), one.generated, one.retained) == (
            panel[g].kept.tolist(), panel[g].order.tolist(), panel[g].pair_bits.tolist(), panel[g].generated, panel[g].retained), g
    for g in (2, 3, 33, 69):
        assert_dedup(panel[g], sets[g], scs[g], thr[g], dist_of(f"many {g}", sets[g]), g)


def test_dedup_long_sequences(eng, monkeypatch):
    """Records of 2500 and 2505 bases at t = 10, two genes."""
    monkeypatch.setenv("SHK_DEDUP_DEVICE_PAIRS", "0")
    rng = random.Random(45)
    sets = []
    for g in range(2):
        a = _seq(rng, 2500)
        b = a[:700] + _seq(rng, 5) + a[700:]                 # 2505 bases, 5 insertions
        sets.append([a, b, _mutate(rng, a, 10), _mutate(rng, b, 6), _mutate(rng, a, 14), _seq(rng, 2500)])
    scs = [[3.0, 2.0, 2.0, 1.0, 1.0, 0.0]] * 2
    got = eng.pcr_dedup_panel(sets, scs, 10, want_pairs=True)
    for g in range(2):
        assert {len(s) for s in sets[g][:2]} == {2500, 2505}
        d = dist_of(f"long {g}", sets[g])
        assert any(x <= 10 for row in d for x in row[1:]) and any(10 < x < 40 for row in d for x in row)
        assert_dedup(got[g], sets[g], scs[g], 10, d, g)


def test_dedup_thresholds_31_and_32_in_one_panel(eng, monkeypatch, capfd):
    monkeypatch.setenv("SHK_DEDUP_DEVICE_PAIRS", "0")
    monkeypatch.setenv("SHK_TRACE", "1")
    rng = random.Random(46)
    base = _seq(rng, 150)
    step = lambda ch: "ACGT"[("ACGT".index(ch) + 1) % 4]
    seqs = ["".join(step(ch) if i % 2 == 0 and i < 2 * e else ch for i, ch in enumerate(base)) for e in (0, 1, 31, 32, 33, 36, 64, 65)]
    seqs.append(base[:40] + base[45:])  # and a length difference
    scores = [float(-i) for i in range(len(seqs))]
    capfd.readouterr()
    got = eng.pcr_dedup_panel([seqs, seqs], [scores, scores], [31, 32], want_pairs=True)
    ((genes, on_dev, on_host, pre),) = trace_lines(capfd)
    assert genes == 2 and on_dev == 36 - prefiltered(seqs, 31) and on_host == 36 - prefiltered(seqs, 32) and on_dev and on_host
    d = dist_of("31/32", seqs)
    dists = {x for row in d for x in row}
    assert {30, 31, 32} <= dists and any(32 < x < 40 for x in dists)  # pairs at, just below and just above either threshold
    assert_dedup(got[0], seqs, scores, 31, d, "t 31 on the device")
    assert_dedup(got[1], seqs, scores, 32, d, "t 32 on the host")


@pytest.mark.parametrize("route", list(ROUTES))
def test_dedup_greedy_order_and_truncation(eng, route, monkeypatch):
    monkeypatch.setenv("SHK_DEDUP_DEVICE_PAIRS", ROUTES[route])
    a = "ACGT" * 10
    b = "T" + a[1:]            # A ~ B at t = 1
    c = b[:-1] + "A"           # B ~ C, A !~ C
    (got,) = eng.pcr_dedup_panel([[c, b, a]], [[1.0, 2.0, 3.0]], 1, want_pairs=True)
    assert got.order.tolist() == [2, 1, 0] and got.pair_bits.tolist() == [True, False, True]
    assert got.kept.tolist() == [2, 0] and got.retained == 2    # greedy, not transitive: A and C both stay
    (got,) = eng.pcr_dedup_panel([[c, b, a]], [[1.0, 3.0, 2.0]], 1)
    assert got.kept.tolist() == [1]                             # B first: both others are its duplicates
    rng = random.Random(47)
    far = [_seq(rng, 50) for _ in range(25)]
    d = dist_of("25 distant", far)
    assert min(d[i][j] for i in range(25) for j in range(i)) > 10
    scores = [float(i % 7) for i in range(25)]
    (got,) = eng.pcr_dedup_panel([far], [scores], 10, want_pairs=True)
    assert (got.generated, got.retained, len(got.kept)) == (25, 25, 20)
    assert_dedup(got, far, scores, 10, d, "truncation")
    # equal scores and equal sequences: the bytes decide, then nothing can
    (got,) = eng.pcr_dedup_panel([["ACGTAC", "ACGT", "ACGTAC", "AAGT"]], [[1.0, 1.0, 1.0, 1.0]], 0)
    assert got.order.tolist() == [3, 1, 0, 2] and got.kept.tolist() == [3, 1, 0]


# ---- the whole pipeline ----

def revcomp(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


def canonical(kmers, k):
    def rc(x):
        r = 0
        for _ in range(k):
            r = (r << 2) | (3 - (x & 3))
            x >>= 2
        return r
    return np.array(sorted({min(int(x), rc(int(x))) for x in kmers}), dtype=np.uint64)


def model_products(k, graph, ann, **params):
    """products_ref.run_gene on a PrunedGraph or a six-array tuple and the ThreadingAnnotations the library returned."""
    a = None
    if ann is not None:
        a = ref.Annotations(ann.support_total.tolist(), ann.support_unambiguous.tolist(),
                            {(int(x), int(y)): int(c) for (x, y), c in zip(ann.links, ann.link_counts)})
    if not isinstance(graph, tuple):
        graph = (graph.node_sub_kmers, graph.node_flags, graph.edge_src, graph.edge_tgt, graph.edge_counts, graph.coverage_ratio)
    return ref.run_gene(k, *graph, a, ref.Params(**params))


def debruijn_gene(reads, k, first, last):
    """The de Bruijn graph of the reads at k as six arrays: nodes and edges in order of first appearance, counts the
    occurrences, ratios count / median; `first` / `last`: the (k-1)-mers flagged start / end."""
    code = lambda x: int("".join(format("ACGT".index(ch), "02b") for ch in x), 2)
    node_of, edges = {}, {}
    for r in reads:
        for i in range(len(r) - k + 1):
            ends = [node_of.setdefault(x, len(node_of)) for x in (r[i:i + k - 1], r[i + 1:i + k])]
            edges.setdefault(r[i:i + k], [ends[0], ends[1], 0])[2] += 1
    sub = np.array([code(x) for x in node_of], dtype=np.uint64)
    flags = np.array([(1 if x == first else 0) | (2 if x == last else 0) for x in node_of], dtype=np.uint8)
    es, et, ec = (np.array([e[i] for e in edges.values()], dtype=np.uint32) for i in range(3))
    return (sub, flags, es, et, ec, ec / float(np.median(ec)))


def test_18s_pipeline_yields_the_amplicon():
    """pcr_18s_padded.txt ×10 at k 21 with the reference's primers and parameters (mod.rs:1249-1281): primer_kmers →
    extend → prune → filter → thread → products.  One product, the model's, the amplicon of the golden sequence."""
    seq = open(os.path.join(G, "pcr_18s_padded.txt")).read().strip()
    bases = np.frombuffer(seq.encode() * 10, dtype=np.uint8).copy()
    offsets = np.arange(11, dtype=np.uint64) * np.uint64(len(seq))
    with sa.KmerEngine(21, 1, 100) as e:
        e.ingest_reads(bases, offsets)
        e.finalize()
        prim = e.primer_kmers([sa.Primer(s, trim=15, mismatches=2, min_count=3) for s in (FWD_18S, REV_18S)])
        graphs = e.pcr_extend_panel(prim, [dict(min_count=3, max_num_nodes=500_000)])
        pruned = e.pcr_prune_panel(graphs)
        lists = e.filter_reads_panel(bases, offsets, [canonical(np.concatenate([prim[0][0], prim[1][0]]), 21)])
        assert len(lists[0]) == 10
        anns = e.thread_reads_panel(pruned, bases, offsets, lists)
        (got,) = e.pcr_products_panel(pruned, anns, min_length=0, max_length=2500)
        (bare,) = e.pcr_products_panel(pruned, None, min_length=0, max_length=2500)
    want = model_products(21, pruned[0], anns[0], min_length=0, max_length=2500)
    assert len(want.products) == 1 and got.retained == want.retained == 1
    assert (got.paths_found, got.generated, got.states_explored) == (want.paths_found, len(want.records), want.states_explored)
    assert_records(got, want.products, "18S")
    (product,) = got.sequences
    assert product in seq and product.startswith("GTTGATCCTGCCAGT") and len(product) > 1700
    tail, primer_rc = product[-15:], revcomp("TGCAGGTTCACCTAC")
    assert sum(x != y for x, y in zip(tail, primer_rc)) <= 2
    assert got.fasta("s", "18s") == f">s_18s_0 {want.products[0].desc('s', '18s', 0)}\n{product}\n"
    assert bare.sequences == [product] and np.isnan(bare.score_fields[0, 3:]).all() and not np.isnan(got.score_fields).any()


def test_genes_with_reads():
    """Genes with their reads through thread_reads_panel into the products, against the model on the same arrays:
    prune_cases.threaded_gene() unpruned (the tip's root is a branch, its reads leave links) and pruned; a real bubble —
    30 reads of a sequence, 12 of a variant with one substitution, a read that enters it — whose minority branch the
    counts alone would visit second and the reads rank by support; and a gene without reads, which has no annotations."""
    t = pcs.threaded_gene()
    c = t.case
    k = c.k
    sub, fl, es, et, ec = (t.sub_kmers,) + c.arrays()[1:]
    ec = np.asarray(ec, dtype=np.uint32)
    unpruned = (sub, fl, es, et, ec, ec / float(np.median(ec)))
    rng = random.Random(49)
    seq = _seq(rng, 70)
    var = seq[:35] + "ACGT"[("ACGT".index(seq[35]) + 1) % 4] + seq[36:]
    bubble_reads = [seq] * 30 + [var] * 12 + [var[20:50]] * 9
    bubble = debruijn_gene(bubble_reads, k, seq[:k - 1], seq[-(k - 1):])
    reads = list(t.reads) + [r.encode() for r in bubble_reads]
    n0 = len(t.reads)
    with sa.KmerEngine(k, 1, 100) as e:
        bases, offsets = e._pack(reads)
        (pruned,) = e.pcr_prune_panel([unpruned[:5]])
        graphs = [unpruned, pruned, bubble, pruned]
        lists = [list(range(n0)), list(range(n0)), list(range(n0, len(reads))), []]
        as_thread = lambda g: (g[0], g[2], g[3]) if isinstance(g, tuple) else g
        anns = e.thread_reads_panel([as_thread(g) for g in graphs], bases, offsets, lists)
        anns[3] = None  # no reads: no annotations (mod.rs:664-697)
        assert len(anns[0].links) > 0 and len(anns[2].links) > 0
        for thr in (0, 10):
            got = e.pcr_products_panel(graphs, anns, dedup_edit_threshold=thr)
            for g, a, p in zip(graphs, anns, got):
                want = model_products(k, g, a, dedup_edit_threshold=thr)
                assert want.products and (p.retained, p.generated, p.paths_found) == (want.retained, len(want.records), want.paths_found)
                assert_records(p, want.products, thr)
    want = model_products(k, bubble, anns[2], dedup_edit_threshold=0)
    assert want.prefs and min(want.prefs.values()) < 1.0 and sorted(r.sequence for r in want.products) == sorted([seq, var])
    assert np.isnan(got[3].score_fields[:, 3:]).all() and not np.isnan(got[1].score_fields).any()


@pytest.mark.parametrize("route", list(ROUTES))
def test_products_panel_crafted_cases(route, monkeypatch):
    """Every crafted case of one k in one panel: the products equal the model's, on both dedup routes."""
    monkeypatch.setenv("SHK_DEDUP_DEVICE_PAIRS", ROUTES[route])
    cs = [x for x in pc.cases() if x.k == 9]
    with sa.KmerEngine(9, 1, 100) as e:
        got = e.pcr_products_panel([x.graph() for x in cs], [_ann(x) for x in cs], dedup_edit_threshold=[x.params.dedup_edit_threshold for x in cs],
                                   **_params(cs))
    n_products = 0
    for x, p in zip(cs, got):
        want = ref.run_gene(x.k, *x.graph(), x.ann, x.params)
        assert (p.retained, p.generated) == (want.retained, len(want.records)), x.name
        assert_records(p, want.products, x.name)
        n_products += len(want.products)
    assert n_products > 30 and any(p.retained < p.generated for p in got)


# ---- errors and states ----

def raw_dedup(e, seqs, soff, roff, scores, thr, n_genes, pair_cap=None):
    seqs, soff, roff = np.frombuffer(seqs, dtype=np.uint8), np.array(soff, np.uint64), np.array(roff, np.uint64)
    scores, thr = np.array(scores, np.float64), np.array(thr, np.uint32)
    kept = np.zeros(20 * max(n_genes, 1), np.uint32)
    poff = np.full(n_genes + 1, 77, np.uint64)
    words = np.zeros(64, np.uint64)
    out = _PcrDedupOut(kept.ctypes.data, None, None, None, None, words.ctypes.data if pair_cap is not None else None, poff.ctypes.data,
                       pair_cap or 0, 0, 0, 0, 0.0)
    rc = e._L.shk_pcr_dedup_panel(e._h, seqs.ctypes.data, soff.ctypes.data, roff.ctypes.data, scores.ctypes.data, thr.ctypes.data, n_genes, C.byref(out))
    return rc, e._L.shk_last_error(e._h).decode(), poff


def test_errors(eng):
    ok = (b"ACGTACGTAC", [0, 4, 8, 10], [0, 1, 3], [1.0, 2.0, 3.0], [1, 1], 2)
    assert raw_dedup(eng, *ok)[0] == 0
    rc, msg, _ = raw_dedup(eng, ok[0], ok[1], [0, 2, 1], *ok[3:])
    assert rc == -2 and "gene 1" in msg and "record_offsets decrease" in msg
    rc, msg, _ = raw_dedup(eng, ok[0], [0, 4, 3, 10], *ok[2:])
    assert rc == -2 and "gene 1" in msg and "record 0" in msg and "seq_offsets decrease" in msg
    rc, msg, _ = raw_dedup(eng, b"ACGTACNTAC", *ok[1:])
    assert rc == -2 and "gene 1" in msg and "none of ACGT" in msg
    rc, msg, _ = raw_dedup(eng, b"", [0], [0] * 4098, [], [0] * 4097, 4097)
    assert rc == -2 and "4097" in msg
    rc, msg, poff = raw_dedup(eng, *ok, pair_cap=0)
    assert rc == -2 and "pair_cap" in msg and poff.tolist() == [0, 0, 1]
    assert raw_dedup(eng, *ok, pair_cap=1)[0] == 0
    # the paths' errors arrive through the context's call as through the host's
    d = pc.paths_diamond().case("diamond", threaded=False)
    sub, fl, es, et, ec, ratio = d.graph()
    bad_t = et.copy()
    bad_t[0] = 9
    with sa.KmerEngine(3, 1, 100) as e3:
        with pytest.raises(ShkError) as err:
            e3.pcr_products_panel([d.graph(), (sub, fl, es, bad_t, ec, ratio)])
        assert err.value.code == -2 and "gene 1" in str(err.value) and "endpoint" in str(err.value)
        bad_s = sub.copy()
        bad_s[2] = 16
        with pytest.raises(ShkError) as err:
            e3.pcr_products_panel([(bad_s, fl, es, et, ec, ratio)])
        assert "sub-k-mer" in str(err.value)
        assert e3.pcr_products_panel([]) == [] and e3.pcr_dedup_panel([], []) == []
        (p,) = e3.pcr_products_panel([d.graph()], dedup_edit_threshold=0)   # the context is usable after the errors
        assert_records(p, ref.run_gene(3, *d.graph(), None, ref.Params(dedup_edit_threshold=0)).products, "after the errors")


def test_states(monkeypatch):
    """In the middle of a counting job the finalize histogram is what it would have been; an owner share and a
    two-device context answer alike; a second call reuses the scratch."""
    monkeypatch.setenv("SHK_DEDUP_DEVICE_PAIRS", "0")
    rng = random.Random(48)
    base = _seq(rng, 80)
    seqs = [_mutate(rng, base, rng.randrange(0, 8)) for _ in range(20)]
    scores = [float(i % 3) for i in range(20)]
    d = dist_of("states", seqs)
    spec = sa.SynthSpec(genome_len=5000, sub_per_64k=300, n_per_64k=60)
    bases, offsets = sa.synth_reads(spec, 0, 400)
    with sa.KmerEngine(21, 1, 100) as plain:
        plain.ingest_reads(bases, offsets)
        plain.finalize()
        want_histo = plain.histograms().copy()
    with sa.KmerEngine(21, 1, 100) as e:
        half = int(offsets[200])
        e.ingest_reads(bases[:half], offsets[:201])
        (mid,) = e.pcr_dedup_panel([seqs], [scores], 3, want_pairs=True)   # between two ingests
        e.ingest_reads(bases[half:], offsets[200:] - offsets[200])
        e.finalize()
        assert np.array_equal(e.histograms(), want_histo)
        (again,) = e.pcr_dedup_panel([seqs], [scores], 3, want_pairs=True)  # after finalize, the scratch reused
        (third,) = e.pcr_dedup_panel([seqs], [scores], 3, want_pairs=True)
        assert np.array_equal(e.histograms(), want_histo)
    for got in (mid, again, third):
        assert_dedup(got, seqs, scores, 3, d, "states")
    with sa.KmerEngine(21, 1, 100, n_owners=2, owner_id=1) as share:
        assert_dedup(share.pcr_dedup_panel([seqs], [scores], 3, want_pairs=True)[0], seqs, scores, 3, d, "owner share")
    with sa.KmerEngine(21, 1, 100, device_ids=[0, 0]) as multi:
        assert_dedup(multi.pcr_dedup_panel([seqs], [scores], 3, want_pairs=True)[0], seqs, scores, 3, d, "two devices")
