"""The host side of sPCR's last stage without a GPU: the model (products_ref) against the reference's own unit-test
expectations, shk_pcr_paths_panel against the model on every crafted case and on random graphs, shk_edit_within against
the full matrix, and the FASTA text.  Everything is compared as arrays, doubles bit for bit."""
from __future__ import annotations

import random

import numpy as np
import pytest

import products_cases as pc
import products_ref as ref
import sharkmer_amd as sa
from sharkmer_amd.engine import ThreadingAnnotations, ShkError


# ---- the model reproduces the reference's unit tests ----

def _graph(case):
    return ref.StableDiGraph(*case.graph())


def _case(name):
    (c,) = [c for c in pc.cases() if c.name == name]
    return c


def test_model_bubble_rs_unit_tests():
    g = _graph(_case("bubble.rs diamond"))
    bubbles = ref.detect_simple_bubbles(g)
    assert len(bubbles) == 1 and len(bubbles[0][2]) == 2                      # test_detect_simple_bubble
    c = _case("bubble.rs read support")
    prefs = ref.resolve_bubbles(_graph(c), c.ann)
    assert prefs[0] > prefs[1] and prefs[2] > prefs[3]                        # test_resolve_with_read_support
    assert ref.detect_simple_bubbles(_graph(_case("bubble.rs linear"))) == []  # test_no_bubble_linear
    assert ref.detect_simple_bubbles(_graph(_case("bubble.rs depth-limited chains"))) == []  # test_depth_limited_branches_not_a_bubble
    c = _case("bubble.rs tie")
    first = ref.resolve_bubbles(_graph(c), c.ann)
    assert all(ref.resolve_bubbles(_graph(c), c.ann) == first for _ in range(10))  # test_bubble_tiebreak_is_deterministic
    assert sorted(first) == [0, 1, 2, 3] and set(first.values()) == {1.0}


def test_model_paths_rs_unit_tests():
    c = _case("paths.rs linear")
    paths = ref.get_assembly_paths(_graph(c), c.k, c.params, None)
    assert [[n for n, _ in p] for p in paths] == [[0, 1, 2, 3]]               # test_linear_path
    assert paths[0][0][1] is None and all(e is not None for _, e in paths[0][1:])
    c = _case("paths.rs diamond")
    assert len(ref.get_assembly_paths(_graph(c), c.k, c.params, None)) == 2   # test_diamond_finds_both_paths
    for name in ("paths.rs no start nodes", "paths.rs max length", "paths.rs budget 0"):
        c = _case(name)                                                       # test_no_start_nodes_gives_empty,
        assert ref.get_assembly_paths(_graph(c), c.k, c.params, None) == []   # test_max_length_caps_paths, test_dfs_budget_..
    children = ref.sorted_children(_graph(_case("paths.rs sorted_children")), 0, None)
    assert [(t, e) for t, e, _ in children] == [(1, 0), (2, 1)]               # test_sorted_children_order


def test_model_rules_the_cases_are_about():
    """What each crafted case is meant to show, shown on the model — so that a case that stopped exercising its rule is
    noticed."""
    c = _case("shared tail")
    prefs = ref.resolve_bubbles(_graph(c), c.ann)
    assert prefs[0] == 1.0 and prefs[4] == prefs[1] < 1.0    # c → d: the lower-ranked branch wrote last
    c = _case("edge in two sources")
    prefs = ref.resolve_bubbles(_graph(c), c.ann)
    assert prefs[4] == prefs[5] == 2.0 / 12.0                # c → t: the later source's value, not s1's 1.0
    c = _case("cycling branch")
    prefs = ref.resolve_bubbles(_graph(c), c.ann)
    assert sorted(prefs) == [3, 4, 5, 6]
    c = _case("phasing reverses")
    prefs = ref.resolve_bubbles(_graph(c), c.ann)
    assert prefs[3] == 1.0 and prefs[1] < 1.0
    c = _case("wrapping sums")
    prefs = ref.resolve_bubbles(_graph(c), c.ann)
    assert prefs[3] == 14.0 / float(0x20000000) and prefs[0] == 1.0           # 3 × 0x60000000 wraps to 0x20000000
    assert ref.resolve_bubbles(_graph(_case("branches of 50 steps")), _case("branches of 50 steps").ann)
    assert ref.resolve_bubbles(_graph(_case("branches of 51 steps")), _case("branches of 51 steps").ann) == {}
    c = _case("equal counts")
    assert [p[1][1] for p in ref.get_assembly_paths(_graph(c), c.k, c.params, None)] == [0, 1]
    n_paths = [len(ref.get_assembly_paths(_graph(_case(f"cycle, {v} visits")), 9, _case(f"cycle, {v} visits").params, None)) for v in (1, 2, 3)]
    assert n_paths[0] == 1 and n_paths[0] < n_paths[1] < n_paths[2]
    c = _case("end before min_path_nodes")
    assert [[n for n, _ in p] for p in ref.get_assembly_paths(_graph(c), c.k, c.params, None)] == [[0, 1, 2, 3]]
    c = _case("start is an end")
    assert [[n for n, _ in p] for p in ref.get_assembly_paths(_graph(c), c.k, c.params, None)][0] == [0, 1, 0]
    c = _case("max_length <= k")
    assert [[n for n, _ in p] for p in ref.get_assembly_paths(_graph(c), c.k, c.params, None)] == [[0, 1]]
    c = _case("ladder cut at 20")
    r = ref.run_gene(c.k, *c.graph(), c.ann, c.params)
    assert r.paths_found == 40 and [x.start_node for x in r.records] == [0] * 20 + [1] * 20
    c = _case("ladder, 37 states")
    st = []
    ref.get_assembly_paths(_graph(c), c.k, c.params, None, st)
    assert st == [37, 37]
    r = ref.run_gene(9, *_case("cv above 1, plain").graph(), None, ref.Params())
    assert r.records[0].score["coverage_cv"] > 1.0 and r.records[0].score["zero_support_edges"] is None
    r = ref.run_gene(9, *_case("12 zero-support edges, threaded").graph(), _case("12 zero-support edges, threaded").ann, ref.Params())
    assert r.records[0].score["zero_support_edges"] == 12 and r.records[0].composite == 8.0 * 0.5 ** 10 * (2.0 / 14.0)


# ---- shk_pcr_paths_panel against the model ----

def _ann(case):
    if case.ann is None:
        return None
    links = np.array(sorted(case.ann.branch_links), dtype=np.uint32).reshape(-1, 2)
    counts = np.array([case.ann.branch_links[k] for k in sorted(case.ann.branch_links)], dtype=np.uint32)
    return ThreadingAnnotations(np.array(case.ann.support_total, dtype=np.uint32), np.array(case.ann.support_unambiguous, dtype=np.uint32),
                                links, counts, np.zeros(0, dtype=np.uint32), 0)


def expected_records(case):
    """The model's answer for a case in the shape of PcrProducts: (per-record arrays, counters)."""
    r = ref.run_gene(case.k, *case.graph(), case.ann, case.params)
    return r


def _none(x):
    return float("nan") if x is None else float(x)


def assert_records(got, want_records, what):
    """A PcrProducts against a list of the model's Records; doubles by their bits."""
    assert got.sequences == [r.sequence for r in want_records], what
    assert got.start_node.tolist() == [r.start_node for r in want_records], what
    assert got.path_nodes.tolist() == [r.path_nodes for r in want_records], what
    assert got.count_min.tolist() == [r.count_min for r in want_records], what
    assert got.count_max.tolist() == [r.count_max for r in want_records], what
    bits = lambda xs: np.array(xs, dtype=np.float64).view(np.uint64).tolist()
    assert bits(got.count_mean) == bits([r.count_mean for r in want_records]), what
    assert bits(got.count_median) == bits([r.count_median for r in want_records]), what
    assert bits(got.score) == bits([r.composite for r in want_records]), what
    fields = [[_none(r.score[f]) for f in sa.PCR_SCORE_FIELDS] for r in want_records]
    assert bits(got.score_fields.reshape(-1)) == bits(np.array(fields, dtype=np.float64).reshape(-1)), what


def assert_paths(got, case):
    want = expected_records(case)
    assert (got.paths_found, got.generated, got.states_explored) == (want.paths_found, len(want.records), want.states_explored), case.name
    assert_records(got, want.records, case.name)


def _params(cases):
    return {f: [getattr(c.params, f) for c in cases] for f in ("min_length", "max_length", "max_dfs_states", "max_paths_per_pair", "max_node_visits")}


@pytest.mark.parametrize("case", pc.cases(), ids=lambda c: c.name)
def test_paths_panel_case_alone(case):
    (got,) = sa.pcr_paths_panel(case.k, [case.graph()], [_ann(case)], **_params([case]))
    assert_paths(got, case)


def test_paths_panel_all_cases_in_one_panel():
    for k in sorted({c.k for c in pc.cases()}):
        cs = [c for c in pc.cases() if c.k == k]
        got = sa.pcr_paths_panel(k, [c.graph() for c in cs], [_ann(c) for c in cs], **_params(cs))
        for g, c in zip(got, cs):
            assert_paths(g, c)


def test_paths_panel_random_graphs():
    rng = random.Random(20260816)
    cs = [pc.random_case(rng, f"random {i}") for i in range(300)]
    assert sum(len(expected_records(c).records) > 0 for c in cs) > 40   # (the generator does reach the search)
    assert sum(bool(expected_records(c).prefs) for c in cs) > 15        # (and the bubbles)
    for k in sorted({c.k for c in cs}):
        sel = [c for c in cs if c.k == k]
        got = sa.pcr_paths_panel(k, [c.graph() for c in sel], [_ann(c) for c in sel], **_params(sel))
        for g, c in zip(got, sel):
            assert_paths(g, c)


def test_paths_panel_empty_and_small_room():
    assert sa.pcr_paths_panel(21, [], None) == []
    c = pc.ladder(5, 4).case("ladder, four starts", threaded=False)   # 80 records a gene: more than the binding's first room
    big = [c] * 3
    got = sa.pcr_paths_panel(c.k, [x.graph() for x in big], None, **_params(big))
    assert [g.generated for g in got] == [80] * 3
    for g in got:
        assert_paths(g, c)


def test_paths_panel_errors():
    c = _case("paths.rs diamond")
    sub, fl, es, et, ec, ratio = c.graph()

    def err(k=3, ann=None, **kw):
        g = dict(sub=sub, fl=fl, es=es, et=et, ec=ec, ratio=ratio)
        g.update(kw)
        with pytest.raises(ShkError) as e:
            sa.pcr_paths_panel(k, [c.graph(), (g["sub"], g["fl"], g["es"], g["et"], g["ec"], g["ratio"])], ann)
        assert e.value.code == -2
        return str(e.value)

    bad_t = et.copy()
    bad_t[2] = 4
    assert "gene 1" in err(et=bad_t) and "endpoint" in err(et=bad_t)
    bad_f = fl.copy()
    bad_f[1] = 4
    assert "gene 1" in err(fl=bad_f) and "flags 4" in err(fl=bad_f)
    assert "k 1" in err(k=1) and "k 32" in err(k=32)
    bad_s = sub.copy()
    bad_s[3] = 16
    assert "gene 1" in err(sub=bad_s) and "sub-k-mer" in err(sub=bad_s)
    a = ThreadingAnnotations(np.zeros(4, np.uint32), np.zeros(4, np.uint32), np.array([[0, 4]], np.uint32), np.ones(1, np.uint32),
                             np.zeros(0, np.uint32), 0)
    assert "gene 1" in err(ann=[None, a]) and "link" in err(ann=[None, a])
    with pytest.raises(ShkError) as e:
        sa.pcr_paths_panel(3, [c.graph()] * 4097, None)
    assert e.value.code == -2 and "SHK_PCR_MAX_GENES" in str(e.value)


def test_paths_panel_decreasing_offsets():
    """Offsets are the binding's own work, so this one goes to the C entry point directly."""
    import ctypes as C
    from sharkmer_amd.engine import _PcrGraphs, _PcrPathsParams, _PcrRecords, load_library
    L = load_library()
    noff = np.array([0, 2, 1], dtype=np.uint64)
    eoff = np.array([0, 0, 0], dtype=np.uint64)
    sub, fl = np.zeros(2, np.uint64), np.zeros(2, np.uint8)
    G = _PcrGraphs(2, 0, sub.ctypes.data, fl.ctypes.data, noff.ctypes.data, None, None, None, None, eoff.ctypes.data, None, None, None,
                   None, None, None, None)
    prm = (_PcrPathsParams * 2)()
    roff = np.zeros(3, dtype=np.uint64)
    R = _PcrRecords(roff.ctypes.data)
    err = C.create_string_buffer(256)
    assert L.shk_pcr_paths_panel(5, C.byref(G), prm, C.byref(R), err, len(err)) == -2
    assert b"gene 1" in err.value and b"node_offsets decrease" in err.value
    noff[:] = [0, 1, 2]
    eoff[:] = [0, 1, 0]
    es = np.zeros(1, np.uint32)
    G.edge_src = G.edge_tgt = G.edge_counts = es.ctypes.data
    assert L.shk_pcr_paths_panel(5, C.byref(G), prm, C.byref(R), err, len(err)) == -2
    assert b"gene 1" in err.value and b"edge_offsets decrease" in err.value


# ---- shk_edit_within against the full matrix ----

BOUNDARY_LENGTHS = (0, 1, 31, 32, 33, 63, 64, 65, 127, 128, 129)
BOUNDARY_T = (0, 1, 10, 31, 32, 2 ** 32 - 1)


def _seq(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n))


def _mutate(rng, s, edits):
    s = list(s)
    for _ in range(edits):
        kind = rng.randrange(3)
        if kind == 0 and s:
            s[rng.randrange(len(s))] = rng.choice("ACGT")
        elif kind == 1:
            s.insert(rng.randrange(len(s) + 1), rng.choice("ACGT"))
        elif s:
            del s[rng.randrange(len(s))]
    return "".join(s)


def _check_within(a, b, t):
    assert sa.edit_within(a, b, t) == (ref.levenshtein(a, b) <= t), (a, b, t)


def test_edit_within_random_pairs():
    rng = random.Random(7)
    for _ in range(400):
        a = _seq(rng, rng.randrange(90), rng.choice(("A", "AC", "ACGT", "ACGTNacgt")))
        b = _mutate(rng, a, rng.randrange(25)) if rng.random() < 0.7 else _seq(rng, rng.randrange(90))
        d = ref.levenshtein(a, b)
        for t in {rng.randrange(30), d, max(d - 1, 0), d + 1}:   # a random t, exactly t, t + 1, t - 1
            _check_within(a, b, t)


def test_edit_within_boundary_set():
    rng = random.Random(8)
    seqs = {n: _seq(rng, n) for n in BOUNDARY_LENGTHS}
    near = {n: _mutate(rng, seqs[n], 9) for n in BOUNDARY_LENGTHS}
    for la in BOUNDARY_LENGTHS:
        for lb in BOUNDARY_LENGTHS:
            for t in BOUNDARY_T:
                _check_within(seqs[la], seqs[lb], t)
                _check_within(seqs[la], near[lb], t)


def test_edit_within_shifts_and_length_differences():
    rng = random.Random(9)
    core = _seq(rng, 150)
    for t in (0, 1, 10, 31, 32, 40):
        head, tail = _seq(rng, t), _seq(rng, t)
        _check_within(head + core, core + tail, t)          # t insertions at the head against t deletions at the tail
        _check_within(head + core, core + tail, 2 * t)
        _check_within(core, core + tail, t)                 # a length difference of exactly t
        _check_within(core, core + tail + "A", t)           # and of t + 1
        assert sa.edit_within(core, core + tail, t) and not sa.edit_within(core, core + tail + "A", t)


def test_edit_within_takes_any_bytes():
    assert sa.edit_within(b"\x00\xff\x00", b"\x00\xfe\x00", 1) and not sa.edit_within(b"\x00\xff\x00", b"\x00\xfe\x01", 1)
    assert sa.edit_within(b"", b"", 0) and not sa.edit_within(b"", b"A", 0) and sa.edit_within(b"", b"A", 1)


# ---- FASTA text ----

def _products(medians, scores, means):
    n = len(medians)
    return sa.PcrProducts(["ACGT" * (i + 1) for i in range(n)], np.zeros(n, np.uint32), np.full(n, 2, np.uint64), np.array(means, np.float64),
                          np.array(medians, np.float64), np.arange(n, dtype=np.uint64), np.arange(n, dtype=np.uint64) + 7,
                          np.array(scores, np.float64), np.zeros((n, 6)), n, n, n, n)


def test_fasta_text():
    p = _products([12.0, 12.5, 3.0], [0.125, 0.375, 2.675], [1.005, 2.5, 1e3])
    want = (">s1_18S_0 sample=s1 gene=18S product=0 length=4 kmer_count_mean=1.00 kmer_count_median=12 kmer_count_min=0 kmer_count_max=7 score=0.12\n"
            "ACGT\n"
            ">s1_18S_1 sample=s1 gene=18S product=1 length=8 kmer_count_mean=2.50 kmer_count_median=12.5 kmer_count_min=1 kmer_count_max=8 score=0.38\n"
            "ACGTACGT\n"
            ">s1_18S_2 sample=s1 gene=18S product=2 length=12 kmer_count_mean=1000.00 kmer_count_median=3 kmer_count_min=2 kmer_count_max=9 score=2.67\n"
            "ACGTACGTACGT\n")
    # 0.125 and 0.375 are exact ties: to even, 0.12 and 0.38; 1.005 and 2.675 lie below the tie in binary: 1.00 and 2.67
    assert p.fasta("s1", "18S") == want


def test_fasta_matches_the_model_on_a_case():
    c = _case("cv above 1, threaded")
    (got,) = sa.pcr_paths_panel(c.k, [c.graph()], [_ann(c)], **_params([c]))
    want = expected_records(c).records
    text = "".join(f">x_g_{i} {r.desc('x', 'g', i)}\n{r.sequence}\n" for i, r in enumerate(want))
    assert want and got.fasta("x", "g") == text
