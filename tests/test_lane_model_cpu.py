"""The per-lane model of tests/lane_model.py, pinned before it judges the engine (tests/test_gpu_sequences.py):
whatever the model and the oracle's one-shot driver share — histogram columns, totals, the merged table — must be
equal when the model is fed the same reads in any number of calls, and its insert must be KmerCounts::insert with
the saturating cases of test_oracle_kat.py.  No GPU."""
import gzip
import hashlib
import json
import os

import numpy as np
import pytest

import pcr_ref
from lane_model import LaneModel, ModelError, SHK_ERR_BAD_ARG, SHK_ERR_STATE, U32_MAX
from test_gpu_fuzz import draw_reads

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
STATS = ("n_reads_ingested", "n_bases_read", "n_bases_ingested", "n_kmers_ingested", "n_unique_kmers", "n_hashed_kmers",
         "any_saturated")
N_CASES = 36
LANES = [0, 1, 3, 10, 129]


def assert_model_is_run(model, run, what):
    assert np.array_equal(model.columns(), run.histograms()), what
    want, got = run.stats, model.totals()
    for f in STATS + (("n_singleton_kmers",) if model.chunks else ()):
        assert got[f] == want[f], (f, what)
    mk, mc = model.export()
    rk, rc = run.merged().export()
    assert np.array_equal(mk, rk) and np.array_equal(mc, rc), what
    model.finalize()  # the reference's invariants hold on a pure ingest


@pytest.mark.parametrize("case", range(N_CASES))
def test_ingest_in_any_number_of_calls_is_the_one_shot_run(orc, case):
    """Cuts anywhere (inside a 1000-read block, twice at the same place: an empty call), k 1…31, 0 to 129 lanes."""
    rng = np.random.default_rng(77_000 + case)
    k = 1 + (case * 7) % 31 if case >= 4 else (1, 2, 30, 31)[case]  # (every residue: 7 and 31 are coprime)
    chunks = LANES[case % len(LANES)]
    histo_max = int(rng.choice([1, 5, 50, 300]))
    shape, bases, offsets = draw_reads(rng)
    n = len(offsets) - 1
    n_cuts = int(rng.integers(1, 6))
    inner = sorted(int(x) for x in rng.integers(0, n + 1, size=n_cuts))
    if case % 3 == 0:
        inner = sorted(inner + [inner[0]])  # an empty call
    if n > 1500:
        inner = sorted(inner + [1000 * int(rng.integers(1, n // 1000 + 1)) - int(rng.integers(1, 999))])  # inside a block
    cuts = [0] + inner + [n]
    what = dict(case=case, k=k, chunks=chunks, histo_max=histo_max, shape=shape, n=n, cuts=cuts)
    run = orc.run_batch(bases, offsets, k, chunks, histo_max)
    model = LaneModel(orc, k, chunks, histo_max)
    model.retain_reads()
    for a, b in zip(cuts[:-1], cuts[1:]):
        if (a + b) % 2:   # either way of handing a run of reads over: a window of the offsets, or a copy from 0
            model.ingest_reads(bases, offsets[a:b + 1])
        else:
            lo, hi = int(offsets[a]), int(offsets[b])
            model.ingest_reads(bases[lo:hi], offsets[a:b + 1] - offsets[a])
    assert model.read_index == n
    assert_model_is_run(model, run, what)
    # the retained list is the concatenation of what went in, whatever the cuts and the lanes
    raw = bases.tobytes()
    assert model.retained == [raw[int(a):int(b)] for a, b in zip(offsets[:-1], offsets[1:])], what
    assert model.retained_info() == dict(reads=n, bases=int(offsets[-1])), what
    rb, ro = model.retained_export(0, n)
    assert np.array_equal(rb, bases[:int(offsets[-1])]) and np.array_equal(ro, offsets), what
    mid = cuts[len(cuts) // 2]
    rb, ro = model.retained_export(mid, n - mid)
    assert np.array_equal(rb, bases[int(offsets[mid]):int(offsets[-1])]) and np.array_equal(ro, offsets[mid:] - offsets[mid]), what


def test_every_k_and_every_lane_count_is_drawn():
    ks = {1 + (c * 7) % 31 if c >= 4 else (1, 2, 30, 31)[c] for c in range(N_CASES)}
    assert ks == set(range(1, 32)) and N_CASES >= 30 and {LANES[c % 5] for c in range(N_CASES)} == set(LANES)


def test_explicit_chunks_and_a_moved_read_index_are_the_same_run(orc):
    """drain_batch with the chunk the striping would have chosen (io.rs:356-358), and set_read_index in front of a
    shard: both rebuild the one-shot run."""
    rng = np.random.default_rng(5)
    _, bases, offsets = draw_reads(np.random.default_rng(12))
    n = len(offsets) - 1
    k, chunks = 17, 3
    run = orc.run_batch(bases, offsets, k, chunks, 50)
    a, b = LaneModel(orc, k, chunks, 50), LaneModel(orc, k, chunks, 50)
    for i, s in enumerate(range(0, n, 1000)):
        e = min(s + 1000, n)
        lo, hi = int(offsets[s]), int(offsets[e])
        a.ingest_batch(i % chunks, bases[lo:hi], offsets[s:e + 1] - offsets[s])
    assert a.read_index == 0
    for s in sorted(range(0, n, 700), key=lambda _: rng.random()):  # shards in any order
        e = min(s + 700, n)
        b.set_read_index(s)
        b.ingest_reads(bases, offsets[s:e + 1])
    for m in (a, b):
        assert_model_is_run(m, run, "explicit")


def _fastq_seqs(path):
    op = gzip.open if path.endswith(".gz") else open
    with op(path, "rb") as f:
        lines = f.read().split(b"\n")
    return [lines[i + 1] for i in range(0, len(lines) - 3, 4)]


def test_the_committed_golden_run_through_the_model(orc):
    """tests/golden/golden_k21_c3.*: -k 21 --chunks 3 --histo-max 50 over the two committed FASTQ files."""
    seqs = _fastq_seqs(os.path.join(G, "reads_main.fastq.gz")) + _fastq_seqs(os.path.join(G, "reads_part2.fastq"))
    want = json.load(open(os.path.join(G, "golden_k21_c3.stats.json")))
    assert len(seqs) == want["n_reads_read"]
    model = LaneModel(orc, 21, 3, 50)
    for a in range(0, len(seqs), 333):  # (not the reference's batches of 1000)
        part = seqs[a:a + 333]
        off = np.zeros(len(part) + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(s) for s in part])
        model.ingest_reads(np.frombuffer(b"".join(part), dtype=np.uint8), off)
    model.finalize()
    got = model.totals()
    for f in STATS + ("n_singleton_kmers",):
        assert got[f] == want[f], f
    rows = [l.split("\t") for l in open(os.path.join(G, "golden_k21_c3.histo")).read().splitlines()[2:]]
    table = np.array([[int(x) for x in r[1:]] for r in rows], dtype=np.uint64)  # (count 1…51) × chunk
    assert [int(r[0]) for r in rows] == list(range(1, 52))
    cols = model.columns()
    assert not cols[:, 0].any() and np.array_equal(cols[:, 1:], table.T)
    final = [l.split("\t") for l in open(os.path.join(G, "golden_k21_c3.final.histo")).read().splitlines()]
    final = [r for r in final if r and r[0].isdigit()]
    assert [int(r[-1]) for r in final] == [int(x) for x in cols[-1][1:1 + len(final)]]


def test_insert_is_kmercounts_insert(orc):
    """test_oracle_kat.py's cases (counting.rs:384-399, 183-200) through the model: accumulate, saturate, a count of
    0 creates the entry, the histogram follows the stored (capped) count and the warning is raised."""
    m = LaneModel(orc, 5, 1, 10)
    with pytest.raises(ModelError, match="No reads were ingested"):
        m.finalize()
    m.insert(0, [42, 42], [3, 7])
    m.insert(0, [1, 1], [U32_MAX, 1])
    assert list(m.get_count([42, 1, 99])) == [10, U32_MAX, 0]
    assert m.totals()["any_saturated"] == 1 and list(m.columns()[0]) == [0] * 10 + [1, 1]
    m.finalize()  # (one lane: Σ lane counts = Σ merged counts, capped alike)
    # across lanes (test_extend_with_histogram_saturation): 0xFFFFFFFE + 5 is stored as u32::MAX, io.rs:1042-1047 fails
    m = LaneModel(orc, 5, 2, 10)
    m.insert(0, [7], [U32_MAX - 1])
    before = m.columns().copy()
    m.insert(1, [7], [5])
    assert list(before[0]) == [0] * 11 + [1] and np.array_equal(m.columns(), np.array([[0] * 11 + [1]] * 2))
    assert list(m.get_count([7])) == [U32_MAX] and m.totals()["any_saturated"] == 1
    with pytest.raises(ModelError, match="hashed kmers"):
        m.finalize()
    # a near-saturating insert moves exactly one bin when an ingest reaches it
    m = LaneModel(orc, 3, 1, 10)
    m.ingest_reads(np.frombuffer(b"ACGTT", dtype=np.uint8), [0, 5])  # ACG ×2 (CGT), AAC ×1 (GTT)
    key = orc.kmers_from_ascii("ACG", 3)[0]
    assert list(m.columns()[0]) == [0, 1, 1] + [0] * 9
    m.insert(0, [key], [U32_MAX - 2])
    assert list(m.columns()[0]) == [0, 1, 0] + [0] * 8 + [1] and m.totals()["any_saturated"] == 1
    # count 0 (test_insert_with_count_zero_keeps_the_key): a key of the table in no bin
    m = LaneModel(orc, 11, 1, 10)
    m.insert(0, [1, 20, 2, 11], [0, 5, 0, 11])
    assert list(m.get_count([1, 20, 2, 11, 7])) == [0, 5, 0, 11, 0]
    with pytest.raises(ModelError, match="unique kmers in the histogram"):
        m.finalize()
    ks, cs = m.export()
    assert list(zip(ks.tolist(), cs.tolist())) == [(1, 0), (2, 0), (11, 11), (20, 5)]
    m0 = LaneModel(orc, 11, 0, 10)  # no histogram, no such invariant (io.rs:1133-1158)
    m0.insert(0, [1], [0])
    assert m0.finalize().n_unique == 1 and m0.columns().shape == (0, 12)
    m.reset()
    assert m.is_empty() and len(m.export()[0]) == 0


def test_an_invalid_byte_is_named_in_input_order(orc):
    m = LaneModel(orc, 5, 2, 10)
    with pytest.raises(ModelError, match="Invalid character 'x' in sequence. Only ACGTN allowed."):
        m.ingest_reads(np.frombuffer(b"ACGTACGTxACGTyACGT", dtype=np.uint8), [0, 4, 18])
    assert m.is_empty()


def test_the_sweep_s_default_draw_covers_every_position_and_kind(orc):
    """The call-sequence sweep (tests/test_gpu_sequences.py) without an engine: its default seeds, drawn and applied
    to the model alone, meet every position and context kind that its own coverage test asks of a GPU run (the
    routes need the engine).  Also a run of the sweep's own code: a draw the model refuses fails here first."""
    import test_gpu_sequences as seq
    met = {}
    for seed, s in enumerate(dry_sequences(orc)):
        for item in s.met_here:
            met.setdefault(item, []).append(seed)
    assert len(seq.POSITIONS) == 27
    missing = [p for p in seq.POSITIONS + ("kind plain", "kind multi-device") if len(met.get(p, ())) < 2]
    assert not missing, (missing, met)


_dry = []


def dry_sequences(orc):
    """The default seeds' sequences applied to the model alone, once for the tests that read them."""
    import test_gpu_sequences as seq
    if not _dry:
        for seed in range(seq.DEFAULT_SEEDS):
            s = seq.dry_sequence(orc, seed)
            s.model = None   # (what the tests read is met_here, facts and ops: the oracle's tables go now)
            _dry.append(s)
    return _dry


def test_the_sweep_s_third_generator_is_not_vacuous(orc):
    """What the retained and panel operations of the default seeds are expected to answer, from the model alone: filters
    that keep reads, threadings with support and with branch links, prunings that remove nodes, dedups with pairs on
    both sides of their threshold.  (Conditions on the draw: if one fails, the draw is what has to change.)"""
    import test_gpu_sequences as seq
    facts = {}
    for s in dry_sequences(orc):
        for name, what in s.facts:
            facts.setdefault(name, []).append(what)
    filters = facts["filter_retained"]
    assert 2 * sum(f["nonempty"] for f in filters) >= len(filters) > 0
    threads = facts["thread_retained"] + facts["thread_panel"]
    assert sum(t["read_edges"] > 0 for t in threads) >= 10 and sum(t["links"] > 0 for t in threads) >= 3
    assert sum(p["removed"] > 0 for p in facts["prune_panel"]) >= 5
    assert sum(d["within"] and d["outside"] for d in facts["dedup_panel"]) >= 5
    n_third = [sum(1 for o in s.ops if o[0] in seq.RETAIN_OPS) for s in dry_sequences(orc)]
    assert 2 * seq.DEFAULT_SEEDS <= sum(n_third) <= 6 * seq.DEFAULT_SEEDS  # (about two to six operations a sequence)


def test_the_graph_observations_leave_the_first_draw_as_it_was():
    """shk_neighborhood and shk_pcr_extend come from a second generator: without them draw_plan(seed) is, for every
    default seed, the plan the sweep drew before they existed (the hash is of that draw's repr)."""
    import test_gpu_sequences as seq
    h = hashlib.sha256()
    n_graph = 0
    for seed in range(seq.DEFAULT_SEEDS):
        contexts, hooks, ops = seq.draw_plan(seed)
        ops = [o for o in ops if o[0] not in seq.RETAIN_OPS]
        base = [o for o in ops if o[0] not in seq.GRAPH_OPS]
        assert (contexts, hooks, base) == seq.draw_base_plan(seed)
        n_graph += len(ops) - len(base)
        h.update(repr((contexts, hooks, base)).encode())
    assert seq.DEFAULT_SEEDS == 96 and h.hexdigest() == "4a017601738b1b7d2396d1b9a9f163ef8f466ec8ee85b189defd05e8fa99e9a3"
    assert n_graph > 2 * seq.DEFAULT_SEEDS  # (about one to five operations of 10-30)


def test_the_third_generator_leaves_the_second_draw_as_it_was():
    """The retained and panel operations come from a third generator: without them draw_plan(seed) is, for every default
    seed, the plan with the graph observations that the sweep drew before they existed (the hash is of that plan's
    repr).  What the generator decides beside the contexts is not in them."""
    import test_gpu_sequences as seq
    h = hashlib.sha256()
    for seed in range(seq.DEFAULT_SEEDS):
        contexts, hooks, ops = seq.draw_plan(seed)
        second = [o for o in ops if o[0] not in seq.RETAIN_OPS]
        assert (contexts, hooks, second) == seq.draw_graph_plan(seed)
        h.update(repr((contexts, hooks, second)).encode())
        props = seq.draw_properties(seed)
        assert len(props) == len(contexts) and all(set(c) == {"k", "chunks", "histo_max", "flags", "hint", "kind"} for c in contexts)
        for c, p in zip(contexts, props):   # retention on one device, the flag on several
            assert not (p["retain"] and p["group_graph"]) and not p[("retain", "group_graph")[c["kind"] == "plain"]]
    assert h.hexdigest() == "9cf56f8cfac95e70177655ca3bee93500600ba2b8271c2deafc40102a2b02467"


def test_neighborhood_and_pcr_extend_over_the_merged_table(orc):
    """The model's two graph calls are tests/pcr_ref.py over the oracle's merged table after the same ingests (in
    several calls, three lanes), whatever the bounds; an insert with count 0 leaves a key that stops a walk."""
    _, bases, offsets = draw_reads(np.random.default_rng(12))
    n = min(len(offsets) - 1, 1500)
    bases, offsets = bases[:int(offsets[n])], offsets[:n + 1]
    k, chunks = 15, 3
    run = orc.run_batch(bases, offsets, k, chunks, 50)
    keys, counts = run.merged().export()
    table = pcr_ref.table_dict(keys, counts)
    model = LaneModel(orc, k, chunks, 50)
    for a in range(0, n, 700):
        model.ingest_reads(bases, offsets[a:min(a + 700, n) + 1])
    mask = (1 << (2 * (k - 1))) - 1
    top = np.argsort(counts, kind="stable")[::-1][:12]
    nodes = [int(x) >> 2 for x in keys[top[:6]]] + [int(x) & mask for x in keys[top[6:]]] + [5, mask]
    dirs = [1 + i % 3 for i in range(len(nodes))]
    walked = 0
    for kw in (dict(min_count=1), dict(min_count=2, max_levels=3), dict(min_count=1, cap=64), dict(min_count=1, cap=0),
               dict(min_count=1, fringe_cap=64, max_levels=6), dict(min_count=int(counts.max())), dict(min_count=0, max_levels=1)):
        got = model.neighborhood(nodes, dirs, **kw)
        want = pcr_ref.neighborhood(nodes, dirs, table, k, kw["min_count"], kw.get("max_levels", 0), kw.get("cap", 1 << 16),
                                    kw.get("fringe_cap", 1 << 16), levels=pcr_ref.neighborhood_levels(nodes, dirs, table, k, kw["min_count"]))
        assert got == want, kw
        walked += got[4]
    assert walked > 10
    some = np.flatnonzero(counts >= 2)  # (the top counts of these reads are low-complexity runs: few neighbours)
    some = some[::len(some) // 8][:8]
    fwd = (keys[some[:4]], counts[some[:4]])
    rev = (keys[some[4:]], counts[some[4:]])
    for kw in (dict(min_count=2, table_min_count=2, high_coverage_ratio=10.0, max_num_nodes=1200, sweep=True),
               dict(min_count=2, table_min_count=1, high_coverage_ratio=1.5, max_num_nodes=50, sweep=False)):
        g, used, steps = model.pcr_extend(fwd, rev, **kw)
        w, wused, wsteps = pcr_ref.pcr_extend(fwd, rev, table, k, **kw)
        assert (g.sub_kmer, g.flags(), g.edges, g.found_path, used, steps) == (w.sub_kmer, w.flags(), w.edges, w.found_path, wused, wsteps)
        assert len(g.sub_kmer) > 8 and g.edges
    # a key of count 0 is in the table and is no edge
    x = int(keys[top[0]])
    node = x >> 2
    first = model.neighborhood([node], [1], 1, max_levels=1)
    assert x in first[0] or int(pcr_ref.revcomp(x, k)) in first[0]
    zeroed = LaneModel(orc, k, 1, 50)
    zeroed.insert(0, [x], [0])
    assert zeroed.neighborhood([node], [1], 0, max_levels=1) == ([], [], [], [], 1)
    assert list(zeroed.export()[1]) == [0]


def test_the_graph_calls_sum_lanes_with_saturation_and_refuse_as_the_abi_does(orc):
    """Two lanes whose counts add past 2^32 − 1: the count reported is 2^32 − 1, accepted at min_count 2^32 − 1 where
    2^32 − 2 is not.  A multi-device context is SHK_ERR_STATE, k = 1 and more seeds than fringe_cap SHK_ERR_BAD_ARG."""
    k = 5
    m = LaneModel(orc, k, 2, 10)
    x, y = 0b0001101100, 0b0110110001  # ACGTA → CGTAC, canonical both (AC… < GT…)
    assert x <= pcr_ref.revcomp(x, k) and y <= pcr_ref.revcomp(y, k) and (x & 0xFF) == y >> 2
    m.insert(0, [x, y], [U32_MAX - 1, U32_MAX - 2])
    m.insert(1, [x], [7])
    assert m.neighborhood([x >> 2], [1], U32_MAX) == ([x], [U32_MAX], [], [], 2)
    assert m.neighborhood([x >> 2], [1], U32_MAX - 2)[:2] == ([x, y], [U32_MAX, U32_MAX - 2])
    g, used, steps = m.pcr_extend(([x], [U32_MAX]), ([], []), min_count=U32_MAX, table_min_count=1, high_coverage_ratio=10.0,
                                  max_num_nodes=100, sweep=False)
    assert g.edges == [(0, 1, U32_MAX)] and (used, steps) == (U32_MAX, 1)  # (y, at 2^32 − 3, is below the threshold)
    with pytest.raises(ModelError) as e:
        m.neighborhood([1, 2], [3, 1], 1, fringe_cap=2)
    assert e.value.code == SHK_ERR_BAD_ARG
    with pytest.raises(ModelError) as e:
        m.neighborhood([1 << 8], [1], 1)
    assert e.value.code == SHK_ERR_BAD_ARG
    for call in (lambda mm: mm.neighborhood([0], [1], 1), lambda mm: mm.pcr_extend(([], []), ([], []))):
        with pytest.raises(ModelError) as e:
            call(LaneModel(orc, k, 2, 10, multi_device=True))
        assert e.value.code == SHK_ERR_STATE and "multi-device context" in str(e.value)
        with pytest.raises(ModelError) as e:
            call(LaneModel(orc, 1, 2, 10))
        assert e.value.code == SHK_ERR_BAD_ARG
    # SHK_FLAG_GROUP_GRAPH: the multi-device context answers as the merged view
    flagged = LaneModel(orc, k, 2, 10, multi_device=True, group_graph=True)
    flagged.insert(0, [x, y], [U32_MAX - 1, U32_MAX - 2])
    flagged.insert(1, [x], [7])
    assert flagged.neighborhood([x >> 2], [1], U32_MAX) == m.neighborhood([x >> 2], [1], U32_MAX)
    assert flagged.neighborhood_panel([([x >> 2], [1], U32_MAX - 2, 64, 64)] * 2, 0) == [m.neighborhood([x >> 2], [1], U32_MAX - 2, 0, 64, 64)] * 2


def test_retention_is_a_switch_and_a_list_and_refuses_as_the_abi_does(orc):
    reads = [b"ACGTACGTTGCA", b"", b"NNACGTN", b"TTTTTTGCA"]
    bases = np.frombuffer(b"".join(reads), dtype=np.uint8)
    offsets = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.uint64)
    m = LaneModel(orc, 5, 3, 10)
    for call in (lambda: m.retained_export(0, 0), lambda: m.filter_retained([[1]]), lambda: m.thread_retained([], [])):
        with pytest.raises(ModelError, match="reads are not retained") as e:
            call()
        assert e.value.code == SHK_ERR_STATE
    assert m.retained_info() == dict(reads=0, bases=0)
    m.ingest_reads(bases, offsets)
    assert m.retained == []
    with pytest.raises(ModelError, match="holds reads already") as e:
        m.retain_reads()
    assert e.value.code == SHK_ERR_STATE
    m.reset()
    m.retain_reads()
    m.retain_reads()   # on twice over an empty store: accepted
    m.set_read_index(999)   # whatever the read index and the lane: arrival order
    m.ingest_reads(bases, offsets[:3])
    m.ingest_batch(2, bases, offsets[2:])
    assert m.retained == reads and m.retained_info() == dict(reads=4, bases=len(bases))
    with pytest.raises(ModelError, match="retained already"):
        m.retain_reads()
    with pytest.raises(ModelError, match="outside the 4 retained reads") as e:
        m.retained_export(3, 2)
    assert e.value.code == SHK_ERR_BAD_ARG
    rb, ro = m.retained_export(1, 2)
    assert bytes(rb) == b"NNACGTN" and ro.tolist() == [0, 0, 7] and m.retained_export(4, 0)[1].tolist() == [0]
    m.reset()   # emptied; the switch stays
    assert m.retained == [] and m.retain
    m.ingest_reads(bases, offsets[:2])
    assert m.retained == reads[:1]
    m.retain_reads(False)
    assert m.retained == [] and not m.retain
    multi = LaneModel(orc, 5, 3, 10, multi_device=True, group_graph=True)   # the flag changes nothing here
    for call in (lambda: multi.retain_reads(), lambda: multi.retained_info(), lambda: multi.retained_export(0, 0),
                 lambda: multi.filter_retained([[1]]), lambda: multi.thread_retained([], [])):
        with pytest.raises(ModelError, match="not available on a multi-device context") as e:
            call()
        assert e.value.code == SHK_ERR_STATE


def test_the_model_s_panel_answers_are_the_reference_modules(orc):
    """One fixed input each: the model's filter is panel_cases.expected (the oracle's filter_matches), its threading
    tests/thread_ref.py as thread_panel_cases.expected reads it, its pruning tests/prune_ref.py, its dedup
    tests/products_ref.py, its panel neighbourhood tests/pcr_ref.py — the sweep and the model cannot share a mistake there."""
    import panel_cases as pc
    import products_ref
    import prune_cases
    import thread_panel_cases as tp
    # the filter: the several-genes case (a read in three genes, a duplicate k-mer, an empty gene)
    case = [c for c in pc.crafted_cases(orc) if "a read in three genes" in c.name][0]
    m = LaneModel(orc, case.k, 1, 10)
    assert m.filter_reads_panel(case.reads, case.genes) == pc.expected(orc, case) == [[0], [0, 1], [], [0, 1, 3], [0, 1], []]
    m.retain_reads()
    m.ingest_reads(*pack(case.reads))
    assert m.filter_retained(case.genes) == pc.expected(orc, case)
    # the threading: every crafted case as one panel (reads with an invalid byte cannot be retained: the host form), and
    # the paired panel through the store
    for p, retained in ((tp.crafted_panel(), False), (tp.paired_panel(), True), (tp.lists_panel(), False)):
        m = LaneModel(orc, p.k, 1, 10)
        graphs = [(g.sub_kmer, g.edges) for g in p.graphs]
        want = [tp.rows(a, len(g.edges)) for a, g in zip(tp.expected(p), p.graphs)]
        assert m.thread_reads_panel(p.reads, graphs, p.lists, p.read_index, p.mate) == want, p.name
        if retained:
            m.retain_reads()
            m.ingest_reads(*pack(p.reads))
            assert m.thread_retained(graphs, p.lists, p.read_index, p.mate) == want and want[0][5] == 1, p.name
    with pytest.raises(ModelError) as e:
        LaneModel(orc, 1, 1, 10).thread_reads_panel([], [], [])
    assert e.value.code == SHK_ERR_BAD_ARG
    # the pruning: every crafted case, in one panel per k
    cases = prune_cases.cases()
    for k in sorted({c.k for c in cases}):
        some = [c for c in cases if c.k == k]
        got = LaneModel(orc, k, 1, 10).prune_panel([(c.flags, [e[0] for e in c.edges], [e[1] for e in c.edges], [e[2] for e in c.edges]) for c in some],
                                                    [c.fraction for c in some], [c.stages for c in some])
        assert got == [c.expected() for c in some]
    assert any(sum(c.expected().node_keep) < len(c.flags) for c in cases)
    # the dedup: the greedy pass follows the sorted order, not the input's
    a, b, c = "ACGTACGTAC", "ACGTACGTAA", "ACGTACGTTA"   # a–b and b–c are one apart, a–c two
    seqs, scores = [c, b, a], [1.0, 2.0, 3.0]
    (got,) = LaneModel.dedup_panel([seqs], [scores], [1])
    order = products_ref.sort_order(seqs, scores)
    kept, retained = products_ref.sort_and_deduplicate(seqs, scores, 1)
    assert got == (order, products_ref.pair_matrix(seqs, order, 1), kept, 3, retained)
    assert got == ([2, 1, 0], [True, False, True], [2, 0], 3, 2)


def pack(reads):
    offsets = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.uint64)
    return np.frombuffer(b"".join(reads), dtype=np.uint8), offsets
