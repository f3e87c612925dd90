"""The per-lane model of tests/lane_model.py, pinned before it judges the engine (tests/test_gpu_sequences.py):
whatever the model and the oracle's one-shot driver share — histogram columns, totals, the merged table — must be
equal when the model is fed the same reads in any number of calls, and its insert must be KmerCounts::insert with
the saturating cases of test_oracle_kat.py.  No GPU."""
import gzip
import json
import os

import numpy as np
import pytest

from lane_model import LaneModel, ModelError, U32_MAX
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
    for a, b in zip(cuts[:-1], cuts[1:]):
        if (a + b) % 2:   # either way of handing a run of reads over: a window of the offsets, or a copy from 0
            model.ingest_reads(bases, offsets[a:b + 1])
        else:
            lo, hi = int(offsets[a]), int(offsets[b])
            model.ingest_reads(bases[lo:hi], offsets[a:b + 1] - offsets[a])
    assert model.read_index == n
    assert_model_is_run(model, run, what)


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
    for seed in range(seq.DEFAULT_SEEDS):
        for item in seq.dry_run(orc, seed):
            met.setdefault(item, []).append(seed)
    missing = [p for p in seq.POSITIONS + ("kind plain", "kind multi-device") if len(met.get(p, ())) < 2]
    assert not missing, (missing, met)
