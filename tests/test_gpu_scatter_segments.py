"""Cursor segments of k_scatter32's page regions (SHK_SC32_SEGS = S): on the immediate one-level route a partition's
region is S segments, each with its own cursor word and capacity; a scatter workgroup reserves in segment
blockIdx.x % S, and k_pages32 — the first pass and the one that materialises a virtual table — reads a lane's S segments
into the same counts.  Tables: 256 pages at k = 19 (the scatter's run-time fan-out), 1024 pages at k = 21 (its LOGP = 10
variant, the flagship's) — and 256 pages at k = 21, whose records take 34 bits: 8-byte records, k_scatter64, where the
hook must change nothing.  Each with one lane's regions and with three lanes' (all-lanes mode).  Everything is
bit-exact against the oracle for every S; the route is read off the timing slots."""
import numpy as np
import pytest

import sharkmer_amd as sa
from test_gpu_fused_hist import genome_reads

pytestmark = pytest.mark.gpu

FLAGS = sa.FLAG_FORCE_PAGED | sa.FLAG_TIMING
# name → (k, capacity_hint, pages, reads of 150 bp, genome): the batches are large enough for the paged route on their own
SHAPES = {"p256": (21, 700_000, 256, 12_000, 100_000), "p256k19": (19, 700_000, 256, 12_000, 100_000),
          "p1024": (21, 3_000_000, 1024, 40_000, 300_000)}
REC32 = {"p256": False, "p256k19": True, "p1024": True}   # 4-byte records: k_scatter32 + k_pages32, the fused histogram
SEGS = [1, 2, 8]
LANES = [0, 3]
_cache = {}


def case(orc, shape, chunks, kind, hm=10000):
    """(bases, offsets, oracle run, its keys, its counts) of a named input; computed once, never modified."""
    key = (shape, chunks, kind, hm)
    if key in _cache:
        return _cache[key]
    k, hint, pages, n_reads, genome = SHAPES[shape]
    rng = np.random.default_rng(pages + 7 * chunks)
    if kind == "full":
        bases, offsets = genome_reads(rng, genome, n_reads, 150, p_n=0.002)
    elif kind == "tiles3":                    # three tiles of 16384 positions: most segments of most partitions stay empty
        bases, offsets = genome_reads(rng, genome, 3 * 16384 // 150, 150, p_n=0.002)
    elif kind == "repeat":                    # every read is the same sequence of period 10: ten hot k-mers, every
        unit = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=10)]   # other partition empty — the hot
        bases = np.tile(unit, 15 * 3000)      # ones overflow their segments (≈ 1420 records per tile and k-mer, three
        offsets = np.arange(3001, dtype=np.uint64) * np.uint64(150)                   # tiles or more against ≤ 3072)
    else:
        raise KeyError(kind)
    bases.setflags(write=False)
    offsets.setflags(write=False)
    ref = orc.run_batch(bases, offsets, k, chunks, hm)
    rk, rc = ref.merged().export()
    _cache[key] = (bases, offsets, ref, rk, rc)
    return _cache[key]


def check_hist(eng, ref, chunks):
    assert np.array_equal(eng.histograms(), ref.histograms())
    cnt, st = eng.counters(), ref.stats
    for f in ("n_reads_ingested", "n_bases_read", "n_bases_ingested", "n_kmers_ingested", "n_unique_kmers", "n_hashed_kmers"):
        assert cnt[f] == st[f], f
    if chunks > 0:
        assert cnt["n_singleton_kmers"] == st["n_singleton_kmers"]
    return cnt


def check_table(eng, rk, rc):
    gk, gc = eng.export_table()
    assert np.array_equal(gk, rk) and np.array_equal(gc, rc)


def n_mat(eng):
    return eng.timings().get("materialise", (0.0, 0))[1]


def engine(shape, chunks, hm=10000):
    k, hint, pages, _, _ = SHAPES[shape]
    eng = sa.KmerEngine(k, chunks, hm, capacity_hint=hint, flags=FLAGS)
    assert eng.table_geometry()[0] == pages
    return eng


@pytest.fixture(autouse=True)
def _hooks(monkeypatch, segs):
    monkeypatch.setenv("SHK_SLICE_KB", str(1 << 20))  # (a host batch as ONE launch)
    if segs is None:
        monkeypatch.delenv("SHK_SC32_SEGS", raising=False)
    else:
        monkeypatch.setenv("SHK_SC32_SEGS", str(segs))


def check_segs(eng, shape, segs):
    """The hook took effect: the last launch's page regions had `segs` cursor segments (8-byte records: always one)."""
    assert eng.scatter_segments() == (segs if REC32[shape] else 1)


def one_fused_launch(tim, shape):
    """4-byte records: one scatter and one page pass, which left the histogram rows, and nobody wrote a table.  8-byte
    records: one level (a pass per lane), and neither rows nor a virtual table."""
    assert "pscan" not in tim, tim
    if REC32[shape]:
        assert tim["scatter"][1] == 1 and tim["pages"][1] == 1, tim
        assert "histo_rows" in tim and "histo" not in tim and "materialise" not in tim, tim
    else:
        assert tim["scatter"][1] >= 1 and "histo_rows" not in tim and "materialise" not in tim, tim


@pytest.mark.parametrize("segs", SEGS)
@pytest.mark.parametrize("chunks", LANES)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_job_table_reset_job(orc, shape, chunks, segs):
    """A histogram-only job; lookup and export afterwards (the virtual table is written from the segments); reset, and
    the same job again."""
    bases, offsets, ref, rk, rc = case(orc, shape, chunks, "full")
    with engine(shape, chunks) as eng:
        assert eng.scatter_segments() == 0
        eng.ingest_reads(bases, offsets)
        check_segs(eng, shape, segs)
        eng.finalize()
        cnt = check_hist(eng, ref, chunks)
        one_fused_launch(eng.timings(), shape)
        assert cnt["n_spilled"] == 0
        assert np.array_equal(eng.lookup(rk[::97]), rc[::97])
        assert n_mat(eng) == (1 if REC32[shape] else 0)
        check_table(eng, rk, rc)
        assert n_mat(eng) == (1 if REC32[shape] else 0) and (eng.timings()["pages"][1] == 1 or not REC32[shape])
        eng.reset()
        eng.reset_timings()
        eng.ingest_reads(bases, offsets)
        eng.finalize()
        check_hist(eng, ref, chunks)
        tim = eng.timings()
        assert (tim["scatter"][1] == 1 and tim["pages"][1] == 1 or not REC32[shape]) and ("histo_rows" in tim) == REC32[shape], tim
        check_table(eng, rk, rc)


@pytest.mark.parametrize("segs", SEGS)
@pytest.mark.parametrize("chunks", LANES)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_second_ingest(orc, shape, chunks, segs):
    """Two ingests on one context: the second one's page pass is not fresh — it reads the segments into a table that
    holds the first one's counts."""
    bases, offsets, ref, rk, rc = case(orc, shape, chunks, "full")
    half = (len(offsets) - 1) // 2
    with engine(shape, chunks) as eng:
        eng.ingest_reads(bases, offsets[:half + 1])
        eng.ingest_reads(bases, offsets[half:])      # (offsets are positions in `bases`)
        check_segs(eng, shape, segs)
        eng.finalize()
        check_hist(eng, ref, chunks)
        tim = eng.timings()
        assert (tim["scatter"][1] == 2 and tim["pages"][1] == 2 or not REC32[shape]) and "pscan" not in tim, tim
        check_table(eng, rk, rc)


@pytest.mark.parametrize("segs", SEGS)
@pytest.mark.parametrize("chunks", LANES)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_three_tiles(orc, shape, chunks, segs):
    """327 reads: three workgroups scatter, so at most three segments of a partition hold anything — and with three
    lanes the batch is lane 0's alone (a block of 1000 reads is one lane's): one lane's pass, not a fresh one."""
    bases, offsets, ref, rk, rc = case(orc, shape, chunks, "tiles3")
    with engine(shape, chunks) as eng:
        eng.ingest_reads(bases, offsets)
        check_segs(eng, shape, segs)
        eng.finalize()
        check_hist(eng, ref, chunks)
        tim = eng.timings()
        assert tim["scatter"][1] == 1 and tim["pages"][1] == 1 and "pscan" not in tim, tim
        if chunks == 0:
            one_fused_launch(tim, shape)
        check_table(eng, rk, rc)


@pytest.mark.parametrize("segs", SEGS)
@pytest.mark.parametrize("chunks", LANES)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_one_repeated_sequence(orc, shape, chunks, segs):
    """Hot partitions overflow their segments: the excess takes the spill path, and the result is exact."""
    bases, offsets, ref, rk, rc = case(orc, shape, chunks, "repeat")
    with engine(shape, chunks) as eng:
        eng.ingest_reads(bases, offsets)
        check_segs(eng, shape, segs)
        eng.finalize()
        cnt = check_hist(eng, ref, chunks)
        tim = eng.timings()
        assert (tim["scatter"][1] == 1 or not REC32[shape]) and tim["pages"][1] >= 1 and "pscan" not in tim, tim
        assert cnt["n_spilled"] > 10_000
        check_table(eng, rk, rc)


@pytest.mark.parametrize("segs", SEGS)
@pytest.mark.parametrize("chunks", LANES)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_histo_max_below_every_sum(orc, shape, chunks, segs):
    """18x coverage and more against histo_max = 3: all but a few sums land in the last bin."""
    bases, offsets, ref, rk, rc = case(orc, shape, chunks, "full", hm=3)
    with engine(shape, chunks, hm=3) as eng:
        eng.ingest_reads(bases, offsets)
        check_segs(eng, shape, segs)
        eng.finalize()
        check_hist(eng, ref, chunks)
        one_fused_launch(eng.timings(), shape)


@pytest.mark.parametrize("segs", [None])
@pytest.mark.parametrize("chunks", LANES)
def test_the_library_s_own_choice(orc, chunks, segs):
    """Without the hook: four segments for one lane's regions, one for an all-lanes launch (and its lanes' regions are
    what they were)."""
    bases, offsets, ref, rk, rc = case(orc, "p1024", chunks, "full")
    with engine("p1024", chunks) as eng:
        eng.ingest_reads(bases, offsets)
        assert eng.scatter_segments() == (4 if chunks == 0 else 1)
        eng.finalize()
        check_hist(eng, ref, chunks)
        one_fused_launch(eng.timings(), "p1024")
        check_table(eng, rk, rc)
