"""The table a histogram job never writes.  A fresh fused page pass (k_pages32<true, HIST, false>) leaves the histogram
rows, the totals, its spills and n_distinct — and no table: the table is then VIRTUAL, defined by the records and cursors
of that launch, and whoever touches it first (tb_fresh) has the ordinary fresh pass run over them (the "materialise"
timing slot).  Everything here is bit-exact against the oracle; the route is read off the timing slots.
SHK_LAZY_TABLE is read at every launch: 0 = the pass always writes the table, 1 = the library's choice (a context that has
materialised once writes eagerly from then on), 2 = virtual wherever the pass is fused."""
import numpy as np
import pytest

import sharkmer_amd as sa
from test_gpu_fused_hist import genome_reads, HINT

pytestmark = pytest.mark.gpu

FLAGS = sa.FLAG_FORCE_PAGED | sa.FLAG_TIMING
_cache = {}


def case(orc, name):
    """(bases, offsets, k, chunks, histo_max, oracle run) of a named input; computed once, never modified."""
    if name in _cache:
        return _cache[name]
    k, hm = 21, 10000
    if name in ("lanes0", "lanes3", "lanes10", "fold"):
        chunks = {"lanes0": 0, "lanes3": 3, "lanes10": 10, "fold": 3}[name]
        hm = 7 if name == "fold" else 10000        # "fold": histo_max below every sum (20x coverage)
        rng = np.random.default_rng(100 + chunks + hm)
        # ragged reads with N runs: 37 … 163 bases, blocks of 1000 reads go round the lanes
        g = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=20000)]
        lens = rng.integers(37, 164, size=11500 if chunks == 10 else 4300)
        starts = rng.integers(0, len(g) - 163, size=len(lens))
        bases = np.concatenate([g[s:s + n] for s, n in zip(starts, lens)]).copy()
        bases[rng.random(len(bases)) < 0.002] = ord("N")
        for at in rng.integers(0, len(bases) - 40, size=25):
            bases[at:at + 30] = ord("N")
        offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    elif name == "other":                          # a second job's reads: another genome
        chunks = 3
        bases, offsets = genome_reads(np.random.default_rng(77), 15000, 3500, 90, p_n=0.002)
    elif name == "spill":                          # k = 17 on 8 pages: 150 k distinct k-mers do not fit, and a hot region overflows
        k, chunks, hm = 17, 2, 1000
        rng = np.random.default_rng(31)
        bases, offsets = genome_reads(rng, 150000, 4000, 100, p_n=0.001)
        hot = rng.random(4000) < 0.3
        b2 = bases.reshape(4000, 100)
        b2[hot] = ord("A")
        bases = b2.reshape(-1)
    elif name == "grow":                           # k = 19 on 256 pages
        k, chunks, hm = 19, 2, 1000
        bases, offsets = genome_reads(np.random.default_rng(41), 20000, 4000, 100, p_n=0.001)
    else:
        raise KeyError(name)
    bases.setflags(write=False)
    offsets.setflags(write=False)
    ref = orc.run_batch(bases, offsets, k, chunks, hm)
    rk, rc = ref.merged().export()
    _cache[name] = (bases, offsets, k, chunks, hm, ref, rk, rc)
    return _cache[name]


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


@pytest.fixture(autouse=True)
def _one_launch_per_batch(monkeypatch):
    monkeypatch.setenv("SHK_SLICE_KB", str(1 << 20))  # (a host batch as ONE launch: a second slice is a second ingest)


@pytest.mark.parametrize("name", ["lanes0", "lanes3", "lanes10", "fold"])
def test_histogram_job_then_export(orc, name):
    bases, offsets, k, chunks, hm, ref, rk, rc = case(orc, name)
    with sa.KmerEngine(k, chunks, hm, capacity_hint=HINT, flags=FLAGS) as eng:
        eng.ingest_reads(bases, offsets)
        eng.finalize()
        cnt = check_hist(eng, ref, chunks)
        tim = eng.timings()
        assert "histo_rows" in tim and "histo" not in tim, tim       # the fused pass's histogram …
        assert "materialise" not in tim and tim["pages"][1] == 1, tim  # … and nobody wrote a table
        assert cnt["n_spilled"] == 0
        check_table(eng, rk, rc)                                      # export after finalize
        assert n_mat(eng) == 1
        check_table(eng, rk, rc)                                      # again, and a lookup: the table is there now
        assert np.array_equal(eng.lookup(rk[:200]), rc[:200])
        assert n_mat(eng) == 1 and eng.timings()["pages"][1] == 1
        eng.finalize()
        check_hist(eng, ref, chunks)                                  # (nothing was added to the totals a second time)


def test_second_ingest(orc):
    bases, offsets, k, chunks, hm, ref, rk, rc = case(orc, "lanes3")
    with sa.KmerEngine(k, chunks, hm, capacity_hint=HINT, flags=FLAGS) as eng:
        eng.ingest_reads(bases, offsets[:2501])      # paged now, fresh, fused: virtual
        eng.sync()
        assert n_mat(eng) == 0
        eng.ingest_reads(bases, offsets[2500:])      # (offsets are positions in `bases`)
        eng.finalize()
        check_hist(eng, ref, chunks)
        assert n_mat(eng) == 1
        check_table(eng, rk, rc)
        assert n_mat(eng) == 1


@pytest.mark.parametrize("first", ["lookup", "insert"])
def test_first_caller_behind_a_virtual_table(orc, first):
    bases, offsets, k, chunks, hm, ref, rk, rc = case(orc, "lanes3")
    with sa.KmerEngine(k, chunks, hm, capacity_hint=HINT, flags=FLAGS) as eng:
        eng.ingest_reads(bases, offsets)
        if first == "lookup":
            probe = np.concatenate([rk[::7], np.array([0, 5, (1 << 42) - 1], dtype=np.uint64)])
            want = np.concatenate([rc[::7], np.zeros(3, dtype=np.uint32)])
            present = np.isin(probe[-3:], rk)
            want[-3:][present] = rc[np.searchsorted(rk, probe[-3:][present])]
            assert np.array_equal(eng.lookup(probe), want)
            assert n_mat(eng) == 1
            eng.finalize()
            check_hist(eng, ref, chunks)
            check_table(eng, rk, rc)
        else:
            eng.insert(np.array([rk[3], rk[10]], dtype=np.uint64), np.array([5, 9], dtype=np.uint32), chunk_id=2)
            assert n_mat(eng) == 1
            eng.finalize()
            want = rc.copy()
            want[3] += 5
            want[10] += 9
            check_table(eng, rk, want)
            h = ref.histograms().copy()              # column 2 = lanes 0..2 merged
            for i, add in ((3, 5), (10, 9)):
                h[2][int(rc[i])] -= 1
                h[2][int(rc[i]) + add] += 1
            assert np.array_equal(eng.histograms(), h)
        assert n_mat(eng) == 1


def test_insert_that_grows_the_table(orc):
    bases, offsets, k, chunks, hm, ref, rk, rc = case(orc, "grow")
    rng = np.random.default_rng(43)
    ik = np.unique(rng.integers(0, 1 << 38, size=1_150_000, dtype=np.uint64))   # > half of 2^21 slots
    ic = rng.integers(1, 4, size=len(ik), dtype=np.uint32)
    with sa.KmerEngine(k, chunks, hm, capacity_hint=1_000_000, flags=FLAGS) as eng:
        assert eng.table_geometry()[0] == 256
        eng.ingest_reads(bases, offsets)
        eng.sync()
        assert n_mat(eng) == 0
        eng.insert(ik, ic, chunk_id=1)
        assert n_mat(eng) == 1 and eng.counters()["n_grows"] >= 1
        eng.finalize()
        gk, gc = eng.export_table()
    wk, inv = np.unique(np.concatenate([rk, ik]), return_inverse=True)
    wc = np.zeros(len(wk), dtype=np.uint64)
    np.add.at(wc, inv, np.concatenate([rc, ic]).astype(np.uint64))
    assert np.array_equal(gk, wk) and np.array_equal(gc.astype(np.uint64), wc)


@pytest.mark.parametrize("mode", ["1", "0"])
def test_spills(orc, monkeypatch, mode):
    """A capacity hint far too low: the histogram-only pass spills what its pages cannot take (and the scatter what its
    hot region cannot) — the repair needs the table, so it is written: exact, spill path taken, table right."""
    monkeypatch.setenv("SHK_LAZY_TABLE", mode)
    bases, offsets, k, chunks, hm, ref, rk, rc = case(orc, "spill")
    with sa.KmerEngine(k, chunks, hm, capacity_hint=30_000, flags=FLAGS) as eng:
        assert eng.table_geometry()[0] == 8
        eng.ingest_reads(bases, offsets)
        eng.finalize()
        cnt = check_hist(eng, ref, chunks)
        assert cnt["n_spilled"] > 10_000 and cnt["n_grows"] >= 1
        assert n_mat(eng) == (1 if mode == "1" else 0)
        check_table(eng, rk, rc)
        assert n_mat(eng) == (1 if mode == "1" else 0)


def test_reset_drops_the_virtual_table(orc, monkeypatch):
    monkeypatch.setenv("SHK_LAZY_TABLE", "2")
    a = case(orc, "lanes3")
    bases, offsets, k, chunks, hm, ref, rk, rc = case(orc, "other")
    with sa.KmerEngine(k, chunks, hm, capacity_hint=HINT, flags=FLAGS) as eng:
        eng.ingest_reads(a[0], a[1])                 # job A: virtual, never written
        eng.finalize()
        eng.reset()
        assert n_mat(eng) == 0
        eng.ingest_reads(bases, offsets)             # job B
        eng.finalize()
        check_hist(eng, ref, chunks)
        assert n_mat(eng) == 0
        check_table(eng, rk, rc)                     # B's records, and only B's
        assert n_mat(eng) == 1
        eng.reset()                                  # a reset right behind a virtual launch nobody has looked at
        eng.ingest_reads(a[0], a[1])
        eng.reset()
        eng.ingest_reads(bases, offsets)
        check_table(eng, rk, rc)
        eng.finalize()
        check_hist(eng, ref, chunks)


@pytest.mark.parametrize("mode", ["1", "2"])
def test_switch_off(orc, monkeypatch, mode):
    monkeypatch.setenv("SHK_LAZY_TABLE", mode)
    bases, offsets, k, chunks, hm, ref, rk, rc = case(orc, "lanes3")
    with sa.KmerEngine(k, chunks, hm, capacity_hint=HINT, flags=FLAGS) as eng:
        eng.ingest_reads(bases, offsets)
        assert np.array_equal(eng.lookup(rk[:50]), rc[:50])
        assert n_mat(eng) == 1
        eng.reset()
        eng.reset_timings()
        eng.ingest_reads(bases, offsets)             # the job after a materialise writes eagerly (2: it does not)
        eng.finalize()
        check_hist(eng, ref, chunks)
        assert "histo_rows" in eng.timings()
        assert np.array_equal(eng.lookup(rk[:50]), rc[:50])
        assert n_mat(eng) == (1 if mode == "2" else 0)
        check_table(eng, rk, rc)


@pytest.mark.parametrize("name", ["lanes0", "lanes10", "spill"])
def test_route_parity(orc, monkeypatch, name):
    bases, offsets, k, chunks, hm, ref, rk, rc = case(orc, name)
    out = {}
    for mode in ("0", "2"):
        monkeypatch.setenv("SHK_LAZY_TABLE", mode)
        with sa.KmerEngine(k, chunks, hm, capacity_hint=30_000 if name == "spill" else HINT, flags=FLAGS) as eng:
            eng.ingest_reads(bases, offsets)
            eng.finalize()
            h, c = eng.histograms(), eng.counters()
            m0 = n_mat(eng)
            t = eng.export_table()
            out[mode] = (h, {f: v for f, v in c.items() if f not in ("n_spilled", "n_grows", "table_capacity")}, t, m0, n_mat(eng))
    assert np.array_equal(out["0"][0], out["2"][0]) and np.array_equal(out["0"][0], ref.histograms())
    assert out["0"][1] == out["2"][1]
    for m in ("0", "2"):
        assert np.array_equal(out[m][2][0], rk) and np.array_equal(out[m][2][1], rc)
    assert out["0"][3:] == (0, 0)
    assert out["2"][3:] == ((1, 1) if name == "spill" else (0, 1))


@pytest.mark.parametrize("mode", ["1", "2"])
@pytest.mark.parametrize("name", ["lanes0", "lanes3"])
def test_device_batch_in_sub_launches(orc, monkeypatch, name, mode):
    """One device-resident batch counted as several launches (a batch above the bases-per-launch bound; SHK_SUB_KB
    lowers the bound to 128 Ki bases here, so ≈ 430 k bases are four launches or more).  Every launch's scatter takes
    the regions and cursors of the one before: the first launch — fresh and fused — writes its table, nothing is
    replayed, and the last launch is not fresh.  Then a batch below the bound on the same context: virtual again."""
    import torch
    monkeypatch.setenv("SHK_LAZY_TABLE", mode)
    monkeypatch.setenv("SHK_SUB_KB", "128")
    bases, offsets, k, chunks, hm, ref, rk, rc = case(orc, name)
    assert len(bases) > 3 * (128 << 10)
    db = torch.from_numpy(bases.copy()).cuda()
    do = torch.from_numpy(offsets.astype(np.int64)).cuda()
    torch.cuda.synchronize()
    with sa.KmerEngine(k, chunks, hm, capacity_hint=HINT, flags=FLAGS) as eng:
        eng.ingest_reads_device(db.data_ptr(), do.data_ptr(), len(offsets) - 1, len(bases))
        eng.sync()
        tim = eng.timings()
        assert tim["pages"][1] >= 4 and "materialise" not in tim, tim
        eng.finalize()
        check_hist(eng, ref, chunks)
        check_table(eng, rk, rc)
        assert n_mat(eng) == 0
        monkeypatch.delenv("SHK_SUB_KB")
        eng.reset()
        eng.reset_timings()
        eng.ingest_reads_device(db.data_ptr(), do.data_ptr(), len(offsets) - 1, len(bases))   # one launch
        eng.finalize()
        check_hist(eng, ref, chunks)
        assert eng.timings()["pages"][1] == 1 and n_mat(eng) == 0
        check_table(eng, rk, rc)
        assert n_mat(eng) == 1


def test_sliced_host_batch_stays_eager(orc, monkeypatch):
    """Slices of one host batch: every slice but the last is followed by a launch that needs the table, so none of
    them leaves it virtual — no materialising pass, and the context keeps its choice for later jobs."""
    monkeypatch.setenv("SHK_SLICE_KB", "64")
    bases, offsets, k, chunks, hm, ref, rk, rc = case(orc, "lanes3")
    with sa.KmerEngine(k, chunks, hm, capacity_hint=HINT, flags=FLAGS) as eng:
        eng.ingest_reads(bases, offsets)
        eng.finalize()
        check_hist(eng, ref, chunks)
        tim = eng.timings()
        assert tim["pages"][1] > 1 and "materialise" not in tim, tim
        check_table(eng, rk, rc)
        assert n_mat(eng) == 0
        monkeypatch.setenv("SHK_SLICE_KB", str(1 << 20))
        eng.reset()
        eng.reset_timings()
        eng.ingest_reads(bases, offsets)             # one launch: virtual again
        eng.finalize()
        check_hist(eng, ref, chunks)
        assert n_mat(eng) == 0
        check_table(eng, rk, rc)
        assert n_mat(eng) == 1
