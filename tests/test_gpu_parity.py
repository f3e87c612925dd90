"""GPU parity tests: the HIP path, called through the C ABI (sharkmer_amd.KmerEngine is a
ctypes shim over include/shk.h), against the CPU oracle on identical inputs.  Bit-exact:
every comparison is integer equality.  Test names follow the reference's own tests
(src/kmer/mod.rs, src/kmer/counting.rs, tests/spcr_18s.rs) where they mirror one."""
import os

import numpy as np
import pytest

import sharkmer_amd as sa

pytestmark = pytest.mark.gpu

FLAGSETS = [0, sa.FLAG_FORCE_DIRECT, sa.FLAG_FORCE_PAGED]


def pack(seqs):
    bs = [s.encode() if isinstance(s, str) else bytes(s) for s in seqs]
    offsets = np.zeros(len(bs) + 1, dtype=np.uint64)
    if bs:
        offsets[1:] = np.cumsum([len(b) for b in bs])
    return np.frombuffer(b"".join(bs), dtype=np.uint8), offsets


def ragged_reads(rng, n, max_len=200, p_n=0.01, alphabet=b"ACGT"):
    """Variable-length reads incl. empty, shorter than k, all-N."""
    lens = rng.integers(0, max_len, size=n)
    lens[rng.random(n) < 0.05] = 0
    total = int(lens.sum())
    codes = rng.integers(0, len(alphabet), size=total)
    bases = np.frombuffer(alphabet, dtype=np.uint8)[codes].copy()
    bases[rng.random(total) < p_n] = ord("N")
    offsets = np.zeros(n + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(lens)
    return bases, offsets


def check_against_oracle(orc, bases, offsets, k, chunks, histo_max, flags=0, hint=0, splits=None,
                         check_table=True):
    ref = orc.run_batch(bases, offsets, k, chunks, histo_max)
    with sa.KmerEngine(k, chunks, histo_max, capacity_hint=hint, flags=flags) as eng:
        n = len(offsets) - 1
        cuts = [0] + sorted(splits or []) + [n]
        for a, b in zip(cuts[:-1], cuts[1:]):
            eng.ingest_reads(bases, offsets[a:b + 1])
        eng.finalize()
        got = eng.histograms()
        cnt = eng.counters()
        keys, cnts = eng.export_table() if check_table else (None, None)
    want = ref.histograms()
    assert got.shape == want.shape
    assert np.array_equal(got, want), f"histogram mismatch k={k} chunks={chunks}"
    st = ref.stats
    assert cnt["n_reads_ingested"] == st["n_reads_ingested"]
    assert cnt["n_bases_read"] == st["n_bases_read"]
    assert cnt["n_bases_ingested"] == st["n_bases_ingested"]
    assert cnt["n_kmers_ingested"] == st["n_kmers_ingested"]
    assert cnt["n_unique_kmers"] == st["n_unique_kmers"]
    assert cnt["n_hashed_kmers"] == st["n_hashed_kmers"]
    if chunks > 0:
        assert cnt["n_singleton_kmers"] == st["n_singleton_kmers"]
    if check_table:
        rk, rc = ref.merged().export()
        assert np.array_equal(keys, rk) and np.array_equal(cnts, rc)
    return cnt


# ---- known-answer tests through the C ABI ------------------------------------------------

@pytest.mark.parametrize("flags", FLAGSETS)
def test_ingest_seq(flags):
    """counting.rs:482-490: ACGT, k=3 → one canonical k-mer with count 2."""
    with sa.KmerEngine(3, 1, 10, flags=flags) as eng:
        eng.ingest_seq("ACGT")
        eng.finalize()
        c = eng.counters()
        assert c["n_unique_kmers"] == 1 and c["n_kmers_ingested"] == 2
        assert list(eng.histograms()[0]) == [0, 0, 1] + [0] * 9


def test_histogram_kat():
    """kmer/mod.rs:288-305: counts {5,5,7,11,12}, histo_max 10."""
    with sa.KmerEngine(11, 1, 10) as eng:
        eng.insert([1, 20, 2, 11, 12], [5, 5, 7, 11, 12])
        eng.finalize()
        assert list(eng.histograms()[0]) == [0, 0, 0, 0, 0, 2, 0, 1, 0, 0, 0, 2]


def test_reset_reopens_an_empty_context(orc):
    """shk_reset: the context is as new (table, counters, read index, histogram) whatever was in it, and
    whatever is called first afterwards — a read of the table, an insert, an ingest."""
    spec = sa.SynthSpec(genome_len=40_000, sub_per_64k=200, n_per_64k=50)
    bases, offsets = sa.synth_reads(spec, 0, 6_000)
    ref = orc.run_batch(bases, offsets, 15, 3, 50)
    rk, rc = ref.merged().export()
    with sa.KmerEngine(15, 3, 50, capacity_hint=60_000) as eng:
        for first in ("lookup", "insert", "ingest", "export", "finalize"):
            eng.ingest_reads(bases[:int(offsets[2_500])], offsets[:2_501])   # something to forget
            if first != "ingest":
                eng.finalize()
            eng.reset()
            if first == "lookup":
                assert not eng.lookup(rk[:200]).any()
            elif first == "insert":
                eng.insert([int(rk[0])], [3])
                assert list(eng.lookup(rk[:2])) == [3, 0]
                eng.reset()
            elif first == "export":
                ks, cs = eng.export_table()
                assert len(ks) == 0
            elif first == "finalize":
                with pytest.raises(sa.ShkError, match="No reads were ingested"):
                    eng.finalize()
            eng.ingest_reads(bases, offsets)
            eng.finalize()
            assert np.array_equal(eng.histograms(), ref.histograms()), first
            c = eng.counters()
            assert c["n_kmers_ingested"] == ref.stats["n_kmers_ingested"] and c["n_reads_ingested"] == 6_000
            gk, gc = eng.export_table()
            assert np.array_equal(gk, rk) and np.array_equal(gc, rc), first


def test_insert_with_count_zero_keeps_the_key():
    """counting.rs:152-154: insert(kmer, 0) creates the entry, so it is a unique k-mer of the table
    (counting.rs:258-260) that sits in no histogram bin (move_count(0, 0) is a no-op, histogram.rs:51-55)
    — the reference's own invariant io.rs:1120-1132 then fails.  The histogram scan must take
    occupancy from the keys here, not from the counts."""
    with sa.KmerEngine(11, 1, 10) as eng:
        eng.insert([1, 20, 2, 11], [0, 5, 0, 11])
        assert list(eng.lookup([1, 20, 2, 11, 7])) == [0, 5, 0, 11, 0]
        with pytest.raises(sa.ShkError, match="unique kmers in the histogram"):
            eng.finalize()
        ks, cs = eng.export_table()
        assert sorted(zip(ks.tolist(), cs.tolist())) == [(1, 0), (2, 0), (11, 11), (20, 5)]


def test_insert_accumulates_and_saturates():
    """counting.rs:384-399."""
    with sa.KmerEngine(5, 1, 10) as eng:
        eng.insert([42], [3])
        eng.insert([42], [7])
        eng.insert([1], [0xFFFFFFFF])
        eng.insert([1], [1])
        assert list(eng.lookup([42, 1, 99])) == [10, 0xFFFFFFFF, 0]


def test_extend_with_histogram_saturation_across_lanes(orc):
    """counting.rs:183-200 + io.rs:1023-1047 through the device histogram scan: lanes {0xFFFFFFFE, 5} of one
    k-mer merge to the CAPPED count u32::MAX, every column bins the stored (capped) count, the saturation
    warning is raised, and — Σ merged counts ≠ Σ ingested counts — the reference's invariant fails the run.
    Expected values come from the oracle's own extend_with_histogram on the same chunk tables."""
    k, histo_max = 5, 10
    lanes = [{7: 0xFFFFFFFE, 3: 2, 11: 10}, {7: 5, 3: 3, 20: 1}, {7: 1, 20: 0xFFFFFFFF}]
    merged, h = orc.KmerCounts(k), orc.Histogram(histo_max)
    want_cols, want_sat = [], False
    for tbl in lanes:
        kc = orc.KmerCounts(k)
        for key, cnt in tbl.items():
            kc.insert(key, cnt)
        want_sat |= merged.extend_with_histogram(kc, h)
        want_cols.append(np.array(h.get_vector(), dtype=np.uint64))
    n_ingested = sum(sum(t.values()) for t in lanes)
    with sa.KmerEngine(k, len(lanes), histo_max) as eng:
        for lane, tbl in enumerate(lanes):
            eng.insert(list(tbl), list(tbl.values()), chunk_id=lane)
        with pytest.raises(sa.ShkError) as ei:
            eng.finalize()
        assert ei.value.code == -6  # SHK_ERR_INVARIANT, io.rs:1042-1047
        assert ei.value.msg == (f"The total count of hashed kmers ({merged.get_n_kmers()}) does not equal "
                                f"the number of ingested kmers ({n_ingested})")
        # the reference has computed histo_vecs by then (io.rs:1023-1028 precede the check): they stay readable
        got = eng.histograms()
        c = eng.counters()
        assert [int(x) for x in eng.lookup([7, 3, 11, 20])] == [merged.get_count(x) for x in (7, 3, 11, 20)]
    assert want_sat and c["any_saturated"] == 1
    assert np.array_equal(got, np.stack(want_cols))
    assert list(got[0]) == [0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 1, 1]          # 3:2, 11:10, 7 → overflow bin
    assert c["n_hashed_kmers"] == merged.get_n_kmers() and c["n_unique_kmers"] == 4


@pytest.mark.parametrize("flags", FLAGSETS)
def test_saturating_add_under_ingest(orc, flags):
    """counting.rs:82-85: ingest increments saturate exactly at u32::MAX."""
    seq = "ACGTTGCATGCATGAC" * 4
    kms = sorted(set(orc.kmers_from_ascii(seq, 5)))
    target = kms[0]
    n_occ = orc.kmers_from_ascii(seq, 5).count(target)
    assert n_occ >= 2
    with sa.KmerEngine(5, 1, 10, flags=flags) as eng:
        eng.insert([target], [0xFFFFFFFF - 1])
        eng.ingest_seq(seq)
        assert int(eng.lookup([target])[0]) == 0xFFFFFFFF
        other = kms[1]
        assert int(eng.lookup([other])[0]) == orc.kmers_from_ascii(seq, 5).count(other)


_CASES = ["CGTAATGCGGCGA", "CGTANATGCGGCGA", "NCGTANATGCGGCGA", "NCGTANATGCGGCGANN",
          "NNCGTANATGCGGCGA", "TANCACN", "NTANCACNAGAAAATC", "AAAA", "ACGTACGTACGT"]


@pytest.mark.parametrize("k", [3, 5, 9, 11])
def test_kmers_from_ascii_cases(orc, k):
    """kmer/mod.rs:249-270: the reference's 9 N-placement strings, one per read."""
    bases, offsets = pack(_CASES)
    check_against_oracle(orc, bases, offsets, k, 1, 20)
    for seq in _CASES:  # and each string on its own: exact multiset of k-mers
        want = sorted(orc.kmers_from_ascii(seq, k))
        with sa.KmerEngine(k, 0, 10) as eng:
            eng.ingest_seq(seq)
            keys, cnts = eng.export_table()
        got = sorted(int(x) for x, c in zip(keys, cnts) for _ in range(int(c)))
        assert got == want, (seq, k)


def test_short_sequences(orc):
    """kmer/mod.rs:272-278 + chunk.rs:27: reads shorter than k count as reads, emit nothing."""
    bases, offsets = pack(["ACGT", "ACGTACGTA", "", "NNN", "A"])
    cnt = check_against_oracle(orc, bases, offsets, 9, 1, 10)
    assert cnt["n_reads_ingested"] == 5 and cnt["n_kmers_ingested"] == 1
    assert cnt["n_bases_ingested"] == 14 and cnt["n_bases_read"] == 17


@pytest.mark.parametrize("seq,bad", [("ACGTX", "X"), ("acgt", "a"), ("ACG T", " "), ("ACGT\n", "\n")])
def test_invalid_character(seq, bad):
    """encoding.rs:353-356: same message; the run is aborted (context poisoned)."""
    with sa.KmerEngine(3, 1, 10) as eng:
        eng.ingest_seq("ACGTACGT")
        with pytest.raises(sa.ShkError) as e:
            eng.ingest_seqs(["ACGT", seq, "ACZT"])
        assert e.value.code == -1
        assert e.value.msg == f"Invalid character '{bad}' in sequence. Only ACGTN allowed."
        with pytest.raises(sa.ShkError):
            eng.finalize()


def test_no_reads_is_an_error():
    """io.rs:578-580."""
    with sa.KmerEngine(21, 1, 10) as eng:
        with pytest.raises(sa.ShkError) as e:
            eng.finalize()
        assert e.value.code == -5 and "No reads were ingested" in e.value.msg


@pytest.mark.parametrize("k,histo_max", [(0, 10), (32, 10), (21, 0), (21, 1_000_001)])
def test_validate_args(k, histo_max):
    """cli.rs:659-677."""
    with pytest.raises(sa.ShkError) as e:
        sa.KmerEngine(k, 1, histo_max)
    assert e.value.code == -2


# ---- randomized parity vs the oracle ---------------------------------------------------------

@pytest.mark.parametrize("flags", FLAGSETS)
@pytest.mark.parametrize("k,chunks", [(21, 1), (21, 0), (31, 3), (5, 2), (1, 1), (3, 10), (13, 7)])
def test_ragged_parity(orc, k, chunks, flags):
    rng = np.random.default_rng(1000 * k + chunks)
    bases, offsets = ragged_reads(rng, 12_345)
    check_against_oracle(orc, bases, offsets, k, chunks, 50, flags=flags)


@pytest.mark.parametrize("flags", FLAGSETS)
def test_parity_variant_errors_and_n(orc, flags):
    """SURVEY.md §8d parity variant: 0.5 % substitutions, 0.1 % N, tiny genome so counts exceed
    histo_max (overflow bin) and singletons dominate."""
    spec = sa.SynthSpec(genome_len=2000, sub_per_64k=328, n_per_64k=66)
    bases, offsets = sa.synth_reads(spec, 0, 30_000)
    cnt = check_against_oracle(orc, bases, offsets, 21, 5, 100, flags=flags)
    assert cnt["n_singleton_kmers"] > 0


def test_split_calls_match_single_call(orc):
    """State persists across calls like FastqReadState across files (io.rs:498-512): batches
    of 1000 span call boundaries."""
    rng = np.random.default_rng(7)
    bases, offsets = ragged_reads(rng, 9_876, max_len=120)
    check_against_oracle(orc, bases, offsets, 15, 4, 30, splits=[1, 999, 1000, 1001, 2500, 7777])


def test_explicit_chunk_batches(orc):
    """shk_ingest_batch = drain_batch body: caller-chosen chunk per batch."""
    rng = np.random.default_rng(11)
    bases, offsets = ragged_reads(rng, 5_000, max_len=100)
    ref = orc.run_batch(bases, offsets, 11, 3, 40)
    with sa.KmerEngine(11, 3, 40) as eng:
        for b in range(5):
            eng.ingest_batch(b % 3, bases, offsets[b * 1000:(b + 1) * 1000 + 1])
        eng.finalize()
        assert np.array_equal(eng.histograms(), ref.histograms())


@pytest.mark.parametrize("flags", FLAGSETS)
def test_growth_and_spill_keep_results_exact(orc, flags):
    """No capacity hint, nearly all k-mers distinct: the table must grow (and may spill)
    without losing or double counting anything."""
    rng = np.random.default_rng(3)
    n = 20_000
    codes = rng.integers(0, 4, size=n * 150)
    bases = np.frombuffer(b"ACGT", dtype=np.uint8)[codes].copy()
    offsets = np.arange(n + 1, dtype=np.uint64) * 150
    cnt = check_against_oracle(orc, bases, offsets, 31, 2, 10, flags=flags, check_table=False)
    assert cnt["n_grows"] >= 1
    assert cnt["n_unique_kmers"] > 2_000_000


def test_incremental_histogram_consistency(orc):
    """tests/spcr_18s.rs:437-528: the final histogram does not depend on the chunk count."""
    spec = sa.SynthSpec(genome_len=50_000, sub_per_64k=328, n_per_64k=66)
    bases, offsets = sa.synth_reads(spec, 0, 40_000)
    finals = []
    for chunks in (1, 20):
        with sa.KmerEngine(21, chunks, 1000) as eng:
            eng.ingest_reads(bases, offsets)
            eng.finalize()
            finals.append(eng.histograms()[-1])
    assert np.array_equal(finals[0], finals[1])
    ref = orc.run_batch(bases, offsets, 21, 20, 1000)
    assert np.array_equal(finals[1], ref.histograms()[-1])


def test_lookup_canonical(orc):
    """counting.rs:205-209, 224-226."""
    seq = "ACGGTCATTGCAAGCTAGCTAGGATCGA"
    with sa.KmerEngine(7, 0, 10) as eng:
        eng.ingest_seq(seq)
        kc = orc.KmerCounts(7)
        kc.ingest_seq(seq)
        fwd = [orc.seq_to_kmer(seq[i:i + 7]) for i in range(len(seq) - 6)]
        assert list(eng.lookup(fwd, canonical=True)) == [kc.get_canonical_count(x) for x in fwd]
        assert list(eng.lookup(fwd, canonical=False)) == [kc.get_count(x) for x in fwd]


# ---- device-resident input + device generator --------------------------------------------------

def test_device_synth_matches_host_generator():
    import torch
    spec = sa.SynthSpec(genome_len=10_000, sub_per_64k=400, n_per_64k=80)
    n = 3_001
    hb, ho = sa.synth_reads(spec, 17, n)
    with sa.KmerEngine(21, 1, 10) as eng:
        db = torch.empty(n * 150, dtype=torch.uint8, device="cuda")
        do = torch.empty(n + 1, dtype=torch.int64, device="cuda")
        eng.synth_reads_device(spec, 17, n, db.data_ptr(), do.data_ptr())
        assert np.array_equal(db.cpu().numpy(), hb)
        assert np.array_equal(do.cpu().numpy().astype(np.uint64), ho)


def test_device_resident_ingest(orc):
    import torch
    spec = sa.SynthSpec(genome_len=30_000, sub_per_64k=328, n_per_64k=66)
    n = 25_000
    hb, ho = sa.synth_reads(spec, 0, n)
    ref = orc.run_batch(hb, ho, 21, 4, 200)
    with sa.KmerEngine(21, 4, 200) as eng:
        db = torch.from_numpy(hb).cuda()
        do = torch.from_numpy(ho.astype(np.int64)).cuda()
        torch.cuda.synchronize()
        eng.ingest_reads_device(db.data_ptr(), do.data_ptr(), n, len(hb))
        eng.finalize()
        assert np.array_equal(eng.histograms(), ref.histograms())


# ---- BASELINE.json config 2 at full size: 1 M reads, k=21 ------------------------------------------

@pytest.mark.parametrize("flags", FLAGSETS)
def test_config2_full_size(orc, flags):
    spec = sa.SynthSpec(genome_len=3_000_000)
    n = 1_000_000
    bases, offsets = sa.synth_reads(spec, 0, n)
    ref = orc.run_batch(bases, offsets, 21, 1, 10000)
    with sa.KmerEngine(21, 1, 10000, capacity_hint=3_000_000, flags=flags) as eng:
        eng.ingest_reads(bases, offsets)
        eng.finalize()
        got = eng.histograms()
        cnt = eng.counters()
    assert np.array_equal(got, ref.histograms())
    assert cnt["n_kmers_ingested"] == 130 * n
    # size-independent properties: Σ freq·count = k-mer occurrences; Σ freq = distinct
    col = got[0].astype(object)
    assert sum(int(f) * i for i, f in enumerate(col)) == 130 * n  # no count exceeds histo_max here
    assert int(got[0].sum()) == cnt["n_unique_kmers"]


# ---- BASELINE.json config 3 semantics: host input streamed in slices, copy/compute overlap ------------

@pytest.mark.parametrize("host_pack", ["0", "1"])
@pytest.mark.parametrize("k,chunks,empty", [pytest.param(31, 1, False, id="31-1"), pytest.param(21, 4, False, id="21-4"),
                                            pytest.param(21, 1, True, id="200-empty-reads")])
def test_streamed_slices_match_oracle(orc, monkeypatch, k, chunks, empty, host_pack):
    """A large host batch crosses PCIe in slices of whole reads (the next slices copying while the current one is
    counted); forcing 64 KiB slices exercises many slice boundaries, including ones inside a 1000-read block.
    host_pack: the slices as ASCII (0), or packed 2-bit on the host first — what a batch of some size gets on a host
    with the cores for it (SHK_HOST_PACK pins either).
    empty: a call of 200 reads without a base between them — one slice that copies offsets alone, whatever its size."""
    monkeypatch.setenv("SHK_SLICE_KB", "16" if empty else "64")
    monkeypatch.setenv("SHK_HOST_PACK", host_pack)
    rng = np.random.default_rng(99)
    bases, offsets = pack([b""] * 200) if empty else ragged_reads(rng, 20_000, max_len=160, p_n=0.01)
    check_against_oracle(orc, bases, offsets, k, chunks, 60, check_table=False)


def test_host_packed_ascii_batch_reports_the_first_invalid_byte(orc, monkeypatch):
    """Host packing looks at every byte before anything of its slice is copied: the first offender in input order,
    the reference's text (encoding.rs:353-356), the context poisoned as by the device-side check — and several calls
    in a row (one and many slices each) give the oracle's histogram."""
    monkeypatch.setenv("SHK_SLICE_KB", "64")
    monkeypatch.setenv("SHK_HOST_PACK", "1")
    rng = np.random.default_rng(12)
    bases, offsets = ragged_reads(rng, 9_000, max_len=160)
    ref = orc.run_batch(bases, offsets, 21, 3, 60)
    with sa.KmerEngine(21, 3, 60) as eng:
        for a, b in ((0, 2_500), (2_500, 2_600), (2_600, 7_000), (7_000, 9_000)):
            eng.ingest_reads(bases, offsets[a:b + 1])
        eng.finalize()
        assert np.array_equal(eng.histograms(), ref.histograms())
        c = eng.counters()
        for f in ("n_reads_ingested", "n_bases_read", "n_bases_ingested", "n_kmers_ingested", "n_unique_kmers"):
            assert c[f] == ref.stats[f], f
        eng.reset()
        bad = bases.copy()
        bad[int(offsets[4_000]) + 3] = ord("y")
        bad[int(offsets[3_000]) + 5] = 0xE9
        with pytest.raises(sa.ShkError, match="Invalid character 'é' in sequence. Only ACGTN allowed."):
            eng.ingest_reads(bad, offsets)
        with pytest.raises(sa.ShkError, match="Invalid character 'é'"):   # poisoned: the run is over
            eng.ingest_reads(bases, offsets[:11])


def test_deferred_errors_overlap_calls_and_still_report(orc, monkeypatch):
    """SHK_FLAG_DEFER_ERRORS: a host-buffer ingest returns once its last slice is queued (the next call's copies
    run under it, on the staging sets taken in turn); the result is the oracle's, and an invalid byte is reported
    by the NEXT call with the reference's text."""
    monkeypatch.setenv("SHK_SLICE_KB", "64")
    rng = np.random.default_rng(5)
    bases, offsets = ragged_reads(rng, 9_000, max_len=160)
    ref = orc.run_batch(bases, offsets, 21, 3, 60)
    with sa.KmerEngine(21, 3, 60, flags=sa.FLAG_DEFER_ERRORS) as eng:
        for a, b in ((0, 2_500), (2_500, 2_600), (2_600, 7_000), (7_000, 9_000)):  # 1, many and few slices per call
            eng.ingest_reads(bases, offsets[a:b + 1])
        eng.finalize()
        assert np.array_equal(eng.histograms(), ref.histograms())
        eng.reset()
        bad = bases[:int(offsets[50])].copy()
        bad[int(offsets[20]) + 3] = ord("Q")
        eng.ingest_reads(bad, offsets[:51])  # queued: nobody has looked yet
        with pytest.raises(sa.ShkError, match="Invalid character 'Q' in sequence. Only ACGTN allowed."):
            eng.ingest_reads(bases, offsets[:11])


def test_config3_shape_k31_properties():
    """k=31 at a size the oracle would take minutes for: size-independent properties only —
    Σ freq·count = k-mer occurrences, Σ freq = distinct, chunk-count invariance of the final
    column, error-free 150-bp reads ⇒ 120 k-mers per read."""
    spec = sa.SynthSpec(genome_len=20_000_000)
    n = 3_000_000
    finals = []
    for chunks in (1, 6):
        with sa.KmerEngine(31, chunks, 2000, capacity_hint=20_000_000) as eng:
            for part in range(3):  # three host batches, generated on the fly
                b, o = sa.synth_reads(spec, part * (n // 3), n // 3)
                eng.ingest_reads(b, o)
            eng.finalize()
            h = eng.histograms()
            c = eng.counters()
        assert c["n_kmers_ingested"] == 120 * n
        last = h[-1].astype(object)
        assert sum(int(f) * i for i, f in enumerate(last)) == 120 * n
        assert int(h[-1].sum()) == c["n_unique_kmers"]
        for j in range(1, chunks):  # cumulative columns only ever gain k-mers
            assert int(h[j].sum()) >= int(h[j - 1].sum())
        finals.append(h[-1])
    assert np.array_equal(finals[0], finals[1])


def test_config3_full_size_properties(orc):
    """BASELINE.json configs[2] at its full size — 100 M reads of 150 bp, k=31, a 300 Mb genome (a
    2^30-slot table), streamed in batches of 4 M reads — generated on the device and counted from
    HBM (tools/config3_run.py is the timed twin of this, incl. the host-streamed variant).  The
    table-based oracle would need hours: size-independent properties, plus an EXACT probe set — 10^5
    k-mers of sampled reads counted over all 100 M reads with the oracle's extractor on the host cores
    (tests/probe_util.py) against the engine's point lookups."""
    from probe_util import ProbeChecker
    n, L, k, batch = 100_000_000, 150, 31, 4_000_000
    spec = sa.SynthSpec(genome_len=300_000_000, read_len=L)
    pc = ProbeChecker(orc, k, 1, L)
    with sa.KmerEngine(k, 1, 10000, capacity_hint=300_000_000) as eng:
        d_bases = eng.alloc_device(batch * L * 2)      # two batches in flight at most
        d_off = eng.alloc_device((batch + 1) * 8)
        try:
            for s_batch in (0, 11, 24):                # probe candidates: reads from three places of the stream
                eng.synth_reads_device(spec, s_batch * batch + 1234, 300, d_bases, d_off)
                eng.sync()
                pc.add_sample(pc._fetch(eng, d_bases, 300), 300)
            pc.freeze()
            for b in range(n // batch):
                buf = d_bases + (b & 1) * batch * L
                eng.synth_reads_device(spec, b * batch, batch, buf, d_off)
                eng.ingest_reads_device(buf, d_off, batch, batch * L)
                pc.count_async(pc._fetch(eng, buf, batch), batch, b * batch)
            eng.finalize()
            h = eng.histograms()
            c = eng.counters()
            got = eng.lookup(pc.probes)
        finally:
            eng.sync()
            eng.free_device(d_bases)
            eng.free_device(d_off)
    want = pc.merged()
    pc.close()
    assert len(pc.probes) == 100_000 and int(want.min()) >= 1
    assert np.array_equal(got, want)                                        # exact, k-mer by k-mer
    assert c["n_reads_ingested"] == n and c["n_bases_ingested"] == n * L
    assert c["n_kmers_ingested"] == (L - k + 1) * n
    col = h[0].astype(object)
    assert sum(int(f) * i for i, f in enumerate(col)) == (L - k + 1) * n   # Σ freq·count = occurrences
    assert int(h[0].sum()) == c["n_unique_kmers"]                           # Σ freq = distinct
    assert c["n_unique_kmers"] <= 300_000_000 - k + 1                       # error-free reads of one genome
    assert 30 <= int(np.argmax(h[0][2:]) + 2) <= 50                         # coverage peak: 50 × 120/150 = 40


def test_config4_share_on_a_table_of_2_33_slots(orc):
    """BASELINE.json configs[3]'s table on one GPU: a 3 Gb genome is a 2^33-slot table (2^20 pages,
    the most the geometry allows: page bits + 11 home-bucket bits out of 32 hash bits; 103 GB), the
    partition has two full levels (1024 × 1024) and everything is counted by deferred page passes.
    ALL 125 M reads of one GPU's share (SHK_SHARE4_READS: fewer, for a quick look; 28 s on the box, most of it the
    oracle's extractor over the reads on 16 CPUs); properties, plus an EXACT probe set (10^5 k-mers of sampled reads,
    counted over all the reads by the oracle's extractor) against point lookups: the global-memory probe
    must find what the page workgroups inserted, with exactly the right count."""
    from probe_util import ProbeChecker
    n, L, k, batch = int(os.environ.get("SHK_SHARE4_READS", 125_000_000)), 150, 21, 5_000_000
    assert n % batch == 0 and n >= 6 * batch
    spec = sa.SynthSpec(genome_len=3_000_000_000, read_len=L)
    pc = ProbeChecker(orc, k, 1, L)
    with sa.KmerEngine(k, 1, 1000, capacity_hint=3_000_000_000) as eng:
        assert eng.table_geometry()[0] == 1 << 20
        d_bases = eng.alloc_device(batch * L)
        d_off = eng.alloc_device((batch + 1) * 8)
        try:
            for s_batch in (0, 3, 5):
                eng.synth_reads_device(spec, s_batch * batch + 777, 300, d_bases, d_off)
                eng.sync()
                pc.add_sample(pc._fetch(eng, d_bases, 300), 300)
            pc.freeze()
            for b in range(n // batch):
                eng.synth_reads_device(spec, b * batch, batch, d_bases, d_off)
                eng.ingest_reads_device(d_bases, d_off, batch, batch * L)
                pc.count_async(pc._fetch(eng, d_bases, batch), batch, b * batch)
            eng.finalize()
            h = eng.histograms()
            c = eng.counters()
            got = eng.lookup(pc.probes)
        finally:
            eng.sync()
            eng.free_device(d_bases)
            eng.free_device(d_off)
    want = pc.merged()
    pc.close()
    assert np.array_equal(got, want) and int(want.min()) >= 1
    assert c["n_kmers_ingested"] == (L - k + 1) * n and c["n_grows"] == 0
    col = h[0].astype(object)
    assert sum(int(f) * i for i, f in enumerate(col)) == (L - k + 1) * n
    assert int(h[0].sum()) == c["n_unique_kmers"]
    # coverage 1.04 of k-mer starts: distinct ≈ G·(1 − e^(−1.04)) — random placement, so within 1 %
    expect = 3e9 * (1 - np.exp(-(L - k + 1) * n / 3e9))
    assert abs(c["n_unique_kmers"] - expect) < 0.01 * expect


# ---- shapes that stress the paged path's LDS sort and page regions -------------------------------------

@pytest.mark.parametrize("flags", FLAGSETS)
def test_long_reads_fill_whole_tiles(orc, flags):
    """Few very long reads: almost every position of a 16 Ki-base tile ends a k-mer, so the
    tile's sorted-entry region (entries + one pad per page) is used to the full."""
    rng = np.random.default_rng(5)
    n, L = 24, 40_000
    bases = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=n * L)].copy()
    offsets = np.arange(n + 1, dtype=np.uint64) * L
    check_against_oracle(orc, bases, offsets, 21, 2, 30, flags=flags, check_table=False)


@pytest.mark.parametrize("flags", FLAGSETS)
def test_skewed_low_complexity_input(orc, flags):
    """One k-mer (poly-A) makes up most of the batch: its page's region of the scatter buffer
    overflows and the excess must arrive through the spill path, exactly."""
    rng = np.random.default_rng(6)
    n = 30_000
    seqs = []
    for i in range(n):
        if rng.random() < 0.9:
            seqs.append(b"A" * 150)
        else:
            seqs.append(np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=150)].tobytes())
    bases, offsets = pack(seqs)
    cnt = check_against_oracle(orc, bases, offsets, 21, 3, 100, flags=flags)
    if flags == sa.FLAG_FORCE_PAGED:
        assert cnt["n_spilled"] > 0


# ---- two-level partition (tables with more pages than one LDS sort fans out to) -------------------------

def _rows_with_hooks(rows, hooked):
    """Parameter rows (ids as pytest makes them from the values) + rows that also switch one engine hook off."""
    return ([pytest.param(*r, None, id="-".join(map(str, r))) for r in rows] +
            [pytest.param(*r, hook, id="-".join(map(str, r)) + "-" + hook + "=0") for r, hook in hooked])


@pytest.mark.parametrize("k,chunks,lvl1,hook_off", _rows_with_hooks(
    [(21, 1, 2), (31, 3, 3), (13, 2, 0), (23, 2, 2), (25, 3, 3), (24, 1, 1)],
    [((25, 3, 3), "SHK_S64_INTERLEAVE"),    # k_scatter64 in its linear layout feeds the plain re-scatter
     ((31, 3, 3), "SHK_SCATTER64")]))       # k_part_scatter_sorted at a fan-out k_scatter64 would otherwise take
def test_two_level_partition_small(orc, monkeypatch, k, chunks, lvl1, hook_off):
    """Force the super-page + re-scatter path on a small table: 8+ pages, level 1 fans out to
    2^lvl1 super-pages, level 2 to the pages inside each."""
    monkeypatch.setenv("SHK_TWO_LEVEL_MIN_PAGES", "4")
    monkeypatch.setenv("SHK_LEVEL1_LOG", str(lvl1))
    if hook_off:
        monkeypatch.setenv(hook_off, "0")
    spec = sa.SynthSpec(genome_len=150_000, sub_per_64k=328, n_per_64k=66)
    bases, offsets = sa.synth_reads(spec, 0, 60_000)
    cnt = check_against_oracle(orc, bases, offsets, k, chunks, 200, flags=sa.FLAG_FORCE_PAGED,
                               hint=400_000, check_table=False)
    assert cnt["table_capacity"] >= 8 * 8192


@pytest.mark.parametrize("chunks", [2, 10, 16])
@pytest.mark.parametrize("dirty", [False, True])
def test_two_level_many_lanes_one_page_launch(orc, monkeypatch, chunks, dirty):
    """Chunk lanes on the forced two-level geometry: a batch over several lanes takes ONE level-1 pass, ONE
    level-2 pass and ONE page launch that keeps a page's tags in LDS for all its lanes — and, the table's memory
    never having been cleared (or holding the leftovers of a job before the reset: `dirty`), that launch is the
    FRESH one, which writes every lane of every page whole.  A second batch then goes through the ordinary pass."""
    monkeypatch.setenv("SHK_TWO_LEVEL_MIN_PAGES", "4")
    monkeypatch.setenv("SHK_LEVEL1_LOG", "2")
    spec = sa.SynthSpec(genome_len=150_000, sub_per_64k=328, n_per_64k=66)
    bases, offsets = sa.synth_reads(spec, 0, 50_000)
    ref = orc.run_batch(bases, offsets, 21, chunks, 200)
    with sa.KmerEngine(21, chunks, 200, capacity_hint=400_000) as eng:
        if dirty:
            ob, oo = sa.synth_reads(sa.SynthSpec(genome_len=90_000, sub_per_64k=900), 3, 20_000)
            eng.ingest_reads(ob, oo)
            eng.finalize()
            eng.reset()
        eng.ingest_reads(bases, offsets[:30_001])   # → FRESH page launch (at the latest when finalize asks)
        eng.sync()
        eng.ingest_reads(bases, offsets[30_000:])   # → ordinary page launch over the same pages
        eng.finalize()
        assert np.array_equal(eng.histograms(), ref.histograms())
        c = eng.counters()
        keys, cnts = eng.export_table()
    for f in ("n_reads_ingested", "n_bases_ingested", "n_kmers_ingested", "n_unique_kmers", "n_hashed_kmers"):
        assert c[f] == ref.stats[f], f
    rk, rc = ref.merged().export()
    assert np.array_equal(keys, rk) and np.array_equal(cnts, rc)


def test_two_level_partition_large_table():
    """A table past MAX_PARTS pages (64 M distinct-k-mer hint ⇒ 16 Ki pages) takes the two-level
    path by itself; properties at a size the oracle is too slow for."""
    spec = sa.SynthSpec(genome_len=30_000_000)
    n = 3_400_000  # two batches of 1.7 M reads: each fits one counting launch (≤ 2^28 bases)
    with sa.KmerEngine(21, 1, 1000, capacity_hint=64_000_000, flags=sa.FLAG_TIMING) as eng:
        for part in range(2):
            b, o = sa.synth_reads(spec, part * (n // 2), n // 2)
            eng.ingest_reads(b, o)
        eng.finalize()
        h = eng.histograms()
        c = eng.counters()
        t = eng.timings()
    assert "pages" in t and "direct" not in t and "pscan" in t  # pscan slot = the level-2 re-scatter
    assert c["n_kmers_ingested"] == 130 * n
    col = h[0].astype(object)
    assert sum(int(f) * i for i, f in enumerate(col)) == 130 * n
    assert int(h[0].sum()) == c["n_unique_kmers"] and c["n_spilled"] == 0
    # 17x coverage of a 30 Mb genome: nearly every genomic 21-mer seen at least once
    assert 0.99 * 30_000_000 < c["n_unique_kmers"] <= 30_000_000


# ---- parameter extremes ------------------------------------------------------------------------------

@pytest.mark.parametrize("chunks,paged_max,hint,flags", [(40, 0, 0, 0), (40, 16, 0, 0), (100, 0, 0, 0), (100, 0, 600_000, "paged"), (128, 0, 600_000, "paged"),
                                                         (130, 0, 0, 0), (64, 0, 9_000_000, 0)])
def test_many_chunk_lanes(orc, monkeypatch, chunks, paged_max, hint, flags):
    """Chunk counts well beyond the usual ten — the reference takes any (its own historical runs: n = 100,
    sharkmer_viewer/tests/data/Cordagalma.stats:1).  Up to 128 lanes the paged passes take them (round 4: the limit was
    16, and 40 lanes ran through the global atomics at a sixth of the rate); beyond that — or with the limit pinned back
    to 16 — the atomics path with per-tile lanes; a large table puts 64 lanes through the two-level route."""
    if paged_max:
        monkeypatch.setenv("SHK_PAGED_MAX_LANES", str(paged_max))
    spec = sa.SynthSpec(genome_len=20_000, sub_per_64k=328, n_per_64k=66)
    bases, offsets = sa.synth_reads(spec, 0, 45_500 if chunks <= 40 else 135_500)
    check_against_oracle(orc, bases, offsets, 21, chunks, 300, check_table=chunks == 100 and not flags,
                         flags=sa.FLAG_FORCE_PAGED if flags == "paged" else 0, hint=hint)


@pytest.mark.parametrize("histo_max", [1, 1_000_000])
def test_histo_max_extremes(orc, histo_max):
    """cli.rs:668-673: 0 < histo_max ≤ 1_000_000; counts above fold into the last bin."""
    spec = sa.SynthSpec(genome_len=1_000, sub_per_64k=100)
    bases, offsets = sa.synth_reads(spec, 0, 20_000)
    check_against_oracle(orc, bases, offsets, 15, 2, histo_max, check_table=False)


@pytest.mark.parametrize("k", [2, 16, 20, 30])
def test_even_k_is_accepted_by_the_library(orc, k):
    """"k odd" is the CLI's rule (cli.rs:667); the kmer module takes any 0 < k < 32
    (encoding.rs:333), palindromic k-mers included (fwd == rev)."""
    rng = np.random.default_rng(k)
    bases, offsets = ragged_reads(rng, 6_000, max_len=120)
    check_against_oracle(orc, bases, offsets, k, 2, 40)


# ---- the merged table's read API as sPCR uses it -------------------------------------

@pytest.mark.parametrize("oligo_len,min_count", [(8, 1), (12, 2), (20, 3)])
def test_find_oligos_in_kmers(orc, oligo_len, min_count):
    """pcr/primers.rs:163-226: start-of-k-mer matches as is, reverse-orientation matches
    reverse-complemented, count threshold applied."""
    spec = sa.SynthSpec(genome_len=30_000, sub_per_64k=200)
    bases, offsets = sa.synth_reads(spec, 0, 12_000)
    k = 21
    ref = orc.run_batch(bases, offsets, k, 2, 100)
    merged = ref.merged()
    keys, _ = merged.export()
    rng = np.random.default_rng(oligo_len)
    # oligos: prefixes of some table k-mers (forward hits), suffix-revcomps of others (rc hits), noise
    pick = rng.choice(len(keys), size=40, replace=False)
    oligos = [int(keys[i]) >> (2 * (k - oligo_len)) for i in pick[:20]]
    oligos += [orc.revcomp_kmer(int(keys[i]) & ((1 << (2 * oligo_len)) - 1), oligo_len) for i in pick[20:]]
    oligos += [int(x) for x in rng.integers(0, 1 << (2 * oligo_len), size=10)]
    want_k, want_c = merged.find_oligos(oligos, oligo_len, min_count)
    with sa.KmerEngine(k, 2, 100) as eng:
        eng.ingest_reads(bases, offsets)
        eng.finalize()
        got_k, got_c = eng.find_oligos(oligos, oligo_len, min_count)
        with pytest.raises(sa.ShkError):
            eng.find_oligos(oligos, k, 1)  # oligo_len must be < k (primers.rs:181-186)
    assert len(want_k) > 0
    assert np.array_equal(got_k, want_k) and np.array_equal(got_c, want_c)


@pytest.mark.parametrize("seq,k,oligo,min_count,expected", [
    ("ACGTACGT", 5, "ACG", 1, None), ("AAAAAAAAAA", 5, "GGG", 1, []), ("AACCCAACC", 5, "AAC", 2, []),
    ("TTTTTTT", 5, "AAA", 1, ["AAAAA"]), ("ACGTACGT", 5, "ACGT", 1, None)])
def test_find_oligos_reference_cases(orc, seq, k, oligo, min_count, expected):
    """The reference's own cases, pcr/primers.rs:603-695, through the C ABI."""
    kc = orc.KmerCounts(k)
    kc.ingest_seq(seq)
    want_k, want_c = kc.find_oligos([orc.seq_to_kmer(oligo)], len(oligo), min_count)
    bases = np.frombuffer(seq.encode(), dtype=np.uint8)
    with sa.KmerEngine(k, 1, 100) as eng:
        eng.ingest_reads(bases, np.array([0, len(seq)], dtype=np.uint64))
        eng.finalize()
        got_k, got_c = eng.find_oligos([orc.seq_to_kmer(oligo)], len(oligo), min_count)
    assert np.array_equal(got_k, want_k) and np.array_equal(got_c, want_c)
    if expected is not None:
        assert [orc.kmer_to_seq(int(x), k) for x in got_k] == expected
    else:
        assert len(got_k) > 0


# ---- 4-byte-record path (k_part_scatter_sorted<.., true> + k_pages32): 11 ≤ 2k - log_pages ≤ 32 ----------

@pytest.mark.parametrize("k,chunks,hint", [(6, 1, 0), (11, 3, 0), (13, 1, 0), (16, 2, 0), (16, 1, 40_000),
                                           (17, 1, 20_000), (19, 4, 300_000), (21, 1, 4_200_000)])
def test_rec32_path_parity(orc, k, chunks, hint):
    """Records are the low bits of the mixed key; tags in LDS; keys rebuilt with unmix_key on insert.
    Includes the boundary 2k - log_pages = 32 (k=16 on a one-page table, k=21 on 1024 pages) and a
    first pass into an empty table followed by passes into a populated one."""
    spec = sa.SynthSpec(genome_len=60_000, sub_per_64k=300, n_per_64k=40)
    bases, offsets = sa.synth_reads(spec, 0, 24_000)
    check_against_oracle(orc, bases, offsets, k, chunks, 200, flags=sa.FLAG_FORCE_PAGED, hint=hint,
                         splits=[8_000, 16_000])


def test_rec32_matches_8byte_records(orc, monkeypatch):
    """Same input through both record formats: identical tables."""
    spec = sa.SynthSpec(genome_len=200_000, sub_per_64k=100)
    bases, offsets = sa.synth_reads(spec, 0, 40_000)
    out = []
    for rec32 in ("1", "0"):
        monkeypatch.setenv("SHK_REC32", rec32)
        with sa.KmerEngine(15, 2, 100, flags=sa.FLAG_FORCE_PAGED) as eng:
            eng.ingest_reads(bases, offsets)
            eng.finalize()
            out.append((eng.histograms(), eng.export_table()))
    assert np.array_equal(out[0][0], out[1][0])
    assert np.array_equal(out[0][1][0], out[1][1][0]) and np.array_equal(out[0][1][1], out[1][1][1])


# ---- PrimerReadFilter::matches over a batch --------------------------------------------

@pytest.mark.parametrize("k", [5, 21, 31])
def test_filter_reads_matches_reference_semantics(orc, k):
    """pcr/read_filter.rs:43-55: per read, false on any byte outside ACGTN, else any k-mer in the set."""
    spec = sa.SynthSpec(genome_len=50_000, sub_per_64k=200, n_per_64k=100)
    bases, offsets = sa.synth_reads(spec, 0, 3_000)
    bases = bases.copy()
    rng = np.random.default_rng(k)
    for r in rng.choice(3_000, size=40, replace=False):      # a few reads with an invalid byte
        bases[int(offsets[r]) + int(rng.integers(0, 150))] = ord("X")
    seqs = [bytes(bases[int(offsets[i]):int(offsets[i + 1])]) for i in range(3_000)]
    seqs += [b"", b"ACG", b"N" * 40]                          # empty, shorter than k, all N
    bases2, offsets2 = pack(seqs)
    primers = orc.KmerCounts(k)
    for r in rng.choice(3_000, size=25, replace=False):      # primer set: k-mers of a few (valid) reads
        if b"X" not in seqs[r]:
            primers.ingest_seq(seqs[r][20:20 + k + 6])
    pk, _ = primers.export()
    want = np.array([primers.filter_matches(sq) for sq in seqs])
    with sa.KmerEngine(k, 1, 10) as eng:
        got = eng.filter_reads(bases2, offsets2, pk)
        none = eng.filter_reads(bases2, offsets2, np.zeros(0, dtype=np.uint64))
    assert want.sum() > 25 and (~want).sum() >= 40  # both classes present (k=5 matches nearly everywhere)
    assert np.array_equal(got, want)
    assert not none.any()                                     # test_empty_filter, read_filter.rs:62-67


# ---- §8f row 4, second half: kmers_from_ascii in read order (what thread_reads extracts) ------------------------

_KFA_CASES = ["CGTAATGCGGCGA", "CGTANATGCGGCGA", "NCGTANATGCGGCGA", "NCGTANATGCGGCGANN",
              "NNCGTANATGCGGCGA", "TANCACN", "NTANCACNAGAAAATC", "AAAA", "ACGTACGTACGT", "", "N"]


@pytest.mark.parametrize("k", [3, 5, 9, 11])
def test_kmers_from_ascii_kats_on_device(orc, k):
    """kmer/mod.rs:249-278 (test_kmers_from_ascii_matches_read_pipeline, ..._short_sequences) and the
    vector of kmer/mod.rs:61-156, asked of the device's kmers_from_ascii."""
    with sa.KmerEngine(k, 1, 10) as eng:
        for seq in _KFA_CASES:
            assert list(eng.kmers_from_ascii(seq)) == orc.kmers_from_ascii(seq, k), seq
        if k == 9:
            assert list(eng.kmers_from_ascii("CGTAATGCGGCG")) == orc.kmers_from_ascii("CGTAATGCGGCG", 9)
            assert list(eng.kmers_from_ascii("ACGT")) == [] and len(eng.kmers_from_ascii("ACGTACGTA")) == 1
        for seq, bad in [("ACGTX", "X"), ("acgt", "a"), ("ACG T", " ")]:   # encoding.rs:353-356
            with pytest.raises(sa.ShkError) as e:
                eng.kmers_from_ascii(seq)
            assert f"Invalid character '{bad}' in sequence. Only ACGTN allowed." in str(e.value)


@pytest.mark.parametrize("k", [7, 21, 31])
def test_kmers_from_reads_batch_in_read_order(orc, k):
    """pcr/threading.rs:97-101: per read, kmers_from_ascii's vector in order; a read with an invalid
    byte is skipped (no k-mers, its byte reported)."""
    spec = sa.SynthSpec(genome_len=40_000, sub_per_64k=300, n_per_64k=400)
    bases, offsets = sa.synth_reads(spec, 0, 2_000)
    bases = bases.copy()
    rng = np.random.default_rng(100 + k)
    bad_reads = {int(r): int(rng.integers(0, 150)) for r in rng.choice(2_000, size=30, replace=False)}
    for r, pos in bad_reads.items():
        bases[int(offsets[r]) + pos] = ord("x")
    seqs = [bytes(bases[int(offsets[i]):int(offsets[i + 1])]) for i in range(2_000)]
    seqs += [b"", b"ACG", b"N" * 40, b"ACGT" * 20 + b"N" + b"TTGCA" * 9]
    bases2, offsets2 = pack(seqs)
    with sa.KmerEngine(k, 1, 10) as eng:
        got, bad = eng.kmers_from_reads(bases2, offsets2)
    assert len(got) == len(seqs)
    for i, sq in enumerate(seqs):
        if i in bad_reads:
            assert bad[i] == ord("x") and len(got[i]) == 0
        else:
            assert bad[i] == 0
            assert list(got[i]) == orc.kmers_from_ascii(sq, k), i


def test_all_lanes_uneven_blocks_overflow_to_spill(orc):
    """ALL-LANES mode sizes a (lane, page) region for an even share of the batch (+50 %); with
    read lengths that differ by block one lane gets several times that — the excess must take the
    spill path and nothing may be lost or double counted."""
    rng = np.random.default_rng(5)
    genome = rng.integers(0, 4, size=400_000)
    lut = np.frombuffer(b"ACGT", dtype=np.uint8)
    seqs = []
    for blk in range(30):                      # 30 blocks of 1000 reads over 3 lanes
        L = 400 if blk % 3 == 0 else 25        # lane 0 gets ~16× the bases of lanes 1 and 2
        starts = rng.integers(0, len(genome) - L, size=1000)
        seqs += [lut[genome[s:s + L]].tobytes() for s in starts]
    bases, offsets = pack(seqs)
    cnt = check_against_oracle(orc, bases, offsets, 15, 3, 500, flags=sa.FLAG_FORCE_PAGED, hint=400_000)
    import os
    if all(os.environ.get(v, "1") != "0" for v in ("SHK_REC32", "SHK_SCATTER32_LDS", "SHK_ALL_LANES")):
        assert cnt["n_spilled"] > 0  # (with the mode switched off by a test hook there is nothing to overflow)


# ---- deferred page passes: small batches into a large table wait, partitioned, for one page pass -----------

@pytest.mark.parametrize("k,chunks,hint,budget", [(21, 3, 4_200_000, 0), (21, 1, 4_200_000, 700_000),
                                                  (15, 4, 0, 0), (16, 2, 300_000, 150_000), (13, 0, 0, 0),
                                                  # k-mers too long for a 4-byte remainder: 8-byte records wait
                                                  (31, 3, 1_100_000, 0), (31, 1, 1_100_000, 400_000),
                                                  (27, 2, 2_200_000, 250_000)])
def test_deferred_page_passes(orc, monkeypatch, k, chunks, hint, budget):
    """Default flags, batches far smaller than the table: every ingest only partitions (the
    records accumulate in (lane, page) regions), a page pass runs when the budget is used up or
    somebody needs the table.  Mid-stream lookups must see everything ingested so far."""
    _deferred_page_passes(orc, monkeypatch, k, chunks, hint, budget)


@pytest.mark.parametrize("k,chunks,hint,budget,lvl1,hook_off", _rows_with_hooks(
    [(31, 2, 1_100_000, 0, 3), (29, 3, 1_100_000, 300_000, 5), (21, 2, 4_200_000, 500_000, 4), (23, 2, 1_100_000, 0, 3),
     (25, 3, 1_100_000, 300_000, 4), (23, 1, 2_200_000, 250_000, 2)],
    [((29, 3, 1_100_000, 300_000, 5), "SHK_S64_INTERLEAVE")]))   # the deferred level-2 pass reads a linear level-1 buffer
def test_deferred_page_passes_two_level(orc, monkeypatch, k, chunks, hint, budget, lvl1, hook_off):
    """The same with the super-page + re-scatter partition forced: the level-2 pass appends to the
    waiting page regions (8-byte records for k = 31 / 29 / 25 / 23, 4-byte ones for k = 21)."""
    monkeypatch.setenv("SHK_TWO_LEVEL_MIN_PAGES", "4")
    monkeypatch.setenv("SHK_LEVEL1_LOG", str(lvl1))
    if hook_off:
        monkeypatch.setenv(hook_off, "0")
    _deferred_page_passes(orc, monkeypatch, k, chunks, hint, budget)


@pytest.mark.parametrize("k,chunks", [(21, 1), (31, 2)])
def test_growth_that_finds_no_room_beside_the_waiting_regions(orc, monkeypatch, k, chunks):
    """A window planned under a capacity hint may hold most of the card; if the table has to grow all the same (the
    hint was too low) and finds no room, the — by then empty — regions are given back and planned anew beside the larger
    table (grow_to).  SHK_TEST_GROW_NOMEM makes every growth's first try fail while regions exist.  Exact all the same."""
    monkeypatch.setenv("SHK_TEST_GROW_NOMEM", "1")
    spec = sa.SynthSpec(genome_len=6_000_000, sub_per_64k=100, n_per_64k=30)
    bases, offsets = sa.synth_reads(spec, 0, 45_000)
    ref = orc.run_batch(bases, offsets, k, chunks, 100)
    with sa.KmerEngine(k, chunks, 100, capacity_hint=1_100_000) as eng:
        for a in range(0, 45_000, 1_500):
            eng.ingest_reads(bases, offsets[a:a + 1_501])
        eng.finalize()
        assert np.array_equal(eng.histograms(), ref.histograms())
        c = eng.counters()
    assert c["n_grows"] >= 1 and c["n_unique_kmers"] == ref.stats["n_unique_kmers"]


@pytest.mark.parametrize("k,chunks", [(21, 1), (21, 3), (31, 2)])
def test_grouped_flush_with_a_hint_far_too_low(orc, monkeypatch, k, chunks):
    """A capacity hint is a promise the engine must survive: with one the deferred window never ends for the
    table's sake, so a hint far too low lets a page pass meet several times more new k-mers than its pages hold —
    every one of them a spilled record.  A flush whose records could outnumber the spill list goes over the pages
    in groups and parks what each group spills in host memory until no record waits for the old geometry any more
    (here: forced groups of 7 pages); the table then grows through the ordinary repair path.  Exact all the same."""
    monkeypatch.setenv("SHK_FLUSH_GROUP_PAGES", "7")
    spec = sa.SynthSpec(genome_len=6_000_000, sub_per_64k=100, n_per_64k=30)   # ≈ 5 M distinct k-mers …
    bases, offsets = sa.synth_reads(spec, 0, 45_000)
    ref = orc.run_batch(bases, offsets, k, chunks, 100)
    with sa.KmerEngine(k, chunks, 100, capacity_hint=1_100_000) as eng:          # … promised: 1.1 M
        for a in range(0, 45_000, 1_500):
            eng.ingest_reads(bases, offsets[a:a + 1_501])
        eng.finalize()
        assert np.array_equal(eng.histograms(), ref.histograms())
        c = eng.counters()
        keys, cnts = eng.export_table()
    assert c["n_grows"] >= 1
    if chunks == 1:  # (several lanes take the owner-layout route, whose windows end before the pages overflow)
        assert c["n_spilled"] > 10_000
    for f in ("n_kmers_ingested", "n_unique_kmers", "n_hashed_kmers", "n_bases_ingested"):
        assert c[f] == ref.stats[f], f
    rk, rc = ref.merged().export()
    assert np.array_equal(keys, rk) and np.array_equal(cnts, rc)


def _deferred_page_passes(orc, monkeypatch, k, chunks, hint, budget):
    if budget:
        monkeypatch.setenv("SHK_DEFER_BUDGET", str(budget))
    spec = sa.SynthSpec(genome_len=120_000, sub_per_64k=200, n_per_64k=60)
    n_reads, step = 42_000, 1_500
    bases, offsets = sa.synth_reads(spec, 0, n_reads)
    ref = orc.run_batch(bases, offsets, k, chunks, 300)
    mid_run = orc.run_batch(bases[:int(offsets[21_000])], offsets[:21_001], k, chunks, 300)
    mid = mid_run.merged()  # (a view into mid_run: keep that alive)
    mk, mc = mid.export()
    probe = mk[:: max(len(mk) // 500, 1)]
    with sa.KmerEngine(k, chunks, 300, capacity_hint=hint, flags=sa.FLAG_TIMING) as eng:
        for a in range(0, n_reads, step):
            b = min(a + step, n_reads)
            eng.ingest_reads(bases[int(offsets[a]):int(offsets[b])], offsets[a:b + 1] - offsets[a])
            if b == 21_000:  # a table read in the middle of the stream
                got = eng.lookup(probe)
                want = np.array([mid.get_count(int(x)) for x in probe], dtype=np.uint32)
                assert np.array_equal(got, want)
        eng.finalize()
        assert np.array_equal(eng.histograms(), ref.histograms()) or chunks == 0
        c = eng.counters()
        gk, gc = eng.export_table()
        t = eng.timings()
    st = ref.stats
    assert c["n_kmers_ingested"] == st["n_kmers_ingested"] and c["n_unique_kmers"] == st["n_unique_kmers"]
    rk, rc = ref.merged().export()
    assert np.array_equal(gk, rk) and np.array_equal(gc, rc)
    if "scatter" in t:  # the deferred path ran: fewer page passes than partition launches
        # (a budget below two batches' worth of records cannot defer anything: every 1500-read batch — the
        # engine books a launch at its upper bound, one record per base of its 16 Ki-base tiles — uses it
        # up and ends its own window, one page pass per partition launch)
        batch_records = (-(-step * 150 // 16384) + (3 if chunks > 1 else 0)) * 16384  # (+ a partial tile per 1000-read block)
        if budget and budget < 2 * batch_records:
            assert t["pages"][1] <= t["scatter"][1] + 1
        else:
            assert t["pages"][1] < t["scatter"][1]
        if not budget and hint:  # … just the mid-stream lookup’s and finalize’s when the table is large and the budget untouched
            assert t["pages"][1] <= 3 * max(chunks, 1)  # (8-byte records: one page launch per lane and pass)


def test_deferred_invalid_byte_poisons_before_anything_is_counted(orc):
    spec = sa.SynthSpec(genome_len=50_000)
    bases, offsets = sa.synth_reads(spec, 0, 6_000)
    bad = bases.copy()
    bad[int(offsets[4_500]) + 7] = ord("Z")
    with sa.KmerEngine(15, 2, 100) as eng:
        eng.ingest_reads(bases[:int(offsets[3_000])], offsets[:3_001])
        with pytest.raises(sa.ShkError, match="Invalid character 'Z' in sequence. Only ACGTN allowed."):
            eng.ingest_reads(bad[int(offsets[3_000]):], offsets[3_000:] - offsets[3_000])
            eng.finalize()
        with pytest.raises(sa.ShkError):
            eng.finalize()


def test_sampled_kernel_timing():
    """SHK_FLAG_TIMING_SAMPLED: only the launches of jobs 1, 5, 9, … after shk_reset_timings are bracketed with
    events (bench.py divides by those); the counts do not care."""
    spec = sa.SynthSpec(genome_len=50_000)
    bases, offsets = sa.synth_reads(spec, 0, 4_000)
    with sa.KmerEngine(21, 1, 100, flags=sa.FLAG_TIMING | sa.FLAG_TIMING_SAMPLED) as eng:
        eng.reset_timings()
        hists = []
        for _ in range(9):
            eng.reset()
            eng.ingest_reads(bases, offsets)
            eng.finalize()
            hists.append(eng.histograms())
        tim = eng.timings()
    assert all(np.array_equal(h, hists[0]) for h in hists)
    assert tim["histo"][1] == 3 and tim["mark"][1] == 3   # jobs 1, 5 and 9
    with sa.KmerEngine(21, 1, 100, flags=sa.FLAG_TIMING) as eng:
        eng.reset_timings()
        for _ in range(3):
            eng.reset()
            eng.ingest_reads(bases, offsets)
            eng.finalize()
        assert eng.timings()["histo"][1] == 3


# ---- BASELINE configs[2]'s table geometry against the oracle -----------------------------------------------------------

def test_config3_geometry_against_the_oracle(orc):
    """k = 31 with a hint of 300 M: 2^17 pages, two full partition levels of 8-byte records, deferred page passes — on
    600 k reads: the final histogram, counters and a sample of point lookups against the oracle.  (Narrow records
    behind level 2 — 45 bits of the mixed key as a u32 and a u16 array, 6 bytes instead of 8 — were built, tested here in
    both forms and measured on the full config: re-scatter 39.6 against 39.1 ms, pages 31.9 against 31.9; the two
    kernels are not bound by the bytes they move.  Not kept.)"""
    spec = sa.SynthSpec(genome_len=2_000_000, sub_per_64k=200, n_per_64k=40)
    n_reads, step = 600_000, 150_000
    bases, offsets = sa.synth_reads(spec, 0, n_reads)
    ref = orc.run_batch(bases, offsets, 31, 2, 300)
    with sa.KmerEngine(31, 2, 300, capacity_hint=300_000_000, flags=sa.FLAG_TIMING) as eng:
        assert eng.table_geometry()[0] == 1 << 17
        for a in range(0, n_reads, step):
            eng.ingest_reads(bases, offsets[a:a + step + 1])
        eng.finalize()
        assert np.array_equal(eng.histograms(), ref.histograms())
        c = eng.counters()
        assert "pscan" in eng.timings() and "pages" in eng.timings()
        rk, rc = ref.merged().export()
        probe = rk[:: max(len(rk) // 2000, 1)]
        want = rc[:: max(len(rk) // 2000, 1)]
        assert np.array_equal(eng.lookup(probe), want)
    for f in ("n_kmers_ingested", "n_unique_kmers", "n_hashed_kmers", "n_bases_ingested", "n_reads_ingested"):
        assert c[f] == ref.stats[f], f


# ---- the process-wide block cache (shk_release_cached_memory) -------------------------------------------------------

def test_contexts_reuse_cached_blocks_and_give_them_back(orc):
    """Device and pinned blocks a context gives back are kept for the next one (mapping and unmapping memory is what
    setting a context up and taking it down costs); nothing may depend on what a recycled block holds — three contexts
    in a row over different inputs and geometries, each against the oracle — and shk_release_cached_memory hands
    everything back to the driver."""
    import torch
    sa.release_cached_memory()
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for seed, k, chunks, flags in ((1, 21, 3, 0), (2, 31, 1, sa.FLAG_FORCE_PAGED), (3, 17, 4, sa.FLAG_FORCE_DIRECT)):
        rng = np.random.default_rng(seed)
        bases, offsets = ragged_reads(rng, 6_000, max_len=200)
        check_against_oracle(orc, bases, offsets, k, chunks, 80, flags=flags)
    held = free0 - torch.cuda.mem_get_info()[0]
    assert held > 0, "nothing was kept for the next context"
    sa.release_cached_memory()
    assert free0 - torch.cuda.mem_get_info()[0] < held // 4
