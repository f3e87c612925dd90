"""GPU tests of sPCR's primer seed discovery in one pass (shk_primer_kmers, k_primer_scan): get_primer_kmers
(src/pcr/primers.rs:234-480) for whole panels against tests/primer_ref.py — the reference restated literally
(resolve_primer, permute_sequences level by level, find_oligos_in_kmers per level, the round-by-round cap) over the
CPU oracle's merged table.  k-mers, counts, levels, their order and the per-level hits must be equal."""
import os
import random

import numpy as np
import pytest

import sharkmer_amd as sa
import primer_ref as ref

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CODES = {"A": "RWMDHVN", "C": "YSMBHVN", "G": "RSKBDVN", "T": "YWKBDHN"}  # codes that allow the base


def oracle_table(orc, bases, offsets, k, chunks):
    run = orc.run_batch(bases, offsets, k, chunks, 100)
    return run.merged().export()  # (copies: run may go)


def expected(primers, keys, counts, k):
    for p in primers:  # every direction's variant limit before any scan (primers.rs:440-450)
        ref.check_variant_limit(p.seq, p.trim, k)
    return [ref.get_primer_kmers(p.seq, keys, counts, k, p.trim, p.mismatches, p.min_count, p.max_kmers,
                                 check_variants=False) for p in primers]


def assert_same(got, want, primers=None):
    assert len(got) == len(want)
    for i, ((gk, gc, gl, gh), (wk, wc, wl, wh)) in enumerate(zip(got, want)):
        what = primers[i] if primers else i
        assert np.array_equal(gk, wk), (what, gk[:8], wk[:8])
        assert np.array_equal(gc, wc), what
        assert np.array_equal(gl, wl), what
        assert np.array_equal(gh, wh), (what, gh[:5], wh[:5])


def reads_of(seq, copies):
    b = np.frombuffer(seq.encode() * copies, dtype=np.uint8).copy()
    return b, np.arange(copies + 1, dtype=np.uint64) * np.uint64(len(seq))


def rc_str(s):
    return s[::-1].translate(str.maketrans("ACGTN", "TGCAN"))


def random_primers(rng, genome_reads, k, n, max_kmers=(0, 1, 3, 40, 10_000)):
    """Primers cut from reads of the genome, from either strand, with ambiguity codes and 0-3 substitutions."""
    bases, offsets = genome_reads
    out = []
    while len(out) < n:
        r = rng.randrange(len(offsets) - 1)
        s = bases[int(offsets[r]):int(offsets[r + 1])].tobytes().decode()
        ln = rng.randint(8, 28)
        at = rng.randrange(0, len(s) - ln)
        p = s[at:at + ln]
        if "N" in p:
            continue
        if rng.random() < 0.5:
            p = rc_str(p)
        p = list(p)
        for _ in range(rng.choice((0, 0, 1, 2, 3))):
            i = rng.randrange(ln)
            p[i] = rng.choice(CODES.get(p[i], p[i]))
        for _ in range(rng.choice((0, 0, 1, 2, 3))):
            i = rng.randrange(ln)
            if p[i] in "ACGT":
                p[i] = rng.choice([b for b in "ACGT" if b != p[i]])
        trim = rng.choice((0, 4, 6, 8, 10, 12, 15, k - 1, k, k + 3))
        out.append(sa.Primer("".join(p), trim=trim, mismatches=rng.randint(0, 3), min_count=rng.randint(1, 3),
                             max_kmers=rng.choice(max_kmers)))
    return out


def test_reference_integration_case(orc):
    """test_integration (pcr/mod.rs:1331-1350): the padded 18S ×10 at k 21, the 18S primer pair, min_count 3 → one
    forward and one reverse primer k-mer."""
    seq = open(os.path.join(G, "pcr_18s_padded.txt")).read().strip()
    bases, offsets = reads_of(seq, 10)
    k = 21
    keys, counts = oracle_table(orc, bases, offsets, k, 1)
    fwd, rev = "AACCTGGTTGATCCTGCCAGT", "TGATCCTTCTGCAGGTTCACCTAC"
    params = dict(trim=15, mismatches=2, min_count=3)
    with sa.KmerEngine(k, 1, 100) as eng:
        eng.ingest_reads(bases, offsets)
        eng.finalize()
        gf, gr = eng.primer_pair_kmers(fwd, rev, **params)
    wf, wr = expected([sa.Primer(fwd, **params), sa.Primer(rev, **params)], keys, counts, k)
    assert len(gf[0]) == 1 and len(gr[0]) == 1
    assert_same([gf, gr], [wf, wr])
    assert list(gf[1]) == [10] and list(gr[1]) == [10]


@pytest.mark.parametrize("k,chunks", [(11, 1), (15, 3), (21, 1), (25, 3), (31, 1), (20, 3)])
def test_random_panels_against_reference(orc, k, chunks):
    """k ∈ {11, 15, 21, 25, 31} and an even k, 1 and 3 chunk lanes; 40 primer directions in one call with trims from
    0 to k + 3, mismatches 0-3, min_count 1-3 and max_kmers ∈ {0, 1, 3, 40, 10⁴}."""
    rng = random.Random(1000 + k)
    spec = sa.SynthSpec(genome_len=40_000, sub_per_64k=400, n_per_64k=30, seed_genome=k)
    bases, offsets = sa.synth_reads(spec, 0, 1200)
    keys, counts = oracle_table(orc, bases, offsets, k, chunks)
    primers = random_primers(rng, (bases, offsets), k, 40)
    want = expected(primers, keys, counts, k)
    with sa.KmerEngine(k, chunks, 100) as eng:
        eng.ingest_reads(bases, offsets)
        eng.finalize()
        got = eng.primer_kmers(primers)
    assert_same(got, want, primers)
    assert sum(len(w[0]) for w in want) > 0
    assert tie_cuts(primers, want, keys, counts, k) > 0


def tie_cuts(primers, want, keys, counts, k):
    """Primers whose cap falls inside a level between equal counts: the first hit left out has the last count kept."""
    n = 0
    for p, (wk, wc, wl, wh) in zip(primers, want):
        if 0 < p.max_kmers == len(wk) and wh[int(wl[-1])] > np.sum(wl == wl[-1]):
            more = ref.get_primer_kmers(p.seq, keys, counts, k, p.trim, p.mismatches, p.min_count, p.max_kmers + 1)
            n += int(more[2][-1] == wl[-1] and more[1][-1] == wc[-1])
    return n


def test_agrees_with_find_oligos(orc):
    """Unambiguous primers at mismatches 0 with an unbounded cap: the same (k-mer, count) set as shk_find_oligos."""
    rng = random.Random(5)
    k = 19
    spec = sa.SynthSpec(genome_len=30_000, sub_per_64k=300, seed_genome=9)
    bases, offsets = sa.synth_reads(spec, 0, 1500)
    primers = [sa.Primer(p.seq, trim=rng.choice((5, 7, 10, 14)), mismatches=0, min_count=p.min_count, max_kmers=100_000)
               for p in random_primers(rng, (bases, offsets), k, 16)]
    primers = [p for p in primers if set(p.seq) <= set("ACGT")]
    with sa.KmerEngine(k, 2, 100) as eng:
        eng.ingest_reads(bases, offsets)
        eng.finalize()
        got = eng.primer_kmers(primers)
        for p, (gk, gc, gl, gh) in zip(primers, got):
            P = ref.trim_primer(p.seq, p.trim, k)
            wk, wc = eng.find_oligos([ref.string_to_oligo(P)], len(P), p.min_count)
            o = np.argsort(gk, kind="stable")
            assert np.array_equal(gk[o], wk) and np.array_equal(gc[o], wc)
            assert not gl.any() and int(gh[0]) == len(wk) and not gh[1:].any()


def test_forced_overflow_many_candidates(orc, monkeypatch):
    """More than 10⁵ candidates (short primers, three mismatches): a candidate buffer of one record (the rerun with
    the levels cut at each primer's cap) gives what an ample buffer gives, and what the reference gives."""
    k = 15
    spec = sa.SynthSpec(genome_len=300_000, seed_genome=77)
    bases, offsets = sa.synth_reads(spec, 0, 6000)
    keys, counts = oracle_table(orc, bases, offsets, k, 1)
    primers = [sa.Primer("ACGTTGCA", trim=5, mismatches=3, min_count=1, max_kmers=10_000),
               sa.Primer("GGATCCRA", trim=6, mismatches=2, min_count=1, max_kmers=40),
               sa.Primer("TTGACYAGT", trim=9, mismatches=3, min_count=2, max_kmers=3),
               sa.Primer("CATGCATG", trim=5, mismatches=1, min_count=1, max_kmers=200_000)]
    want = expected(primers, keys, counts, k)
    assert sum(int(w[3].sum()) for w in want) >= 100_000
    with sa.KmerEngine(k, 1, 100) as eng:
        eng.ingest_reads(bases, offsets)
        eng.finalize()
        monkeypatch.setenv("SHK_PRIMER_CANDIDATES", "10000000")
        ample = eng.primer_kmers(primers)
        monkeypatch.setenv("SHK_PRIMER_CANDIDATES", "1")
        forced = eng.primer_kmers(primers)
    assert_same(ample, want, primers)
    assert_same(forced, want, primers)


def test_counts_near_u32_max_over_lanes(orc):
    """Merged counts are the saturating sum over chunk lanes (as k_find_oligos reads them): canonical k-mers inserted
    into three lanes with counts near 2^32 − 1."""
    k = 21
    rng = np.random.default_rng(3)
    raw = rng.integers(0, 1 << (2 * k), size=4000, dtype=np.uint64)
    keys = np.unique(np.minimum(raw, ref.revcomp(raw, k)))
    big = np.uint32(0xFFFFFFF0)
    with sa.KmerEngine(k, 3, 100) as eng:
        for lane in range(3):
            c = np.where(np.arange(len(keys)) % (lane + 2) == 0, big - np.uint32(lane), np.uint32(lane + 1)).astype(np.uint32)
            eng.insert(keys, c, chunk_id=lane)
        tk, tc = eng.export_table()
        assert (tc == 0xFFFFFFFF).any() and ((tc > 0xF0000000) & (tc < 0xFFFFFFFF)).any()
        primers = [sa.Primer("".join("ACGT"[(int(x) >> (2 * (k - 1 - i))) & 3] for i in range(k)), trim=t, mismatches=m,
                             min_count=mc, max_kmers=mk)
                   for x, t, m, mc, mk in [(keys[0], 8, 2, 1, 40), (keys[7], 6, 1, 0xFFFFFFF0, 40),
                                           (keys[100], 10, 3, 2, 10_000), (keys[5], 7, 2, 0xFFFFFFFF, 5)]]
        got = eng.primer_kmers(primers)
    want = expected(primers, tk, tc, k)
    assert_same(got, want, primers)
    assert any((w[1] == 0xFFFFFFFF).any() for w in want)


def test_owner_share_scans_its_pages(orc):
    """An owner share (n_owners = 4, drop mode): its answer is the reference's on the k-mers it owns."""
    from test_gpu_owner import _owner_of
    k, W = 21, 4
    spec = sa.SynthSpec(genome_len=50_000, sub_per_64k=300, seed_genome=21)
    bases, offsets = sa.synth_reads(spec, 0, 1500)
    keys, counts = oracle_table(orc, bases, offsets, k, 1)
    primers = random_primers(random.Random(4), (bases, offsets), k, 32)
    for o in range(W):
        own = _owner_of(keys, k, W) == o
        want = expected(primers, keys[own], counts[own], k)
        with sa.KmerEngine(k, 1, 100, n_owners=W, owner_id=o) as eng:
            eng.ingest_reads(bases, offsets)
            eng.finalize()
            got = eng.primer_kmers(primers)
        assert_same(got, want, primers)


def test_multi_device_context_equals_one(orc):
    """A multi-device context (device 0 repeated): per share, union, select — equal to one context and the
    reference."""
    k = 21
    spec = sa.SynthSpec(genome_len=50_000, sub_per_64k=300, seed_genome=22)
    bases, offsets = sa.synth_reads(spec, 0, 2000)
    keys, counts = oracle_table(orc, bases, offsets, k, 3)
    primers = random_primers(random.Random(6), (bases, offsets), k, 32)
    want = expected(primers, keys, counts, k)
    out = []
    for devs in (None, [0, 0], [0, 0, 0, 0]):
        with sa.KmerEngine(k, 3, 100, device_ids=devs) as eng:
            eng.ingest_reads(bases, offsets)
            eng.finalize()
            out.append(eng.primer_kmers(primers))
    for got in out:
        assert_same(got, want, primers)


def test_mid_stream_and_after_reset(orc, monkeypatch):
    """After an ingest without finalize the call sees everything ingested so far; after a reset it sees nothing; the
    overflow rerun in a multi-device context too."""
    k = 17
    spec = sa.SynthSpec(genome_len=40_000, sub_per_64k=300, seed_genome=23)
    bases, offsets = sa.synth_reads(spec, 0, 1600)
    half = 700
    primers = random_primers(random.Random(8), (bases, offsets), k, 32)
    primers.append(sa.Primer("ACGTAC", trim=6, mismatches=2, min_count=1, max_kmers=10_000))
    kh, ch = oracle_table(orc, bases[:int(offsets[half])], offsets[:half + 1], k, 2)
    ka, ca = oracle_table(orc, bases, offsets, k, 2)
    for devs in (None, [0, 0]):
        with sa.KmerEngine(k, 2, 100, device_ids=devs) as eng:
            eng.ingest_reads(bases, offsets[:half + 1])
            assert_same(eng.primer_kmers(primers), expected(primers, kh, ch, k), primers)
            eng.ingest_reads(bases, offsets[half:])
            monkeypatch.setenv("SHK_PRIMER_CANDIDATES", "5")
            assert_same(eng.primer_kmers(primers), expected(primers, ka, ca, k), primers)
            monkeypatch.delenv("SHK_PRIMER_CANDIDATES")
            eng.reset()
            for gk, gc, gl, gh in eng.primer_kmers(primers):
                assert len(gk) == 0 and not gh.any()
            eng.ingest_reads(bases, offsets[:half + 1])
            eng.finalize()
            assert_same(eng.primer_kmers(primers), expected(primers, kh, ch, k), primers)


def test_even_k_palindrome_yields_once(orc):
    """Even k: a palindromic k-mer x = revcomp(x) has f = r and is yielded once."""
    k = 12
    pal = "ACGTAATTACGT"  # its own reverse complement
    assert rc_str(pal) == pal
    bases, offsets = reads_of(pal, 4)
    keys, counts = oracle_table(orc, bases, offsets, k, 1)
    primers = [sa.Primer("ACGTAAT", trim=7, mismatches=1, min_count=1), sa.Primer("ACGTAAT", trim=7, mismatches=0,
                                                                                 min_count=1)]
    want = expected(primers, keys, counts, k)
    with sa.KmerEngine(k, 1, 100) as eng:
        eng.ingest_reads(bases, offsets)
        eng.finalize()
        got = eng.primer_kmers(primers)
    assert_same(got, want, primers)
    x = ref.string_to_oligo(pal)
    assert list(got[1][0]).count(x) == 1


def test_errors_and_empty_primers():
    """The texts of shk_last_error, the too-many check of every direction before the character check, and primers
    that are never searched (trim 0, empty, max_kmers 0)."""
    with sa.KmerEngine(21, 1, 100) as eng:
        eng.ingest_reads(*reads_of("ACGT" * 40, 3))
        with pytest.raises(sa.ShkError) as e:
            eng.primer_pair_kmers("ACGTXACGTAAC", "NNNNNNNNNNNNNNN")
        assert e.value.msg.startswith("Primer NNNNNNNNNNNNNNN has too many ambiguous bases: 1073741824")
        with pytest.raises(sa.ShkError) as e:
            eng.primer_pair_kmers("ACGTACGTAAC", "ACGTXACGT")
        assert e.value.code == -1 and e.value.msg == "Invalid nucleotide X in ACGTXACGT"
        got = eng.primer_kmers([sa.Primer("ACGT", trim=0), sa.Primer(""), sa.Primer("ACGTXACGT", max_kmers=0),
                                sa.Primer("ACGTACGT", min_count=1)])
        for gk, gc, gl, gh in got[:3]:
            assert len(gk) == 0 and not gh.any()
        assert len(got[3][0]) > 0
