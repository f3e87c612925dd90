"""CPU checks of sPCR's primer seed discovery (shk_primer_compile, shk_primer_kmers): the ABI, the reference's
preprocessing KATs (src/pcr/primers.rs, pcr/mod.rs), its edge cases and error texts, and the equivalence the GPU scan
rests on — a string's mismatch level is the number of positions whose base the IUPAC code does not allow — pinned
against literal enumeration of the level sets.  No GPU: shk_primer_compile touches no device."""
import os
import random
import re

import numpy as np
import pytest

import primer_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sa():
    import __graft_entry__ as g
    g.build()
    import sharkmer_amd
    return sharkmer_amd


def test_symbols_exported_declared_and_bound(sa):
    import ctypes
    from sharkmer_amd.engine import ABI_SYMBOLS, lib_path
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "shk.h")).read(), flags=re.S)
    L = ctypes.CDLL(lib_path())
    for name in ("shk_primer_compile", "shk_primer_kmers"):
        assert name in ABI_SYMBOLS
        assert re.search(rf"\b{name}\s*\(", hdr)
        assert hasattr(L, name)
    assert "typedef struct shk_primer" in hdr and "SHK_PRIMER_LEVELS 33" in hdr
    assert sa.PRIMER_LEVELS == 33 and hasattr(sa.KmerEngine, "primer_kmers") and hasattr(sa.KmerEngine, "primer_pair_kmers")
    p = sa.Primer("ACGT")
    assert (p.trim, p.mismatches, p.min_count, p.max_kmers) == (15, 2, 2, 40)  # PCRParams' defaults


def test_reference_kats(sa):
    # test_primer_preprocessing_steps (pcr/mod.rs:1287-1297): 991 variants of the reverse primer at r = 2
    L, sizes = sa.primer_compile(sa.Primer("TGATCCTTCTGCAGGTTCACCTAC", trim=15, mismatches=2), 21)
    assert L == 15 and sizes == [1, 45, 945] and sum(sizes) == 991
    # primers.rs:759-821: ACGTACGT, k 8, trim 7 → CGTACGT, three levels
    L, sizes = sa.primer_compile(sa.Primer("ACGTACGT", trim=7, mismatches=2), 8)
    assert L == 7 and len(sizes) == 3
    assert ref.trim_primer("ACGTACGT", 7, 8) == "CGTACGT"
    assert sizes == [len(s) for s in ref.levels_literal("CGTACGT", 2)]
    # resolve_primer counts (primers.rs:520-556)
    for p, n in [("ACGT", 1), ("AR", 2), ("RY", 4), ("N", 4)]:
        assert sa.primer_compile(sa.Primer(p, trim=15, mismatches=0), 21)[1] == [n]
        assert len(ref.resolve_primer(p)) == n


def test_edge_cases(sa):
    # trim ≥ k clamps to k − 1
    assert sa.primer_compile(sa.Primer("ACGTACGTACGTACGTACGTACGT", trim=40, mismatches=0), 11)[0] == 10
    assert sa.primer_compile(sa.Primer("ACGTACGTACGTACGTACGTACGT", trim=11, mismatches=0), 11)[0] == 10
    # a primer shorter than trim is kept whole; mismatches clamp to L
    L, sizes = sa.primer_compile(sa.Primer("ACG", trim=15, mismatches=7), 21)
    assert L == 3 and sizes == [1, 9, 27, 27]
    # trim 0 or an empty primer: no levels and no error (also with an invalid character, or too many variants)
    for p in (sa.Primer("ACGT", trim=0), sa.Primer(""), sa.Primer("AXGT", trim=0), sa.Primer("N" * 20, trim=0)):
        assert sa.primer_compile(p, 21) == (0, [])
    # too many variants: the reference's text exactly
    with pytest.raises(sa.ShkError) as e:
        sa.primer_compile(sa.Primer("NNNNNNNNNNNNNNN"), 21)
    assert e.value.msg == ("Primer NNNNNNNNNNNNNNN has too many ambiguous bases: 1073741824 resolved variants "
                           "exceeds limit of 10000. Reduce ambiguity or use a more specific primer.")
    with pytest.raises(ref.RefError) as e2:
        ref.check_variant_limit("NNNNNNNNNNNNNNN", 15, 21)
    assert str(e2.value) == e.value.msg
    # trimmed before it is resolved: the N's cut off do not count
    assert sa.primer_compile(sa.Primer("NNNNNNNNNNACGTACGTACGTACGTA", trim=15, mismatches=0), 21)[1] == [1]
    # an invalid character: the whole text without an ambiguity code, the prefix with one
    with pytest.raises(sa.ShkError) as e:
        sa.primer_compile(sa.Primer("ACGTXACGT"), 21)
    assert e.value.code == -1 and e.value.msg == "Invalid nucleotide X in ACGTXACGT"
    with pytest.raises(ref.RefError) as e2:
        ref.string_to_oligo("ACGTXACGT")
    assert str(e2.value) == e.value.msg
    with pytest.raises(sa.ShkError) as e:
        sa.primer_compile(sa.Primer("ACGTRaCGT"), 21)
    assert e.value.msg.startswith("Invalid nucleotide a in ")
    # … cut off by the trim: never looked at; with max_kmers 0: never converted
    assert sa.primer_compile(sa.Primer("XXACGTACGT", trim=8, mismatches=0), 21)[1] == [1]
    assert sa.primer_compile(sa.Primer("ACGTXACGT", max_kmers=0), 21)[0] == 9
    # the variant limit comes before the character check
    with pytest.raises(sa.ShkError) as e:
        sa.primer_compile(sa.Primer("XNNNNNNNNN"), 21)
    assert "too many ambiguous bases" in e.value.msg


def _random_iupac(rng, L):
    return "".join(rng.choice("ACGTACGTACGTRYSWKMBDHVN") for _ in range(L))


def test_levels_are_mismatch_counts_against_enumeration(sa):
    """For a few hundred random IUPAC primers (L ≤ 6, M ≤ 3) and every one of the 4^L strings: the level by the bit
    masks k_primer_scan uses equals the level by literal enumeration (resolve_primer + permute_sequences), and the
    level sizes shk_primer_compile reports equal the literal sets' (and the encoded ones the helper scans with)."""
    rng = random.Random(7)
    k = 9
    for _ in range(300):
        L = rng.randint(1, 6)
        M = rng.randint(0, 3)
        p = _random_iupac(rng, L)
        lev = ref.levels_literal(p, M)
        level_of = {s: m for m, ss in enumerate(lev) for s in ss}
        assert sa.primer_compile(sa.Primer(p, trim=k - 1, mismatches=M), k) == (L, [len(s) for s in lev])
        enc = ref.levels_encoded(p, M)
        assert [sorted(ref.string_to_oligo(s) for s in ss) for ss in lev] == [list(map(int, e)) for e in enc]
        for v in range(4 ** L):
            s = "".join("ACGT"[(v >> (2 * (L - 1 - i))) & 3] for i in range(L))
            x = (v << (2 * (k - L))) | rng.getrandbits(2 * (k - L))  # the string at the start of a k-mer
            m = ref.mask_level(x, p, k)
            assert level_of.get(s, None) == (m if m <= min(M, L) else None), (p, M, s)


def test_helper_scan_matches_oracle_find_oligos(orc):
    """The helper's per-level find_oligos_in_kmers (np.isin) against the oracle's KmerCounts.find_oligos (pinned by
    KATs) on levels of at most 3000 oligos."""
    import sharkmer_amd as sa_
    spec = sa_.SynthSpec(genome_len=30_000, sub_per_64k=200, n_per_64k=20, seed_genome=3)
    bases, offsets = sa_.synth_reads(spec, 0, 3000)
    k = 15
    run = orc.run_batch(bases, offsets, k, 2, 100)
    merged = run.merged()  # (a view into run: run must outlive it)
    keys, counts = merged.export()
    g = bases[offsets[0]:offsets[1]].tobytes().decode()
    checked = 0
    for p in (g[10:22], "ACGTRY" + g[50:56], g[80:94]):
        for m, lvl in enumerate(ref.levels_encoded(p, 2)):
            if not 0 < len(lvl) <= 3000:
                continue
            for mc in (1, 2):
                gk, gc = ref.find_oligos_in_kmers(lvl, len(p), keys, counts, k, mc)
                o = np.argsort(gk, kind="stable")
                wk, wc = merged.find_oligos(lvl, len(p), mc)
                assert np.array_equal(gk[o], wk) and np.array_equal(gc[o], wc)
                checked += len(wk)
    assert checked > 0
