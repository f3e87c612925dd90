"""GPU test of the table scans on a context with an owned page range (shk_set_owned_pages): shk_export_table,
shk_find_oligos and shk_primer_kmers read the owned slots only.  Two half ranges together must answer what the whole
table answers, an empty range nothing, and the whole range given as an owned one the whole table's answers again."""
import numpy as np
import pytest

import sharkmer_amd as sa

pytestmark = pytest.mark.gpu

K, CHUNKS, OLIGO_LEN = 15, 2, 10


def answers(eng, oligos, primers):
    """(export, find_oligos, per-primer level_hits) over the slots the context scans now."""
    ek, ec = eng.export_table()
    fk, fc = eng.find_oligos(oligos, OLIGO_LEN, min_count=1)
    pk = eng.primer_kmers(primers)
    return (ek, ec), (fk, fc), np.stack([p[3] for p in pk]), sum(len(p[0]) for p in pk)


def joined(a, b):
    """Two (kmers, counts) answers as one, sorted by k-mer the way the bindings sort a single one."""
    k = np.concatenate([a[0], b[0]])
    c = np.concatenate([a[1], b[1]])
    o = np.argsort(k, kind="stable")
    return k[o], c[o]


def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_owned_range_scans():
    spec = sa.SynthSpec(genome_len=20_000, sub_per_64k=300, n_per_64k=60)
    bases, offsets = sa.synth_reads(spec, 0, 2000)
    # two primers cut from the reads themselves (no N), one mismatch allowed
    seqs = []
    for r in range(len(offsets) - 1):
        s = bases[int(offsets[r]):int(offsets[r + 1])].tobytes().decode()
        if "N" not in s[:20] and len(s) >= 20:
            seqs.append(s[:20])
        if len(seqs) == 2:
            break
    assert len(seqs) == 2
    primers = [sa.Primer(s, trim=10, mismatches=1, min_count=1, max_kmers=40) for s in seqs]
    with sa.KmerEngine(K, CHUNKS, 100, device=0) as eng:
        eng.ingest_reads(bases, offsets)
        eng.finalize()
        n = eng.table_geometry()[0]
        if n == 1:
            eng.reserve_pages(2)
            n = eng.table_geometry()[0]
        assert n >= 2 and n % 2 == 0
        ek, ec = eng.export_table()
        assert len(ek) > 1000
        # a handful of oligos: the leading bases of exported k-mers
        oligos = np.unique(ek[:: max(len(ek) // 5, 1)][:5] >> np.uint64(2 * (K - OLIGO_LEN)))
        whole = answers(eng, oligos, primers)
        assert same(whole[0], (ek, ec))
        assert len(whole[1][0]) >= len(oligos) and whole[2].sum() > 0

        eng.set_owned_pages(0, n // 2)
        lo = answers(eng, oligos, primers)
        eng.set_owned_pages(n // 2, n)
        hi = answers(eng, oligos, primers)
        assert len(lo[0][0]) and len(hi[0][0])  # (the hash spreads the k-mers: neither half is empty)
        assert same(joined(lo[0], hi[0]), whole[0])
        assert same(joined(lo[1], hi[1]), whole[1])
        assert np.array_equal(lo[2] + hi[2], whole[2])

        for p in (0, n // 2, n):
            eng.set_owned_pages(p, p)
            none = answers(eng, oligos, primers)
            assert len(none[0][0]) == 0 and len(none[0][1]) == 0
            assert len(none[1][0]) == 0
            assert not none[2].any() and none[3] == 0

        eng.set_owned_pages(0, n)
        again = answers(eng, oligos, primers)
        assert same(again[0], whole[0]) and same(again[1], whole[1])
        assert np.array_equal(again[2], whole[2]) and again[3] == whole[3]
