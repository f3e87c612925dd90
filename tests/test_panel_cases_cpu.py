"""The crafted cases of the panel read filter (tests/panel_cases.py) hold what their names say — checked against the
oracle alone, so that a case cannot silently stop exercising what it is there for.  No GPU."""
import panel_cases as pc

T = pc.T


def test_every_claim_holds_under_the_oracle(orc):
    cases = pc.crafted_cases(orc)
    kinds = set()
    for case in cases:
        rows = pc.expected(orc, case)
        assert len(rows) == len(case.genes)
        assert case.claims, case.name
        for claim in case.claims:
            what, a = claim[0], claim[1:]
            kinds.add(what)
            if what == "windows":
                assert len(case.reads[a[0]]) - case.k + 1 == a[1], (case.name, claim)
            elif what == "hits":
                seq = case.reads[a[1]] if isinstance(a[1], int) else a[1]
                assert pc.hit_positions(orc, case.genes[a[0]], seq, case.k) == a[2], (case.name, claim)
            elif what == "match":
                assert (a[1] in rows[a[0]]) == a[2], (case.name, claim)
            elif what == "straddles":
                assert a[0] // T != (a[0] + case.k - 1) // T, (case.name, claim)
            elif what == "byte":
                assert case.reads[a[0]][a[1]:a[1] + 1] == a[2], (case.name, claim)
            elif what == "rows":
                assert rows == a[0], (case.name, claim)
            else:
                raise AssertionError(claim)
    assert kinds == {"windows", "hits", "match", "straddles", "byte", "rows"}


def test_the_cases_cover_the_list(orc):
    cases = pc.crafted_cases(orc)
    assert sorted(set(c.k for c in cases)) == [2, 3, 5, 21, 31]
    assert sorted(len(c.genes) for c in cases if "the only matching gene" in c.name) == [1, 64, 65, 130, 4096]
    for c in cases:
        if "the only matching gene" in c.name:  # the matching genes are the first, the last and both sides of each word edge
            n = len(c.genes)
            hit = [g for g, row in enumerate(pc.expected(orc, c)) if row]
            assert hit == sorted(set(p for p in (0, 31, 32, 63, 64, 95, 96, 127, 128, 2047, 2048, n - 1) if p < n)), c.name
    # every class of read the filter treats differently occurs, and has both answers where it can
    reads = [r for c in cases for r in c.reads]
    assert any(len(r) == 0 for r in reads) and any(set(r) == {ord("N")} for r in reads)
    assert any(len(r) > 3 * T + 21 for r in reads)
    assert any(any(ch not in b"ACGTN" for ch in r) for r in reads)
    none = [c for c in cases if "no read matches" in c.name]
    assert len(none) == 1 and not any(pc.expected(orc, none[0]))


def test_big_batch_has_every_gene_matched_and_reads_without_a_match(orc):
    for k in (5, 21, 31):
        seqs, single, genes, rows = pc.big_batch(orc, k)
        assert len(seqs) == 3003 and len(genes) == 12 and len(single) > 0
        assert all(len(r) > 0 for r in rows), k
        matched = set(i for r in rows for i in r)
        assert len(seqs) - len(matched) >= 40, k
        assert sum(1 for s in seqs if b"X" in s) == 40


def test_stride_batch_gives_a_wave_consecutive_reads_that_differ(orc):
    k, genes, kinds, kind_genes, order = pc.stride_batch(orc)
    assert kind_genes[0] == [0, 33, 69] and kind_genes[1] == [31, 32] and kind_genes[4] == [64] and kind_genes[9] == [5]
    assert kind_genes[10] == [0, 33, 69]  # kind 2 is kind 10 with an invalid byte two steps behind the hits: nothing
    assert kinds[2] == pc.put(kinds[10], 140, b"X") and kind_genes[2] == [] and 140 // T >= 2
    assert pc.hit_positions(orc, [x for g in (0, 33, 69) for x in genes[g]], kinds[10], k) == [0, 7, 19]
    assert kinds[5][:40] == kinds[1] and kinds[5][149:] == b"x" and kind_genes[5] == []
    assert all(kind_genes[j] == [] for j in (3, 6, 7, 8))
    assert pc.hit_positions(orc, genes[5], kinds[9], k) == [125] and len(kinds[9]) - k + 1 > 2 * T
    # whatever the grid — 16 waves per workgroup, one or two workgroups per CU, up to 256 CUs — every wave gets several
    # reads, and every kind is followed by every kind on some wave
    n = len(order)
    for n_waves in (4096, 8192):
        assert n >= 4 * n_waves
        pairs = set(zip(order[:-n_waves].tolist(), order[n_waves:].tolist()))
        assert len(pairs) == len(kinds) ** 2, n_waves
    rows = pc.stride_rows(orc)
    assert sum(len(r) for r in rows) > n // 2 and rows[1] == []
