"""The batch all four read walkers are held to (tests/read_walk_cases.py) holds what its reads are named for — checked
against the oracle alone, so that a read cannot silently stop exercising what it is there for.  No GPU."""
import pytest

import read_walk_cases as rw
import thread_ref as ref

T = rw.T


@pytest.mark.parametrize("k", rw.KS)
def test_every_claim_holds_under_the_oracle(orc, k):
    b = rw.batch(orc, k)
    have = set(b.set_kmers)
    matches = rw.expected_matches(orc, b)
    kinds = set()
    claimed = set()
    for what, i, *a in b.claims:
        kinds.add(what)
        claimed.add(i)
        read, name = b.reads[i], (k, b.names[i])
        if what == "hits":
            assert rw.hit_positions(orc, have, read, k) == a[0], name
        elif what == "byte":
            assert read[a[0]:a[0] + 1] == a[1], name
        elif what == "valid":
            assert all(c in b"ACGTN" for c in read) == a[0], name
        elif what == "match":
            assert matches[i] == a[0], name
        elif what == "healed":
            assert rw.hit_positions(orc, have, rw.put(read, a[0], a[1]), k) == a[2], name
        else:
            raise AssertionError(what)
    assert kinds == {"hits", "byte", "valid", "match", "healed"}
    assert claimed == set(range(len(b.reads)))  # no read without a claim
    assert len(b.reads) <= 300 and any(matches) and not all(matches)


@pytest.mark.parametrize("k", rw.KS)
def test_the_batch_covers_the_list(orc, k):
    b = rw.batch(orc, k)
    assert set(rw.lengths(k)) <= set(len(r) for r in b.reads)
    assert rw.lengths(k) == [0, k - 1, k, k + 1, 63, 64, 65, 64 + k - 2, 64 + k - 1, 64 + k, 127, 128, 129, 200]
    n_at = set(p for r in b.reads for p in range(len(r)) if r[p:p + 1] == b"N" and set(r) != {ord("N")})
    assert {62, 63, 64, 65, 199} <= n_at
    bad_at = set(p for r in b.reads if r != r.lower() for p in range(len(r)) if r[p] not in b"ACGTN")
    assert bad_at == {0, 63, 64, 64 + k - 1, 199}
    assert sum(1 for r in b.reads if r and r == r.lower()) == 1
    # the only set k-mer at window 63, at 64, and in the last window of a read of several steps
    have = set(b.set_kmers)
    only = [rw.hit_positions(orc, have, r, k) for r in b.reads if len(r) == rw.LONG and all(c in b"ACGT" for c in r)]
    for w in (63, 64, rw.LONG - k):
        assert [w] in only, w
    # the marker ends in the base an N decodes to when only its two code bits are looked at
    assert b.marker[-1:] == b"A" and ((ord("N") >> 1) ^ (ord("N") >> 2)) & 3 == ((ord("A") >> 1) ^ (ord("A") >> 2)) & 3
    # the expected k-mer lists: a valid read has one per window without an N, an invalid one none and its first bad byte
    for r, (kmers, bad) in zip(b.reads, rw.expected_kmers(orc, b)):
        if bad:
            assert kmers == [] and bad == next(c for c in r if c not in b"ACGTN")
        else:
            assert len(kmers) == sum(1 for w in range(len(r) - k + 1) if b"N" not in r[w:w + k])


@pytest.mark.parametrize("k", rw.KS)
def test_the_linear_graph_lies_across_the_step_edge_and_some_reads_thread_it(orc, k):
    b = rw.batch(orc, k)
    nodes, edges, edge_kmers, first = rw.linear_graph(b)
    g = ref.Graph(nodes, edges)
    canon = [orc.kmers_from_ascii(x, k)[0] for x in edge_kmers]
    assert [min(x, ref.revcomp(x, k)) for x in (ref.reconstruct_edge_kmer(g, e) for e in range(len(edges)))] == canon
    src = b.reads[b.names.index("only set k-mer at window 64")]
    assert src[first:first + k] == edge_kmers[0]
    assert first < T - 1 and first + len(edges) > T + 1  # windows 63 and 64 of that read are edges
    ann = ref.thread_reads(g, b.reads, k)
    read_edges = ref.as_arrays(ann, len(edges))[4]
    assert read_edges[b.reads.index(src)] >= len(edges)  # (at k = 3 the background repeats the chain's k-mers)
    assert [n > 0 for n in read_edges] == rw.expected_matches(orc, b, canon)
    assert 0 < sum(1 for n in read_edges if n) < len(b.reads)
    if k == 3:  # equal k-mers along the chain: several candidates under one key
        assert len(set(canon)) < len(canon)
