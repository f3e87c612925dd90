"""The read-threading model (tests/thread_ref.py) against the reference's own unit tests (src/pcr/threading.rs:423-628),
restated, and the coverage of the random sweep that the GPU tests run shk_thread_reads over (tests/thread_cases.py).  No
GPU."""
import os
import re

import thread_cases as tc
import thread_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def canonical_edge_kmer(g, e, k):
    x = ref.reconstruct_edge_kmer(g, e)
    return min(x, ref.revcomp(x, k))


# ---- threading.rs:423-628 ------------------------------------------------------------------------------------------------

def test_build_edge_lookup():
    lookup = ref.build_edge_lookup(tc.linear_graph(), 3)
    assert len(lookup) == 2
    assert all(len(c) == 1 for c in lookup.values())


def test_contiguous_run_linear():
    g = tc.linear_graph()
    lookup = ref.build_edge_lookup(g, 3)
    runs = ref.find_contiguous_runs([canonical_edge_kmer(g, 0, 3), canonical_edge_kmer(g, 1, 3)], lookup, g)
    assert len(runs) == 1 and len(runs[0]) == 2


def test_contiguous_run_gap():
    g = tc.linear_graph()
    lookup = ref.build_edge_lookup(g, 3)
    gap = 0xDEADBEEF
    assert gap not in lookup
    runs = ref.find_contiguous_runs([canonical_edge_kmer(g, 0, 3), gap, canonical_edge_kmer(g, 1, 3)], lookup, g)
    assert [len(r) for r in runs] == [1, 1]


def test_inverted_repeat_disambiguation():
    g = tc.inverted_repeat_graph()
    e_x, e_bridge, e_rcx = 0, 1, 2
    lookup = ref.build_edge_lookup(g, 3)
    canonical = canonical_edge_kmer(g, e_x, 3)
    assert canonical == canonical_edge_kmer(g, e_rcx, 3)
    assert lookup[canonical] == [e_x, e_rcx]
    runs = ref.find_contiguous_runs([canonical, canonical_edge_kmer(g, e_bridge, 3), canonical], lookup, g)
    assert [e for r in runs for e in r][2] == e_rcx


def test_unambiguous_linear():
    assert ref.is_run_unambiguous(tc.linear_graph(), [0, 1])


def test_branch_point_detection():
    g = tc.branch_graph()
    assert not ref.is_run_unambiguous(g, [0, 1])
    links = {}
    ref.record_branch_links(g, [0, 1], links)
    assert links == {(0, 1): 1}


# ---- the model on the crafted cases: the answers that can be read off the case ----------------------------------------

def _case(name):
    return next(c for c in tc.crafted_cases() if c[0].startswith(name))


def test_crafted_answers():
    _, g, reads = _case("4-cycle")
    tot, una, links, counts, re_ = ref.as_arrays(ref.thread_reads(g, reads[:1], 3), 4)
    assert tot == [3, 3, 3, 3] and una == [3, 3, 3, 3] and links == [] and re_ == [12]
    _, g, reads = _case("three candidates")
    tot, una, links, counts, re_ = ref.as_arrays(ref.thread_reads(g, reads[:1], 3), 4)
    assert tot == [0, 1, 0, 1] and re_ == [2]  # CA → AA(1), then the candidate whose source is node 1
    _, g, reads = _case("linear: a run across an N")
    ann = ref.thread_reads(g, reads[:1], 3)
    assert ann.events.get("run_across_n") == 1 and ann.read_edges == [2]
    _, g, reads = _case("linear: an invalid byte")
    assert ref.thread_reads(g, reads, 3).read_edges == [0, 2, 0, 0]
    _, g, reads = _case("linear: lengths")
    ann = ref.thread_reads(g, reads, 3)
    assert ann.read_edges == [0, 0, 1, 2, 0, 2, 2]
    assert ann.support_unambiguous == {0: 4, 1: 3}  # the reverse complement: the same keys backwards, two runs of one
    _, g, reads = _case("self-loop at a branch node")
    tot, una, links, counts, _ = ref.as_arrays(ref.thread_reads(g, reads[:1], 3), 2)
    assert tot == [3, 1] and una == [0, 0] and links == [[0, 0], [0, 1]] and counts == [2, 1]
    _, g, reads = _case("three parallel edges")
    tot, una, links, counts, _ = ref.as_arrays(ref.thread_reads(g, reads[:1], 3), 4)
    assert tot == [1, 1, 0, 0] and una == [0, 0, 0, 0] and links == [[0, 1]] and counts == [1]


# ---- the sweep covers what it is there for ---------------------------------------------------------------------------------

def test_sweep_coverage():
    assert len(tc.SWEEP_SEEDS) <= 40
    seen, ks = {}, set()
    for seed in tc.SWEEP_SEEDS:
        k, g, reads, read_index, mate = tc.random_case(seed)
        ks.add(k)
        assert max(len(r) for r in reads) <= 3 * 64
        ann = ref.thread_reads_paired(g, reads, read_index, mate, k)
        for name, n in ann.events.items():
            seen[name] = seen.get(name, 0) + n
        assert ref.thread_reads(g, reads, k).support_total == ann.support_total
    assert ks == {4, 5, 6, 7}
    for name in ("resolved_by_adjacency_not_first", "resolved_to_first", "ambiguous_run_3", "run_across_n",
                 "edge_twice_in_run", "pair_both_mapped"):
        assert seen.get(name, 0) > 0, (name, seen)


def test_tile_constant_matches_kernel():
    from sharkmer_amd.engine import THREAD_TILE
    src = open(os.path.join(ROOT, "sharkmer_amd", "csrc", "shk_device.hip.h")).read()
    assert int(re.search(r"constexpr uint32_t THREAD_TILE = (\d+);", src).group(1)) == THREAD_TILE
