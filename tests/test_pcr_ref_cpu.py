"""CPU checks of sPCR's graph extension: tests/pcr_ref.py — the model the GPU tests compare shk_neighborhood and
shk_pcr_extend against — pinned to the reference's own known answers (src/pcr/graph.rs:653-745, src/pcr/mod.rs:422-425
and 1331-1371, src/pcr/threading.rs:371-410), and the ABI of the new entry points.  No GPU."""
import os
import re

import numpy as np
import pytest

import nb_cases
import pcr_ref as ref
import primer_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def sa():
    import __graft_entry__ as g
    g.build()
    import sharkmer_amd
    return sharkmer_amd


def test_symbols_exported_declared_and_bound(sa):
    import ctypes
    from sharkmer_amd.engine import ABI_SYMBOLS, KERNEL_NAMES, lib_path
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "shk.h")).read(), flags=re.S)
    L = ctypes.CDLL(lib_path())
    for name in ("shk_neighborhood", "shk_pcr_extend", "shk_pcr_node_budget"):
        assert name in ABI_SYMBOLS
        assert re.search(rf"\b{name}\s*\(", hdr)
        assert hasattr(L, name)
    assert "typedef struct shk_pcr_extend_params" in hdr and re.search(r"SHK_K_EXTEND = 15\b", hdr)
    assert "#define SHK_ABI_VERSION 2" in hdr and "#define SHK_N_KERNELS 16" in hdr
    assert KERNEL_NAMES[15] == "extend" and len(KERNEL_NAMES) == 16
    assert hasattr(sa.KmerEngine, "neighborhood") and hasattr(sa.KmerEngine, "pcr_extend")
    from sharkmer_amd.engine import _PcrExtendParams
    assert ctypes.sizeof(_PcrExtendParams) == 32  # two u32, f64, u64, two u32


def test_node_budget(sa):
    """graph.rs:653-675, and the library's shk_pcr_node_budget (host only) against the model."""
    assert ref.compute_node_budget(0) == 100_000
    assert ref.compute_node_budget(150_000_000) == 100_000
    assert ref.compute_node_budget(750_000_000) == 500_000
    assert ref.compute_node_budget(2**64 - 1) == 500_000
    mid = (150_000_000 + 750_000_000) // 2
    assert 100_000 < ref.compute_node_budget(mid) < 500_000
    assert ref.compute_node_budget(mid) == 300_000
    for n in (0, 1, 150_000_000, 150_000_001, 299_999_999, mid, 449_123_457, 749_999_999, 750_000_000, 2**64 - 1):
        assert sa.pcr_node_budget(n) == ref.compute_node_budget(n), n


def test_median_cases():
    """graph.rs:686-745."""
    assert ref.median_via_select([]) is None
    assert ref.median_via_select([42]) == 42.0
    assert ref.median_via_select([9, 1, 5]) == 5.0
    assert ref.median_via_select([11, 1, 9, 5]) == 7.0
    assert ref.median_via_select([7, 3]) == 5.0
    assert ref.median_via_select([5, 15, 10]) == 10.0
    large, huge = 2**32 - 2, 2**32 - 1
    assert abs(ref.median_via_select([large, huge]) - (float(large) + float(huge)) / 2.0) < 1.0


def test_coverage_thresholds():
    """mod.rs:403-428: the dedup example of mod.rs:422-425 ([4, 4, 4, 2] → [4, 2]) and the other branches."""
    assert ref.compute_coverage_thresholds(8, 2) == [4, 2]       # step (4 − 2) / 3 = 0
    assert ref.compute_coverage_thresholds(10, 5) == [5]         # high ≤ min_count
    assert ref.compute_coverage_thresholds(3, 2) == [2]
    assert ref.compute_coverage_thresholds(0, 2) == [2]          # an empty primer set: get_max_count = 0
    assert ref.compute_coverage_thresholds(100, 2) == [50, 34, 18, 2]
    assert ref.compute_coverage_thresholds(40, 3) == [20, 15, 10, 3]


def test_18s_integration_case(orc):
    """test_integration (mod.rs:1331-1371): the padded 18S ×10 at k 21 — one forward and one reverse primer k-mer, a
    seed graph of 2 nodes (1 start, 1 end), and the extension at min_count 5 with the default budget meets."""
    seq = open(os.path.join(G, "pcr_18s_padded.txt")).read().strip()
    k, copies = 21, 10
    bases = np.frombuffer(seq.encode() * copies, dtype=np.uint8).copy()
    offsets = np.arange(copies + 1, dtype=np.uint64) * np.uint64(len(seq))
    run = orc.run_batch(bases, offsets, k, 1, 100)  # (kept alive while its merged table is read)
    keys, counts = run.merged().export()
    assert len(keys) == len(seq) - k + 1 and int(counts.sum()) == (len(seq) - k + 1) * copies
    fwd = primer_ref.get_primer_kmers("AACCTGGTTGATCCTGCCAGT", keys, counts, k, 15, 2, 3)
    rev = primer_ref.get_primer_kmers("TGATCCTTCTGCAGGTTCACCTAC", keys, counts, k, 15, 2, 3)
    assert len(fwd[0]) == 1 and len(rev[0]) == 1
    seed = ref.create_seed_graph(fwd[0], rev[0], k)
    assert len(seed.sub_kmer) == 2 and sum(seed.is_start) == 1 and sum(seed.is_end) == 1
    table = ref.table_dict(keys, counts)
    g = ref.extend_graph(seed, table, k, 5, 1, 10.0, ref.DEFAULT_MAX_NUM_NODES)
    assert g.found_path
    assert len(g.sub_kmer) > 1700 and not g.budget_break
    # every edge's k-mer is in the table with the edge's count
    for i, (_, _, c) in enumerate(g.edges):
        assert ref.canonical_count(table, g.edge_kmer(i), k) == c == 10
    # the same through the sweep entry: thresholds of min(10, 10) / 2 = 5 down to 3; the first step already meets
    g2, used, steps = ref.pcr_extend(fwd[:2], rev[:2], table, k, min_count=3, table_min_count=1, sweep=True,
                                     max_num_nodes=ref.DEFAULT_MAX_NUM_NODES)
    assert (used, steps, g2.found_path) == (5, 1, True) and g2.edges == g.edges and g2.sub_kmer == g.sub_kmer
    # the neighbourhood of the two seeds holds every k-mer the extension used
    ks, cs, fn, fd, L = ref.neighborhood(seed.sub_kmer, [1, 2], table, k, 5)
    assert not fn and L > 1700
    assert {min(g.edge_kmer(i), ref.revcomp(g.edge_kmer(i), k)) for i in range(len(g.edges))} <= set(ks)


def test_edge_kmer_reconstruction():
    """make_test_graph (threading.rs:371-410): AA → AC → CG with the edge k-mers AAC and ACG."""
    g = ref.Graph([0b0000, 0b0001, 0b0110], [True, False, False], [False, False, True], [(0, 1, 10), (1, 2, 8)])
    assert g.edge_kmer(0) == 0b000001 and g.edge_kmer(1) == 0b000110
    assert g.flags() == [1, 0, 2]
    # the same graph grown by the model from a table that holds AAC ×10 and ACG ×8 (canonical: both are their own minimum)
    table = {0b000001: 10, 0b000110: 8}
    for x in table:
        assert x <= ref.revcomp(x, 3)
    got = ref.extend_graph(ref.Graph([0b0000], [True], [False]), table, 3, 1, 1, 10.0, 100)
    # … and on along the other strand, since the table is canonical: CGT = revcomp(ACG), GTT = revcomp(AAC)
    assert got.sub_kmer == [0b0000, 0b0001, 0b0110, 0b1011, 0b1111]
    assert got.edges == [(0, 1, 10), (1, 2, 8), (2, 3, 8), (3, 4, 10)]
    assert [got.edge_kmer(i) for i in range(2)] == [0b000001, 0b000110] and not got.found_path


def test_neighborhood_whole_level_rule():
    """The truncation rule on a table small enough to follow by hand (k = 3): levels AA → AC → CG → GT → TT (the last
    two over the reverse complements of ACG and AAC, which add no k-mer)."""
    table = {0b000001: 10, 0b000110: 8}
    lv = ref.neighborhood_levels([0], [1], table, 3, 1)
    assert [e for e, _ in lv] == [[(0, 1)], [(1, 1)], [(0b0110, 1)], [(0b1011, 1)], [(0b1111, 1)]]
    assert [sorted(nk) for _, nk in lv] == [[1], [6], [], [], []]
    assert ref.neighborhood([0], [1], table, 3, 1) == ([1, 6], [10, 8], [], [], 5)
    assert ref.neighborhood([0], [1], table, 3, 1, max_levels=3) == ([1, 6], [10, 8], [0b1011], [1], 3)
    assert ref.neighborhood([0], [1], table, 3, 1, fringe_cap=1)[4] == 5
    assert ref.neighborhood([0], [1], table, 3, 1, max_levels=1) == ([1], [10], [1], [1], 1)
    assert ref.neighborhood([0], [1], table, 3, 1, cap=1) == ([1], [10], [1], [1], 1)
    assert ref.neighborhood([0], [1], table, 3, 1, cap=0) == ([], [], [0], [1], 0)
    assert ref.neighborhood([0], [1], table, 3, 9) == ([1], [10], [], [], 2)
    assert ref.neighborhood([0b1111], [2], table, 3, 1) == ([1, 6], [10, 8], [], [], 5)  # TT backwards: the same k-mers
    with pytest.raises(ValueError):
        ref.neighborhood([0, 1], [1, 1], table, 3, 1, fringe_cap=1)


# ---- the crafted tables of tests/nb_cases.py ----------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(nb_cases.CASES))
def test_crafted_cases_have_their_designed_level_sizes(name):
    """Each builder's table, walked by the model alone, has exactly the level sizes it was designed to have (chains
    that met by chance would change them: the builders' generator seed is the first at which this passes) — so the
    GPU comparison on the same table (tests/test_gpu_nb_edges.py) is one at that shape.  Canonical keys only."""
    case = nb_cases.CASES[name]()
    table = nb_cases.merged_table(case.inserts)
    assert all(x <= ref.revcomp(x, case.k) for x in table) and len(case.seeds) == len(case.dirs)
    assert all(0 <= lane < max(case.chunks, 1) and len(ks) == len(cs) for lane, ks, cs in case.inserts)
    lv = ref.neighborhood_levels(case.seeds, case.dirs, table, case.k, case.min_count)
    assert [len(e) for e, _ in lv] == case.sizes, name
    if case.hand_over:  # the level where the search changes kernels: the first past the narrow kernel's size, or back
        a, b = case.sizes[case.hand_over - 1], case.sizes[case.hand_over]
        assert (a > nb_cases.NARROW) != (b > nb_cases.NARROW)


def test_crafted_lane_counts_meet_their_thresholds_only_summed():
    """The lanes table: no single lane's count of a chain-A key reaches the threshold, the sum is exactly it, chain B's
    is one short; two keys saturate over lanes, one is 2^32 − 2, one was inserted with count 0 and nothing else."""
    case = nb_cases.lanes()[0]
    table = nb_cases.merged_table(case.inserts)
    per_lane = [dict(zip(ks, cs)) for _, ks, cs in case.inserts]
    hist = sorted(table.values())
    assert hist.count(nb_cases.LANES_MIN) == 5 and hist.count(nb_cases.LANES_MIN - 1) == 5
    for x, c in table.items():
        if c in (nb_cases.LANES_MIN, nb_cases.LANES_MIN - 1):
            assert max(l.get(x, 0) for l in per_lane) < nb_cases.LANES_MIN and sum(l.get(x, 0) for l in per_lane) == c
    assert hist.count(nb_cases.U32_MAX) == 2 and hist.count(nb_cases.U32_MAX - 1) == 1 and hist.count(0) == 1
    for x, c in table.items():
        if c == nb_cases.U32_MAX:
            assert sum(l.get(x, 0) for l in per_lane) > nb_cases.U32_MAX > max(l.get(x, 0) for l in per_lane)


def test_growth_inserts_are_out_of_every_canonical_lookup_s_reach():
    lane, keys, counts = nb_cases.growth_inserts()
    assert len(keys) == len(counts) == 300_000 and lane == 0
    assert all(x > ref.revcomp(x, 7) for x in set(keys))
