"""CPU tests of the panel read-threading cases (thread_panel_cases.py): from the model alone, that every crafted panel
holds what it is named for — so that the GPU tests (test_gpu_thread_panel.py) compare against answers that exercise what
they claim to — and that the library exports the two entry points."""
import ctypes

import thread_cases as tc
import thread_panel_cases as tp


def test_library_exports_the_panel_entry_points():
    from sharkmer_amd.engine import ABI_SYMBOLS, lib_path
    lib = ctypes.CDLL(lib_path())
    for name in ("shk_thread_reads_panel", "shk_thread_reads_panel_device"):
        assert name in ABI_SYMBOLS
        assert getattr(lib, name) is not None
    assert lib.shk_abi_version() == 2  # the new symbols are additive


def test_crafted_panel_is_thread_cases_gene_by_gene():
    p = tp.crafted_panel()
    cases = tc.crafted_cases()
    assert len(p.graphs) == len(cases) and sum(len(x) for x in p.lists) == len(p.reads) == sum(len(c[2]) for c in cases)
    for (name, g, reads), graph, ids in zip(cases, p.graphs, p.lists):
        assert graph == g and [p.reads[i] for i in ids] == reads, name
    r = tp.reverse(p)
    assert r.graphs == p.graphs[::-1] and r.lists == p.lists[::-1] and r.reads == p.reads
    want = tp.expected(p)
    assert [tp.rows(a, len(g.edges)) for a, g in zip(tp.expected(r), r.graphs)] == [tp.rows(a, len(g.edges)) for a, g in zip(want, p.graphs)][::-1]
    # the "wrong candidate in front" read resolves by adjacency, past candidate 0
    assert want[tp.crafted_gene("the second adjacent")].events.get("resolved_by_adjacency_not_first", 0) >= 1
    # the panel meets a run across an N, an invalid byte, a branch link and a gene without edges that lists reads
    assert want[tp.crafted_gene("a run across an N")].events.get("run_across_n", 0) >= 1
    assert 0 in want[tp.crafted_gene("an invalid byte")].read_edges
    assert want[tp.crafted_gene("a link recorded per crossing")].branch_links
    assert not p.graphs[tp.crafted_gene("nodes without edges")].edges and p.lists[tp.crafted_gene("nodes without edges")]


def test_twins_get_different_supports():
    for swap in (False, True):
        p = tp.twin_panel(swap)
        assert p.graphs[0].edges == p.graphs[1].edges and p.graphs[0].sub_kmer == p.graphs[1].sub_kmer
        assert not set(p.lists[0]) & set(p.lists[1])
        a, b = tp.expected(p)
        if swap:
            a, b = b, a
        assert a.support_total == {0: 1, 1: 2} and b.support_total == {0: 2}  # edge 1: the first twin's alone


def test_shared_read_maps_in_each_gene():
    p = tp.shared_read_panel()
    (shared,) = set(p.lists[0]) & set(p.lists[1]) & set(p.lists[2])
    for ann, ids in zip(tp.expected(p), p.lists):
        assert all(ann.read_edges[j] >= 2 for j, i in enumerate(ids) if i == shared)
    assert p.lists[2].count(shared) == 2  # and twice in one list: it counts twice
    assert tp.expected(p)[2].support_total[0] == 3


def test_lists_panel_holds_its_shapes():
    p = tp.lists_panel()
    want = tp.expected(p)
    assert p.lists[1] == [] and p.lists[0] and p.lists[2] and not want[1].support_total
    assert not p.graphs[3].edges and p.lists[3] and want[3].read_edges == [0, 0, 0]
    assert sum(0 in ids for ids in p.lists) >= 3                   # read 0 is in three genes and more
    assert p.lists[2].count(3) == 2 and want[2].support_total[0] == 3
    assert p.lists[4] == sorted(p.lists[4], reverse=True) and len(p.lists[4]) == 7  # descending; slices of 3, 3, 1
    assert want[4].read_edges == [2, 0, 2, 2, 2, 1, 2]           # per list position, in that order: not its own reverse
    assert len(p.lists[5]) == 1


def test_paired_panel():
    p = tp.paired_panel()
    a, b = tp.expected(p)
    assert (a.n_paired_links, b.n_paired_links) == (1, 0)
    assert b.read_edges[0] > 0  # gene B's R1 of the pair does map: what is missing is its mate
    unpaired = tp.expected(p._replace(read_index=None, mate=None))
    assert [x.n_paired_links for x in unpaired] == [0, 0]


def test_many_panel():
    p = tp.many_panel()
    want = tp.expected(p)
    assert len(p.graphs) == tp.MANY_GENES
    for g, ann in enumerate(want):
        assert bool(ann.support_total) == (g != tp.MANY_EMPTY), g


def test_sweep_groups_cover_the_seeds():
    groups = tp.sweep_groups()
    used = [s for g in groups for s in g]
    assert len(used) == len(set(used))
    assert len(set(tc.SWEEP_SEEDS) - set(used)) <= len(tc.SWEEP_SEEDS) // 4  # at most a quarter left out (none is)
    assert len(used) == 40 and len(groups) == 12
    for seeds in groups:
        assert 2 <= len(seeds) <= 6 and len({tc.random_case(s)[0] for s in seeds}) == 1
    p = tp.sweep_panel(groups[0])
    assert any(set(a) & set(b) for i, a in enumerate(p.lists) for b in p.lists[i + 1:])  # lists overlap
    assert any(len(set(x)) < len(x) for x in p.lists)                                    # and repeat
