"""The crafted graphs of prune_cases.py have, on the model (prune_ref.py), the property each was built for; and the
entry point the GPU tests call is declared, exported and bound.  No GPU is needed."""
import ctypes
import os
import re

import pytest

import prune_cases as pcs
import prune_ref as ref
import sharkmer_amd.engine as eng
from pcr_ref import median_via_select

K = pcs.K
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def kept(name):
    """(the case, its expected answer, the names of the named nodes that survive)"""
    c = pcs.case(name)
    want = c.expected()
    return c, want, {n for n, v in c.names.items() if want.node_keep[v]}


def main_path(c):
    return {n for n in c.names if n in ("start", "end") or re.fullmatch(r"m\d+", n)}


def test_symbol_is_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "shk.h")).read()
    assert re.search(r"\bint\s+shk_pcr_prune_panel\s*\(", header)
    assert re.search(r"#define\s+SHK_ABI_VERSION\s+2\b", header) and re.search(r"#define\s+SHK_N_KERNELS\s+16\b", header)
    assert "shk_pcr_prune_panel" in eng.ABI_SYMBOLS
    import __graft_entry__ as entry
    entry.build()
    lib = ctypes.CDLL(eng.lib_path())
    assert lib.shk_pcr_prune_panel is not None
    assert lib.shk_abi_version() == 2
    assert callable(eng.KmerEngine.pcr_prune_panel) and callable(eng.KmerEngine.pcr_prune)
    assert {"node_index", "edge_index", "coverage_ratio", "median", "tip_rounds", "tips_removed", "unreachable_removed"} <= set(
        eng.PrunedGraph.__dataclass_fields__)


def test_reference_graphs():
    """pruning.rs:242-341: the node counts its tests assert."""
    for name, n in (("ref median odd", 3), ("ref low tip forward", 4), ("ref high tip kept", 4), ("ref orphan", 3),
                    ("ref dead branch", 3), ("ref empty", 0)):
        c, want, names = kept(name)
        assert c.k == 3 and sum(want.node_keep) == n, name
    assert pcs.case("ref median odd").expected().median == 20.0
    assert "tip" not in kept("ref low tip forward")[2] and "tip" in kept("ref high tip kept")[2]
    assert "orphan" not in kept("ref orphan")[2] and "b" not in kept("ref dead branch")[2]
    assert (pcs.case("ref low tip forward").stages, pcs.case("ref orphan").stages) == (1, 2)


def test_tip_lengths():
    c, want, names = kept("tips of k-1")
    assert names == main_path(c) and want.tip_rounds >= K - 1 and want.tips_removed == 2 * (K - 1)
    c, want, names = kept("tips of k")
    assert len(names) == len(c.flags) and want.tip_rounds == 0


def test_thresholds():
    c, want, names = kept("threshold 11.85")
    med = median_via_select([e[2] for e in c.edges])
    assert len(c.edges) % 2 == 0 and med == 39.5 and med * c.fraction != int(med * c.fraction)
    assert "at ceil" in names and "below ceil" not in names
    assert {c.edges[e][2] for e in range(len(c.edges))} >= {11, 12}
    c, want, names = kept("fraction 0")
    assert "one" in names and "zero" not in names and "zero in" not in names
    c, want, names = kept("fraction 1e12")
    assert "max" not in names and "in max" not in names and {f"long{i}" for i in range(K)} <= names
    c, want, names = kept("no edges")
    assert names == {"start", "end", "both"} and want.tip_rounds == 1 and want.median == 0.0 and want.coverage_ratio == []


def test_synchronous_rounds():
    for name, stem in (("synchronous rounds", K - 2), ("synchronous rounds, stem k-1", K - 1)):
        c, want, names = kept(name)
        assert names == main_path(c), name
        assert want.tip_rounds >= 3 and want.tip_rounds == stem + 1 and want.tips_removed == stem + 2, name
    # one at a time instead: after d0 has gone, d1's walk takes the whole stem in — at a stem of k − 1 it is a tip of k
    c = pcs.case("synchronous rounds, stem k-1")
    g = ref.StableDiGraph(c.flags, *zip(*c.edges))
    assert ref.tip_length_backward(g, c.names["d1"]) == 1
    g.remove_node(c.names["d0"])
    assert ref.tip_length_backward(g, c.names["d1"]) == K


def test_small_shapes():
    c, want, names = kept("late dead end")
    g = ref.StableDiGraph(c.flags, *zip(*c.edges))
    assert g.neighbors_directed(c.names["x"], ref.OUTGOING) and g.neighbors_directed(c.names["x"], ref.INCOMING)
    assert "x" not in names and "y" not in names and want.tip_rounds == 2
    c, want, names = kept("start dead end")
    assert names == main_path(c) and want.tips_removed == 0 and want.unreachable_removed == 1
    c, want, names = kept("start and end")
    assert {"both", "both on path"} <= names and len(names) == len(c.flags)
    c, want, names = kept("parallel edges")
    assert names == main_path(c)
    g = ref.StableDiGraph(c.flags, *zip(*c.edges))
    assert len(g.neighbors_directed(c.names["p"], ref.OUTGOING)) == 2 and len(set(g.neighbors_directed(c.names["p"], ref.OUTGOING))) == 1
    assert ref.tip_length_backward(g, c.names["c4"]) == 3
    c, want, names = kept("self-loop")
    assert names == {"start", "m0", "end"} and want.tips_removed == 0 and want.unreachable_removed == 1
    assert (c.names["m0"], c.names["m0"], 7) in [(c.edges[e][0], c.edges[e][1], c.edges[e][2]) for e in want.edge_index]
    c, want, names = kept("cycle on the path")
    assert names == {"start", "m0", "m1", "m2", "end"} and len(want.edge_index) == 5
    c, want, names = kept("starts and ends")
    assert names == {"start", "m0", "m1", "end", "start 2", "end 2"} and want.tips_removed == 0 and want.unreachable_removed == 2


@pytest.mark.parametrize("m", [1023, 1024, 1025])
def test_width(m):
    c = pcs.case(f"width {m}")
    want = c.expected()
    assert len(c.flags) == 2 + m * (1 + K)
    assert want.tips_removed == 0 and want.unreachable_removed == m * K and sum(want.node_keep) == 2 + m
    assert want.edge_src == [0 if i % 2 == 0 else 2 + i // 2 for i in range(2 * m)]  # renumbered: start 0, end 1, the mids


def test_depth():
    c, want, names = kept("depth 3000")
    assert len(c.flags) == 3001 and sum(want.node_keep) == 3000 and "tip" not in names and want.tip_rounds == 1


def test_many_genes():
    genes = pcs.many_genes()
    assert len(genes) == 600 and sum(not g.flags for g in genes) > 80
    assert all(len(g.flags) in (0, 3) for g in genes)
    assert {sum(g.expected().node_keep) for g in genes} == {0, 2, 3}
    assert not genes[3].flags and genes[4].flags and not genes[10].flags


def test_model_is_consistent():
    """Every case: the compacted arrays are the survivors in ascending index, renumbered; ratios are count / median."""
    for c in pcs.cases() + pcs.many_genes()[:8]:
        w = c.expected()
        assert w.node_index == [v for v, kp in enumerate(w.node_keep) if kp], c.name
        assert w.edge_index == [i for i, e in enumerate(c.edges) if w.node_keep[e[0]] and w.node_keep[e[1]]], c.name
        assert [w.node_index[s] for s in w.edge_src] == [c.edges[i][0] for i in w.edge_index], c.name
        assert [w.node_index[t] for t in w.edge_tgt] == [c.edges[i][1] for i in w.edge_index], c.name
        assert w.tips_removed + w.unreachable_removed + sum(w.node_keep) == len(c.flags), c.name
        if w.edge_counts and w.median > 0:
            assert w.coverage_ratio == [x / w.median for x in w.edge_counts], c.name


def test_threaded_gene():
    t = pcs.threaded_gene()
    c, want = t.case, t.case.expected()
    g = ref.StableDiGraph(c.flags, *zip(*c.edges))
    assert len(c.flags) == 71 + 5 and len(c.edges) == 70 + 5 and len(set(t.sub_kmers.tolist())) == len(c.flags)
    assert len(t.tip) == 5 < c.k and len(g.neighbors_directed(t.branch, ref.OUTGOING)) == 2
    assert sorted(e[2] for e in c.edges) == [1] * 5 + [30] * 60 + [31] * 10
    assert [v for v, kp in enumerate(want.node_keep) if not kp] == sorted(t.tip) and want.tip_rounds == 5
    assert want.unreachable_removed == 0 and want.median == 30.0
