"""Crafted graphs for the shk_pcr_prune_panel tests, shared by the CPU test of the cases themselves
(test_prune_cases_cpu.py) and the GPU tests (test_gpu_pcr_prune_panel.py).  Every expected answer is prune_ref's, never
the library's; what each case is there for is asserted by test_prune_cases_cpu.py.  Each builder computes its case once."""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

import prune_ref as ref

K = 5
START, END = 1, 2
_cache = {}


class Case(NamedTuple):
    name: str
    k: int
    flags: list
    edges: list        # (src, tgt, count)
    fraction: float
    stages: int
    names: dict        # node name → index, for the assertions

    def arrays(self):
        """(node_sub_kmers, node_flags, edge_src, edge_tgt, edge_counts): a graph as pcr_prune_panel takes it.  A node's
        sub_kmer is its index + 1, so that what is carried through can be told apart."""
        return (np.arange(1, len(self.flags) + 1, dtype=np.uint64), np.array(self.flags, dtype=np.uint8),
                np.array([e[0] for e in self.edges], dtype=np.uint32), np.array([e[1] for e in self.edges], dtype=np.uint32),
                np.array([e[2] for e in self.edges], dtype=np.uint32))

    def expected(self) -> ref.Pruned:
        if self.name not in _cache:
            _cache[self.name] = ref.prune(self.flags, [e[0] for e in self.edges], [e[1] for e in self.edges],
                                          [e[2] for e in self.edges], self.k, self.fraction, self.stages)
        return _cache[self.name]


class Builder:
    def __init__(self):
        self.flags, self.edges, self.names = [], [], {}

    def node(self, name=None, flags=0):
        self.flags.append(flags)
        if name is not None:
            self.names[name] = len(self.flags) - 1
        return len(self.flags) - 1

    def edge(self, s, t, count):
        self.edges.append((s, t, count))

    def path(self, nodes, count):
        for a, b in zip(nodes, nodes[1:]):
            self.edge(a, b, count)

    def main(self, n_mid=12, count=100):
        """start → m0 → … → end: long enough by default that its count is the graph's median whatever hangs on it"""
        p = [self.node("start", START)] + [self.node(f"m{i}") for i in range(n_mid)] + [self.node("end", END)]
        self.path(p, count)
        return p

    def chain(self, prefix, n):
        return [self.node(f"{prefix}{i}") for i in range(n)]

    def case(self, name, k=K, fraction=0.1, stages=3):
        return Case(name, k, self.flags, self.edges, fraction, stages, self.names)


def _reference_cases():
    """The graphs of pruning.rs:242-341 (k = 3 there), each under the stage its test calls."""
    out = []
    b = Builder()  # test_global_median_edge_count_odd
    a, m, c = b.node("a", START), b.node("b"), b.node("c", END)
    b.edge(a, m, 10), b.edge(m, c, 20), b.edge(a, c, 30)
    out.append(b.case("ref median odd", k=3))
    b = Builder()  # test_remove_low_coverage_tip_forward
    s, a, m, e, tip = b.node("start", START), b.node("a"), b.node("b"), b.node("end", END), b.node("tip")
    b.edge(s, a, 100), b.edge(a, m, 100), b.edge(m, e, 100), b.edge(m, tip, 1)
    out.append(b.case("ref low tip forward", k=3, stages=1))
    b = Builder()  # test_preserve_high_coverage_tip
    s, a, e, tip = b.node("start", START), b.node("a"), b.node("end", END), b.node("tip")
    b.edge(s, a, 10), b.edge(a, e, 10), b.edge(a, tip, 10)
    out.append(b.case("ref high tip kept", k=3, stages=1))
    b = Builder()  # test_reachability_pruning_removes_orphan
    s, a, e = b.node("start", START), b.node("a"), b.node("end", END)
    b.node("orphan")
    b.edge(s, a, 10), b.edge(a, e, 10)
    out.append(b.case("ref orphan", k=3, stages=2))
    b = Builder()  # test_reachability_pruning_removes_dead_branch
    s, a, e, d = b.node("start", START), b.node("a"), b.node("end", END), b.node("b")
    b.edge(s, a, 10), b.edge(a, e, 10), b.edge(s, d, 10)
    out.append(b.case("ref dead branch", k=3, stages=2))
    out.append(Builder().case("ref empty", k=3, stages=2))  # test_reachability_pruning_empty_graph
    return out


def _tips(n_tip, name):
    """A forward tip hanging off m0 and a backward tip running into m1, n_tip nodes each, count 1 on a main path of 100."""
    b = Builder()
    p = b.main()
    f = b.chain("f", n_tip)
    b.path([p[1]] + f, 1)
    r = b.chain("r", n_tip)
    b.path(r + [p[2]], 1)
    return b.case(name, stages=1)


def _threshold():
    """Six edges whose median is 39.5; × 0.3 = 11.85: a one-node tip on an edge of 12 stays, one on an edge of 11 goes."""
    b = Builder()
    p = [b.node("start", START), b.node("a"), b.node("b"), b.node("c"), b.node("end", END)]
    for (s, t), c in zip(zip(p, p[1:]), (39, 40, 41, 42)):
        b.edge(s, t, c)
    b.edge(p[1], b.node("at ceil"), 12)
    b.edge(p[2], b.node("below ceil"), 11)
    return b.case("threshold 11.85", fraction=0.3, stages=1)


def _fraction_zero():
    """min_tip is 1.0: a tip on an edge of 1 stays, a tip on an edge of 0 goes; so does a backward tip of 0."""
    b = Builder()
    p = b.main(3)
    b.edge(p[1], b.node("one"), 1)
    b.edge(p[2], b.node("zero"), 0)
    b.edge(b.node("zero in"), p[3], 0)
    return b.case("fraction 0", fraction=0.0, stages=1)


def _fraction_huge():
    """min_tip is 1e14, above every u32: each short tip goes whatever its count; the tips of k nodes stay."""
    b = Builder()
    p = b.main(3)
    b.edge(p[1], b.node("max"), 0xFFFFFFFF)
    b.edge(b.node("in max"), p[2], 0xFFFFFFFF)
    b.path([p[3]] + b.chain("long", K), 0xFFFFFFFF)
    return b.case("fraction 1e12", fraction=1e12, stages=1)


def _no_edges():
    b = Builder()
    b.node("start", START), b.node("plain a"), b.node("end", END), b.node("plain b"), b.node("both", START | END)
    return b.case("no edges", stages=1)


def _synchronous(n_stem, name):
    """m0 → a stem of n_stem nodes → a fork into two one-node dead ends, all on count 1.  Both dead ends are judged on
    the round's graph (their parent has out-degree 2: length 1) and leave together; the stem then goes node by node.
    Judged one after the other, the second dead end would be walked back through the stem: 1 + n_stem nodes, which at
    n_stem = k − 1 is a tip of k nodes that stays for good (at k − 2 it is one node short of that)."""
    b = Builder()
    p = b.main()
    stem = b.chain("s", n_stem)
    b.path([p[1]] + stem, 1)
    b.edge(stem[-1], b.node("d0"), 1)
    b.edge(stem[-1], b.node("d1"), 1)
    return b.case(name, stages=1)


def _late_dead_end():
    """x is no dead end in the input; it becomes one when y has gone."""
    b = Builder()
    p = b.main(1)
    x, y = b.node("x"), b.node("y")
    b.path([p[1], x, y], 1)
    return b.case("late dead end", stages=1)


def _start_dead_end():
    """A start node nothing leaves: the tips keep it (it is a start), reachability removes it (it reaches no end)."""
    b = Builder()
    p = b.main()
    b.edge(p[1], b.node("start 2", START), 1)
    return b.case("start dead end")


def _start_and_end():
    b = Builder()
    b.main(1)
    b.node("both", START | END)
    both_on_path = b.node("both on path", START | END)
    b.edge(b.names["m0"], both_on_path, 100)
    b.edge(both_on_path, b.names["end"], 100)
    return b.case("start and end")


def _parallel():
    """Degrees count edges.  t hangs on two parallel edges (in-degree 2: its walk ends at once).  c4 ends a chain of k
    nodes whose c1 ⇒ c2 step is doubled: the walk back from c4 stops at c2 (two incoming edges) after 3 nodes, so the
    chain goes, end first; counted by distinct neighbours it would be a tip of k nodes and stay."""
    b = Builder()
    p = b.main()
    par, t = b.node("p"), b.node("t")
    b.edge(p[1], par, 1), b.edge(par, t, 1), b.edge(par, t, 1)
    c = b.chain("c", K)
    b.path([p[2]] + c[:2], 1)
    b.edge(c[1], c[2], 1), b.edge(c[1], c[2], 1)
    b.path(c[2:], 1)
    return b.case("parallel edges", stages=1)


def _self_loop():
    """A self-loop counts on both sides: on the path node it changes nothing; `looped` is no dead end because of its
    own loop, so the tips leave it and reachability takes it."""
    b = Builder()
    p = b.main(1)
    b.edge(p[1], p[1], 7)
    looped = b.node("looped")
    b.edge(p[1], looped, 1), b.edge(looped, looped, 1)
    return b.case("self-loop")


def _cycle():
    b = Builder()
    p = b.main(3)
    b.edge(p[3], p[1], 50)  # m2 → m0
    b.edge(p[2], b.node("tip"), 1)
    return b.case("cycle on the path")


def _many_ends():
    """Two starts, three ends: `end far` hangs on a well-covered node nothing reaches, so the tips keep both and
    reachability removes both."""
    b = Builder()
    p = b.main(2)
    b.edge(b.node("start 2", START), p[1], 80)
    b.edge(p[2], b.node("end 2", END), 90)
    b.edge(b.node("source"), b.node("end far", END), 100)
    return b.case("starts and ends")


def _width(m):
    """start → m mids → end, and off every mid a well-covered dead branch of k nodes: the tips keep the branches (k
    nodes, and counts at the median), reachability removes them — levels of m nodes on both searches."""
    b = Builder()
    s, e = b.node("start", START), b.node("end", END)
    for i in range(m):
        mid = b.node()
        b.edge(s, mid, 10), b.edge(mid, e, 10)
        b.path([mid] + [b.node() for _ in range(K)], 10)
    return b.case(f"width {m}")


def _depth():
    """3000 nodes from start to end, one low tip in the middle: as many levels as nodes."""
    b = Builder()
    p = b.main(2998, 20)
    b.edge(p[1500], b.node("tip"), 1)
    return b.case("depth 3000")


def cases() -> list:
    if "cases" not in _cache:
        _cache["cases"] = _reference_cases() + [
            _tips(K - 1, "tips of k-1"), _tips(K, "tips of k"), _threshold(), _fraction_zero(), _fraction_huge(), _no_edges(),
            _synchronous(K - 2, "synchronous rounds"), _synchronous(K - 1, "synchronous rounds, stem k-1"), _late_dead_end(),
            _start_dead_end(), _start_and_end(), _parallel(), _self_loop(), _cycle(), _many_ends(), _width(1023), _width(1024),
            _width(1025), _depth()]
    return _cache["cases"]


def case(name) -> Case:
    (c,) = [c for c in cases() if c.name == name]
    return c


THREAD_K = 11


class ThreadedGene(NamedTuple):
    case: Case
    sub_kmers: np.ndarray   # the nodes' (k-1)-mers, 2 bits a base, A C G T = 0 1 2 3
    reads: list             # bytes
    branch: int             # the node where the tip leaves the path
    tip: list               # its nodes


def threaded_gene() -> ThreadedGene:
    """A gene with reads, for the hand-over to shk_thread_reads_panel: the de Bruijn graph at k = 11 of thirty copies of an
    80-base sequence and one read that follows it up to a substitution and ends four bases later — a tip of five nodes
    on count 1 off a path on count 30.  Unpruned, the node before the tip is a branch and every read through it leaves
    a branch link; pruned, it is a plain path node and no read leaves any."""
    if "threaded" in _cache:
        return _cache["threaded"]
    import random
    k = THREAD_K
    rng = random.Random(k)
    seq = "".join(rng.choice("ACGT") for _ in range(80))
    pos = 40
    variant = seq[20:pos] + "ACGT"[("ACGT".index(seq[pos]) + 1) % 4] + seq[pos + 1:pos + 5]
    reads = [seq.encode()] * 30 + [variant.encode()]
    code = lambda s: int("".join(format("ACGT".index(c), "02b") for c in s), 2)
    b = Builder()
    node_of, subs, edge_of = {}, [], {}
    for r in reads:
        r = r.decode()
        for i in range(len(r) - k + 1):
            ends = []
            for sub in (r[i:i + k - 1], r[i + 1:i + k]):
                if sub not in node_of:
                    node_of[sub] = b.node(sub, (START if sub == seq[:k - 1] else 0) | (END if sub == seq[-(k - 1):] else 0))
                    subs.append(code(sub))
                ends.append(node_of[sub])
            if r[i:i + k] not in edge_of:
                edge_of[r[i:i + k]] = len(b.edges)
                b.edges.append((ends[0], ends[1], 0))
            e = edge_of[r[i:i + k]]
            b.edges[e] = (ends[0], ends[1], b.edges[e][2] + 1)
    tip = [v for sub, v in node_of.items() if sub not in seq]
    (branch,) = [s for s, t, _ in b.edges if t in tip and s not in tip]
    _cache["threaded"] = ThreadedGene(b.case("threaded gene", k=k), np.array(subs, dtype=np.uint64), reads, branch, tip)
    return _cache["threaded"]


MANY_GENES = 600


def many_genes() -> list:
    """600 genes of three nodes — more than the card holds workgroups — in four shapes by turns, every seventh one empty."""
    if "many" in _cache:
        return _cache["many"]
    out = []
    for i in range(MANY_GENES):
        b = Builder()
        if i % 7 != 3:
            s, a, e = b.node("start", START), b.node("a"), b.node("end", END)
            shape = i % 4
            if shape == 0:
                b.edge(s, a, 5 + i), b.edge(a, e, 5 + i)        # a path: all stay
            elif shape == 1:
                b.edge(s, e, 100 + i), b.edge(s, a, 1)           # a low tip
            elif shape == 2:
                b.edge(s, a, 9)                                  # the end is never reached: nothing stays
            else:
                b.edge(s, e, 3), b.edge(s, e, 4 + i), b.edge(a, e, 50)  # parallel edges; a well-covered source nothing reaches
        out.append(b.case(f"gene {i}"))
    _cache["many"] = out
    return out
