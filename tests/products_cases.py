"""Crafted genes for the last stage of sPCR (shk_pcr_paths_panel, shk_pcr_products_panel): the reference's own eleven
unit-test graphs (pcr/bubble.rs:277-517, pcr/paths.rs:429-615) and one case per rule of resolve_bubbles, the budgeted
search and the score that a wrong reading would get wrong.  A case is arrays in the layout shk_pcr_prune_panel and
shk_thread_reads_panel hand out, the gene's parameters, and nothing else; the expected answers come from
products_ref.run_gene."""
from __future__ import annotations

import random
from typing import NamedTuple

import numpy as np

from products_ref import Annotations, Params

START, END = 1, 2


class Case(NamedTuple):
    name: str
    k: int
    sub: np.ndarray
    flags: np.ndarray
    es: np.ndarray
    et: np.ndarray
    ec: np.ndarray
    ratio: np.ndarray
    ann: Annotations | None
    params: Params

    def graph(self):
        return (self.sub, self.flags, self.es, self.et, self.ec, self.ratio)


class Builder:
    def __init__(self, k=9):
        self.k, self.subs, self.flags, self.edges, self.links = k, [], [], [], {}

    def node(self, flags=0, sub=None):
        self.subs.append(len(self.subs) if sub is None else sub)
        self.flags.append(flags)
        return len(self.subs) - 1

    def edge(self, s, t, count=10, ratio=1.0, total=0, unamb=0):
        self.edges.append((s, t, count, ratio, total, unamb))
        return len(self.edges) - 1

    def chain(self, s, t, n_inner, **kw):
        """s → n_inner new nodes → t; the edges."""
        out, prev = [], s
        for _ in range(n_inner):
            v = self.node()
            out.append(self.edge(prev, v, **kw))
            prev = v
        out.append(self.edge(prev, t, **kw))
        return out

    def link(self, incoming, outgoing, count):
        self.links[(incoming, outgoing)] = count

    def case(self, name, threaded=True, **params) -> Case:
        col = lambda i, dt: np.array([e[i] for e in self.edges], dtype=dt)
        ann = Annotations([e[4] for e in self.edges], [e[5] for e in self.edges], dict(self.links)) if threaded else None
        return Case(name, self.k, np.array(self.subs, dtype=np.uint64), np.array(self.flags, dtype=np.uint8), col(0, np.uint32),
                    col(1, np.uint32), col(2, np.uint32), col(3, np.float64), ann, Params(**params))


# ---- the reference's unit tests ----

def make_bubble_graph(supports=(0, 0, 0, 0), unamb=(0, 0, 0, 0)) -> Builder:
    """bubble.rs:281-341: n0 -e0-> n1 -e2-> n3, n0 -e1-> n2 -e3-> n3."""
    b = Builder(k=3)
    n = [b.node(START), b.node(), b.node(), b.node(END)]
    for (s, t, c), sup, un in zip(((0, 1, 5), (0, 2, 3), (1, 3, 5), (2, 3, 3)), supports, unamb):
        b.edge(n[s], n[t], c, total=sup, unamb=un)
    return b


def depth_limited() -> Builder:
    """bubble.rs:435-474: two chains of 60 nodes from one source."""
    b = Builder(k=7)
    source = b.node(START, sub=0)
    for base in (1000, 2000):
        prev = source
        for i in range(60):
            v = b.node(sub=base + i + 1)
            b.edge(prev, v, 5)
            prev = v
    return b


def linear(n_inner, k=3, count=10) -> Builder:
    b = Builder(k=k)
    s = b.node(START)
    inner = [b.node() for _ in range(n_inner)]
    e = b.node(END)
    for x, y in zip([s] + inner, inner + [e]):
        b.edge(x, y, count)
    return b


def paths_diamond() -> Builder:
    b = Builder(k=3)
    s, a, c, e = b.node(START), b.node(), b.node(), b.node(END)
    b.edge(s, a, 10), b.edge(s, c, 5), b.edge(a, e, 10), b.edge(c, e, 5)
    return b


def sorted_children_graph() -> Builder:
    b = Builder(k=3)
    s, lo, hi = b.node(START), b.node(), b.node()
    b.edge(s, lo, 1), b.edge(s, hi, 100)
    return b


def reference_cases() -> list:
    return [
        make_bubble_graph().case("bubble.rs diamond"),
        make_bubble_graph((10, 2, 10, 2), (8, 1, 8, 1)).case("bubble.rs read support"),
        linear(0).case("bubble.rs linear"),
        depth_limited().case("bubble.rs depth-limited chains"),
        make_bubble_graph((10, 10, 10, 10), (5, 5, 5, 5)).case("bubble.rs tie"),
        linear(2).case("paths.rs linear", threaded=False, min_length=0, max_length=100),
        paths_diamond().case("paths.rs diamond", threaded=False, min_length=0, max_length=100),
        Builder(k=3).case("paths.rs no start nodes", threaded=False, min_length=0, max_length=100),
        linear(3).case("paths.rs max length", threaded=False, min_length=0, max_length=5),
        linear(1).case("paths.rs budget 0", threaded=False, min_length=0, max_length=100, max_dfs_states=0),
        sorted_children_graph().case("paths.rs sorted_children", threaded=False),
    ]


# ---- bubbles ----

def _bubble(b: Builder, s, t, inner=(1, 1), counts=(10, 10), totals=(0, 0)):
    return [b.chain(s, t, n, count=c, total=tt, unamb=tt) for n, c, tt in zip(inner, counts, totals)]


def bubble_cases() -> list:
    out = []
    # a shared tail after the reconvergence: both branches run on through c → d to the branching d
    b = Builder()
    s, a, a2, c, d, x, y = b.node(START), b.node(), b.node(), b.node(), b.node(), b.node(END), b.node(END)
    b.edge(s, a, 4, total=9), b.edge(s, a2, 6, total=2), b.edge(a, c, 4, total=9), b.edge(a2, c, 6, total=2)
    b.edge(c, d, 10, total=7), b.edge(d, x, 5), b.edge(d, y, 5)
    out.append(b.case("shared tail", dedup_edit_threshold=0))
    # one chain edge inside branches of two sources: c → t belongs to s1's branch over a and to s2's branch; s2 is later
    b = Builder()
    s1, a, bb, c, s2, b2, t = b.node(START), b.node(), b.node(), b.node(), b.node(START), b.node(), b.node(END)
    b.edge(s1, a, 5, total=8), b.edge(s1, bb, 5, total=2), b.edge(a, c, 5, total=8), b.edge(bb, t, 5, total=2)
    b.edge(c, t, 5, total=1), b.edge(s2, c, 5, total=1), b.edge(s2, b2, 5, total=6), b.edge(b2, t, 5, total=6)
    out.append(b.case("edge in two sources", dedup_edit_threshold=0))
    # a branch that cycles back, beside a real bubble
    b = Builder()
    s, a, a2, p, q, t = b.node(START), b.node(), b.node(), b.node(), b.node(), b.node(END)
    b.edge(s, a, 9, total=50), b.edge(a, a2, 9, total=50), b.edge(a2, a, 9, total=50)
    b.edge(s, p, 8, total=1), b.edge(p, t, 8, total=1), b.edge(s, q, 7, total=5), b.edge(q, t, 7, total=5)
    out.append(b.case("cycling branch", dedup_edit_threshold=0))
    # the sink a dead end
    b = Builder()
    s, t = b.node(START), b.node(END)
    _bubble(b, s, t, counts=(3, 9), totals=(6, 1))
    out.append(b.case("dead-end sink", dedup_edit_threshold=0))
    # parallel edges s ⇉ a
    b = Builder()
    s, a, t = b.node(START), b.node(), b.node(END)
    b.edge(s, a, 3, total=1), b.edge(s, a, 9, total=4), b.edge(a, t, 5, total=5), b.edge(a, t, 6, total=0)
    out.append(b.case("parallel edges", dedup_edit_threshold=0))
    # phasing links that reverse what the support alone says
    b = Builder()
    p, s, t = b.node(START), b.node(), b.node(END)
    pe = b.edge(p, s, 10, total=9)
    br = _bubble(b, s, t, counts=(10, 10), totals=(5, 4))
    b.link(pe, br[1][0], 10)
    b.link(pe, br[0][0], 1)
    out.append(b.case("phasing reverses", dedup_edit_threshold=0))
    # all supports zero
    b = Builder()
    s, t = b.node(START), b.node(END)
    _bubble(b, s, t, counts=(2, 7))
    out.append(b.case("zero supports", dedup_edit_threshold=0))
    # u32 sums that wrap
    b = Builder()
    s, t = b.node(START), b.node(END)
    _bubble(b, s, t, inner=(2, 1), counts=(5, 5), totals=(0x60000000, 7))
    out.append(b.case("wrapping sums", dedup_edit_threshold=0))
    # branches of exactly 50 steps (49 inner nodes: the sink is looked at in step 50) and of 51
    for inner in (49, 50):
        b = Builder()
        s, t = b.node(START), b.node(END)
        _bubble(b, s, t, inner=(inner, inner), counts=(9, 3), totals=(1, 2))
        out.append(b.case(f"branches of {inner + 1} steps", dedup_edit_threshold=0))
    return out


# ---- the search ----

def ladder(rungs=5, starts=2) -> Builder:
    """2^rungs paths from each start: between consecutive posts two routes of one inner node each."""
    b = Builder()
    ss = [b.node(START) for _ in range(starts)]
    post = b.node()
    for s in ss:
        b.edge(s, post, 10)
    for r in range(rungs):
        nxt = b.node(END if r == rungs - 1 else 0)
        b.chain(post, nxt, 1, count=10 + r)
        b.chain(post, nxt, 1, count=20 - r)
        post = nxt
    return b


def search_cases() -> list:
    out = []
    b = Builder()
    s, a, c, e = b.node(START), b.node(), b.node(), b.node(END)
    b.edge(s, a, 5), b.edge(s, c, 5), b.edge(a, e, 5), b.edge(c, e, 5)
    out.append(b.case("equal counts", threaded=False, dedup_edit_threshold=0))
    for visits in (1, 2, 3):
        b = Builder()
        s, a, c, e = b.node(START), b.node(), b.node(), b.node(END)
        b.edge(s, a, 9), b.edge(a, c, 9), b.edge(c, a, 8), b.edge(c, e, 3), b.edge(a, a, 2)
        out.append(b.case(f"cycle, {visits} visits", threaded=False, max_node_visits=visits, dedup_edit_threshold=0))
    b = Builder()
    s, e1, x, e2 = b.node(START), b.node(END), b.node(), b.node(END)
    b.edge(s, e1, 5), b.edge(e1, x, 5), b.edge(x, e2, 5)
    out.append(b.case("end before min_path_nodes", threaded=False, min_length=b.k + 1, dedup_edit_threshold=0))
    b = Builder()
    s, a, e = b.node(START | END), b.node(), b.node(END)
    b.edge(s, a, 5), b.edge(a, s, 4), b.edge(a, e, 3)
    out.append(b.case("start is an end", threaded=False, dedup_edit_threshold=0))
    b = Builder()
    s, e, a, e2 = b.node(START), b.node(END), b.node(), b.node(END)
    b.edge(s, e, 5), b.edge(s, a, 6), b.edge(a, e2, 6)
    out.append(b.case("max_length <= k", threaded=False, max_length=b.k, dedup_edit_threshold=0))
    for ml in (9, 10, 11):  # k, k + 1, k + 2 at k = 9
        out.append(linear(1, k=9).case(f"min_length {ml}", threaded=False, min_length=ml))
    out.append(ladder().case("ladder cut at 20", threaded=False, dedup_edit_threshold=0))
    out.append(ladder().case("ladder, 37 states", threaded=False, max_dfs_states=37, dedup_edit_threshold=1))
    out.append(ladder(3, 1).case("ladder, 3 paths", threaded=False, max_paths_per_pair=3, dedup_edit_threshold=2))
    return out


# ---- the score ----

def score_cases() -> list:
    out = []
    for threaded in (False, True):
        tag = "threaded" if threaded else "plain"
        b = Builder()
        s, a, c, e = b.node(START), b.node(), b.node(), b.node(END)
        b.edge(s, a, 1, total=3, unamb=2), b.edge(a, c, 1, total=3, unamb=1), b.edge(c, e, 100, total=2, unamb=2)
        out.append(b.case(f"cv above 1, {tag}", threaded=threaded))
        b = Builder()
        s, a, e = b.node(START), b.node(), b.node(END)
        b.edge(s, a, 10, ratio=7.5, total=1, unamb=1), b.edge(a, e, 11, ratio=0.25, total=4, unamb=3)
        out.append(b.case(f"coverage ratio above 5, {tag}", threaded=threaded))
        for zeros in (0, 1, 12):
            b = Builder()
            s, e = b.node(START), b.node(END)
            prev = s
            for i in range(14):
                v = e if i == 13 else b.node()
                b.edge(prev, v, 7 + i % 3, total=0 if i < zeros else 5, unamb=i)
                prev = v
            out.append(b.case(f"{zeros} zero-support edges, {tag}", threaded=threaded))
    return out


def cases() -> list:
    return reference_cases() + bubble_cases() + search_cases() + score_cases()


def random_case(rng: random.Random, name="random") -> Case:
    """A small arbitrary graph: <= 12 nodes, <= 24 edges, parallel edges and self-loops allowed, random flags, supports,
    links and small budgets."""
    k = rng.choice((2, 3, 5, 11, 31))
    n = rng.randint(0, 12)
    mask = (1 << (2 * (k - 1))) - 1
    b = Builder(k=k)
    for _ in range(n):
        b.node(rng.choice((0, 0, 0, START, END, START | END)), sub=rng.randint(0, mask))
    ne = rng.randint(0, 24) if n else 0
    chainy = rng.random() < 0.5  # half the graphs lean on paths, so that branches run to sinks
    for _ in range(ne):
        s = rng.randrange(n)
        t = (s + 1) % n if chainy and rng.random() < 0.7 else rng.randrange(n)
        b.edge(s, t, rng.choice((0, 1, 2, 5, 5, 9, 1000, 0xFFFFFFFF)), rng.choice((0.0, 0.5, 1.0, 5.0, 5.5, 40.0)),
               rng.choice((0, 0, 1, 3, 3, 8, 0xFFFFFFF0)), rng.randint(0, 9))
    for _ in range(rng.randint(0, 6) if ne else 0):
        b.link(rng.randrange(ne), rng.randrange(ne), rng.choice((1, 2, 7, 0x80000000)))
    return b.case(name, threaded=rng.random() < 0.7, min_length=rng.choice((0, 0, k, k + 1, k + 3)),
                  max_length=rng.choice((0, k, k + 2, k + 6, 10000)), max_dfs_states=rng.choice((0, 1, 5, 30, 2000)),
                  max_paths_per_pair=rng.choice((0, 1, 3, 20)), max_node_visits=rng.choice((0, 1, 2, 3)),
                  dedup_edit_threshold=rng.choice((0, 1, 2, 10)))
