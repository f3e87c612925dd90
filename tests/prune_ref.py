"""sPCR's graph cleanup restated literally, as the expected answer of the shk_pcr_prune_panel tests:
remove_low_coverage_tips, tip_length_backward / _forward and reachability_pruning (src/pcr/pruning.rs:19-214) and
annotate_coverage_ratios (src/pcr/graph.rs:533-546), on the array form shk_pcr_extend_panel hands out (flags, edge
endpoints, edge counts).  A small StableDiGraph stands in for petgraph's: removing a node removes its edges and leaves
every other index alone; neighbors_directed lists one entry per edge (parallel edges severally, a self-loop on both
sides).  Python ints, floats and lists throughout: it shares nothing with the library's CSR sides or kernel."""
from __future__ import annotations

from dataclasses import dataclass

from pcr_ref import median_via_select

OUTGOING, INCOMING = 0, 1


class StableDiGraph:
    def __init__(self, flags, edge_src, edge_tgt, edge_counts):
        self.flags = [int(f) for f in flags]
        self.alive = [True] * len(self.flags)
        self.edges = [(int(s), int(t), int(c)) for s, t, c in zip(edge_src, edge_tgt, edge_counts)]
        self.edge_alive = [True] * len(self.edges)
        self.out_e = [[] for _ in self.flags]
        self.in_e = [[] for _ in self.flags]
        for e, (s, t, _) in enumerate(self.edges):
            self.out_e[s].append(e)
            self.in_e[t].append(e)

    def node_indices(self):
        return [v for v, a in enumerate(self.alive) if a]

    def edge_indices(self):
        return [e for e, a in enumerate(self.edge_alive) if a]

    def node_count(self):
        return sum(self.alive)

    def is_start(self, v):
        return bool(self.flags[v] & 1)

    def is_end(self, v):
        return bool(self.flags[v] & 2)

    def edges_directed(self, v, direction):
        return list(self.out_e[v] if direction == OUTGOING else self.in_e[v])

    def neighbors_directed(self, v, direction):
        if direction == OUTGOING:
            return [self.edges[e][1] for e in self.out_e[v]]
        return [self.edges[e][0] for e in self.in_e[v]]

    def remove_node(self, v):
        for e in self.out_e[v]:
            self.edge_alive[e] = False
            t = self.edges[e][1]
            if t != v:
                self.in_e[t].remove(e)
        for e in self.in_e[v]:
            self.edge_alive[e] = False
            s = self.edges[e][0]
            if s != v:
                self.out_e[s].remove(e)
        self.out_e[v], self.in_e[v] = [], []
        self.alive[v] = False


def global_median_edge_count(graph):
    """pruning.rs:151-154."""
    return median_via_select([graph.edges[e][2] for e in graph.edge_indices()])


def tip_length_backward(graph, node):
    """pruning.rs:99-124."""
    length = 0
    current = node
    while True:
        length += 1
        incoming = graph.neighbors_directed(current, INCOMING)
        if len(incoming) != 1:
            break
        parent = incoming[0]
        if len(graph.neighbors_directed(parent, OUTGOING)) > 1:
            break
        if graph.is_start(parent):
            break
        current = parent
        if length > len(graph.flags):  # (a cycle of plain nodes: the reference would not come back; no case builds one)
            raise RuntimeError("tip_length_backward does not terminate on this graph")
    return length


def tip_length_forward(graph, node):
    """pruning.rs:128-149."""
    length = 0
    current = node
    while True:
        length += 1
        outgoing = graph.neighbors_directed(current, OUTGOING)
        if len(outgoing) != 1:
            break
        child = outgoing[0]
        if len(graph.neighbors_directed(child, INCOMING)) > 1:
            break
        if graph.is_end(child):
            break
        current = child
        if length > len(graph.flags):
            raise RuntimeError("tip_length_forward does not terminate on this graph")
    return length


def remove_low_coverage_tips(graph, k, tip_coverage_fraction):
    """pruning.rs:19-95 → (rounds that removed something, nodes removed)."""
    median_count = global_median_edge_count(graph)
    if median_count is None:
        median_count = 1.0
    x = median_count * tip_coverage_fraction
    min_tip_count = x if x > 1.0 else 1.0  # f64::max(1.0): 1.0 for a NaN product as well
    rounds = total = 0
    removed = 1
    while removed > 0:
        removed = 0
        nodes_to_remove = []
        for node in graph.node_indices():
            if graph.is_end(node) or graph.is_start(node):
                continue
            no_outgoing = len(graph.neighbors_directed(node, OUTGOING)) == 0
            no_incoming = len(graph.neighbors_directed(node, INCOMING)) == 0
            if not no_outgoing and not no_incoming:
                continue
            if no_outgoing:
                if tip_length_backward(graph, node) >= k:
                    continue
                max_incoming_count = max([graph.edges[e][2] for e in graph.edges_directed(node, INCOMING)], default=0)
                if float(max_incoming_count) >= min_tip_count:
                    continue
            if no_incoming:
                if tip_length_forward(graph, node) >= k:
                    continue
                max_outgoing_count = max([graph.edges[e][2] for e in graph.edges_directed(node, OUTGOING)], default=0)
                if float(max_outgoing_count) >= min_tip_count:
                    continue
            nodes_to_remove.append(node)
        for node in nodes_to_remove:
            graph.remove_node(node)
            removed += 1
        rounds += removed > 0
        total += removed
    return rounds, total


def reachability_pruning(graph):
    """pruning.rs:170-214 → nodes removed."""
    forward_reachable = set()
    stack = [n for n in graph.node_indices() if graph.is_start(n)]
    while stack:
        n = stack.pop()
        if n not in forward_reachable:
            forward_reachable.add(n)
            stack.extend(graph.neighbors_directed(n, OUTGOING))
    backward_reachable = set()
    stack = [n for n in graph.node_indices() if graph.is_end(n)]
    while stack:
        n = stack.pop()
        if n not in backward_reachable:
            backward_reachable.add(n)
            stack.extend(graph.neighbors_directed(n, INCOMING))
    nodes_to_remove = [n for n in graph.node_indices() if n not in forward_reachable or n not in backward_reachable]
    for node in nodes_to_remove:
        graph.remove_node(node)
    return len(nodes_to_remove)


def annotate_coverage_ratios(graph):
    """graph.rs:533-546 → ({edge: ratio}, median or None); an edge keeps get_dbedge's 0.0 where nothing is written."""
    ratio = {e: 0.0 for e in graph.edge_indices()}
    median = median_via_select([graph.edges[e][2] for e in graph.edge_indices()])
    if median is None or median <= 0.0:
        return ratio, median
    for e in graph.edge_indices():
        ratio[e] = float(graph.edges[e][2]) / median
    return ratio, median


@dataclass
class Pruned:
    """One gene of shk_pcr_prune_panel's answer, as lists."""
    node_keep: list
    node_index: list
    node_flags: list
    edge_index: list
    edge_src: list       # renumbered
    edge_tgt: list
    edge_counts: list
    coverage_ratio: list
    median: float        # of the pruned graph, 0.0 without edges
    tip_rounds: int
    tips_removed: int
    unreachable_removed: int


def prune(flags, edge_src, edge_tgt, edge_counts, k, tip_coverage_fraction=0.1, stages=3) -> Pruned:
    """do_pcr's sequence (src/pcr/mod.rs:631-697) under `stages` (bit 0 the tips, bit 1 reachability; 0 = both)."""
    stages = stages or 3
    g = StableDiGraph(flags, edge_src, edge_tgt, edge_counts)
    rounds = tips = unreachable = 0
    if stages & 1:
        rounds, tips = remove_low_coverage_tips(g, k, tip_coverage_fraction)
    if stages & 2:
        unreachable = reachability_pruning(g)
    ratio, median = annotate_coverage_ratios(g)
    nodes, edges = g.node_indices(), g.edge_indices()
    pos = {v: i for i, v in enumerate(nodes)}
    return Pruned([int(a) for a in g.alive], nodes, [g.flags[v] for v in nodes], edges, [pos[g.edges[e][0]] for e in edges],
                  [pos[g.edges[e][1]] for e in edges], [g.edges[e][2] for e in edges], [ratio[e] for e in edges],
                  0.0 if median is None else median, rounds, tips, unreachable)
