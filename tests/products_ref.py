"""sPCR's last stage restated literally, as the expected answer of the shk_pcr_paths_panel / shk_pcr_dedup_panel /
shk_pcr_products_panel tests: resolve_bubbles with detect_simple_bubbles, rank_branches and branch_sort_key
(src/pcr/bubble.rs:52-275), sorted_children and get_assembly_paths (src/pcr/paths.rs:42-186),
generate_sequences_from_paths (:190-356), sort_and_deduplicate (:360-427), the renumbering of src/pcr/mod.rs:785-813 and
PathScore::composite (mod.rs:80-113), on the array form shk_pcr_prune_panel and shk_thread_reads_panel hand out.

A small StableDiGraph stands in for petgraph's.  The ONE property taken from knowledge of the crate rather than from the
reference's text: `edges_directed(v, dir)` of petgraph 0.6 yields a node's edges NEWEST FIRST — `add_edge` links the new
edge at the head of its node's list — and removing nodes (all the pruning does) keeps the relative order of the others;
so on arrays in EdgeIndex order a node's edges come in DESCENDING edge index.

Python ints, floats, dicts and lists throughout, a full-matrix Levenshtein distance: it shares nothing with the
library's CSR, its banded DP or its kernel.  Python's float is the f64 of the reference, `/`, `*`, `+`, sqrt are IEEE
operations in both, and sums run in the reference's order, so doubles are compared bit for bit."""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from functools import cmp_to_key
from typing import NamedTuple

from pcr_ref import median_via_select

OUTGOING, INCOMING = 0, 1
MAX_BUBBLE_DEPTH = 50     # bubble.rs:17
MAX_NUM_AMPLICONS = 20    # paths.rs:20
U32 = 0xFFFFFFFF


class Annotations(NamedTuple):
    """ThreadingAnnotations (threading.rs:54-62): edge_support per edge, branch_links as {(incoming, outgoing): count}."""
    support_total: list
    support_unambiguous: list
    branch_links: dict


class Params(NamedTuple):
    min_length: int = 0
    max_length: int = 10000
    max_dfs_states: int = 100000
    max_paths_per_pair: int = 20
    max_node_visits: int = 2
    dedup_edit_threshold: int = 10


class StableDiGraph:
    def __init__(self, sub_kmers, flags, edge_src, edge_tgt, edge_counts, coverage_ratio):
        self.sub = [int(x) for x in sub_kmers]
        self.flags = [int(f) for f in flags]
        self.edges = [(int(s), int(t)) for s, t in zip(edge_src, edge_tgt)]
        self.count = [int(c) for c in edge_counts]
        self.ratio = [float(r) for r in coverage_ratio]
        self.out_e = [[] for _ in self.flags]
        self.in_e = [[] for _ in self.flags]
        for e, (s, t) in enumerate(self.edges):  # add_edge: the new edge goes to the head of both lists
            self.out_e[s].insert(0, e)
            self.in_e[t].insert(0, e)

    def node_indices(self):
        return range(len(self.flags))

    def edges_directed(self, v, direction):
        return list(self.out_e[v] if direction == OUTGOING else self.in_e[v])

    def target(self, e):
        return self.edges[e][1]


def total_cmp(a: float, b: float) -> int:
    """f64::total_cmp for the values met here (no NaN): -0.0 below +0.0, else the usual order."""
    ka, kb = (math.copysign(1.0, a), a), (math.copysign(1.0, b), b)
    if a == b:
        return (ka[0] > kb[0]) - (ka[0] < kb[0])
    return (a > b) - (a < b)


# ---- bubble.rs ----

def detect_simple_bubbles(graph):
    """bubble.rs:101-184 → [(source, sink, branches)], the bubbles of one source in first-seen order of the sink."""
    bubbles = []
    for source in graph.node_indices():
        outgoing = graph.edges_directed(source, OUTGOING)
        if len(outgoing) < 2:
            continue
        branch_endpoints = {}
        for first_edge in outgoing:
            current = graph.target(first_edge)
            branch_edges = [first_edge]
            visited = {source}
            depth = 0
            terminated_naturally = False
            while True:
                if depth >= MAX_BUBBLE_DEPTH:
                    break
                depth += 1
                if current in visited:
                    break
                visited.add(current)
                next_edges = graph.edges_directed(current, OUTGOING)
                if len(next_edges) == 1:
                    branch_edges.append(next_edges[0])
                    current = graph.target(next_edges[0])
                else:
                    terminated_naturally = True
                    break
            if terminated_naturally:
                branch_endpoints.setdefault(current, []).append(branch_edges)
        for sink, branches in branch_endpoints.items():
            if len(branches) >= 2 and sink != source:
                bubbles.append((source, sink, branches))
    return bubbles


def branch_sort_key(graph, edges):
    if not edges:
        return 0
    src, tgt = graph.edges[edges[0]]
    return (graph.sub[src] << 2) | (graph.sub[tgt] & 3)


def rank_branches(graph, bubble, ann: Annotations):
    """bubble.rs:187-255 → [(edges, total_read_support, phasing_support)] best first; u32 sums wrap (release build)."""
    source, _, branches = bubble
    rankings = []
    for branch_edges in branches:
        total = 0
        for e in branch_edges:
            total = (total + ann.support_total[e]) & U32
        phasing = 0
        if branch_edges:
            for incoming in graph.edges_directed(source, INCOMING):
                c = ann.branch_links.get((incoming, branch_edges[0]))
                if c is not None:
                    phasing = (phasing + c) & U32
        rankings.append((list(branch_edges), total, phasing))

    def cmp(a, b):
        a_total, b_total = (a[1] + a[2]) & U32, (b[1] + b[2]) & U32
        if a_total != b_total:
            return -1 if b_total < a_total else 1
        ka, kb = branch_sort_key(graph, a[0]), branch_sort_key(graph, b[0])
        return (ka > kb) - (ka < kb)

    rankings.sort(key=cmp_to_key(cmp))  # (stable, like sort_by)
    return rankings


def resolve_bubbles(graph, ann: Annotations) -> dict:
    """bubble.rs:52-87 → {edge: preference}."""
    prefs = {}
    for bubble in detect_simple_bubbles(graph):
        rankings = rank_branches(graph, bubble, ann)
        if len(rankings) >= 2:
            max_support = max((r[1] + r[2]) & U32 for r in rankings)
            for edges, total, phasing in rankings:
                support = (total + phasing) & U32
                preference = float(support) / float(max_support) if max_support > 0 else 1.0
                for e in edges:
                    prefs[e] = preference
    return prefs


# ---- paths.rs ----

def sorted_children(graph, node, prefs):
    """paths.rs:42-64 → [(target, edge, score)] ascending, so that pop() gives the highest."""
    outgoing = []
    for e in graph.edges_directed(node, OUTGOING):
        pref = prefs.get(e, 1.0) if prefs is not None else 1.0
        outgoing.append((graph.target(e), e, float(graph.count[e]) * pref))
    outgoing.sort(key=cmp_to_key(lambda a, b: total_cmp(a[2], b[2])))
    return outgoing


def get_assembly_paths(graph, k, p: Params, prefs, stats=None):
    """paths.rs:78-186 → [[(node, edge or None)]]; stats, when given, receives the states explored per start node."""
    min_path_nodes = 1 if p.min_length <= k else p.min_length - k + 2
    max_path_nodes = 1 if p.max_length <= k else p.max_length - k + 2
    end_nodes = {v for v in graph.node_indices() if graph.flags[v] & 2}
    all_paths = []
    for start in [v for v in graph.node_indices() if graph.flags[v] & 1]:
        paths_from_start = 0
        states_explored = 0
        path = [(start, None)]
        visit_counts = {start: 1}
        child_stack = [sorted_children(graph, start, prefs)]
        while True:
            if paths_from_start >= p.max_paths_per_pair or states_explored >= p.max_dfs_states:
                break
            depth = len(child_stack) - 1
            if child_stack[depth]:
                neighbor, edge_id, _ = child_stack[depth].pop()
                states_explored += 1
                if visit_counts.get(neighbor, 0) >= p.max_node_visits:
                    continue
                path.append((neighbor, edge_id))
                visit_counts[neighbor] = visit_counts.get(neighbor, 0) + 1
                path_len = len(path)
                if neighbor in end_nodes and path_len >= min_path_nodes:
                    all_paths.append(list(path))
                    paths_from_start += 1
                    visit_counts[neighbor] -= 1
                    path.pop()
                    continue
                if path_len >= max_path_nodes:
                    visit_counts[neighbor] -= 1
                    path.pop()
                    continue
                child_stack.append(sorted_children(graph, neighbor, prefs))
            else:
                child_stack.pop()
                if not child_stack:
                    break
                backtrack_node, _ = path.pop()
                visit_counts[backtrack_node] -= 1
        if stats is not None:
            stats.append(states_explored)
    return all_paths


def kmer_to_seq(kmer: int, k: int) -> str:
    return "".join("ACGT"[(kmer >> (2 * (k - i - 1))) & 3] for i in range(k))


def compute_mean(numbers):
    return float(sum(numbers)) / float(len(numbers)) if numbers else 0.0


def compute_median(numbers):
    m = median_via_select(list(numbers))
    return 0.0 if m is None else m


def composite(s) -> float:
    """PathScore::composite, mod.rs:80-113."""
    base = s["kmer_median_count"]
    cv_penalty = 1.0 / s["coverage_cv"] if s["coverage_cv"] > 1.0 else 1.0
    repeat_penalty = 5.0 / s["max_coverage_ratio"] if s["max_coverage_ratio"] > 5.0 else 1.0
    if s["zero_support_edges"] is not None and s["edge_support_fraction"] is not None:
        zero_edges = s["zero_support_edges"]
        zero_penalty = 0.5 ** min(zero_edges, 10) if zero_edges > 0 else 1.0
        support_bonus = max(s["edge_support_fraction"], 0.1)
        read_support_factor = zero_penalty * support_bonus
    else:
        read_support_factor = 1.0
    return base * cv_penalty * repeat_penalty * read_support_factor


@dataclass
class Record:
    sequence: str
    start_node: int
    path_nodes: int
    count_mean: float
    count_median: float
    count_min: int
    count_max: int
    score: dict = field(default_factory=dict)

    @property
    def composite(self):
        return composite(self.score)

    def desc(self, sample, gene, index):
        """The format! of paths.rs:332-343 (Rust's {:.2} is correctly rounded like Python's; {} of an f64 prints 12, 12.5)."""
        med = self.count_median
        med_s = str(int(med)) if med == int(med) else repr(med)
        return (f"sample={sample} gene={gene} product={index} length={len(self.sequence)} kmer_count_mean={self.count_mean:.2f} "
                f"kmer_count_median={med_s} kmer_count_min={self.count_min} kmer_count_max={self.count_max} score={self.composite:.2f}")


def generate_sequences_from_paths(graph, all_paths, k, p: Params, ann):
    """paths.rs:190-356."""
    records = []
    for path in all_paths:
        sequence = ""
        edge_counts = []
        path_edges = []
        for node, edge_opt in path:
            if not sequence:
                sequence = kmer_to_seq(graph.sub[node], k - 1)
            else:
                sequence += "ACGT"[graph.sub[node] & 3]
                edge_counts.append(graph.count[edge_opt])
                path_edges.append(edge_opt)
        if len(sequence) < p.min_length:
            continue
        if not edge_counts:
            continue
        count_mean = compute_mean(edge_counts)
        count_median = compute_median(edge_counts)
        count_min, count_max = min(edge_counts), max(edge_counts)
        if count_mean > 0.0:
            variance = 0.0
            for c in edge_counts:
                diff = float(c) - count_mean
                variance += diff * diff
            variance /= float(len(edge_counts))
            coverage_cv = math.sqrt(variance) / count_mean
        else:
            coverage_cv = 0.0
        max_coverage_ratio = 0.0
        for e in path_edges:
            r = graph.ratio[e]
            if r > max_coverage_ratio:  # f64::max from 0.0 (a NaN ratio is passed over)
                max_coverage_ratio = r
        if ann is not None:
            total_edges = supported_edges = zero_count = 0
            unambiguous_counts = []
            for e in path_edges:
                total_edges += 1
                if ann.support_total[e] > 0:
                    supported_edges += 1
                    unambiguous_counts.append(int(ann.support_unambiguous[e]))
                else:
                    zero_count += 1
                    unambiguous_counts.append(0)
            frac = float(supported_edges) / float(total_edges) if total_edges > 0 else 0.0
            median_unamb = compute_median(unambiguous_counts) if unambiguous_counts else 0.0
            support = (zero_count, median_unamb, frac)
        else:
            support = (None, None, None)
        score = {"kmer_min_count": count_min & U32, "kmer_median_count": count_median, "coverage_cv": coverage_cv,
                 "max_coverage_ratio": max_coverage_ratio, "zero_support_edges": support[0],
                 "median_unambiguous_support": support[1], "edge_support_fraction": support[2]}
        records.append(Record(sequence, path[0][0], len(path), count_mean, count_median, count_min, count_max, score))
    return records


def levenshtein(a, b) -> int:
    """The full matrix, row by row."""
    prev = list(range(len(b) + 1))
    for i in range(1, len(a) + 1):
        cur = [i] + [0] * len(b)
        for j in range(1, len(b) + 1):
            cur[j] = min(prev[j - 1] + (a[i - 1] != b[j - 1]), prev[j] + 1, cur[j - 1] + 1)
        prev = cur
    return prev[len(b)]


def levenshtein_rows(a, b) -> int:
    """The same full matrix with each row as one numpy expression, for records of thousands of bases: the row's
    left-to-right dependency cur[j] = min(x[j], cur[j-1] + 1) is a running minimum of x[j] - j."""
    import numpy as np
    a = np.frombuffer(a.encode() if isinstance(a, str) else bytes(a), dtype=np.uint8)
    b = np.frombuffer(b.encode() if isinstance(b, str) else bytes(b), dtype=np.uint8)
    ramp = np.arange(len(b) + 1, dtype=np.int64)
    prev = ramp.copy()
    for i in range(1, len(a) + 1):
        x = np.empty(len(b) + 1, dtype=np.int64)
        x[0] = i
        x[1:] = np.minimum(prev[:-1] + (b != a[i - 1]), prev[1:] + 1)
        prev = np.minimum.accumulate(x - ramp) + ramp
    return int(prev[len(b)])


def distance_matrix(seqs, distance=levenshtein_rows):
    """All pairwise distances of a record set, computed once and shared by every threshold asked of it."""
    n = len(seqs)
    d = [[0] * n for _ in range(n)]
    for i in range(n):
        for j in range(i + 1, n):
            d[i][j] = d[j][i] = distance(seqs[i], seqs[j])
    return d


def sort_order(seqs, scores):
    """The order of sort_and_deduplicate's sort_by: composite descending (total_cmp), then sequence bytes ascending."""
    def cmp(x, y):
        c = total_cmp(scores[y], scores[x])
        if c:
            return c
        a, b = seqs[x].encode() if isinstance(seqs[x], str) else seqs[x], seqs[y].encode() if isinstance(seqs[y], str) else seqs[y]
        return (a > b) - (a < b)
    return sorted(range(len(seqs)), key=cmp_to_key(cmp))


def pair_matrix(seqs, order, t, dist=None):
    """within-t of every pair i < j of the sorted order, row-major upper triangle."""
    d = dist if dist is not None else distance_matrix(seqs, levenshtein)
    return [d[order[i]][order[j]] <= t for i in range(len(order)) for j in range(i + 1, len(order))]


def sort_and_deduplicate(seqs, scores, t, dist=None):
    """paths.rs:360-427 on sequences and their composite scores → (kept input indices after truncation, retained).
    dist: the set's distance_matrix when the caller has it already."""
    order = sort_order(seqs, scores)
    kept = []
    for r in order:
        if not any((dist[r][q] if dist is not None else levenshtein(seqs[r], seqs[q])) <= t for q in kept):
            kept.append(r)
    return kept[:MAX_NUM_AMPLICONS], len(kept)


class GeneResult(NamedTuple):
    records: list       # generate_sequences_from_paths
    paths_found: int
    states_explored: int
    prefs: dict | None
    products: list      # after sort_and_deduplicate, in product order
    retained: int


def run_gene(k, sub_kmers, flags, edge_src, edge_tgt, edge_counts, coverage_ratio, ann, p: Params) -> GeneResult:
    """do_pcr from resolve_bubbles to the renumbered products (mod.rs:699-813) for one gene."""
    graph = StableDiGraph(sub_kmers, flags, edge_src, edge_tgt, edge_counts, coverage_ratio)
    prefs = resolve_bubbles(graph, ann) if ann is not None else None
    stats = []
    paths = get_assembly_paths(graph, k, p, prefs, stats)
    records = generate_sequences_from_paths(graph, paths, k, p, ann) if paths else []
    kept, retained = sort_and_deduplicate([r.sequence for r in records], [r.composite for r in records], p.dedup_edit_threshold)
    return GeneResult(records, len(paths), sum(stats), prefs, [records[i] for i in kept], retained)
