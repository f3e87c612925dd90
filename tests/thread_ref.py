"""sPCR's read threading restated literally, as the expected answer of the shk_thread_reads tests: build_edge_lookup,
resolve_candidates, find_contiguous_runs, is_run_unambiguous, record_branch_links, thread_reads and thread_reads_paired
(src/pcr/threading.rs:87-364) with kmers_from_ascii (src/kmer/encoding.rs:332-371) and reconstruct_edge_kmer
(src/pcr/graph.rs:127-134), over a graph given as a list of node sub_kmers and a list of (source, target) edges — node
and edge indices are list positions, which is what a StableDiGraph's indices are in ascending order.  Python ints, lists
and dicts throughout: it shares nothing with the library's lookup set, link slots or kernel.

`thread_reads*` also return, under "events", what the walk met on the way — the random sweep's coverage asserts read it."""
from __future__ import annotations

from dataclasses import dataclass, field

UNPAIRED, R1, R2 = 0, 1, 2  # io.rs Mate, as shk_thread_reads' mate bytes


@dataclass
class Graph:
    sub_kmer: list  # DBNode.sub_kmer per node
    edges: list     # (source node, target node) per edge

    def edge_endpoints(self, e):
        return self.edges[e]

    def _degrees(self):
        """neighbors_directed(v, dir).count() for every v: one per edge, parallel edges and self-loops included (counted
        once per graph; the edge list must not change afterwards)."""
        if getattr(self, "_deg", None) is None:
            i, o = {}, {}
            for s, t in self.edges:
                o[s] = o.get(s, 0) + 1
                i[t] = i.get(t, 0) + 1
            self._deg = (i, o)
        return self._deg

    def in_degree(self, v):
        return self._degrees()[0].get(v, 0)

    def out_degree(self, v):
        return self._degrees()[1].get(v, 0)


@dataclass
class Annotations:
    """ThreadingAnnotations (threading.rs:54-62); read_edges is what thread_reads_paired calls all_edges, as a length."""
    support_total: dict = field(default_factory=dict)        # edge -> read_support_total
    support_unambiguous: dict = field(default_factory=dict)  # edge -> read_support_unambiguous
    branch_links: dict = field(default_factory=dict)         # (incoming, outgoing) -> count
    n_paired_links: int = 0
    read_edges: list = field(default_factory=list)
    events: dict = field(default_factory=dict)


class InvalidChar(Exception):
    pass


def revcomp(x: int, k: int) -> int:
    """revcomp_kmer (kmer/encoding.rs:219-262)."""
    r = 0
    for _ in range(k):
        r = (r << 2) | (3 - (x & 3))
        x >>= 2
    return r


def kmers_from_ascii(seq: bytes, k: int):
    """encoding.rs:332-371.  Also returns, per k-mer, whether an N lay between it and the k-mer before it (the model's
    own bookkeeping for the coverage asserts; the reference keeps no such mark)."""
    mask = (1 << (2 * k)) - 1
    kmers, after_n = [], []
    frame = revframe = n_valid = 0
    saw_n = False
    for b in seq:
        if b == ord("N"):
            n_valid = frame = revframe = 0
            saw_n = True
            continue
        if b not in b"ACGT":
            raise InvalidChar(chr(b))
        base = b"ACGT".index(b)
        frame = (frame << 2) | base
        revframe = (revframe >> 2) | ((3 - base) << (2 * (k - 1)))
        n_valid += 1
        if n_valid >= k:
            kmers.append(min(frame & mask, revframe & mask))
            after_n.append(saw_n)
            saw_n = False
    return kmers, after_n


def reconstruct_edge_kmer(g: Graph, e: int) -> int:
    """graph.rs:127-134."""
    s, t = g.edge_endpoints(e)
    return (g.sub_kmer[s] << 2) | (g.sub_kmer[t] & 3)


def build_edge_lookup(g: Graph, k: int) -> dict:
    """threading.rs:203-220: canonical k-mer -> candidate edges, in edge order."""
    lookup = {}
    for e in range(len(g.edges)):
        kmer = reconstruct_edge_kmer(g, e)
        lookup.setdefault(min(kmer, revcomp(kmer, k)), []).append(e)
    return lookup


def resolve_candidates(candidates, prev_edge, g: Graph, events=None):
    """threading.rs:233-256."""
    if len(candidates) == 1:
        return candidates[0]
    if prev_edge is not None:
        prev_target = g.edge_endpoints(prev_edge)[1]
        for cand in candidates:
            if g.edge_endpoints(cand)[0] == prev_target:
                if events is not None:
                    which = "resolved_by_adjacency" if cand == candidates[0] else "resolved_by_adjacency_not_first"
                    events[which] = events.get(which, 0) + 1
                return cand
        if events is not None:
            events["resolved_to_first"] = events.get("resolved_to_first", 0) + 1
    return candidates[0]


def find_contiguous_runs(kmers, lookup, g: Graph, events=None, after_n=None):
    """threading.rs:261-315 → list of runs, each a list of edges."""
    runs, current = [], []
    for i, kmer in enumerate(kmers):
        candidates = lookup.get(kmer)
        if candidates is None:
            if current:
                runs.append(current)
                current = []
            continue
        edge = resolve_candidates(candidates, current[-1] if current else None, g, events)
        if current:
            if g.edge_endpoints(current[-1])[1] == g.edge_endpoints(edge)[0]:
                current.append(edge)
                if events is not None and after_n is not None and after_n[i]:
                    events["run_across_n"] = events.get("run_across_n", 0) + 1
            else:
                runs.append(current)
                current = [edge]
        else:
            current.append(edge)
    if current:
        runs.append(current)
    return runs


def _is_branch(g: Graph, node) -> bool:
    return g.in_degree(node) > 1 or g.out_degree(node) > 1


def is_run_unambiguous(g: Graph, edges) -> bool:
    """threading.rs:321-337."""
    if len(edges) < 2:
        return True
    for a in edges[:-1]:
        if _is_branch(g, g.edge_endpoints(a)[1]):
            return False
    return True


def record_branch_links(g: Graph, edges, branch_links: dict):
    """threading.rs:341-364."""
    for incoming, outgoing in zip(edges, edges[1:]):
        if _is_branch(g, g.edge_endpoints(incoming)[1]):
            branch_links[(incoming, outgoing)] = branch_links.get((incoming, outgoing), 0) + 1


def _thread(g: Graph, reads, k: int, paired: bool) -> Annotations:
    ann = Annotations()
    lookup = build_edge_lookup(g, k)
    pair_runs = {}
    for seq, index, mate in reads:
        try:
            kmers, after_n = kmers_from_ascii(seq, k)
        except InvalidChar:
            ann.read_edges.append(0)
            continue
        runs = find_contiguous_runs(kmers, lookup, g, ann.events, after_n)
        all_edges = []
        for run in runs:
            unambiguous = is_run_unambiguous(g, run)
            for e in run:
                ann.support_total[e] = ann.support_total.get(e, 0) + 1
                if unambiguous:
                    ann.support_unambiguous[e] = ann.support_unambiguous.get(e, 0) + 1
            record_branch_links(g, run, ann.branch_links)
            all_edges.extend(run)
            if not unambiguous and len(run) >= 3:
                ann.events["ambiguous_run_3"] = ann.events.get("ambiguous_run_3", 0) + 1
            if len(set(run)) < len(run):
                ann.events["edge_twice_in_run"] = ann.events.get("edge_twice_in_run", 0) + 1
        ann.read_edges.append(len(all_edges))
        if paired and all_edges:
            if mate == R1:
                pair_runs.setdefault(index // 2, [[], []])[0] = all_edges
            elif mate == R2:
                pair_runs.setdefault(index // 2, [[], []])[1] = all_edges
    for r1_edges, r2_edges in pair_runs.values():
        if r1_edges and r2_edges:
            ann.n_paired_links += 1
    if ann.n_paired_links:
        ann.events["pair_both_mapped"] = ann.n_paired_links
    return ann


def thread_reads(g: Graph, seqs, k: int) -> Annotations:
    """threading.rs:87-123; seqs: byte strings."""
    return _thread(g, [(s, 0, UNPAIRED) for s in seqs], k, False)


def thread_reads_paired(g: Graph, seqs, read_index, mate, k: int) -> Annotations:
    """threading.rs:128-192."""
    return _thread(g, list(zip(seqs, read_index, mate)), k, True)


def as_arrays(ann: Annotations, n_edges: int):
    """The annotation in the form shk_thread_reads hands out: per-edge lists, links ascending by (in, out)."""
    links = sorted(ann.branch_links)
    return ([ann.support_total.get(e, 0) for e in range(n_edges)],
            [ann.support_unambiguous.get(e, 0) for e in range(n_edges)],
            [list(l) for l in links], [ann.branch_links[l] for l in links], list(ann.read_edges))
