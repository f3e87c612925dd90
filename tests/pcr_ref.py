"""sPCR's graph extension restated literally, as the expected answer of the shk_neighborhood / shk_pcr_extend tests:
create_seed_graph and extend_graph (src/pcr/graph.rs:196-528), compute_node_budget and median_via_select
(graph.rs:40-103), compute_coverage_thresholds and the threshold sweep of do_pcr (src/pcr/mod.rs:403-428, 559-619),
over a merged table given as a {canonical k-mer: count} dict (the CPU oracle's `run_batch(...).merged().export()`);
and the level-by-level definition of shk_neighborhood (include/shk.h).  Python ints and dicts throughout: it shares
nothing with the library's sets, kernels or replay (sharkmer_amd/csrc/shk_pcr.cpp)."""
from __future__ import annotations

from collections import deque
from dataclasses import dataclass, field

EXTENSION_EVALUATION_FREQUENCY = 1_000  # graph.rs:16
DEFAULT_MAX_NUM_NODES = 500_000         # graph.rs:22
MIN_NODE_BUDGET = 100_000               # graph.rs:25
BUDGET_LERP_LOW_BP = 150_000_000        # graph.rs:28
BUDGET_LERP_HIGH_BP = 750_000_000       # graph.rs:31
COVERAGE_MULTIPLIER = 2                 # mod.rs:46
COVERAGE_STEPS = 4                      # mod.rs:49
FWD, REV = 0, 1                         # ExtDir


def table_dict(keys, counts) -> dict[int, int]:
    return {int(a): int(b) for a, b in zip(keys, counts)}


def revcomp(x: int, k: int) -> int:
    """revcomp_kmer (kmer/encoding.rs:219-262)."""
    r = 0
    for _ in range(k):
        r = (r << 2) | (3 - (x & 3))
        x >>= 2
    return r


def canonical_count(table: dict[int, int], x: int, k: int) -> int:
    """KmerCounts::get_canonical_count (counting.rs:205-209): 0 when absent."""
    return table.get(min(x, revcomp(x, k)), 0)


def compute_node_budget(n_bases_ingested: int) -> int:
    """graph.rs:40-52."""
    if n_bases_ingested <= BUDGET_LERP_LOW_BP:
        return MIN_NODE_BUDGET
    if n_bases_ingested >= BUDGET_LERP_HIGH_BP:
        return DEFAULT_MAX_NUM_NODES
    fraction = float(n_bases_ingested - BUDGET_LERP_LOW_BP) / float(BUDGET_LERP_HIGH_BP - BUDGET_LERP_LOW_BP)
    return int(float(MIN_NODE_BUDGET) + fraction * float(DEFAULT_MAX_NUM_NODES - MIN_NODE_BUDGET))


def median_via_select(counts):
    """graph.rs:82-103: None when empty; the even-length case averages the two middle order statistics in f64."""
    if not counts:
        return None
    s = sorted(counts)
    mid = len(s) // 2
    if len(s) % 2 == 0:
        return (float(s[mid - 1]) + float(s[mid])) / 2.0
    return float(s[mid])


def compute_coverage_thresholds(primer_count: int, min_count: int) -> list[int]:
    """mod.rs:403-428."""
    high = primer_count // COVERAGE_MULTIPLIER
    if high <= min_count:
        t = [min_count]
    else:
        step = (high - min_count) // (COVERAGE_STEPS - 1)
        t = [max(high - i * step, 0) for i in range(COVERAGE_STEPS)]
        t[-1] = min_count
    out = []
    for x in t:  # Vec::dedup: consecutive repeats
        if not out or out[-1] != x:
            out.append(x)
    return out


@dataclass
class Graph:
    """StableDiGraph<DBNode, DBEdge> with nothing ever removed: indices are insertion order."""
    sub_kmer: list = field(default_factory=list)
    is_start: list = field(default_factory=list)
    is_end: list = field(default_factory=list)
    edges: list = field(default_factory=list)  # (source, target, count) in EdgeIndex order
    found_path: bool = False
    median_refreshes: int = 0   # how often graph.rs:400-405 fired (for the tests' own assertions)
    budget_break: bool = False  # graph.rs:389 fired

    def copy(self) -> "Graph":
        return Graph(list(self.sub_kmer), list(self.is_start), list(self.is_end), list(self.edges))

    def flags(self) -> list[int]:
        return [(1 if s else 0) | (2 if e else 0) for s, e in zip(self.is_start, self.is_end)]

    def edge_kmer(self, i: int) -> int:
        """reconstruct_edge_kmer (graph.rs:127-134)."""
        s, t, _ = self.edges[i]
        return (self.sub_kmer[s] << 2) | (self.sub_kmer[t] & 3)


def create_seed_graph(forward_kmers, reverse_kmers, k: int) -> Graph:
    """graph.rs:196-278."""
    g = Graph()
    lookup: dict[int, int] = {}
    mask = (1 << (2 * (k - 1))) - 1
    for kmer in sorted(int(x) for x in forward_kmers):
        sub = kmer >> 2
        if sub in lookup:
            g.is_start[lookup[sub]] = True
        else:
            lookup[sub] = len(g.sub_kmer)
            g.sub_kmer.append(sub)
            g.is_start.append(True)
            g.is_end.append(False)
    for kmer in sorted(int(x) for x in reverse_kmers):
        sub = revcomp(kmer, k) & mask
        if sub in lookup:
            g.is_end[lookup[sub]] = True
        else:
            lookup[sub] = len(g.sub_kmer)
            g.sub_kmer.append(sub)
            g.is_start.append(False)
            g.is_end.append(True)
    return g


def extend_graph(seed: Graph, table: dict[int, int], k: int, min_count: int, table_min_count: int,
                 high_coverage_ratio: float, max_num_nodes: int) -> Graph:
    """graph.rs:321-528.  `table` with `table_min_count` is the FilteredKmerCounts view (counting.rs:316-342)."""
    g = seed.copy()
    lookup = {s: i for i, s in enumerate(g.sub_kmer)}
    mask = (1 << (2 * (k - 1))) - 1
    prefix_shift = 2 * (k - 1)
    have_edge = set()

    def get_canonical(kmer):  # FilteredKmerCounts::get_canonical
        c = table.get(min(kmer, revcomp(kmer, k)))
        return c if c is not None and c >= table_min_count else None

    def median_edge_count():
        m = median_via_select([e[2] for e in g.edges])
        return float(min_count) if m is None else m

    median = median_edge_count()
    last_median_check = 0
    frontier = deque()
    for node in range(len(g.sub_kmer)):
        if g.is_start[node]:
            frontier.append((node, FWD))
        if g.is_end[node]:
            frontier.append((node, REV))
    processed = (set(), set())
    added_by = ({n for n in range(len(g.sub_kmer)) if g.is_start[n]}, {n for n in range(len(g.sub_kmer)) if g.is_end[n]})
    while frontier:
        node, d = frontier.popleft()
        if node in processed[d]:
            continue
        processed[d].add(node)
        n_nodes = len(g.sub_kmer)
        if n_nodes > max_num_nodes:
            g.budget_break = True
            break
        if n_nodes > last_median_check and n_nodes - last_median_check > EXTENSION_EVALUATION_FREQUENCY:
            median = median_edge_count()
            last_median_check = n_nodes - n_nodes % EXTENSION_EVALUATION_FREQUENCY
            g.median_refreshes += 1
        sub = g.sub_kmer[node]
        candidates = []
        for base in range(4):
            kmer = (sub << 2) | base if d == FWD else (base << prefix_shift) | sub
            c = get_canonical(kmer)
            if c is not None and c >= min_count:
                candidates.append((kmer, c))
        for kmer, c in candidates:
            new_sub = kmer & mask if d == FWD else kmer >> 2
            if new_sub == sub:
                continue
            if new_sub in lookup:
                ex = lookup[new_sub]
                e = (node, ex) if d == FWD else (ex, node)
                if e not in have_edge:
                    have_edge.add(e)
                    g.edges.append((e[0], e[1], c))
                    if ex in added_by[1 - d]:
                        g.found_path = True
            else:
                if float(c) > median * high_coverage_ratio:
                    continue
                nn = len(g.sub_kmer)
                g.sub_kmer.append(new_sub)
                g.is_start.append(False)
                g.is_end.append(False)
                lookup[new_sub] = nn
                added_by[d].add(nn)
                e = (node, nn) if d == FWD else (nn, node)
                have_edge.add(e)
                g.edges.append((e[0], e[1], c))
                frontier.append((nn, d))
    return g


def pcr_extend(fwd, rev, table: dict[int, int], k: int, min_count: int = 2, table_min_count: int = 2,
               high_coverage_ratio: float = 10.0, max_num_nodes: int = MIN_NODE_BUDGET, sweep: bool = True):
    """The extension part of do_pcr (mod.rs:520-619) → (graph of the last step run, threshold used, steps run).
    fwd, rev: (k-mers, counts) of the two primer sets."""
    seed = create_seed_graph(fwd[0], rev[0], k)
    max_f = max((int(c) for c in fwd[1]), default=0)  # get_max_count
    max_r = max((int(c) for c in rev[1]), default=0)
    thresholds = compute_coverage_thresholds(min(max_f, max_r), min_count) if sweep else [min_count]
    cur, used, steps = seed.copy(), thresholds[0], 0
    for t in thresholds:
        cur = extend_graph(seed, table, k, t, table_min_count, high_coverage_ratio, max_num_nodes)
        used, steps = t, steps + 1
        if cur.found_path:
            break
    return cur, used, steps


def iter_levels(nodes, dirs, table, k: int, min_count: int):
    """Level after level of the complete neighbourhood, each with the accepted k-mers its expansion adds: yields
    (level entries as a sorted list of (node, dir bit), {canonical k-mer: count} new in its expansion).  `table`: a
    dict, or anything with its `get`.  Lazy: who stops asking pays for no further level."""
    mask = (1 << (2 * (k - 1))) - 1
    sh = 2 * (k - 1)
    mc = max(min_count, 1)
    level = set()
    for n, d in zip(nodes, dirs):
        n, d = int(n), int(d)
        assert 1 <= d <= 3 and n <= mask
        if d & 1:
            level.add((n, 1))
        if d & 2:
            level.add((n, 2))
    seen, kseen = set(level), set()
    while level:
        new_k, nxt = {}, set()
        for n, d in level:
            for b in range(4):
                x = (n << 2) | b if d == 1 else (b << sh) | n
                cn = min(x, revcomp(x, k))
                c = table.get(cn, 0)
                if c < mc:
                    continue
                if cn not in kseen:
                    new_k[cn] = c
                s = (x & mask if d == 1 else x >> 2, d)
                if s not in seen:
                    nxt.add(s)
        kseen |= set(new_k)
        seen |= nxt
        yield sorted(level), new_k
        level = nxt


def neighborhood_levels(nodes, dirs, table: dict[int, int], k: int, min_count: int):
    """Every level of the complete neighbourhood: [(level entries, {canonical k-mer: count} new in its expansion)]."""
    return list(iter_levels(nodes, dirs, table, k, min_count))


def neighborhood(nodes, dirs, table: dict[int, int], k: int, min_count: int, max_levels: int = 0, cap: int = 1 << 62,
                 fringe_cap: int = 1 << 62, levels=None):
    """shk_neighborhood's whole-level rule (include/shk.h) → (kmers, counts, fringe_nodes, fringe_dirs, levels_done) as
    lists.  `levels`: neighborhood_levels of the same seeds, if the caller has it already; otherwise the levels are
    walked only as far as the rule looks (one past the last it expands)."""
    it = iter(levels) if levels is not None else iter_levels(nodes, dirs, table, k, min_count)
    cur = next(it, None)
    if cur is not None and len(cur[0]) > fringe_cap:
        raise ValueError("more distinct seeds than fringe_cap")
    K, L = {}, 0
    while cur is not None and not (max_levels and L >= max_levels):
        nxt = next(it, None)
        nk = len(K) + len(cur[1])
        nf = len(nxt[0]) if nxt is not None else 0
        if nk > cap or nf > fringe_cap:
            break
        K.update(cur[1])
        L += 1
        cur = nxt
    fringe = cur[0] if cur is not None else []
    ks = sorted(K)
    return ks, [K[x] for x in ks], [n for n, _ in fringe], [d for _, d in fringe], L
