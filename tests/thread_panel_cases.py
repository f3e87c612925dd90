"""Inputs of the panel read-threading tests (shk_thread_reads_panel), shared by the CPU test of the cases themselves
(test_thread_panel_cases_cpu.py) and the GPU tests (test_gpu_thread_panel.py): panels built out of thread_cases' graphs
and reads.  A Panel is one batch of reads, one graph per gene and one list of batch indices per gene; `expected` is, per
gene, thread_ref.thread_reads[_paired] over that gene's listed reads in list order — the model, never the library."""
from __future__ import annotations

import random
from collections import namedtuple

import thread_cases as tc
import thread_ref as ref

Panel = namedtuple("Panel", "name k graphs reads lists read_index mate", defaults=(None, None))


def expected(p: Panel) -> list:
    """→ one thread_ref.Annotations per gene."""
    out = []
    for g, ids in zip(p.graphs, p.lists):
        seqs = [p.reads[i] for i in ids]
        if p.mate is None:
            out.append(ref.thread_reads(g, seqs, p.k))
        else:
            out.append(ref.thread_reads_paired(g, seqs, [p.read_index[i] for i in ids], [p.mate[i] for i in ids], p.k))
    return out


def rows(ann, n_edges: int):
    """An annotation as the tuple the GPU tests compare: as_arrays' five lists and n_paired_links."""
    return tuple(ref.as_arrays(ann, n_edges)) + (ann.n_paired_links,)


def reverse(p: Panel) -> Panel:
    return p._replace(name=p.name + " (genes reversed)", graphs=p.graphs[::-1], lists=p.lists[::-1])


# ---- crafted panels at k = 3 ---------------------------------------------------------------------------------------------
def crafted_panel() -> Panel:
    """thread_cases.crafted_cases() as ONE panel: a gene per case, every read of every case in one batch, each gene
    listing its own reads."""
    graphs, reads, lists = [], [], []
    for _, g, rs in tc.crafted_cases():
        graphs.append(g)
        lists.append(list(range(len(reads), len(reads) + len(rs))))
        reads += rs
    return Panel("thread_cases as a panel", 3, graphs, reads, lists)


def crafted_gene(substr: str) -> int:
    """The gene of crafted_panel() whose case's name holds substr."""
    (at,) = [i for i, c in enumerate(tc.crafted_cases()) if substr in c[0]]
    return at


def twin_panel(swap: bool = False) -> Panel:
    """Two genes with the SAME graph and disjoint lists: the first one's reads support edge 1 (ACG), the second one's
    never touch it — support that leaked from one gene to the next on a workgroup would show there."""
    reads = [b"AACG", b"AAC", b"ACG", b"AAC", b"TTTT", b"AA"]
    lists = [[0, 2], [1, 3, 4, 5]]
    if swap:
        lists = lists[::-1]
    return Panel("twins" + (" swapped" if swap else ""), 3, [tc.linear_graph(), tc.linear_graph()], reads, lists)


def shared_read_panel() -> Panel:
    """Read 1 (AACG) is listed by three genes whose graphs all hold AAC and ACG."""
    par = tc.graph_of(["AA", "AC", "CG"], [(0, 1), (1, 2), (1, 2), (1, 2)])
    return Panel("a read in three genes", 3, [tc.linear_graph(), tc.branch_graph(), par], [b"TTTT", b"AACG", b"AAC", b"AACGG"],
                 [[1, 0], [3, 1], [2, 1, 1]])


def lists_panel() -> Panel:
    """What a list can be: empty between two that are not, given for a graph without edges, shared, with a repeat,
    descending, and of 7 reads — slices of 3, 3 and 1 at SHK_THREAD_PANEL_JOB=3, all shorter than a workgroup's 16 waves."""
    reads = [b"AACG", b"AAC", b"ACG", b"AACGG", b"TTTT", b"CGTT", b"AACNACG", b"AACGX", b"", b"AACG"]
    graphs = [tc.linear_graph(), tc.linear_graph(), tc.branch_graph(), ref.Graph([0, 1], []), tc.linear_graph(), tc.branch_graph()]
    lists = [[0, 1, 6], [], [3, 0, 3], [0, 1, 2], [9, 7, 6, 5, 3, 2, 0], [0]]
    return Panel("lists", 3, graphs, reads, lists)


def paired_panel() -> Panel:
    """Pair 5 (reads 0 and 1, read_index 10 and 11): both mates are listed in gene A, only R1 in gene B.  Pair 6's R2
    maps to nothing."""
    reads = [b"AACG", b"ACG", b"AAC", b"TTTT", b"AACG"]
    return Panel("paired", 3, [tc.linear_graph(), tc.linear_graph()], reads, [[0, 1, 2, 3], [0, 2, 3, 4]],
                 read_index=[10, 11, 12, 13, 20], mate=[1, 2, 1, 2, 0])


MANY_GENES = 40
MANY_EMPTY = 17  # the gene of many_panel() whose reads map to nothing


def many_panel() -> Panel:
    """MANY_GENES genes over the crafted graphs that have edges, in turn; every gene lists reads that map to its graph but
    gene MANY_EMPTY, which lists only reads that map to nothing."""
    pool = [(g, rs) for _, g, rs in tc.crafted_cases() if g.edges and rs]
    graphs, reads, lists = [], [], []
    for j in range(MANY_GENES):
        g, rs = pool[j % len(pool)]
        graphs.append(g)
        if j == MANY_EMPTY:
            rs = [b"TTTTT", b"GGGG", b"N"]
        lists.append([len(reads) + i for i in range(len(rs))] * (1 + j % 3))
        reads += rs
    return Panel("many genes", 3, graphs, reads, lists)


# ---- the random sweep: panels out of thread_cases.random_case ---------------------------------------------------------------
def sweep_groups() -> list:
    """thread_cases.SWEEP_SEEDS grouped by the k random_case draws for them (k = 4 + seed % 4: ten seeds each), every
    group cut into panels of 2, 3 and 5 seeds → 12 panels of 2 to 6 graphs that share k, no seed left out."""
    by_k = {}
    for seed in tc.SWEEP_SEEDS:
        by_k.setdefault(tc.random_case(seed)[0], []).append(seed)
    groups = []
    for k in sorted(by_k):
        seeds = by_k[k]
        at = 0
        for size in (2, 3, 5):
            if len(seeds) - at >= 2:
                groups.append(seeds[at:at + size])
                at += size
    return groups


def sweep_panel(seeds) -> Panel:
    """One batch of all the seeds' reads; gene j = seed j's graph, listing most of its own reads and some of the
    others' (lists overlap), shuffled, with a repeat now and then; read_index / mate as random_case gives them."""
    rng = random.Random(9300 + seeds[0])
    graphs, reads, own, mate = [], [], [], []
    k = None
    for seed in seeds:
        kk, g, rs, _, mt = tc.random_case(seed)
        assert k in (None, kk)
        k = kk
        graphs.append(g)
        own.append(list(range(len(reads), len(reads) + len(rs))))
        reads += rs
        mate += mt
    lists = []
    for j in range(len(seeds)):
        ids = [i for i in own[j] if rng.random() < 0.8] + [i for i in range(len(reads)) if i not in own[j] and rng.random() < 0.15]
        ids += rng.sample(ids, min(len(ids), 2))
        rng.shuffle(ids)
        lists.append(ids)
    return Panel(f"sweep {seeds}", k, graphs, reads, lists, read_index=list(range(100, 100 + len(reads))), mate=mate)
