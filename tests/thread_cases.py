"""Inputs of the read-threading tests, shared by the model's CPU tests (test_thread_ref_cpu.py) and the GPU tests
(test_gpu_thread_reads.py): the crafted k = 3 graphs and reads, and the generator of the random sweep."""
from __future__ import annotations

import random

import thread_ref as ref

COMP = bytes.maketrans(b"ACGTN", b"TGCAN")


def enc(s: str) -> int:
    v = 0
    for ch in s:
        v = (v << 2) | "ACGT".index(ch)
    return v


def dec(x: int, n: int) -> str:
    return "".join("ACGT"[(x >> (2 * (n - 1 - i))) & 3] for i in range(n))


def rc_bytes(s: bytes) -> bytes:
    return s[::-1].translate(COMP)


def graph_of(nodes, edges) -> ref.Graph:
    """nodes: (k−1)-mers as strings; edges: (source, target) node positions."""
    return ref.Graph([enc(n) for n in nodes], list(edges))


# ---- the reference's own test graphs (threading.rs:371-410, 496-545, 600-616) ------------------------------------------
def linear_graph():
    return graph_of(["AA", "AC", "CG"], [(0, 1), (1, 2)])


def inverted_repeat_graph():
    return graph_of(["AA", "AC", "GT", "TT"], [(0, 1), (1, 2), (2, 3)])  # e_x AAC, e_bridge, e_rcx GTT


def branch_graph():
    return graph_of(["AA", "AC", "CG", "GG"], [(0, 1), (1, 2), (1, 3)])  # n1 has out-degree 2


def crafted_cases():
    """(name, graph, reads) at k = 3."""
    cases = []
    lin = linear_graph()
    cases.append(("linear: lengths 0, k-1, k, k+1, a miss, the path's reverse complement",
                  lin, [b"", b"AA", b"AAC", b"AACG", b"TTTT", rc_bytes(b"AACG"), b"AACG"]))
    # AAC N ACG: the windows with the N are dropped, AAC and ACG stay neighbours and e0 → e1 is adjacent
    cases.append(("linear: a run across an N", lin, [b"AACNACG", b"AACNNNACG", b"AANCG"]))
    cases.append(("linear: an invalid byte, last and elsewhere", lin, [b"AACGX", b"AACG", b"xAACG", b"AAC-ACG"]))
    cases.append(("inverted repeat: e_rcx third", inverted_repeat_graph(), [b"AACGTT", b"GTT", b"AAC", rc_bytes(b"AACGTT")]))
    cases.append(("branch: a link recorded per crossing", branch_graph(), [b"AACG", b"AACG", b"AAC", b"ACG", b"AACGG"]))
    # a 4-cycle AC → CC → CA → AA → AC (ACC, CCA, CAA, AAC: no two are reverse complements); three times round in one run
    cyc = graph_of(["AC", "CC", "CA", "AA"], [(0, 1), (1, 2), (2, 3), (3, 0)])
    cases.append(("4-cycle: a tandem read", cyc, [b"ACCA" * 3 + b"AC", b"ACCAAC", b"CAACC"]))
    # three parallel edges AC → CG behind AA → AC: one key, three candidates, all adjacent; AC has out-degree 3
    par = graph_of(["AA", "AC", "CG"], [(0, 1), (1, 2), (1, 2), (1, 2)])
    cases.append(("three parallel edges", par, [b"AACG", b"ACG", b"AACGNAACG"]))
    # one key, three candidates with different sources (three nodes AA): the SECOND is the one behind CA → AA
    tri = graph_of(["AA", "AA", "AA", "AC", "CA"], [(0, 3), (1, 3), (2, 3), (4, 1)])
    cases.append(("three candidates, the second adjacent", tri, [b"CAAC", b"AAC", b"GCAACT"]))
    # a self-loop AA → AA (in- and out-degree both count it) with a way out: AA is a branch node
    loop = graph_of(["AA", "AC"], [(0, 0), (0, 1)])
    cases.append(("self-loop at a branch node", loop, [b"AAAAAC", b"AAA", b"AAAA"]))
    cases.append(("self-loop alone", graph_of(["AA"], [(0, 0)]), [b"AAAAA", b"TTTT"]))
    # in-degree 2 only (AC ← AA, CA) and out-degree 2 only (CG → GA, GT)
    deg = graph_of(["AA", "CA", "AC", "CG", "GA", "GT"], [(0, 2), (1, 2), (2, 3), (3, 4), (3, 5)])
    cases.append(("in-degree 2 only, out-degree 2 only", deg, [b"AACGA", b"CACGT", b"AACG", b"ACGT", b"CAC"]))
    cases.append(("empty graph", ref.Graph([], []), [b"AACG", b"", b"X"]))
    cases.append(("nodes without edges", ref.Graph([0, 1], []), [b"AACG"]))
    cases.append(("empty batch", lin, []))
    return cases


# ---- the random sweep ------------------------------------------------------------------------------------------------------
SWEEP_SEEDS = range(40)


def random_case(seed: int, tile: int = 64):
    """→ (k, graph, reads, read_index, mate).  Node subsets of the (k−1)-mers, edges partly overlap-consistent and partly
    arbitrary, parallel edges, reverse-complement twins of some edges (two candidates under one key); reads are walks
    along the edges — consecutive edge k-mers joined by their overlap, by an N, or end to end — with substitutions, Ns,
    some reverse-complemented, a few with an invalid byte; lengths up to 3·tile."""
    rng = random.Random(9100 + seed)
    k = 4 + seed % 4
    nmask = (1 << (2 * (k - 1))) - 1
    subs = rng.sample(range(nmask + 1), rng.randint(4, 20))
    consistent = [(a, b) for a in range(len(subs)) for b in range(len(subs)) if (subs[a] & (nmask >> 2)) == (subs[b] >> 2)]
    edges = []
    for _ in range(rng.randint(3, 30)):
        if consistent and rng.random() < 0.5:
            edges.append(rng.choice(consistent))
        else:
            edges.append((rng.randrange(len(subs)), rng.randrange(len(subs))))
    for s, t in rng.sample(edges, min(len(edges), rng.randint(0, 4))):  # twins: the edge of the reverse complement
        y = ref.revcomp((subs[s] << 2) | (subs[t] & 3), k)
        ends = []
        for sub in (y >> 2, y & nmask):
            if sub not in subs:
                subs.append(sub)
            ends.append(subs.index(sub))
        edges.append(tuple(ends))
    for _ in range(rng.randint(0, 3)):  # links between edges that already exist, so that walks go on
        a, b = rng.choice(edges), rng.choice(edges)
        edges.append((a[1], b[0]))
    rng.shuffle(edges)
    g = ref.Graph(subs, edges)
    out_edges = {}
    for e, (s, _) in enumerate(edges):
        out_edges.setdefault(s, []).append(e)

    def kmer_str(e):
        return dec(ref.reconstruct_edge_kmer(g, e), k)

    reads = []
    for _ in range(rng.randint(8, 24)):
        want = rng.choice([k - 1, k, k + 1, tile, tile + k - 1, tile + k, 2 * tile + k, 3 * tile]) if rng.random() < 0.5 \
            else rng.randint(0, 3 * tile)
        e = rng.randrange(len(edges))
        s = kmer_str(e)
        while len(s) < want:
            nxt = out_edges.get(edges[e][1])
            if nxt and rng.random() < 0.9:
                e2 = rng.choice(nxt)
                how = rng.random()
                if how < 0.6 and kmer_str(e2)[:k - 1] == s[-(k - 1):] and "N" not in s[-(k - 1):]:
                    s += kmer_str(e2)[-1]
                elif how < 0.85:
                    s += "N" * rng.randint(1, 2) + kmer_str(e2)
                else:
                    s += kmer_str(e2)
                e = e2
            else:
                e = rng.randrange(len(edges))
                s += rng.choice(["", "N", "G"]) + kmer_str(e)
        b = bytearray(s[:max(want, 0)].encode())
        for i in range(len(b)):
            u = rng.random()
            if u < 0.01:
                b[i] = rng.choice(b"ACGT")
            elif u < 0.015:
                b[i] = ord("N")
        if rng.random() < 0.25:
            b = bytearray(rc_bytes(bytes(b)))
        if b and rng.random() < 0.08:
            b[rng.choice([0, len(b) - 1, rng.randrange(len(b))])] = rng.choice(b"XnaR-")
        reads.append(bytes(b))
    read_index = list(range(100, 100 + len(reads)))
    mate = [rng.choice([0, 1, 2]) if rng.random() < 0.2 else 1 + (i & 1) for i in range(len(reads))]
    return k, g, reads, read_index, mate
