"""Crafted tables for shk_neighborhood and shk_pcr_extend: shapes that reads of a random genome never produce, built
k-mer by k-mer for `KmerEngine.insert` (tests/test_gpu_nb_edges.py) — levels of exactly 1023, 1024, 1025 and 2049
entries around the hand-over between the one-workgroup kernel and the wide one, complete de Bruijn graphs, counts that
meet a threshold only as a saturating sum over chunk lanes, a zero-count key in the middle of a chain.  Pure Python.

Every builder returns a `Case`: (k, chunks, inserts, seeds, dirs, sizes, …) with inserts = [(chunk_id, canonical k-mers,
counts)] and sizes = the level sizes the case was DESIGNED to have at its min_count, written down from the construction
and not computed.  tests/test_pcr_ref_cpu.py checks each against pcr_ref.neighborhood_levels, so a GPU comparison on
one of these tables is a comparison at the designed shape."""
from __future__ import annotations

import random
from typing import NamedTuple

import pcr_ref as ref

U32_MAX = 0xFFFFFFFF
NARROW = 1024  # the level size up to which one workgroup carries the search (NB_NARROW, csrc/shk_device.hip.h)


class Case(NamedTuple):
    k: int
    chunks: int
    inserts: list      # [(chunk_id, canonical k-mers, counts)]
    seeds: list        # nodes: (k−1)-mers
    dirs: list
    sizes: list        # designed level sizes at min_count
    min_count: int = 1
    name: str = ""
    hand_over: int = 0  # the level at which the search changes kernels (chains)
    heads: tuple = ()   # first oriented k-mer of every chain / last one: the primer sets of the pcr_extend cases
    tails: tuple = ()


def canonical(x: int, k: int) -> int:
    return min(x, ref.revcomp(x, k))


def merged_table(inserts) -> dict:
    """What shk_lookup(canonical = 1) sees after these inserts: per key the saturating sum over everything inserted
    (KmerCounts::insert saturates, and so does the sum over lanes); a key inserted with count 0 is there with 0."""
    t = {}
    for _, keys, counts in inserts:
        for x, c in zip(keys, counts):
            t[int(x)] = min(t.get(int(x), 0) + int(c), U32_MAX)
    return t


# ---- 1. disjoint random chains: level sizes to order ------------------------------------------------------------

def _walk(rng, k, node, n_steps, not_base=None):
    """n_steps steps forward from `node` over random bases → (nodes after each step, oriented k-mers, first base)."""
    mask = (1 << (2 * (k - 1))) - 1
    nodes, kmers, first = [], [], None
    for i in range(n_steps):
        b = rng.randrange(4)
        while i == 0 and b == not_base:
            b = rng.randrange(4)
        first = b if i == 0 else first
        x = (node << 2) | b
        node = x & mask
        nodes.append(node)
        kmers.append(x)
    return nodes, kmers, first


def _chains(rng, k, lengths, forks=()):
    """Chain i: a path of lengths[i] nodes walked forward from a random head, so it has an entry in levels
    0 … lengths[i] − 1.  forks: (chain, level, n) — the chain's node of that level gets a second successor, the head of a
    branch of n nodes (levels level + 1 … level + n).  Counts 1..6 per k-mer.  → (heads, oriented k-mers, their
    counts, first and last oriented k-mer of every chain)."""
    mask = (1 << (2 * (k - 1))) - 1
    heads, kmers, firsts, lasts, paths = [], [], [], [], []
    for n in lengths:
        head = rng.randrange(mask + 1)
        nodes, xs, first = _walk(rng, k, head, n - 1)
        heads.append(head)
        kmers += xs
        paths.append(([head] + nodes, xs))
        if xs:
            firsts.append(xs[0])
            lasts.append(xs[-1])
    for chain, level, n in forks:
        nodes, xs = paths[chain]
        taken = xs[level] & 3  # the base the chain itself goes on with
        _, bx, _ = _walk(rng, k, nodes[level], n, not_base=taken)
        kmers += bx
        lasts.append(bx[-1])
    counts = [rng.randint(1, 6) for _ in kmers]
    return heads, kmers, counts, tuple(firsts), tuple(lasts)


# generator seeds: the first from 1 at which the CPU size check passes (no two chains meet, no chain's end finds a
# k-mer of another): tests/test_pcr_ref_cpu.py::test_crafted_cases_have_their_designed_level_sizes
CHAIN_RNG_SEED = 14
CHAIN_K = 15


def _chain_case(name, lengths, forks, sizes, hand_over):
    k = CHAIN_K
    rng = random.Random("%d %s" % (CHAIN_RNG_SEED, name))
    heads, kmers, counts, firsts, lasts = _chains(rng, k, lengths, forks)
    return Case(k, 1, [(0, [canonical(x, k) for x in kmers], counts)], heads, [1] * len(heads), sizes, 1, name,
                hand_over, firsts, lasts)


def flat(n):
    """n chains of 6 levels: every level has exactly n entries."""
    return _chain_case("flat%d" % n, [6] * n, (), [n] * 6, 0)


def falling():
    """1025 chains of 5 levels, one ending after 2 and one after 4: 1025, 1025, 1024, 1024, 1023 — the wide kernel hands
    level 2 over to the narrow one."""
    return _chain_case("falling", [2, 4] + [5] * 1023, (), [1025, 1025, 1024, 1024, 1023], 2)


def rising():
    """1023 chains of 4 levels; one forks at level 1 and another at level 2: 1023, 1023, 1024, 1025 — the narrow kernel
    meets a next level of exactly 1024 (it goes on) and then one of 1025 (it hands over)."""
    return _chain_case("rising", [4] * 1023, ((0, 1, 2), (1, 2, 1)), [1023, 1023, 1024, 1025], 3)


def zigzag():
    """One seed without a k-mer, 1023 chains of 5 levels and one of 4; the first chain forks at level 1 into a branch of
    one node: 1025, 1024, 1025, 1024, 1023 — level 0 is the wide kernel's, level 1 fits a workgroup, level 2 is wide
    again and level 3 goes back: the hand-over in both directions, twice."""
    return _chain_case("zigzag", [1] + [5] * 1023 + [4], ((1, 1, 1),), [1025, 1024, 1025, 1024, 1023], 2)


# ---- 2. complete de Bruijn graphs ---------------------------------------------------------------------------------

def canonical_kmers(k):
    return [x for x in range(1 << (2 * k)) if x <= ref.revcomp(x, k)]


def dense(k, every_node):
    """Every canonical k-mer, counts 1..4.  One seed — the homopolymer node, forward: level i ≥ 1 is the nodes whose
    longest prefix of A is k − 1 − i long, 3·4^(i−1) of them — or every node both ways: one level, 2·4^(k−1)."""
    rng = random.Random(1000 + k)
    keys = canonical_kmers(k)
    counts = [rng.randint(1, 4) for _ in keys]
    if every_node:
        n = 1 << (2 * (k - 1))
        seeds, dirs, sizes = list(range(n)), [3] * n, [2 * n]
    else:
        seeds, dirs, sizes = [0], [1], [1] + [3 * 4 ** (i - 1) for i in range(1, k)]
    return Case(k, 1, [(0, keys, counts)], seeds, dirs, sizes, 1, "dense k=%d %s" % (k, "every node" if every_node else "one seed"))


def growth_inserts(k=7, n=300_000):
    """What grows the table under a dense case: n inserts of keys no canonical lookup can reach — the NON-canonical
    k-mers (at k = 7 there is no other key left).  → one (chunk_id, k-mers, counts)."""
    rng = random.Random(77)
    other = [x for x in range(1 << (2 * k)) if x > ref.revcomp(x, k)]
    return (0, [other[rng.randrange(len(other))] for _ in range(n)], [rng.randint(1, 3) for _ in range(n)])


# ---- 3. thresholds met over lanes ---------------------------------------------------------------------------------

LANES_K, LANES_CHUNKS, LANES_MIN = 21, 3, 9


def _lanes_table():
    k = LANES_K
    rng = random.Random(2100)
    heads, kmers, _, firsts, lasts = _chains(rng, k, [6, 6, 5, 6], ())
    a, b, s, z = kmers[0:5], kmers[5:10], kmers[10:14], kmers[14:19]
    at = [(4, 4, 1), (1, 4, 4), (3, 3, 3), (8, 0, 1), (2, 2, 5)]     # each lane < 9, Σ = 9
    below = [(4, 3, 1), (1, 3, 4), (3, 3, 2), (8, 0, 0), (2, 2, 4)]  # Σ = 8
    sat = [(U32_MAX - 5, 10, 0), (1 << 31, 1 << 31, 1 << 31), ((1 << 31) - 1, (1 << 31) - 1, 0), (0, 1, 0)]
    zero = [(5, 0, 0), (0, 5, 0), (0, 0, 0), (0, 0, 5), (5, 0, 0)]   # the middle key: inserted, with count 0
    lanes = [([], []) for _ in range(LANES_CHUNKS)]
    for xs, split in ((a, at), (b, below), (s, sat), (z, zero)):
        for x, parts in zip(xs, split):
            for lane, c in enumerate(parts):
                if c or parts == (0, 0, 0) and lane == 1:
                    lanes[lane][0].append(canonical(x, k))
                    lanes[lane][1].append(c)
    tails = [x & ((1 << (2 * (k - 1))) - 1) for x in lasts]
    return [(i, ks, cs) for i, (ks, cs) in enumerate(lanes)], heads, tails


def lanes():
    """Four chains at k 21 over 3 lanes → the cases that read them: A's counts reach 9 only summed and B's stop at 8; S
    holds two counts that saturate over lanes, then 2^32 − 2, then 1; Z has a key of count 0 in the middle."""
    ins, (ha, hb, hs, hz), (ta, tb, _, _) = _lanes_table()
    mk = lambda name, seeds, dirs, mc, sizes: Case(LANES_K, LANES_CHUNKS, ins, seeds, dirs, sizes, mc, "lanes: " + name)
    return [mk("sum meets the threshold", [ha, hb], [1, 1], LANES_MIN, [2, 1, 1, 1, 1, 1]),
            mk("one below it takes both", [ha, hb], [1, 1], LANES_MIN - 1, [2] * 6),
            mk("backwards from the tails", [ta, tb], [2, 2], LANES_MIN, [2, 1, 1, 1, 1, 1]),
            mk("u32::MAX accepts the saturated sums", [hs], [1], U32_MAX, [1, 1, 1]),
            mk("u32::MAX - 1 takes 2^32 - 2 too", [hs], [1], U32_MAX - 1, [1, 1, 1, 1]),
            mk("a zero count stops the walk", [hz], [1], 1, [1, 1, 1]),
            mk("min_count 0 reads as 1", [hz], [1], 0, [1, 1, 1])]


def _lanes_case(i):
    return lambda: lanes()[i]


# name → builder (built when asked for: a test module's collection stays cheap)
CASES = {"flat%d" % n: (lambda n=n: flat(n)) for n in (1023, 1024, 1025, 2049)}
CASES.update(falling=falling, rising=rising, zigzag=zigzag)
CASES.update({"dense%d_%s" % (k, "all" if e else "one"): (lambda k=k, e=e: dense(k, e)) for k in (2, 3, 4, 5, 6, 7) for e in (False, True)})
CASES.update({"lanes%d" % i: _lanes_case(i) for i in range(7)})
