"""Inputs of the retained-read tests (shk_retain_reads, shk_filter_reads_panel_retained, shk_thread_reads_panel_retained),
shared by the CPU test of the cases themselves (test_retained_cases_cpu.py) and the GPU tests
(test_gpu_retained_reads.py).  The expected value is never the library's: the oracle's KmerCounts.filter_matches per
gene and read for the filter (panel_cases.expected), tests/thread_ref.py per gene for the threading
(thread_panel_cases.expected).

A retained read cannot hold a byte outside ACGTN — the ingest that meets one poisons the context — so the cases that
come from panel_cases and thread_panel_cases have every such read replaced by an EMPTY read: the indices stay as they
are, and an empty read matches and supports nothing, like the invalid one.  Expectations are recomputed over the
substituted reads.

What the store adds to a walk is the read's first bit: a read may start at any bit of a word.  `splits` cuts a case's
reads into ingest calls and puts filler batches in front, so that its reads start at every kind of bit; the alignment
cases place a target's windows, an N, and the store's end against the word edges on purpose."""
from __future__ import annotations

import random
from collections import namedtuple

import panel_cases as pc
import thread_panel_cases as tp

T = pc.T
FILLERS = (0, 1, 63, 64, 65, 127, 129)  # bases retained in front of a target: it starts at bit 0, 1, 63, 0, 1, 63, 1 of a word
KS = (3, 21, 31)


def valid(read: bytes) -> bool:
    return all(c in b"ACGTN" for c in read)


def substitute(reads) -> tuple:
    """→ (the reads with every read that holds a byte outside ACGTN replaced by b"", how many were)."""
    out = [r if valid(r) else b"" for r in reads]
    return out, sum(1 for r in reads if not valid(r))


# ---- the filter's crafted cases and the threading panels, substituted --------------------------------------------------------
def filter_cases(orc) -> list:
    """panel_cases.crafted_cases, every one, with the substitution (claims dropped: they are about the original reads)."""
    return [c._replace(reads=substitute(c.reads)[0], claims=[]) for c in pc.crafted_cases(orc)]


def thread_panels() -> list:
    """The panels of thread_panel_cases, every one, with the substitution."""
    panels = [tp.crafted_panel(), tp.lists_panel(), tp.many_panel(), tp.twin_panel(), tp.twin_panel(True), tp.shared_read_panel(),
              tp.paired_panel()]
    panels += [tp.sweep_panel(seeds) for seeds in tp.sweep_groups()]
    return [p._replace(reads=substitute(p.reads)[0]) for p in panels]


def list_variants(p) -> list:
    """A panel as it is, with every list reversed, and with every list repeated (a read listed twice counts twice)."""
    return [p, p._replace(name=p.name + " (lists reversed)", lists=[ids[::-1] for ids in p.lists]),
            p._replace(name=p.name + " (lists twice)", lists=[list(ids) + list(ids) for ids in p.lists])]


# ---- how a case's reads reach the store ------------------------------------------------------------------------------------------
def filler_batches(total: int, seed: int = 0) -> list:
    """Batches of valid reads that hold `total` bases together: two calls where there is something to cut (an N in
    each piece that has room), one call with one empty read where there is not."""
    rng = random.Random(4100 + 7 * total + seed)
    seq = bytearray(rng.choice(b"ACGT") for _ in range(total))
    for at in range(5, total, 37):
        seq[at] = ord("N")
    seq = bytes(seq)
    if total < 2:
        return [[seq]]
    cut = total // 2
    return [[seq[:cut]], [seq[cut:cut + 1], seq[cut + 1:]]]


SPLITS = ("one call", "one read per call") + tuple(f"{f} bases in front" for f in FILLERS)


def splits(reads) -> list:
    """→ [(name, batches, n_front)]: the reads as one call, one read per call, and behind each of the filler patterns
    (n_front filler reads precede them in the store: a case's read i is retained read n_front + i)."""
    out = [(SPLITS[0], [list(reads)], 0), (SPLITS[1], [[r] for r in reads], 0)]
    for name, f in zip(SPLITS[2:], FILLERS):
        front = filler_batches(f)
        out.append((name, front + [list(reads)], sum(len(b) for b in front)))
    return out


def flat(batches) -> list:
    return [r for b in batches for r in b]


# ---- the alignment cases -----------------------------------------------------------------------------------------------------------
AlignCase = namedtuple("AlignCase", "name k filler genes batches at")  # at: where the reads its claims are about lie (retained indices)


def straddler(k: int) -> int:
    """A window start whose k bases lie in two wave steps, other than window 63."""
    return T + 1 - k


def n_padded(total: int, w: int, kmer: bytes) -> bytes:
    """A read of `total` bases whose only window without an N is the one at w: kmer there, N everywhere else."""
    return b"N" * w + kmer + b"N" * (total - w - len(kmer))


def alignment_cases(orc) -> list:
    cases = []
    for k in KS:
        X = {3: b"ACG", 21: pc.rand_seq(31, 21), 31: pc.rand_seq(32, 31)}[k]
        long = 2 * T + k  # bases of a read of 2T + 1 windows
        hits = [0, T - 1, T, 2 * T, straddler(k)]
        for f in FILLERS:
            front = filler_batches(f, seed=k)
            n_front = sum(len(b) for b in front)
            at = {}
            reads = []

            def add(name, read):
                at[name] = n_front + len(reads)
                reads.append(read)

            # the first target starts at bit f: an N at bit 63 of a word and at bit 0 of the next
            edge = ((f + 1 + 63) // 64) * 64  # the first word edge that has a base of this read in front of it
            S = bytearray(pc.rand_seq(40 + k + f, long))
            S[edge - 1 - f] = S[edge - f] = ord("N")
            add("n_at_edge", bytes(S))
            add("empty_middle", b"")
            add("len_k-1", X[:k - 1])
            add("len_k", X)
            add("len_k+1", X + b"G")
            add("len_64", pc.rand_seq(50 + k + f, 64))
            add("64_windows", pc.rand_seq(51 + k + f, 64 + k - 1))
            for w in hits:
                add(f"only_hit_{w}", n_padded(long, w, X))
            add("no_hit", n_padded(long, T, X[:k // 2] + b"N" + X[k // 2 + 1:]))
            R = pc.rand_seq(60 + k, long)
            add("R", R)
            add("R_rc", pc.rc_bytes(R))
            # the last bases of the store end at a word edge, the hit in the last window; an empty read is last
            so_far = f + sum(len(r) for r in reads)
            pad = (-(so_far + k)) % 64 + 64
            end = pc.rand_seq(70 + k + f, pad) + X
            batches = front + [reads[:]]
            at["ends_at_edge"] = n_front + len(reads)
            batches.append([end])
            at["empty_last"] = at["ends_at_edge"] + 1
            batches.append([b""])
            km = lambda s, w: orc.kmers_from_ascii(s[w:w + k], k)[0]  # noqa: E731
            genes = [[km(X, 0)]]                                       # 0: the planted k-mer
            genes += [[km(R, w)] for w in hits]                        # 1-5: one window of R each (k >= 21: R holds it once)
            genes.append([km(bytes(S), edge - f + 1), km(bytes(S), long - k)])  # 6: the window just behind the two N, and S's last
            genes.append([])                                           # 7: an empty gene
            cases.append(AlignCase(f"k={k}, {f} bases in front", k, f, genes, batches, at))
    return cases


def align_expected(orc, case: AlignCase) -> list:
    return pc.expected(orc, pc.Case(case.name, case.k, case.genes, flat(case.batches), []))


# ---- a big shuffled batch of valid kinds: persistent waves walk several reads each -------------------------------------------------
def big_valid_batch(orc):
    """→ (k, genes, reads, rows) on the pattern of panel_cases.stride_batch, with the kinds that hold an invalid byte left
    out: 40000 reads in pseudo-random order, the expected rows by the oracle per KIND."""
    import numpy as np
    k, genes, kinds, kind_genes, order = pc.stride_batch(orc)
    keep = [j for j, r in enumerate(kinds) if valid(r)]
    assert len(keep) == len(kinds) - 2
    order = np.asarray(keep)[np.random.default_rng(5).integers(0, len(keep), size=pc.STRIDE_READS)]
    rows = [np.flatnonzero(np.isin(order, [j for j in keep if g in kind_genes[j]])).tolist() for g in range(len(genes))]
    return k, genes, [kinds[j] for j in order.tolist()], rows
