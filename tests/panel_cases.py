"""Inputs of the panel read filter's tests (shk_filter_reads_panel), shared by the CPU test of the cases themselves
(test_panel_cases_cpu.py) and the GPU tests (test_gpu_filter_panel.py).  The expected value is always the oracle's
KmerCounts.filter_matches — PrimerReadFilter::matches (pcr/read_filter.rs:43-49) — per gene and per read.

A case is a Case(name, k, genes, reads, claims): genes are lists of canonical k-mers, reads are bytes, and every claim
says what the case is there to exercise, in a form the CPU test checks against the oracle:
    ("windows", read, n)             read has n windows (len − k + 1)
    ("hits", gene, seq, positions)   the window start positions of seq (bytes, or a read index) whose k-mer is in gene
    ("match", gene, read, bool)      whether read matches gene
    ("straddles", position)          the window at that position spans bytes of two wave steps
    ("byte", read, position, b)      read[position] == b
    ("rows", lists)                  the whole expected answer
A hit position is a window START, the kernel's sense (lane l of step s looks at the window starting at 64·s + l)."""
from __future__ import annotations

import random
from collections import namedtuple

import numpy as np

T = 64  # windows per wave step of k_filter_panel
WORD_EDGES = (0, 31, 32, 63, 64, 95, 96, 127, 128, 2047, 2048)  # genes either side of a bitmap word's edge, and of the 64-word round's
COMP = bytes.maketrans(b"ACGTN", b"TGCAN")
Case = namedtuple("Case", "name k genes reads claims")


def rc_bytes(s: bytes) -> bytes:
    return s[::-1].translate(COMP)


def rand_seq(seed: int, n: int) -> bytes:
    rng = random.Random(7700 + seed)
    return bytes(rng.choice(b"ACGT") for _ in range(n))


def put(read: bytes, at: int, b: bytes) -> bytes:
    return read[:at] + b + read[at + 1:]


def hit_positions(orc, gene, seq: bytes, k: int) -> list:
    """Window starts of seq whose window has no N and whose canonical k-mer is in gene (no matter what else seq holds)."""
    have = set(int(x) for x in gene)
    out = []
    for w in range(len(seq) - k + 1):
        win = seq[w:w + k]
        if all(c in b"ACGT" for c in win) and orc.kmers_from_ascii(win, k)[0] in have:
            out.append(w)
    return out


def expected(orc, case) -> list:
    """Per gene, the reads filter_reads keeps (read_filter.rs:52-54), by the oracle."""
    rows = []
    for gene in case.genes:
        kc = orc.KmerCounts(case.k)
        for x in gene:
            kc.insert(int(x), 1)
        rows.append([i for i, r in enumerate(case.reads) if kc.filter_matches(r)])
    return rows


def crafted_cases(orc) -> list:
    cases = []

    def km(seq: bytes, k: int, at: int) -> int:
        return orc.kmers_from_ascii(seq[at:at + k], k)[0]

    # ---- k = 3 and k = 5: minimal reads ------------------------------------------------------------------------------------
    for k, a, b in ((3, b"AAC", b"CGT"), (5, b"AACGA", b"CGTTC")):
        genes = [[km(a, k, 0)], [km(b, k, 0)]]
        reads = [b"", a[:k - 1], a, a + b"G", b"N" * (k + 1), rc_bytes(a), b, rc_bytes(b), b"T" * (k + 1), a[:k - 1] + b"N" + a[k - 1:]]
        claims = [("windows", 0, 1 - k), ("windows", 1, 0), ("windows", 2, 1), ("windows", 3, 2),
                  ("match", 0, 2, True), ("match", 0, 5, True), ("match", 1, 7, True), ("match", 0, 4, False), ("match", 0, 9, False)]
        cases.append(Case(f"k={k}: lengths 0, k-1, k, k+1, all N, reverse complements", k, genes, reads, claims))

    # ---- k = 21: the wave step's boundaries ----------------------------------------------------------------------------------
    k = 21
    S = rand_seq(1, 300)
    cut = lambda n_win, at=0: S[at:at + n_win + k - 1]  # noqa: E731
    R = cut(2 * T + 1)
    at = [0, T - 1, T, 2 * T, 50, T - 2]  # gene g holds the k-mer of window at[g] alone
    genes = [[km(R, k, w)] for w in at]
    reads = [cut(T - 1), cut(T), cut(T + 1), R, rc_bytes(R)]
    claims = [("windows", 0, T - 1), ("windows", 1, T), ("windows", 2, T + 1), ("windows", 3, 2 * T + 1)]
    claims += [("hits", g, 3, [w]) for g, w in enumerate(at)]          # the only hit at window 0, 63, 64, the last
    claims += [("hits", 5, 0, [T - 2]), ("hits", 1, 1, [T - 1]), ("hits", 2, 2, [T])]  # … and each shorter read's last window
    claims += [("straddles", 50), ("match", 3, 2, False), ("match", 2, 1, False), ("match", 0, 4, True), ("match", 3, 4, True)]
    cases.append(Case("k=21: reads of T-1, T, T+1, 2T+1 windows; the only hit at window 0, 63, 64, last, straddling", k, genes, reads, claims))

    # ---- an N inside the would-be hit window, and just outside it ------------------------------------------------------------
    genes = [[km(R, k, 30)]]
    reads = [R, put(R, 40, b"N"), put(R, 30, b"N"), put(R, 50, b"N"), put(R, 29, b"N"), put(R, 51, b"N")]
    claims = [("hits", 0, 0, [30])] + [("byte", i, p, b"N") for i, p in ((1, 40), (2, 30), (3, 50), (4, 29), (5, 51))]
    claims += [("match", 0, i, i in (0, 4, 5)) for i in range(6)]
    cases.append(Case("k=21: an N inside the hit window (first, middle, last byte) and just outside it", k, genes, reads, claims))

    # ---- an invalid byte ----------------------------------------------------------------------------------------------------
    L = S[:260]  # 240 windows, four steps; its hit is in the first
    genes = [[km(R, k, 5)]]
    reads = [R, put(R, 2, b"X"), put(R, 40, b"x"), put(R, 100, b"-"), put(R, len(R) - 1, b"X"), L, put(L, len(L) - 1, b"X"),
             b"ACGTX", b"ACGT", put(R, 5, b"n")]
    claims = [("hits", 0, R, [5]), ("hits", 0, L, [5]), ("windows", 5, 240), ("windows", 7, 5 - k + 1)]
    claims += [("byte", 1, 2, b"X"), ("byte", 2, 40, b"x"), ("byte", 3, 100, b"-"), ("byte", 4, len(R) - 1, b"X"),
               ("byte", 6, len(L) - 1, b"X"), ("byte", 7, 4, b"X")]
    claims += [("match", 0, i, i in (0, 5)) for i in range(10)]
    cases.append(Case("k=21: an invalid byte before the hit, after it in its step, in the last step, in a read shorter than k",
                      k, genes, reads, claims))

    # ---- several genes ---------------------------------------------------------------------------------------------------------
    D = rand_seq(2, 200)  # decoys: k-mers no read of S has
    shared = km(R, k, 77)
    genes = [[km(R, k, 3)], [km(R, k, 70), shared], [], [km(R, k, 100), km(R, k, 100), shared], [km(D, k, 0), shared], [km(D, k, 9)]]
    reads = [R, cut(10, 70), cut(5, 200), rc_bytes(cut(8, 95))]
    claims = [("rows", [[0], [0, 1], [], [0, 1, 3], [0, 1], []])]
    cases.append(Case("k=21: a read in three genes, a k-mer in three genes, a duplicate k-mer, an empty gene between two others",
                      k, genes, reads, claims))
    genes = [[km(D, k, w) for w in range(0, 60, 7)], [], [km(D, k, 100)]]
    cases.append(Case("k=21: no read matches anything", k, genes, [R, cut(T), rc_bytes(R), b"", b"N" * 30],
                      [("rows", [[], [], []])]))

    # ---- the bitmap's word edges: the only matching gene first, last and either side of every 32 ----------------------------
    # (4096 is the limit: beyond 2048 genes the lanes walk a wave's bitmap in two rounds of 64 words)
    D2 = rand_seq(4, 4096 + k)
    for n_genes in (1, 64, 65, 130, 4096):
        where = sorted(set(p for p in WORD_EDGES + (n_genes - 1,) if p < n_genes))
        reads = [rand_seq(100 + j, 40) for j in range(len(where))]  # read j matches gene where[j] alone
        genes = [[km(D2, k, g)] for g in range(n_genes)]
        for j, g in enumerate(where):
            genes[g] = [km(reads[j], k, j)]
        rows = [[] for _ in range(n_genes)]
        for j, g in enumerate(where):
            rows[g] = [j]
        cases.append(Case(f"k=21: {n_genes} genes, the only matching gene at {where}", k, genes, reads, [("rows", rows)]))

    # ---- k = 31 and k = 2 ------------------------------------------------------------------------------------------------------
    k = 31
    Q = rand_seq(3, 100)
    genes = [[km(Q, k, 0)], [km(Q, k, 69)], [km(Q, k, T - k + 5)]]
    reads = [Q, rc_bytes(Q), Q[:99], Q[1:], put(Q, 50, b"N")]
    claims = [("windows", 0, 70), ("hits", 0, 0, [0]), ("hits", 1, 0, [69]), ("hits", 2, 0, [T - k + 5]), ("straddles", T - k + 5),
              ("rows", [[0, 1, 2, 4], [0, 1, 3, 4], [0, 1, 2, 3]])]
    cases.append(Case("k=31: first, last and a straddling window", k, genes, reads, claims))
    k = 2
    genes = [[km(b"AC", k, 0)], [km(b"AA", k, 0)]]
    reads = [b"AC", b"A", b"CAC", b"NN", b"GT", b"TT", b"ANC", b"ACX", b"G" * 70 + b"TT"]
    claims = [("rows", [[0, 2, 4, 8], [5, 8]]), ("windows", 8, 71)]
    cases.append(Case("k=2", k, genes, reads, claims))
    return cases


# ---- the batch of test_filter_reads_matches_reference_semantics (test_gpu_parity.py) and a panel cut from it -------------------
_big = {}


def big_batch(orc, k: int):
    """→ (seqs, single, genes, rows): the 3003 reads of that test (3000 synthetic, 40 of them with an X; an empty one, one
    shorter than k, one all N), its primer set `single`, a 12-gene panel cut from the same reads, and the oracle's answer
    for the panel."""
    if k not in _big:
        import sharkmer_amd as sa
        spec = sa.SynthSpec(genome_len=50_000, sub_per_64k=200, n_per_64k=100)
        bases, offsets = sa.synth_reads(spec, 0, 3_000)
        bases = bases.copy()
        rng = np.random.default_rng(k)
        for r in rng.choice(3_000, size=40, replace=False):
            bases[int(offsets[r]) + int(rng.integers(0, 150))] = ord("X")
        seqs = [bytes(bases[int(offsets[i]):int(offsets[i + 1])]) for i in range(3_000)]
        seqs += [b"", b"ACG", b"N" * 40]
        primers = orc.KmerCounts(k)
        for r in rng.choice(3_000, size=25, replace=False):
            if b"X" not in seqs[r]:
                primers.ingest_seq(seqs[r][20:20 + k + 6])
        single, _ = primers.export()
        genes, tables = [], []
        for r in rng.choice(3_000, size=30, replace=False):
            if b"X" in seqs[r] or len(genes) == 12:
                continue
            kc = orc.KmerCounts(k)
            kc.ingest_seq(seqs[r][20:20 + k + 6])
            if len(kc):
                genes.append(kc.export()[0])
                tables.append(kc)
        assert len(genes) == 12
        rows = [[i for i, s in enumerate(seqs) if kc.filter_matches(s)] for kc in tables]
        _big[k] = (seqs, single, genes, rows)
    return _big[k]


# ---- a batch that gives every wave of the kernel many reads, one after the other ------------------------------------------------
STRIDE_READS = 40_000  # the kernel's grid is at most 2 workgroups of 16 waves on each of 256 CUs: 8192 waves
STRIDE_GENES = 70
_stride = {}


def stride_batch(orc):
    """→ (k, genes, kinds, kind_genes, order): reads[i] = kinds[order[i]], a pseudo-random sequence of a few kinds of
    read, so that the reads a wave walks one after the other (i, i + n_waves, …) differ in every way that matters to the
    state it carries: hits in several bitmap words, a hit cancelled by an invalid byte steps later, no hit at all, no
    window at all.  kind_genes[j] = the genes kind j matches, by the oracle."""
    if not _stride:
        k = 21
        a, b, e, h = (rand_seq(200 + j, 40) for j in range(4))
        tail = rand_seq(210, 110)
        kinds = [a,                                # 0: genes 0, 33 and 69 — three words of the bitmap
                 b,                                # 1: genes 31 and 32 — either side of a word edge
                 put(a + tail, 140, b"X"),         # 2: kind 0's hits in the first step, an invalid byte in the third: nothing
                 rand_seq(220, 40),                # 3: no hit
                 e,                                # 4: gene 64
                 put(b + tail, 149, b"x"),         # 5: kind 1's hits, then an invalid last byte: nothing
                 b"", b"ACGT", b"N" * 40,          # 6, 7, 8: no window, or none without an N
                 tail + h,                         # 9: gene 5, hit in the last step only
                 a + tail]                         # 10: kind 2 without the invalid byte
        D = rand_seq(230, STRIDE_GENES + k)
        genes = [[km_of(orc, D, k, g)] for g in range(STRIDE_GENES)]
        genes[0], genes[33], genes[69] = [km_of(orc, a, k, 0)], [km_of(orc, a, k, 7)], [km_of(orc, a, k, 19), km_of(orc, a, k, 0)]
        genes[31], genes[32] = [km_of(orc, b, k, 3)], [km_of(orc, b, k, 3), km_of(orc, b, k, 11)]
        genes[64], genes[5] = [km_of(orc, e, k, 10)], [km_of(orc, h, k, 15)]
        rows = expected(orc, Case("stride", k, genes, kinds, []))
        kind_genes = [[g for g in range(STRIDE_GENES) if j in rows[g]] for j in range(len(kinds))]
        order = np.random.default_rng(3).integers(0, len(kinds), size=STRIDE_READS)
        _stride["v"] = (k, genes, kinds, kind_genes, order)
    return _stride["v"]


def km_of(orc, seq: bytes, k: int, at: int) -> int:
    return orc.kmers_from_ascii(seq[at:at + k], k)[0]


def stride_rows(orc) -> list:
    """The expected answer for the stride batch: per gene the positions of the kinds that match it."""
    k, genes, kinds, kind_genes, order = stride_batch(orc)
    return [np.flatnonzero(np.isin(order, [j for j in range(len(kinds)) if g in kind_genes[j]])).tolist() for g in range(len(genes))]
