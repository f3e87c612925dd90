"""One small batch per k that all four read walkers are held to — k_filter_reads, k_kmers_from_reads, k_thread_panel and
k_filter_panel — shared by the CPU test of the batch itself (test_read_walk_cases_cpu.py) and the GPU test
(test_gpu_read_walk.py).  The reads sit where the pieces the walkers share can go wrong: the 64-window step of the two
wave-per-read kernels, an N or an invalid byte either side of it, the first and the last window of a read.

A read is built from a background sequence and a MARKER k-mer: the lookup set holds the marker's canonical k-mer (and a
decoy no read has), so a read hits the set exactly where a marker was put.  The marker ends in an A, the base an N
decodes to when its N bit is lost.  batch(orc, k) → Batch(k, set_kmers, reads, names, claims); a claim says what a
read is there for, in a form the CPU test checks against the oracle:
    ("hits", read, positions)     the window start positions of the read whose k-mer is in the set
    ("byte", read, position, b)   reads[read][position] == b
    ("valid", read, bool)         whether every byte of the read is one of ACGTN
    ("match", read, bool)         whether the read matches the set (PrimerReadFilter::matches)
    ("healed", read, position, b, positions)  with byte `position` replaced by b the read hits at `positions`"""
from __future__ import annotations

import random
from collections import namedtuple

T = 64  # windows per wave step of k_thread_panel and k_filter_panel
KS = (3, 21, 31)
LONG = 200
COMP = bytes.maketrans(b"ACGTN", b"TGCAN")
Batch = namedtuple("Batch", "k set_kmers reads names claims marker")
_cache = {}


def rc_bytes(s: bytes) -> bytes:
    return s[::-1].translate(COMP)


def put(read: bytes, at: int, b: bytes) -> bytes:
    assert 0 <= at and at + len(b) <= len(read)
    return read[:at] + b + read[at + len(b):]


def lengths(k: int) -> list:
    return [0, k - 1, k, k + 1, T - 1, T, T + 1, T + k - 2, T + k - 1, T + k, 2 * T - 1, 2 * T, 2 * T + 1, LONG]


def hit_positions(orc, have: set, seq: bytes, k: int) -> list:
    """Window starts of seq whose window has no N and whose canonical k-mer is in `have` (whatever else seq holds)."""
    out = []
    for w in range(len(seq) - k + 1):
        win = seq[w:w + k]
        if all(c in b"ACGT" for c in win) and orc.kmers_from_ascii(win, k)[0] in have:
            out.append(w)
    return out


def batch(orc, k: int) -> Batch:
    if k in _cache:
        return _cache[k]
    rng = random.Random(4200 + k)
    # k = 3: a background over A and C alone, so that the marker CGA (reverse complement TCG) is in no background window
    alphabet = b"AC" if k == 3 else b"ACGT"
    marker = b"CGA" if k == 3 else b"C" + bytes(rng.choice(b"ACGT") for _ in range(k - 2)) + b"A"
    decoy = b"GGC" if k == 3 else bytes(rng.choice(b"ACGT") for _ in range(k))

    def bg(n: int) -> bytes:
        return bytes(rng.choice(alphabet) for _ in range(n))

    reads, names, claims = [], [], []

    def add(name: str, read: bytes, *cl) -> int:
        reads.append(read)
        names.append(name)
        claims.extend((c[0], len(reads) - 1) + tuple(c[1:]) for c in cl)
        return len(reads) - 1

    # ---- every length at which a walker takes another path; the only hit is the LAST window
    for n in lengths(k):
        if n >= k:
            add(f"length {n}, marker in the last window", put(bg(n), n - k, marker), ("hits", [n - k]), ("match", True))
        else:
            add(f"length {n}: no window", bg(n), ("hits", []), ("match", False))
    # ---- the only set k-mer at window 63, at window 64, and in the last window; the reverse strand; no hit at all
    for w in (T - 1, T, LONG - k):
        add(f"only set k-mer at window {w}", put(bg(LONG), w, marker), ("hits", [w]), ("match", True))
    add("reverse complement of a read with the marker at window 64", rc_bytes(put(bg(LONG), T, marker)),
        ("hits", [LONG - k - T]), ("match", True))
    add("no set k-mer", bg(LONG), ("hits", []), ("match", False))
    # ---- an N either side of the step's edge and as the last byte: in place of the marker's final A (the window is no
    #      k-mer; read as an A it would hit), and on the byte next to the marker (the hit stays)
    for p in (T - 2, T - 1, T, T + 1, LONG - 1):
        inside = put(put(bg(LONG), p - k + 1, marker), p, b"N")
        add(f"N at {p}, the marker's last byte", inside, ("byte", p, b"N"), ("hits", []), ("match", False),
            ("healed", p, b"A", [p - k + 1]))
        at = p + 1 if p + 1 + k <= LONG else p - k
        add(f"N at {p}, next to the marker at {at}", put(put(bg(LONG), at, marker), p, b"N"), ("byte", p, b"N"), ("hits", [at]),
            ("match", True))
    # ---- an invalid byte: markers before it and behind it hit, and the read as a whole is refused
    m_lo, m_hi = 5, T + k + 5  # (clear of every position below)
    for p, b in ((0, b"X"), (T - 1, b"x"), (T, b"-"), (T + k - 1, b"n"), (LONG - 1, b"@")):
        good = put(put(bg(LONG), m_lo, marker), m_hi, marker)
        add(f"invalid byte {b!r} at {p}", put(good, p, b), ("byte", p, b), ("valid", False), ("match", False),
            ("healed", p, good[p:p + 1], [m_lo, m_hi]))
    good = put(put(bg(LONG), m_lo, marker), m_hi, marker)
    add("lower case", good.lower(), ("valid", False), ("match", False))
    add("the same read in upper case", good, ("valid", True), ("hits", [m_lo, m_hi]), ("match", True))
    add("all N", b"N" * (T + k), ("valid", True), ("hits", []), ("match", False))

    set_kmers = sorted({orc.kmers_from_ascii(marker, k)[0], orc.kmers_from_ascii(decoy, k)[0]})
    _cache[k] = Batch(k, set_kmers, reads, names, claims, marker)
    return _cache[k]


def expected_matches(orc, b: Batch, set_kmers=None) -> list:
    """PrimerReadFilter::matches per read, by the oracle."""
    kc = orc.KmerCounts(b.k)
    for x in (b.set_kmers if set_kmers is None else set_kmers):
        kc.insert(int(x), 1)
    return [bool(kc.filter_matches(r)) for r in b.reads]


def expected_kmers(orc, b: Batch) -> list:
    """kmers_from_ascii per read, by the oracle → (k-mers, 0), or ([], the first byte outside ACGTN)."""
    out = []
    for r in b.reads:
        bad = [c for c in r if c not in b"ACGTN"]
        out.append(([], bad[0]) if bad else (orc.kmers_from_ascii(r, b.k), 0))
    return out


def linear_graph(b: Batch):
    """→ (node sub_kmers, edges, edge k-mers as bytes, the first edge's window): the chain of the windows either side of the step's edge of the
    "only set k-mer at window 64" read — one node per (k−1)-mer position, so equal (k−1)-mers are different nodes and
    equal k-mers (at k = 3 there are some) are several candidates of one key."""
    read = b.reads[b.names.index(f"only set k-mer at window {T}")]
    w0, n_edges = (T - 4, 8) if b.k == 3 else (T - 24, 40)
    code = {c: i for i, c in enumerate(b"ACGT")}

    def enc(s: bytes) -> int:
        v = 0
        for c in s:
            v = (v << 2) | code[c]
        return v

    nodes = [enc(read[w0 + i:w0 + i + b.k - 1]) for i in range(n_edges + 1)]
    edges = [(i, i + 1) for i in range(n_edges)]
    return nodes, edges, [read[w0 + i:w0 + i + b.k] for i in range(n_edges)], w0
