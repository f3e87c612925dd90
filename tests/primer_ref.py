"""get_primer_kmers (src/pcr/primers.rs:234-480) restated literally, as the expected answer of the primer seed
discovery tests: resolve_primer on strings, permute_sequences level by level, find_oligos_in_kmers per level and the
round-by-round cap of discover_primer_kmers_by_round.  It runs over a merged table given as (keys, counts) arrays (the
CPU oracle's `run_batch(...).merged().export()`), with set membership by np.isin, and shares nothing with the
library's mask formulation (sharkmer_amd/csrc/shk_primer.cpp, k_primer_scan)."""
from __future__ import annotations

import numpy as np

IUPAC = {"R": "AG", "Y": "CT", "S": "GC", "W": "AT", "K": "GT", "M": "AC",
         "B": "CGT", "D": "AGT", "H": "ACT", "V": "ACG", "N": "ACGT"}  # primers.rs:63-77
MAX_RESOLVED_VARIANTS = 10_000  # primers.rs:275
BASE = {"A": 0, "C": 1, "G": 2, "T": 3}


class RefError(Exception):
    """The reference's anyhow error, with its text."""


def trim_primer(seq: str, trim: int, k: int) -> str:
    """primers.rs:244-271."""
    if trim >= k:
        trim = k - 1
    return seq[len(seq) - trim:] if len(seq) > trim else seq


def n_resolved(p: str) -> int:
    """|resolve_primer(p)|: the per-position choices are distinct characters, so the set has their product."""
    n = 1
    for c in p:
        n *= len(IUPAC.get(c, c))
    return n if p else 0


def resolve_primer(p: str) -> set[str]:
    """primers.rs:60-93, literally."""
    seqs: set[str] = set()
    for nuc in p:
        poss = IUPAC.get(nuc, nuc)
        if not seqs:
            seqs = set(poss)
        else:
            seqs = {s + n for s in seqs for n in poss}
    return seqs


def permute_sequences(seqs: set[str], r: int = 1) -> set[str]:
    """primers.rs:101-150 for r = 1 (the only radius preprocess_primer_by_mismatch uses): every sequence with each
    single position replaced by each of A T C G, the sequence itself included."""
    assert r == 1
    out = set()
    for s in seqs:
        for i in range(len(s)):
            for n in "ATCG":
                out.add(s[:i] + n + s[i + 1:])
    return out


def levels_literal(p: str, mismatches: int) -> list[set[str]]:
    """preprocess_primer_by_mismatch's level sets (primers.rs:286-313) on strings (small primers only)."""
    base = resolve_primer(p)
    levels, seen = [base], set(base)
    for _ in range(min(mismatches, len(p))):
        new = permute_sequences(seen) - seen
        seen |= new
        levels.append(new)
    return levels


def string_to_oligo(s: str) -> int:
    """primers.rs:33-55."""
    v = 0
    for c in s:
        if c not in BASE:
            raise RefError(f"Invalid nucleotide {c} in {s}")
        v = (v << 2) | BASE[c]
    return v


def levels_encoded(p: str, mismatches: int) -> list[np.ndarray]:
    """The same level sets as levels_literal, the strings held as their 2-bit values (string_to_oligo): one
    permute_sequences step replaces each position by each base, and the new level is what was not seen."""
    L = len(p)
    base = np.array(sorted(string_to_oligo(s) for s in resolve_primer(p)), dtype=np.uint64)
    levels, seen = [base], base
    for _ in range(min(mismatches, L)):
        cand = [seen]
        for i in range(L):
            sh = np.uint64(2 * (L - 1 - i))
            cleared = seen & ~(np.uint64(3) << sh)
            for b in range(4):
                cand.append(cleared | (np.uint64(b) << sh))
        allm = np.unique(np.concatenate(cand))
        new = np.setdiff1d(allm, seen, assume_unique=True)
        seen = np.union1d(seen, new)
        levels.append(new)
    return levels


def revcomp(x, k: int):
    """revcomp_kmer (kmer/encoding.rs:219-262) on a numpy array or an int."""
    a = np.asarray(x, dtype=np.uint64)
    r = np.zeros_like(a)
    for _ in range(k):
        r = (r << np.uint64(2)) | (np.uint64(3) - (a & np.uint64(3)))
        a = a >> np.uint64(2)
    return r if isinstance(x, np.ndarray) else int(r)


def find_oligos_in_kmers(oligos: np.ndarray, L: int, keys: np.ndarray, counts: np.ndarray, k: int, min_count: int):
    """primers.rs:163-226 over the whole table: (kmers, counts) in table order."""
    assert len(oligos) and 0 < L < k
    mask = np.uint64(((1 << (2 * L)) - 1) << (2 * (k - L)))
    rc_mask = np.uint64((1 << (2 * L)) - 1)
    fwd_set = oligos << np.uint64(2 * (k - L))
    rc_set = revcomp(oligos, L)
    sel = counts >= min_count
    ks, cs = keys[sel], counts[sel]
    fwd = np.isin(ks & mask, fwd_set)
    rc = ~fwd & np.isin(ks & rc_mask, rc_set)
    out_k = np.where(fwd, ks, revcomp(ks, k))
    hit = fwd | rc
    return out_k[hit], cs[hit]


def get_primer_kmers(seq: str, keys: np.ndarray, counts: np.ndarray, k: int, trim: int = 15, mismatches: int = 2,
                     min_count: int = 2, max_kmers: int = 40, check_variants: bool = True):
    """discover_primer_kmers_by_round (primers.rs:375-438) for one direction → (kmers, counts, levels, level_hits[33]):
    the insertion order of the result, and per level the hits before the cap (every level, also those past the cap
    the reference never visits)."""
    p = trim_primer(seq, trim, k)
    hits = np.zeros(33, dtype=np.uint64)
    if check_variants:
        check_variant_limit(seq, trim, k)
    if not p or max_kmers == 0:
        return (np.zeros(0, np.uint64), np.zeros(0, np.uint32), np.zeros(0, np.uint8), hits)
    levels = levels_encoded(p, mismatches)  # (string_to_oligo raises on an invalid character, in round 0)
    result: dict[int, tuple[int, int]] = {}
    for m, variants in enumerate(levels):
        if not len(variants):
            continue
        rk, rcnt = find_oligos_in_kmers(variants, len(p), keys, counts, k, min_count)
        new = [(int(a), int(b)) for a, b in zip(rk, rcnt) if int(a) not in result]
        hits[m] = len(new)
        if len(result) >= max_kmers:
            continue
        new.sort(key=lambda e: (-e[1], e[0]))
        for kmer, c in new[:max_kmers - len(result)]:
            result[kmer] = (c, m)
    ks = np.array(list(result.keys()), dtype=np.uint64)
    cs = np.array([v[0] for v in result.values()], dtype=np.uint32)
    ls = np.array([v[1] for v in result.values()], dtype=np.uint8)
    return ks, cs, ls, hits


def check_variant_limit(seq: str, trim: int, k: int):
    """primers.rs:273-284."""
    p = trim_primer(seq, trim, k)
    n = n_resolved(p)
    if n > MAX_RESOLVED_VARIANTS:
        raise RefError(f"Primer {p} has too many ambiguous bases: {n} resolved variants exceeds limit of "
                       f"{MAX_RESOLVED_VARIANTS}. Reduce ambiguity or use a more specific primer.")


def mask_level(x: int, p: str, k: int) -> int:
    """Mismatch level of the first len(p) bases of k-mer x by the bit-plane formulation of k_primer_scan (the
    allow masks built from the IUPAC table here, the planes by XOR/AND): the number of positions whose base is not
    allowed.  For the equivalence test against levels_literal."""
    L = len(p)
    allow = [0, 0, 0, 0]
    for i, c in enumerate(p):
        for b in IUPAC.get(c, c):
            if b in BASE:
                allow[BASE[b]] |= 1 << (2 * (k - 1 - i))
    lo = 0x5555555555555555
    acc = 0
    for b in range(4):
        y = x ^ (lo * b)
        eq = ~(y | (y >> 1)) & lo
        acc |= eq & allow[b]
    return L - bin(acc).count("1")
