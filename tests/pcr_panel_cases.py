"""Inputs of the panel tests of sPCR's graph extension (shk_neighborhood_panel, shk_pcr_extend_panel), shared by the CPU
test of the cases themselves (test_pcr_panel_cases_cpu.py) and the GPU tests (test_gpu_nb_panel.py,
test_gpu_pcr_extend_panel.py).  Built from pcr_ref (the model), primer_ref and nb_cases; every expected answer is the
model's, never the library's.  Each builder computes its case once and keeps it."""
from __future__ import annotations

import random
from typing import NamedTuple

import numpy as np

import nb_cases
import pcr_ref as ref
import primer_ref

_cache = {}


def rc_str(s):
    return s[::-1].translate(str.maketrans("ACGTN", "TGCAN"))


def oracle_table(orc, bases, offsets, k, chunks=1):
    run = orc.run_batch(bases, offsets, k, chunks, 100)  # (held until the export has copied out of it)
    return run.merged().export()


# ---- 1. the mixed panel: genes that end their sweeps in every way there is ----------------------------------------------

MIXED_K = 21
MIXED_SPEC = dict(genome_len=6000, sub_per_64k=400, n_per_64k=30)  # the reads of test_gpu_pcr_extend.py's pcr_case
MIXED_READS = 600
MIXED_BUDGET = 2500
PRIMER = dict(trim=15, mismatches=2, min_count=2)
ABSENT = "ACGTACGTACGTACGTACGTACGT"  # no k-mer of the table starts or ends like it


class Gene(NamedTuple):
    name: str
    forward: str       # primers (5' → 3'), as the panel file would give them
    reverse: str
    params: dict       # keyword arguments of pcr_extend


class MixedPanel(NamedTuple):
    k: int
    bases: np.ndarray
    offsets: np.ndarray
    keys: np.ndarray
    counts: np.ndarray
    table: dict
    genes: list
    sets: list         # 2 per gene: primer_ref.get_primer_kmers of the forward, then of the reverse primer
    expected: list     # per gene pcr_ref.pcr_extend's (Graph, threshold used, steps run)


def mixed_panel(orc) -> MixedPanel:
    """Primer pairs cut from error-free 3000-base stretches of the genome (window, offset of the forward primer, distance
    to the reverse one), found by trying positions on the model; what each gene is there for is asserted by
    test_pcr_panel_cases_cpu.py."""
    if "mixed" in _cache:
        return _cache["mixed"]
    import sharkmer_amd as sa
    k = MIXED_K
    bases, offsets = sa.synth_reads(sa.SynthSpec(seed_genome=100 + k, **MIXED_SPEC), 0, MIXED_READS)
    keys, counts = oracle_table(orc, bases, offsets, k)
    table = ref.table_dict(keys, counts)
    long_, _ = sa.synth_reads(sa.SynthSpec(genome_len=MIXED_SPEC["genome_len"], read_len=3000, seed_genome=100 + k), 0, 6)
    win = [long_[r * 3000:(r + 1) * 3000].tobytes().decode() for r in range(6)]

    def pair(r, a, d):
        return win[r][a:a + 24], rc_str(win[r][a + d:a + d + 24])

    def swapped(r, a, d):  # the forward primer downstream of the reverse one: the two walks leave each other
        return win[r][a + d:a + d + 24], rc_str(win[r][a:a + 24])

    std = dict(min_count=2, table_min_count=2, high_coverage_ratio=10.0, max_num_nodes=MIXED_BUDGET, sweep=True)
    genes = [
        Gene("first threshold", *pair(2, 45, 842), std),
        Gene("third step", *pair(0, 684, 867), std),
        Gene("second step", *pair(3, 112, 687), std),
        Gene("never found", *swapped(0, 1500, 600), dict(std, max_num_nodes=100_000)),
        Gene("budget", *swapped(2, 1000, 400), std),
        Gene("no forward set", ABSENT, pair(2, 45, 842)[1], std),
        Gene("no set at all", ABSENT, rc_str(ABSENT), std),
        Gene("twin a", *pair(1, 1036, 904), std),
        Gene("no sweep, ratio 1.5", *pair(0, 596, 509), dict(std, min_count=3, high_coverage_ratio=1.5, sweep=False)),
        Gene("twin b", *pair(1, 1036, 904), std),
        Gene("floor 1", *pair(5, 459, 1043), dict(std, table_min_count=1)),
    ]
    sets, expected = [], []
    for g in genes:
        f = primer_ref.get_primer_kmers(g.forward, keys, counts, k, PRIMER["trim"], PRIMER["mismatches"], PRIMER["min_count"])
        r = primer_ref.get_primer_kmers(g.reverse, keys, counts, k, PRIMER["trim"], PRIMER["mismatches"], PRIMER["min_count"])
        sets += [f, r]
        p = g.params
        expected.append(ref.pcr_extend(f[:2], r[:2], table, k, p["min_count"], p["table_min_count"], p["high_coverage_ratio"],
                                       p["max_num_nodes"], p["sweep"]))
    _cache["mixed"] = MixedPanel(k, bases, offsets, keys, counts, table, genes, sets, expected)
    return _cache["mixed"]


def gene_index(panel: MixedPanel, name: str) -> int:
    (at,) = [i for i, g in enumerate(panel.genes) if g.name == name]
    return at


# ---- 2. wide and narrow jobs on one table ----------------------------------------------------------------------------------

WIDE_NARROW = ("flat1023", "flat1024", "flat1025", "rising", "falling")


class NbPanel(NamedTuple):
    k: int
    chunks: int
    inserts: list   # [(chunk_id, canonical k-mers, counts)] for KmerEngine.insert
    table: dict     # the merged table the inserts make
    jobs: list      # [(nodes, dirs, min_count)]
    names: list


def wide_narrow_panel() -> NbPanel:
    """nb_cases' chain cases around the hand-over between the one-workgroup kernel and the wide one, all in ONE table
    (every case draws its chains at random at k 15: they barely meet), one job per case and two thin ones — the first 40
    chains of flat1025 and a single chain of rising — so that wide jobs and narrow ones share a launch."""
    if "wide" in _cache:
        return _cache["wide"]
    cases = [nb_cases.CASES[n]() for n in WIDE_NARROW]
    assert len({(c.k, c.chunks) for c in cases}) == 1
    inserts = [ins for c in cases for ins in c.inserts]
    jobs = [(list(c.seeds), list(c.dirs), c.min_count) for c in cases]
    names = list(WIDE_NARROW)
    jobs.append((list(cases[2].seeds[:40]), list(cases[2].dirs[:40]), 1))
    names.append("flat1025, 40 chains")
    jobs.append((list(cases[3].seeds[5:6]), list(cases[3].dirs[5:6]), 1))
    names.append("rising, one chain")
    _cache["wide"] = NbPanel(cases[0].k, cases[0].chunks, inserts, nb_cases.merged_table(inserts), jobs, names)
    return _cache["wide"]


# ---- 3. more jobs than the card holds workgroups --------------------------------------------------------------------------

MANY_JOBS, MANY_K, MANY_LEVELS = 600, 9, 4
MANY_SPEC = dict(genome_len=40_000, sub_per_64k=400, n_per_64k=30)


class ManyJobs(NamedTuple):
    k: int
    bases: np.ndarray
    offsets: np.ndarray
    table: dict
    jobs: list       # [(nodes, dirs, min_count)], to be run with max_levels = MANY_LEVELS
    max_levels: int


def many_jobs_panel(orc) -> ManyJobs:
    """600 jobs of MANY_LEVELS levels each on a k 9 table, where the graph branches at every node: one to three seed
    nodes per job cut from the reads, no (node, dir) entry in two jobs, min_count 1, 2, 3, 1, … along the jobs."""
    if "many" in _cache:
        return _cache["many"]
    import sharkmer_amd as sa
    k = MANY_K
    bases, offsets = sa.synth_reads(sa.SynthSpec(seed_genome=k, **MANY_SPEC), 0, 1200)
    keys, counts = oracle_table(orc, bases, offsets, k)
    rng = random.Random(600)
    taken, jobs = set(), []
    while len(jobs) < MANY_JOBS:
        nodes, dirs = [], []
        for _ in range(rng.randint(1, 3)):
            r = rng.randrange(len(offsets) - 1)
            s = bases[int(offsets[r]):int(offsets[r + 1])].tobytes().decode()
            at = rng.randrange(0, len(s) - (k - 1))
            p = s[at:at + k - 1]
            d = rng.randint(1, 3)
            n = primer_ref.string_to_oligo(p) if "N" not in p else None
            if n is None or any((n, b) in taken for b in (1, 2)):
                continue
            taken.update((n, b) for b in (1, 2) if d & b)
            nodes.append(n)
            dirs.append(d)
        if nodes:
            jobs.append((nodes, dirs, 1 + len(jobs) % 3))
    _cache["many"] = ManyJobs(k, bases, offsets, ref.table_dict(keys, counts), jobs, MANY_LEVELS)
    return _cache["many"]
