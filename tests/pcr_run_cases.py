"""Inputs and expected answers of the shk_pcr_run tests, shared by test_pcr_run_ref_cpu.py and test_gpu_pcr_run.py: the
mixed panel of pcr_panel_cases as PcrGene entries plus a gene whose path is found and too long, and the padded 18S.  Every
expected answer is pcr_run_ref's (the models), computed once and kept."""
from __future__ import annotations

import os

import numpy as np

import pcr_panel_cases as pc
import pcr_run_ref as ref
import sharkmer_amd as sa

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FWD_18S, REV_18S = "AACCTGGTTGATCCTGCCAGT", "TGATCCTTCTGCAGGTTCACCTAC"
_cache = {}


def mixed_genes(orc) -> list:
    """pcr_panel_cases.mixed_panel's primer pairs with do_pcr's defaults (the sweep, the global floor and budget are
    shk_pcr_run's: the panel's per-gene extension parameters are not taken over), and "too long": the pair of "first
    threshold" with max_length 100, whose path is found and longer than that."""
    p = pc.mixed_panel(orc)
    genes = [sa.PcrGene(g.name, g.forward, g.reverse) for g in p.genes]
    at = pc.gene_index(p, "no set at all")  # (its two primers are one palindrome, which validate_pcr_params refuses: another absent one)
    genes[at] = sa.PcrGene(genes[at].gene_name, pc.ABSENT, pc.ABSENT[:-1] + "A")
    first = p.genes[pc.gene_index(p, "first threshold")]
    genes.append(sa.PcrGene("too long", first.forward, first.reverse, max_length=100))
    return genes


def mixed_expected(orc, mode: str) -> list:
    """mode: "none" (no reads), "reads" (the panel's 600 reads, unpaired), "paired" (the same reads as interleaved
    pairs), "odd" (the first 599 of them as interleaved pairs)."""
    key = ("mixed", mode)
    if key not in _cache:
        p = pc.mixed_panel(orc)
        reads = None if mode == "none" else ref.split_reads(p.bases, p.offsets)
        if mode == "odd":
            reads = reads[:-1]
        _cache[key] = ref.run_pcr(p.keys, p.counts, p.k, mixed_genes(orc), reads, paired=mode in ("paired", "odd"),
                                  max_num_nodes=pc.MIXED_BUDGET)
    return _cache[key]


def case_18s(orc):
    """(sequence, bases, offsets, gene, keys, counts): pcr_18s_padded.txt ten times at k 21 with the primers and
    parameters of mod.rs:1249-1281."""
    if "18s" not in _cache:
        seq = open(os.path.join(GOLDEN, "pcr_18s_padded.txt")).read().strip()
        bases = np.frombuffer(seq.encode() * 10, dtype=np.uint8).copy()
        offsets = np.arange(11, dtype=np.uint64) * np.uint64(len(seq))
        keys, counts = pc.oracle_table(orc, bases, offsets, 21)
        gene = sa.PcrGene("18s", FWD_18S, REV_18S, min_length=0, max_length=2500, min_count=3)
        _cache["18s"] = (seq, bases, offsets, gene, keys, counts)
    return _cache["18s"]


def expected_18s(orc, with_reads: bool, paired: bool = False, n_reads: int = 10):
    """The model's outcome; paired: the first n_reads copies as interleaved pairs (ten identical reads that all map: five
    pairs, four of nine)."""
    key = ("18s", with_reads, paired, n_reads)
    if key not in _cache:
        seq, bases, offsets, gene, keys, counts = case_18s(orc)
        reads = ref.split_reads(bases, offsets)[:n_reads] if with_reads else None
        (_cache[key],) = ref.run_pcr(keys, counts, 21, [gene], reads, paired=paired, max_num_nodes=500_000)
    return _cache[key]
