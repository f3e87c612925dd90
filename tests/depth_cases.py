"""Inputs and expected answers of the depth-sweep tests, shared by test_depth_cases_cpu.py and
test_gpu_pcr_depths.py.  Depth d of a context whose reads were dealt over n chunks is the table of chunks 0..d-1, so every
expected answer is a model's (pcr_run_ref, primer_ref, pcr_ref) over the oracle's table of that SUBSET of the reads —
never the library's.  Each is computed once and kept."""
from __future__ import annotations

import numpy as np

import pcr_panel_cases as pc
import pcr_ref
import pcr_run_cases as cases
import pcr_run_ref as ref

_cache = {}
CHUNKS_18S, CHUNKS_MIXED = 5, 4


def deal(n_reads: int, n_chunks: int) -> np.ndarray:
    """The chunk of every read: read i → chunk i % n_chunks (ingested with ingest_batch(chunk_id, …), so that a few
    hundred reads really spread over the lanes; the 1000-read cadence would put them all in chunk 0)."""
    return np.arange(n_reads) % n_chunks


def subset(bases: np.ndarray, offsets: np.ndarray, keep) -> tuple:
    """The reads `keep` (indices, ascending) as a batch of their own."""
    keep = [int(i) for i in keep]
    parts = [bases[int(offsets[i]):int(offsets[i + 1])] for i in keep]
    lens = np.array([len(p) for p in parts], dtype=np.uint64)
    out = np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint8)
    return np.ascontiguousarray(out, dtype=np.uint8), np.concatenate([[0], np.cumsum(lens, dtype=np.uint64)]).astype(np.uint64)


def below(bases, offsets, n_chunks: int, depth: int) -> tuple:
    """The reads of chunks < depth."""
    chunk = deal(len(offsets) - 1, n_chunks)
    return subset(bases, offsets, np.nonzero(chunk < depth)[0])


def chunk_batches(bases, offsets, n_chunks: int) -> list:
    """[(chunk_id, bases, offsets)]: what a test hands to ingest_batch."""
    chunk = deal(len(offsets) - 1, n_chunks)
    return [(c,) + subset(bases, offsets, np.nonzero(chunk == c)[0]) for c in range(n_chunks)]


def ingest_below(e, bases, offsets, n_chunks: int, depth: int):
    """Feeds e the chunks < depth under their own chunk ids (n_chunks of the context unchanged) and finalizes."""
    for c, b, o in chunk_batches(bases, offsets, n_chunks)[:depth]:
        e.ingest_batch(c, b, o)
    e.finalize()


def depth_table(orc, bases, offsets, k: int, n_chunks: int, depth: int) -> tuple:
    """(keys, counts) of the table at `depth`: the oracle's merged table of the reads below it."""
    key = ("table", bases.ctypes.data, len(bases), k, n_chunks, depth)
    if key not in _cache:
        b, o = below(bases, offsets, n_chunks, depth)
        _cache[key] = pc.oracle_table(orc, b, o, k) if len(o) > 1 else (np.zeros(0, np.uint64), np.zeros(0, np.uint32))
    return _cache[key]


def chunk_bases(orc, bases, offsets, k: int, n_chunks: int) -> list:
    """The oracle's n_bases_ingested of every chunk on its own."""
    key = ("bases", bases.ctypes.data, len(bases), k, n_chunks)
    if key not in _cache:
        _cache[key] = [int(orc.run_batch(b, o, k, 1, 100).stats["n_bases_ingested"]) if len(o) > 1 else 0
                       for _, b, o in chunk_batches(bases, offsets, n_chunks)]
    return _cache[key]


# ---- the padded 18S on 5 chunks: two copies per chunk, min_count 3 → nothing at depth 1, the product from depth 2 on ----

def expected_18s(orc, depth: int):
    key = ("18s", depth)
    if key not in _cache:
        seq, bases, offsets, gene, _, _ = cases.case_18s(orc)
        keys, counts = depth_table(orc, bases, offsets, 21, CHUNKS_18S, depth)
        (_cache[key],) = ref.run_pcr(keys, counts, 21, [gene], None, max_num_nodes=500_000)
    return _cache[key]


# ---- the mixed panel on 4 chunks -----------------------------------------------------------------------------------------

def mixed_expected(orc, depth: int, max_num_nodes: int = pc.MIXED_BUDGET) -> list:
    key = ("mixed", depth, max_num_nodes)
    if key not in _cache:
        p = pc.mixed_panel(orc)
        keys, counts = depth_table(orc, p.bases, p.offsets, p.k, CHUNKS_MIXED, depth)
        _cache[key] = ref.run_pcr(keys, counts, p.k, cases.mixed_genes(orc), None, max_num_nodes=max_num_nodes)
    return _cache[key]


def mixed_table(orc, depth: int) -> dict:
    p = pc.mixed_panel(orc)
    return pcr_ref.table_dict(*depth_table(orc, p.bases, p.offsets, p.k, CHUNKS_MIXED, depth))
