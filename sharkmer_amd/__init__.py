"""sharkmer_amd — MI355X-native incremental k-mer counting engine.

Drop-in for the counting hot path of caseywdunn/sharkmer (src/kmer/* and the
ingest/consolidate loop of src/io.rs).  The product is the C-ABI shared library
built from sharkmer_amd/csrc (include/shk.h); this package is the thin ctypes
host mirror used by tests, bench.py and the multi-GPU driver.  There is no CPU
fallback: importing works anywhere, creating an engine needs a gfx950 GPU.
"""
from .engine import (  # noqa: F401
    KmerEngine, ShkError, N_READS_PER_BATCH, lib_path, load_library,
    FLAG_TIMING, FLAG_FORCE_DIRECT, FLAG_FORCE_PAGED, FLAG_DEFER_ERRORS, FLAG_TIMING_SAMPLED, FLAG_GROUP_GRAPH, FLAG_GROUP_READS, KERNEL_NAMES, RESERVE_NONE,
    Primer, primer_compile, PRIMER_LEVELS, PcrGraph, PrunedGraph, pcr_node_budget,
    PcrProducts, DedupResult, pcr_paths_panel, edit_within, PCR_SCORE_FIELDS, PCR_MAX_AMPLICONS, PCR_MAX_DEPTHS,
    PcrGene, PcrOutcome, parse_pcr_primers, validate_pcr_gene, pcr_validation_report, pcr_failure_reason, write_fasta,
    PCR_SUCCESS, PCR_NO_FORWARD, PCR_NO_REVERSE, PCR_NO_PRIMERS, PCR_NO_PATH, PCR_NODE_BUDGET,
    PackedReads, pack_reads, release_cached_memory, FastqReader, write_histo, write_final_histo, write_stats_yaml, validate_args, run_files,
    fastq_parse_geometry, fastq_device_totals, FASTQ_NO_ANOMALY,
)
from .synth import SynthSpec, synth_reads  # noqa: F401

__version__ = "0.1.0"
SHARKMER_VERSION = "3.1.0"  # reference version whose output formats we emit
