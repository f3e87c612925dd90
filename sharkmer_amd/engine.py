"""ctypes host mirror of the libshk C ABI (include/shk.h).

`KmerEngine` plays the role the reference's `FastqReadState` + `Chunk`s +
`consolidate_and_histogram` play in src/io.rs: sequences go in (explicit chunk
like drain_batch, io.rs:355-361, or striped by read index like read_fastq,
io.rs:335-343), histograms and totals come out (io.rs:1020-1028, 545-552).
Errors surface as `ShkError` carrying the reference's message text.

The library is loaded from sharkmer_amd/csrc/libshk.so (in-tree).  If it is
missing the import of this module still works, but any use raises — there is no
fallback path.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass

import numpy as np

N_READS_PER_BATCH = 1000  # io.rs:15

FLAG_TIMING = 1
FLAG_FORCE_DIRECT = 2
FLAG_FORCE_PAGED = 4
FLAG_TIMING_SAMPLED = 16  # with FLAG_TIMING: only every 4th job's launches are bracketed (include/shk.h)
RESERVE_NONE = 0xFFFFFFFF  # shk_config.reserve_cus: every compute unit (include/shk.h)
FASTQ_GZIP_ALL_MEMBERS = 1  # shk_fastq_open_ex / shk_run_config.fastq_flags (include/shk.h)
FASTQ_BGZF_BATCH = 2        # BGZF members decoded in batches on host threads …
FASTQ_BGZF_DEVICE = 4       # … or on the device (both imply every member)
FASTQ_DEVICE_PARSE = 8      # run_files only, with FASTQ_BGZF_DEVICE: the decoded text stays on the device and is framed there
FASTQ_NO_ANOMALY = (1 << 64) - 1  # shk_fastq_text_result.anomaly_record: none among the records looked at


def _bgzf_flags(bgzf) -> int:
    if bgzf is None:
        return 0
    if bgzf not in ("host", "device"):
        raise ValueError(f"bgzf must be None, 'host' or 'device', not {bgzf!r}")
    return FASTQ_BGZF_BATCH if bgzf == "host" else FASTQ_BGZF_DEVICE
FLAG_DEFER_ERRORS = 8  # host-buffer ingests return once queued; errors surface at the next call (include/shk.h)
FLAG_GROUP_GRAPH = 32  # a multi-device context answers the graph extension calls and pcr_run (opt-in; include/shk.h)
FLAG_GROUP_READS = 64  # a multi-device context retains reads and answers the retained calls (opt-in; include/shk.h)

KERNEL_NAMES = ["mark", "scan", "direct", "scatter", "pages", "histo", "grow", "insert",
                "lookup", "export", "synth", "merge", "pcount", "pscan", "histo_rows", "extend"]

_HERE = os.path.dirname(os.path.abspath(__file__))


def lib_path() -> str:
    # SHK_LIB_PATH: experiment hook to A/B two builds of the same HIP library in one session
    return os.environ.get("SHK_LIB_PATH") or os.path.join(_HERE, "csrc", "libshk.so")


class ShkError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"[shk {code}] {msg}")
        self.code = code
        self.msg = msg


class _Config(C.Structure):
    _fields_ = [("k", C.c_uint32), ("chunks", C.c_uint32), ("histo_max", C.c_uint64),
                ("device", C.c_int32), ("flags", C.c_uint32),
                ("table_capacity_hint", C.c_uint64), ("n_owners", C.c_uint32), ("owner_id", C.c_uint32),
                ("n_devices", C.c_uint32), ("reserve_cus", C.c_uint32), ("device_ids", C.POINTER(C.c_int32)),
                ("reserved", C.c_uint64 * 1)]


class XchgLayout(C.Structure):
    """shk_xchg_layout: how one exchange round's owner segments are laid out (include/shk.h)."""
    _fields_ = [("n_owners", C.c_uint32), ("n_lanes", C.c_uint32), ("log_p1", C.c_uint32),
                ("regions", C.c_uint32), ("region_cap", C.c_uint32), ("record_bytes", C.c_uint32),
                ("segment_records", C.c_uint64)]


class _Counters(C.Structure):
    _fields_ = [("n_reads_ingested", C.c_uint64), ("n_bases_read", C.c_uint64),
                ("n_bases_ingested", C.c_uint64), ("n_kmers_ingested", C.c_uint64),
                ("n_unique_kmers", C.c_uint64), ("n_hashed_kmers", C.c_uint64),
                ("n_singleton_kmers", C.c_uint64), ("any_saturated", C.c_uint32),
                ("n_chunks", C.c_uint32), ("table_capacity", C.c_uint64),
                ("n_grows", C.c_uint64), ("n_spilled", C.c_uint64)]


class _Timings(C.Structure):
    _fields_ = [("ms", C.c_double * 16), ("launches", C.c_uint64 * 16)]


class _RunStats(C.Structure):
    _fields_ = [("sharkmer_version", C.c_char_p), ("command", C.c_char_p), ("sample", C.c_char_p),
                ("kmer_length", C.c_uint32), ("chunks", C.c_uint32), ("n_reads_read", C.c_uint64),
                ("n_bases_read", C.c_uint64), ("n_subreads_ingested", C.c_uint64),
                ("n_bases_ingested", C.c_uint64), ("n_kmers", C.c_uint64), ("n_multi_kmers", C.c_uint64),
                ("n_singleton_kmers", C.c_uint64), ("peak_memory_bytes", C.c_uint64),
                ("has_histogram", C.c_uint32), ("reserved", C.c_uint32)]


class _RunConfig(C.Structure):
    _fields_ = [("inputs", C.POINTER(C.c_char_p)), ("n_inputs", C.c_uint32), ("k", C.c_uint32),
                ("chunks", C.c_uint32), ("device", C.c_int32), ("histo_max", C.c_uint64),
                ("max_reads", C.c_uint64), ("validate_every", C.c_uint64), ("sample", C.c_char_p),
                ("outdir", C.c_char_p), ("command", C.c_char_p), ("version", C.c_char_p),
                ("table_capacity_hint", C.c_uint64), ("batch_reads", C.c_uint64),
                ("batch_bases", C.c_uint64), ("n_devices", C.c_uint32), ("fastq_flags", C.c_uint32),
                ("device_ids", C.POINTER(C.c_int32))]


class _Primer(C.Structure):
    _fields_ = [("seq", C.c_char_p), ("trim", C.c_uint32), ("mismatches", C.c_uint32),
                ("min_count", C.c_uint32), ("max_kmers", C.c_uint32)]


PRIMER_LEVELS = 33  # SHK_PRIMER_LEVELS: level slots per primer in level_hits / n_variants (include/shk.h)


@dataclass(frozen=True)
class Primer:
    """One primer direction of sPCR (PCRParams' forward_seq or reverse_seq, src/pcr/mod.rs) with the fields
    get_primer_kmers reads (pcr/primers.rs:234-480); defaults are the reference's."""
    seq: str
    trim: int = 15
    mismatches: int = 2
    min_count: int = 2
    max_kmers: int = 40  # max_primer_kmers

    def _c(self) -> _Primer:
        return _Primer(self.seq.encode("latin-1"), self.trim, self.mismatches, self.min_count, self.max_kmers)


def primer_compile(primer: Primer, k: int):
    """preprocess_primer_by_mismatch (pcr/primers.rs:237-313) on the host, no device: (trimmed length, level sizes
    as a list of n_levels ints).  Raises ShkError with the reference's text (too many variants, invalid character)."""
    L = load_library()
    tl, nl = C.c_uint32(0), C.c_uint32(0)
    nv = (C.c_uint64 * PRIMER_LEVELS)()
    err = C.create_string_buffer(1024)
    p = primer._c()
    rc = L.shk_primer_compile(C.byref(p), k, C.byref(tl), C.byref(nl), nv, err, len(err))
    if rc != 0:
        raise ShkError(rc, err.value.decode("utf-8", "replace"))
    return int(tl.value), [int(x) for x in nv[:nl.value]]


class _PcrExtendParams(C.Structure):
    _fields_ = [("min_count", C.c_uint32), ("table_min_count", C.c_uint32), ("high_coverage_ratio", C.c_double),
                ("max_num_nodes", C.c_uint64), ("sweep", C.c_uint32), ("reserved", C.c_uint32)]


@dataclass
class PcrGraph:
    """What shk_pcr_extend returns: the graph of the last threshold step run (current_graph, pcr/mod.rs:613) as
    arrays — nodes in NodeIndex order, edges in EdgeIndex order."""
    node_sub_kmers: np.ndarray  # u64, DBNode.sub_kmer
    node_flags: np.ndarray      # u8: 1 is_start, 2 is_end
    edge_src: np.ndarray        # u32 node indices
    edge_tgt: np.ndarray
    edge_counts: np.ndarray     # u32, DBEdge.count
    found_path: bool
    threshold_used: int
    steps_run: int


class _PcrPruneParams(C.Structure):
    _fields_ = [("tip_coverage_fraction", C.c_double), ("stages", C.c_uint32), ("reserved", C.c_uint32)]


class _PcrPruneOut(C.Structure):
    _fields_ = [("node_keep", C.c_void_p), ("out_node_offsets", C.c_void_p), ("out_edge_offsets", C.c_void_p),
                ("node_sub_kmers", C.c_void_p), ("node_flags", C.c_void_p), ("node_index", C.c_void_p), ("node_cap", C.c_uint64),
                ("edge_src", C.c_void_p), ("edge_tgt", C.c_void_p), ("edge_counts", C.c_void_p), ("edge_index", C.c_void_p),
                ("coverage_ratio", C.c_void_p), ("edge_cap", C.c_uint64), ("median", C.c_void_p), ("tip_rounds", C.c_void_p),
                ("tips_removed", C.c_void_p), ("unreachable_removed", C.c_void_p), ("device_ms", C.c_double)]


@dataclass
class PrunedGraph:
    """What shk_pcr_prune_panel returns for a gene: the graph after remove_low_coverage_tips, reachability_pruning and
    annotate_coverage_ratios (pcr/mod.rs:631-697) — the survivors in ascending original index, endpoints renumbered."""
    node_sub_kmers: np.ndarray  # u64
    node_flags: np.ndarray      # u8: 1 is_start, 2 is_end
    edge_src: np.ndarray        # u32, positions in this graph
    edge_tgt: np.ndarray
    edge_counts: np.ndarray     # u32
    node_index: np.ndarray      # u32: each node's index in the graph that went in
    edge_index: np.ndarray      # u32: each edge's index in the graph that went in
    coverage_ratio: np.ndarray  # f64 per edge, DBEdge.coverage_ratio
    median: float               # median edge count of this graph, 0.0 without edges
    node_keep: np.ndarray       # u8 per node of the graph that went in
    tip_rounds: int             # tip rounds that removed something
    tips_removed: int
    unreachable_removed: int


THREAD_TILE = 64  # the list elements one wave step of the read walk (k_thread_panel) covers (THREAD_TILE in csrc/shk_device.hip.h)


class _ThreadOut(C.Structure):
    _fields_ = [("support_total", C.c_void_p), ("support_unambiguous", C.c_void_p), ("link_in", C.c_void_p),
                ("link_out", C.c_void_p), ("link_counts", C.c_void_p), ("link_cap", C.c_uint64), ("n_links", C.c_uint64),
                ("read_edges", C.c_void_p), ("n_paired_links", C.c_uint64)]


class _ThreadPanelOut(C.Structure):
    _fields_ = [("support_total", C.c_void_p), ("support_unambiguous", C.c_void_p), ("link_offsets", C.c_void_p),
                ("link_in", C.c_void_p), ("link_out", C.c_void_p), ("link_counts", C.c_void_p), ("link_cap", C.c_uint64),
                ("n_links", C.c_uint64), ("read_edges", C.c_void_p), ("n_paired_links", C.c_void_p)]


@dataclass
class ThreadingAnnotations:
    """What shk_thread_reads returns: ThreadingAnnotations of pcr/threading.rs:54-62 as arrays."""
    support_total: np.ndarray        # u32 per edge, EdgeReadSupport.read_support_total
    support_unambiguous: np.ndarray  # u32 per edge, EdgeReadSupport.read_support_unambiguous
    links: np.ndarray                # m × 2 u32 (incoming edge, outgoing edge), ascending
    link_counts: np.ndarray          # u32 per link
    read_edges: np.ndarray           # u32 per read: edges it was mapped to
    n_paired_links: int              # paired_links.len(); 0 for the unpaired form


class _PcrGraphs(C.Structure):
    _fields_ = [("n_genes", C.c_uint32), ("reserved", C.c_uint32), ("node_sub_kmers", C.c_void_p), ("node_flags", C.c_void_p),
                ("node_offsets", C.c_void_p), ("edge_src", C.c_void_p), ("edge_tgt", C.c_void_p), ("edge_counts", C.c_void_p),
                ("coverage_ratio", C.c_void_p), ("edge_offsets", C.c_void_p), ("support_total", C.c_void_p),
                ("support_unambiguous", C.c_void_p), ("link_offsets", C.c_void_p), ("link_in", C.c_void_p), ("link_out", C.c_void_p),
                ("link_counts", C.c_void_p), ("has_threading", C.c_void_p)]


class _PcrPathsParams(C.Structure):
    _fields_ = [("min_length", C.c_uint64), ("max_length", C.c_uint64), ("max_dfs_states", C.c_uint64),
                ("max_paths_per_pair", C.c_uint64), ("max_node_visits", C.c_uint64)]


class _PcrRecords(C.Structure):
    _fields_ = [("record_offsets", C.c_void_p), ("seq_offsets", C.c_void_p), ("seqs", C.c_void_p), ("record_cap", C.c_uint64),
                ("seq_cap", C.c_uint64), ("n_records", C.c_uint64), ("n_seq_bytes", C.c_uint64), ("start_node", C.c_void_p),
                ("path_nodes", C.c_void_p), ("count_mean", C.c_void_p), ("count_median", C.c_void_p), ("count_min", C.c_void_p),
                ("count_max", C.c_void_p), ("score", C.c_void_p), ("score_fields", C.c_void_p), ("paths_found", C.c_void_p),
                ("generated", C.c_void_p), ("states_explored", C.c_void_p)]


class _PcrDedupOut(C.Structure):
    _fields_ = [("kept", C.c_void_p), ("generated", C.c_void_p), ("retained", C.c_void_p), ("returned", C.c_void_p),
                ("order", C.c_void_p), ("pair_words", C.c_void_p), ("pair_offsets", C.c_void_p), ("pair_cap", C.c_uint64),
                ("pairs_device", C.c_uint64), ("pairs_host", C.c_uint64), ("pairs_prefiltered", C.c_uint64),
                ("device_ms", C.c_double)]


PCR_SCORE_FIELDS = ("kmer_min_count", "coverage_cv", "max_coverage_ratio", "zero_support_edges", "median_unambiguous_support",
                    "edge_support_fraction")  # SHK_PCR_SCORE_FIELDS; NaN stands for None
PCR_MAX_AMPLICONS = 20  # SHK_PCR_MAX_AMPLICONS = MAX_NUM_AMPLICONS (pcr/paths.rs:20)
PCR_MAX_DEPTHS = 16  # SHK_PCR_MAX_DEPTHS: depths per depth-sweep call


def _fmt_f64(x: float) -> str:
    """Rust's `{}` of an f64 for the values a median takes: 12, 12.5 (never 12.0)."""
    x = float(x)
    return str(int(x)) if x == int(x) else repr(x)


@dataclass
class PcrProducts:
    """A gene's records: what generate_sequences_from_paths made, in enumeration order (pcr_paths_panel), or the final
    products after sort_and_deduplicate in product order 0, 1, .. (pcr_products_panel); one entry per record."""
    sequences: list             # str, ACGT
    start_node: np.ndarray      # u32: the path's first node
    path_nodes: np.ndarray      # u64: nodes on the path
    count_mean: np.ndarray      # f64
    count_median: np.ndarray    # f64
    count_min: np.ndarray       # u64
    count_max: np.ndarray       # u64
    score: np.ndarray           # f64, PathScore::composite
    score_fields: np.ndarray    # n × 6 f64 in the order of PCR_SCORE_FIELDS, NaN = None
    paths_found: int            # get_assembly_paths' paths
    generated: int              # records before the dedup
    states_explored: int        # DFS pops, summed over the start nodes
    retained: int | None = None  # records the dedup kept before the truncation to 20 (pcr_products_panel only)

    def fasta(self, sample: str, gene_name: str) -> str:
        """The reference's FASTA records (pcr/paths.rs:331-343 with product = the record's position, as mod.rs:785-813
        renumbers them), each one header line and one sequence line."""
        out = []
        for i, seq in enumerate(self.sequences):
            out.append(f">{sample}_{gene_name}_{i} sample={sample} gene={gene_name} product={i} length={len(seq)} "
                       f"kmer_count_mean={float(self.count_mean[i]):.2f} kmer_count_median={_fmt_f64(self.count_median[i])} "
                       f"kmer_count_min={int(self.count_min[i])} kmer_count_max={int(self.count_max[i])} "
                       f"score={float(self.score[i]):.2f}\n{seq}\n")
        return "".join(out)


@dataclass
class DedupResult:
    """A gene's answer of pcr_dedup_panel."""
    kept: np.ndarray            # u32: the records kept, indices into the gene's input, in final order (at most 20)
    generated: int
    retained: int               # kept before the truncation
    order: np.ndarray           # u32: sorted position -> input index
    pair_bits: np.ndarray | None  # bool per pair i < j of the sorted order, row-major upper triangle (want_pairs=True)


def _per_gene(value, ng: int, name: str) -> list:
    vals = list(value) if np.ndim(value) else [value] * ng
    if len(vals) != ng:
        raise ValueError(f"one {name} for all genes or one per gene")
    return vals


def _cat(parts, dtype):
    off = np.zeros(len(parts) + 1, dtype=np.uint64)
    if parts:
        off[1:] = np.cumsum([len(x) for x in parts])
    return (np.concatenate(parts).astype(dtype, copy=False) if parts else np.zeros(0, dtype=dtype)), off


def _pcr_graphs(graphs, annotations):
    """(shk_pcr_graphs, the arrays it points into) from the list pcr_prune_panel returns — or (node_sub_kmers, node_flags,
    edge_src, edge_tgt, edge_counts, coverage_ratio) tuples — and the list thread_reads_panel returns, None entries
    allowed."""
    gs = [(g.node_sub_kmers, g.node_flags, g.edge_src, g.edge_tgt, g.edge_counts, g.coverage_ratio) if isinstance(g, PrunedGraph) else g
          for g in graphs]
    ng = len(gs)
    cols = [[np.ascontiguousarray(g[i], dtype=dt).reshape(-1) for g in gs]
            for i, dt in enumerate((np.uint64, np.uint8, np.uint32, np.uint32, np.uint32, np.float64))]
    if any(len(a) != len(b) for a, b in zip(cols[0], cols[1])):
        raise ValueError("node_sub_kmers and node_flags differ in length")
    if any(len({len(c[g]) for c in cols[2:]}) != 1 for g in range(ng)):
        raise ValueError("edge_src, edge_tgt, edge_counts and coverage_ratio differ in length")
    sub, noff = _cat(cols[0], np.uint64)
    fl, _ = _cat(cols[1], np.uint8)
    es, eoff = _cat(cols[2], np.uint32)
    et, _ = _cat(cols[3], np.uint32)
    ec, _ = _cat(cols[4], np.uint32)
    ratio, _ = _cat(cols[5], np.float64)
    keep = [sub, fl, noff, es, et, ec, ratio, eoff]
    G = _PcrGraphs(ng, 0, sub.ctypes.data, fl.ctypes.data, noff.ctypes.data, es.ctypes.data, et.ctypes.data, ec.ctypes.data,
                   ratio.ctypes.data, eoff.ctypes.data, None, None, None, None, None, None, None)
    if annotations is not None and any(a is not None for a in annotations):
        if len(annotations) != ng:
            raise ValueError("one annotations entry (or None) per graph")
        tot, una, lks, lcs = [], [], [], []
        for g, a in enumerate(annotations):
            ne = len(cols[2][g])
            if a is None:
                tot.append(np.zeros(ne, dtype=np.uint32)), una.append(np.zeros(ne, dtype=np.uint32))
                lks.append(np.zeros((0, 2), dtype=np.uint32)), lcs.append(np.zeros(0, dtype=np.uint32))
                continue
            if len(a.support_total) != ne or len(a.support_unambiguous) != ne:
                raise ValueError("annotations take one support entry per edge")
            tot.append(np.ascontiguousarray(a.support_total, dtype=np.uint32))
            una.append(np.ascontiguousarray(a.support_unambiguous, dtype=np.uint32))
            lks.append(np.ascontiguousarray(a.links, dtype=np.uint32).reshape(-1, 2))
            lcs.append(np.ascontiguousarray(a.link_counts, dtype=np.uint32).reshape(-1))
        st, _ = _cat(tot, np.uint32)
        su, _ = _cat(una, np.uint32)
        li, loff = _cat([np.ascontiguousarray(x[:, 0]) for x in lks], np.uint32)
        lo, _ = _cat([np.ascontiguousarray(x[:, 1]) for x in lks], np.uint32)
        lc, _ = _cat(lcs, np.uint32)
        has = np.array([a is not None for a in annotations], dtype=np.uint8)
        keep += [st, su, loff, li, lo, lc, has]
        G.support_total, G.support_unambiguous, G.link_offsets = st.ctypes.data, su.ctypes.data, loff.ctypes.data
        G.link_in, G.link_out, G.link_counts, G.has_threading = li.ctypes.data, lo.ctypes.data, lc.ctypes.data, has.ctypes.data
    return G, keep


def _pcr_params(ng, min_length, max_length, max_dfs_states, max_paths_per_pair, max_node_visits):
    cols = [_per_gene(v, ng, n) for v, n in ((min_length, "min_length"), (max_length, "max_length"), (max_dfs_states, "max_dfs_states"),
                                             (max_paths_per_pair, "max_paths_per_pair"), (max_node_visits, "max_node_visits"))]
    prm = (_PcrPathsParams * max(ng, 1))()
    for g in range(ng):
        prm[g] = _PcrPathsParams(*(int(c[g]) for c in cols))
    return prm


def _pcr_records_call(ng, call, retained=None):
    """Runs call(records struct) with room that grows once to what the call says it needs; one PcrProducts per gene."""
    roff = np.zeros(ng + 1, dtype=np.uint64)
    found, gen, states = (np.zeros(max(ng, 1), dtype=np.uint64) for _ in range(3))
    rcap, scap = max(64 * ng, 1), max(1 << 16, 1)
    for attempt in (0, 1):
        soff = np.zeros(rcap + 1, dtype=np.uint64)
        seqs = np.zeros(scap, dtype=np.uint8)
        start = np.zeros(rcap, dtype=np.uint32)
        nodes, cmin, cmax = (np.zeros(rcap, dtype=np.uint64) for _ in range(3))
        mean, med, score = (np.zeros(rcap, dtype=np.float64) for _ in range(3))
        fields = np.zeros((rcap, len(PCR_SCORE_FIELDS)), dtype=np.float64)
        R = _PcrRecords(roff.ctypes.data, soff.ctypes.data, seqs.ctypes.data, rcap, scap, 0, 0, start.ctypes.data, nodes.ctypes.data,
                        mean.ctypes.data, med.ctypes.data, cmin.ctypes.data, cmax.ctypes.data, score.ctypes.data, fields.ctypes.data,
                        found.ctypes.data, gen.ctypes.data, states.ctypes.data)
        rcode, check = call(R)
        if attempt == 0 and rcode == -2 and (R.n_records > rcap or R.n_seq_bytes > scap):  # too small: it says what it needs
            rcap, scap = max(rcap, int(R.n_records)), max(scap, int(R.n_seq_bytes))
            continue
        check(rcode)
        break
    res = []
    for g in range(ng):
        a, b = int(roff[g]), int(roff[g + 1])
        ss = [seqs[int(soff[r]):int(soff[r + 1])].tobytes().decode("ascii") for r in range(a, b)]
        res.append(PcrProducts(ss, start[a:b].copy(), nodes[a:b].copy(), mean[a:b].copy(), med[a:b].copy(), cmin[a:b].copy(),
                               cmax[a:b].copy(), score[a:b].copy(), fields[a:b].copy(), int(found[g]), int(gen[g]), int(states[g]),
                               None if retained is None else int(retained[g])))
    return res


class _PcrRecordBuf:
    """One shk_pcr_records with arrays of its own (ng genes, rcap records, scap sequence bytes): pcr_run_depths keeps one per
    depth.  struct(): what the call takes; after it, take(struct) copies the needs back and products() reads the arrays."""

    def __init__(self, ng: int, rcap: int, scap: int):
        self.ng, self.rcap, self.scap = ng, rcap, scap
        self.roff = np.zeros(ng + 1, dtype=np.uint64)
        self.found, self.gen, self.states = (np.zeros(max(ng, 1), dtype=np.uint64) for _ in range(3))
        n = max(rcap, 1)
        self.soff = np.zeros(n + 1, dtype=np.uint64)
        self.seqs = np.zeros(max(scap, 1), dtype=np.uint8)
        self.start = np.zeros(n, dtype=np.uint32)
        self.nodes, self.cmin, self.cmax = (np.zeros(n, dtype=np.uint64) for _ in range(3))
        self.mean, self.med, self.score = (np.zeros(n, dtype=np.float64) for _ in range(3))
        self.fields = np.zeros((n, len(PCR_SCORE_FIELDS)), dtype=np.float64)
        self.n_records = self.n_seq_bytes = 0

    def struct(self) -> "_PcrRecords":
        return _PcrRecords(self.roff.ctypes.data, self.soff.ctypes.data, self.seqs.ctypes.data, self.rcap, self.scap, 0, 0,
                           self.start.ctypes.data, self.nodes.ctypes.data, self.mean.ctypes.data, self.med.ctypes.data,
                           self.cmin.ctypes.data, self.cmax.ctypes.data, self.score.ctypes.data, self.fields.ctypes.data,
                           self.found.ctypes.data, self.gen.ctypes.data, self.states.ctypes.data)

    def take(self, R):
        self.n_records, self.n_seq_bytes = int(R.n_records), int(R.n_seq_bytes)

    def short(self) -> bool:
        return self.n_records > self.rcap or self.n_seq_bytes > self.scap

    def products(self) -> list:
        res = []
        for g in range(self.ng):
            a, b = int(self.roff[g]), int(self.roff[g + 1])
            ss = [self.seqs[int(self.soff[r]):int(self.soff[r + 1])].tobytes().decode("ascii") for r in range(a, b)]
            res.append(PcrProducts(ss, self.start[a:b].copy(), self.nodes[a:b].copy(), self.mean[a:b].copy(), self.med[a:b].copy(),
                                   self.cmin[a:b].copy(), self.cmax[a:b].copy(), self.score[a:b].copy(), self.fields[a:b].copy(),
                                   int(self.found[g]), int(self.gen[g]), int(self.states[g]), None))
        return res


def pcr_paths_panel(k: int, graphs, annotations=None, min_length=0, max_length=10000, max_dfs_states=100000, max_paths_per_pair=20,
                    max_node_visits=2) -> list:
    """resolve_bubbles, get_assembly_paths and generate_sequences_from_paths (pcr/bubble.rs, pcr/paths.rs:78-356) for
    every gene of a panel on the host, no device (shk_pcr_paths_panel) → one PcrProducts per gene, records in
    enumeration order.  graphs: the list pcr_prune_panel returns; annotations: the list thread_reads_panel returns, with
    None for a gene that had no reads; each parameter one value for all genes or one per gene."""
    L = load_library()
    G, keep = _pcr_graphs(graphs, annotations)
    ng = G.n_genes
    prm = _pcr_params(ng, min_length, max_length, max_dfs_states, max_paths_per_pair, max_node_visits)
    err = C.create_string_buffer(1024)

    def check(rc):
        if rc != 0:
            raise ShkError(rc, err.value.decode("utf-8", "replace"))

    return _pcr_records_call(ng, lambda R: (L.shk_pcr_paths_panel(k, C.byref(G), prm, C.byref(R), err, len(err)), check))


def edit_within(a, b, t: int) -> bool:
    """Levenshtein distance of two byte strings <= t (shk_edit_within): bounded_levenshtein(a, b, t).is_some()."""
    a = a.encode("latin-1") if isinstance(a, str) else bytes(a)
    b = b.encode("latin-1") if isinstance(b, str) else bytes(b)
    return bool(load_library().shk_edit_within(a, len(a), b, len(b), t))


def pcr_node_budget(n_bases_ingested: int) -> int:
    """compute_node_budget (pcr/graph.rs:40-52)."""
    return int(load_library().shk_pcr_node_budget(n_bases_ingested))


class _PcrGene(C.Structure):
    _fields_ = [("gene_name", C.c_char_p), ("forward_seq", C.c_char_p), ("reverse_seq", C.c_char_p), ("min_length", C.c_uint64),
                ("max_length", C.c_uint64), ("min_count", C.c_uint32), ("mismatches", C.c_uint32), ("trim", C.c_uint32),
                ("dedup_edit_threshold", C.c_uint32), ("max_dfs_states", C.c_uint64), ("max_paths_per_pair", C.c_uint64),
                ("max_node_visits", C.c_uint64), ("max_primer_kmers", C.c_uint32), ("reserved", C.c_uint32),
                ("high_coverage_ratio", C.c_double), ("tip_coverage_fraction", C.c_double)]


class _PcrRunParams(C.Structure):
    _fields_ = [("min_kmer_count", C.c_uint32), ("reads", C.c_uint32), ("paired", C.c_uint32), ("reserved", C.c_uint32),
                ("max_num_nodes", C.c_uint64), ("bases", C.c_void_p), ("offsets", C.c_void_p), ("n_seqs", C.c_uint64),
                ("read_index", C.c_void_p), ("mate", C.c_void_p), ("reserved2", C.c_uint64 * 4)]


_PCR_RUN_U32 = ("status", "n_fwd_kmers", "n_rev_kmers", "max_fwd_count", "max_rev_count", "median_primer_count", "threshold_used",
                "steps_run", "found_path")
_PCR_RUN_U64A = ("n_nodes", "n_edges", "n_pruned_nodes", "n_pruned_edges", "n_reads_matched")


class _PcrRunOut(C.Structure):
    _fields_ = ([("records", _PcrRecords)] + [(f, C.c_void_p) for f in _PCR_RUN_U32 + _PCR_RUN_U64A]
                + [("threaded", C.c_void_p), ("n_paired_links", C.c_void_p), ("low_primer_counts", C.c_void_p), ("reserved", C.c_uint64 * 4)])


class _PcrGeneStat(C.Structure):
    _fields_ = [("gene_name", C.c_char_p), ("status", C.c_uint32), ("n_products", C.c_uint32), ("product_lengths", C.c_void_p)]


class _PcrFileConfig(C.Structure):
    _fields_ = [("genes", C.POINTER(_PcrGene)), ("n_genes", C.c_uint32), ("min_kmer_count", C.c_uint32), ("read_threading", C.c_uint32),
                ("dump", C.c_uint32), ("node_budget_global", C.c_uint64), ("context_flags", C.c_uint64), ("depths", C.c_void_p), ("n_depths", C.c_uint64),
                ("reserved", C.c_uint64 * 1)]


PCR_SUCCESS, PCR_NO_FORWARD, PCR_NO_REVERSE, PCR_NO_PRIMERS, PCR_NO_PATH, PCR_NODE_BUDGET = range(6)  # SHK_PCR_* (include/shk.h)
PCR_READS_NONE, PCR_READS_RETAINED, PCR_READS_HOST = range(3)


@dataclass
class PcrGene:
    """PCRParams as do_pcr reads it (src/pcr/mod.rs), with the reference's defaults: shk_pcr_gene."""
    gene_name: str = ""
    forward_seq: str = ""
    reverse_seq: str = ""
    min_length: int = 0
    max_length: int = 10000
    min_count: int = 2
    mismatches: int = 2
    trim: int = 15
    dedup_edit_threshold: int = 10
    max_dfs_states: int = 100000
    max_paths_per_pair: int = 20
    max_node_visits: int = 2
    max_primer_kmers: int = 40
    high_coverage_ratio: float = 10.0
    tip_coverage_fraction: float = 0.1

    def _c(self) -> _PcrGene:
        return _PcrGene(self.gene_name.encode(), self.forward_seq.encode(), self.reverse_seq.encode(), self.min_length, self.max_length,
                        self.min_count, self.mismatches, self.trim, self.dedup_edit_threshold, self.max_dfs_states,
                        self.max_paths_per_pair, self.max_node_visits, self.max_primer_kmers, 0, self.high_coverage_ratio,
                        self.tip_coverage_fraction)


def _pcr_genes(genes):
    arr = (_PcrGene * max(len(genes), 1))()
    for i, g in enumerate(genes):
        arr[i] = g._c()
    return arr


def parse_pcr_primers(spec: str) -> PcrGene:
    """parse_pcr_primers_string (cli.rs:12-140): "forward=…,reverse=…,name=…[,max-length=…]" → PcrGene; ShkError with
    the reference's text otherwise (shk_pcr_parse_primers)."""
    L = load_front_library()
    raw = spec.encode()
    g = _PcrGene()
    strings, err = C.create_string_buffer(len(raw) + 3), C.create_string_buffer(2048 + 2 * len(raw))
    rc = L.shk_pcr_parse_primers(raw, C.byref(g), strings, len(strings), err, len(err))
    if rc != 0:
        raise ShkError(rc, err.value.decode("utf-8", "replace"))
    return PcrGene(g.gene_name.decode(), g.forward_seq.decode(), g.reverse_seq.decode(), int(g.min_length), int(g.max_length),
                   int(g.min_count), int(g.mismatches), int(g.trim), int(g.dedup_edit_threshold), int(g.max_dfs_states),
                   int(g.max_paths_per_pair), int(g.max_node_visits), int(g.max_primer_kmers), float(g.high_coverage_ratio),
                   float(g.tip_coverage_fraction))


def validate_pcr_gene(gene: PcrGene) -> list:
    """validate_pcr_params (pcr/mod.rs:295-399): the (error, suggestion) pairs, [] for a valid gene."""
    buf = C.create_string_buffer(8192 + 4 * (len(gene.forward_seq.encode()) + len(gene.reverse_seq.encode())))
    c = gene._c()
    n = load_front_library().shk_pcr_validate_gene(C.byref(c), buf, len(buf))
    lines = buf.value.decode("utf-8", "replace").split("\n")
    return [(lines[2 * i], lines[2 * i + 1]) for i in range(n)]


def pcr_validation_report(genes, sources=None) -> str:
    """The bail! text of collect_pcr_params (cli.rs:528-554) over the genes; "" when all are valid."""
    arr = _pcr_genes(genes)
    src = None
    if sources is not None:
        src = (C.c_char_p * max(len(genes), 1))(*[None if s is None else s.encode() for s in sources])
    buf = C.create_string_buffer(4096 + 4096 * len(genes))
    load_front_library().shk_pcr_validation_report(arr, len(genes), src, buf, len(buf))
    return buf.value.decode("utf-8", "replace")


def pcr_failure_reason(status: int):
    r = load_front_library().shk_pcr_failure_reason(status)
    return None if r is None else r.decode()


@dataclass
class PcrOutcome:
    """do_pcr's PcrOutcome for one gene (pcr/mod.rs:286-291) with the diagnostics shk_pcr_run keeps."""
    gene_name: str
    status: int                 # PCR_SUCCESS .. PCR_NODE_BUDGET
    failure_reason: str | None  # the reference's text; None on success
    products: PcrProducts       # the final products in product order (empty on a fail)
    n_fwd_kmers: int
    n_rev_kmers: int
    max_fwd_count: int
    max_rev_count: int
    median_primer_count: int
    threshold_used: int
    steps_run: int
    found_path: bool
    n_nodes: int
    n_edges: int
    n_pruned_nodes: int
    n_pruned_edges: int
    n_reads_matched: int
    threaded: bool
    n_paired_links: int
    low_primer_counts: bool


def _pcr_out_columns(O, ng: int) -> dict:
    """The per-gene column arrays of one out block (shk_pcr_run_out), bound into O."""
    n1 = max(ng, 1)
    cols = {f: np.zeros(n1, dtype=np.uint32) for f in _PCR_RUN_U32}
    cols.update({f: np.zeros(n1, dtype=np.uint64) for f in _PCR_RUN_U64A + ("n_paired_links",)})
    cols.update({f: np.zeros(n1, dtype=np.uint8) for f in ("threaded", "low_primer_counts")})
    for f, a in cols.items():
        setattr(O, f, a.ctypes.data)
    return cols


def _pcr_outcomes(genes, cols: dict, prods) -> list:
    """One PcrOutcome per gene from an out block's columns and its products."""
    out = []
    for g, gene in enumerate(genes):
        v = {f: int(a[g]) for f, a in cols.items()}
        v["found_path"], v["threaded"], v["low_primer_counts"] = bool(v["found_path"]), bool(v["threaded"]), bool(v["low_primer_counts"])
        out.append(PcrOutcome(gene_name=gene.gene_name, failure_reason=pcr_failure_reason(v["status"]), products=prods[g], **v))
    return out


def _records_struct(recs: PcrProducts):
    """One gene's PcrProducts as a shk_pcr_records (and the arrays it points into)."""
    n = len(recs.sequences)
    seqs = np.frombuffer("".join(recs.sequences).encode("ascii"), dtype=np.uint8).copy() if n else np.zeros(1, dtype=np.uint8)
    soff = np.zeros(n + 1, dtype=np.uint64)
    soff[1:] = np.cumsum([len(s) for s in recs.sequences])
    roff = np.array([0, n], dtype=np.uint64)
    cols = [np.ascontiguousarray(a, dtype=dt) for a, dt in ((recs.count_mean, np.float64), (recs.count_median, np.float64),
                                                            (recs.count_min, np.uint64), (recs.count_max, np.uint64),
                                                            (recs.score, np.float64))]
    R = _PcrRecords(roff.ctypes.data, soff.ctypes.data, seqs.ctypes.data, n, len(seqs), n, int(soff[n]), None, None, cols[0].ctypes.data,
                    cols[1].ctypes.data, cols[2].ctypes.data, cols[3].ctypes.data, cols[4].ctypes.data, None, None, None, None)
    return R, [seqs, soff, roff] + cols


def write_fasta(path: str, sample: str, gene_name: str, products: PcrProducts):
    """write_fasta_record (io.rs:144-158) for a gene's products: the headers of PcrProducts.fasta, sequences wrapped at
    80 columns (shk_write_fasta)."""
    R, keep = _records_struct(products)
    g = PcrGene(gene_name=gene_name)._c()
    rc = load_front_library().shk_write_fasta(os.fsencode(path), sample.encode(), C.byref(g), C.byref(R), 0, len(products.sequences))
    if rc != 0:
        raise ShkError(rc, "shk_write_fasta failed")


class _Synth(C.Structure):
    _fields_ = [("seed_genome", C.c_uint64), ("seed_reads", C.c_uint64), ("genome_len", C.c_uint64),
                ("read_len", C.c_uint32), ("sub_per_64k", C.c_uint32), ("n_per_64k", C.c_uint32),
                ("reserved", C.c_uint32)]


class _FastqTextParams(C.Structure):  # shk_fastq_text_params
    _fields_ = [("first_record", C.c_uint64), ("validate_every", C.c_uint64), ("max_records", C.c_uint64),
                ("last", C.c_uint32), ("reserved", C.c_uint32)]


class _FastqTextResult(C.Structure):  # shk_fastq_text_result
    _fields_ = [("n_records", C.c_uint64), ("n_bases", C.c_uint64), ("bytes_consumed", C.c_uint64),
                ("anomaly_record", C.c_uint64), ("anomaly_kind", C.c_uint32), ("reserved", C.c_uint32)]


class _FastqDeviceStats(C.Structure):  # shk_fastq_device_stats
    _fields_ = [("n_batches", C.c_uint64), ("n_members", C.c_uint64), ("n_records", C.c_uint64), ("n_bases", C.c_uint64),
                ("bytes_up", C.c_uint64), ("bytes_down", C.c_uint64), ("kernel_ns", C.c_uint64),
                ("gave_up", C.c_uint32), ("give_up_reason", C.c_uint32)]


# every symbol include/shk.h declares (tests check the .so exports them all)
ABI_SYMBOLS = [
    "shk_abi_version", "shk_create", "shk_destroy", "shk_reset", "shk_last_error", "shk_ingest_batch",
    "shk_ingest_reads", "shk_set_read_index", "shk_ingest_reads_device", "shk_insert_counts", "shk_sync", "shk_finalize",
    "shk_histograms", "shk_get_counters", "shk_get_timings", "shk_reset_timings", "shk_get_lazy_table_timing", "shk_get_scatter_segments",
    "shk_export_table", "shk_lookup", "shk_find_oligos", "shk_primer_compile", "shk_primer_kmers", "shk_filter_reads", "shk_kmers_from_reads", "shk_table_geometry", "shk_table_reserve_pages", "shk_owner_counts", "shk_compact_owners",
    "shk_merge_entries",
    "shk_table_device_ptrs", "shk_merge_pages", "shk_set_owned_pages", "shk_alloc_pinned",
    "shk_free_pinned", "shk_alloc_device", "shk_free_device", "shk_release_cached_memory", "shk_synth_reads_device",
    "shk_fastq_open", "shk_fastq_open_ex", "shk_fastq_close", "shk_fastq_error", "shk_fastq_next_batch", "shk_fastq_next_batch_packed", "shk_fastq_stats",
    "shk_fastq_open_device", "shk_fastq_member_stats", "shk_bgzf_device_totals",
    "shk_fastq_parse_device", "shk_crc32_members_device", "shk_fastq_parse_geometry", "shk_ingest_fastq_files_device", "shk_fastq_device_totals",
    "shk_write_histo", "shk_write_final_histo", "shk_write_stats_yaml", "shk_validate_args",
    "shk_run_error", "shk_run_files",
    "shk_xchg_scatter_device", "shk_xchg_absorb", "shk_xchg_spill", "shk_xchg_spill_clear", "shk_insert_device",
    "shk_xchg_wide_scatter_device", "shk_xchg_feasible", "shk_xchg_scatter_begin", "shk_xchg_scatter_end",
    "shk_stream", "shk_compact_owners_packed", "shk_compact_owners_fixed", "shk_merge_pieces_max", "shk_merge_pieces", "shk_set_owner_share", "shk_finalize_begin", "shk_finalize_end",
    "shk_packed_sizes", "shk_pack_reads", "shk_ingest_packed", "shk_ingest_packed_device", "shk_pack_reads_device",
    "shk_unpack_reads_device",
    "shk_neighborhood", "shk_pcr_extend", "shk_pcr_node_budget", "shk_neighborhood_panel", "shk_pcr_extend_panel",
    "shk_pcr_prune_panel", "shk_pcr_paths_panel", "shk_edit_within", "shk_pcr_dedup_panel", "shk_pcr_products_panel",
    "shk_thread_reads", "shk_thread_reads_device", "shk_thread_reads_panel", "shk_thread_reads_panel_device",
    "shk_filter_reads_panel", "shk_filter_reads_panel_device", "shk_gather_reads_device",
    "shk_retain_reads", "shk_retained_info", "shk_retained_export", "shk_filter_reads_panel_retained",
    "shk_thread_reads_panel_retained",
    "shk_pcr_gene_defaults", "shk_pcr_parse_primers", "shk_pcr_validate_gene", "shk_pcr_validation_report", "shk_pcr_failure_reason",
    "shk_pcr_run", "shk_write_fasta", "shk_write_stats_yaml_pcr", "shk_run_files_pcr",
    "shk_key_owner",
    "shk_chunk_bases", "shk_lookup_depth", "shk_primer_kmers_depths", "shk_neighborhood_panel_depths", "shk_pcr_extend_panel_depths",
    "shk_pcr_run_depths", "shk_pcr_check_depths", "shk_pcr_parse_depths", "shk_write_pcr_depths_tsv",
]

_lib = None


def _share_hip_runtime_with_torch():
    """PyTorch-ROCm wheels bundle their own libamdhip64.so (SONAME libamdhip64.so.7, the same
    as /opt/rocm's).  Two HIP/HSA runtimes in one process cannot both open the GPU, so when
    torch is installed we load ITS copy first (by path, without importing torch); libshk's
    NEEDED libamdhip64.so.7 then binds to it, and a later `import torch` reuses the same
    file.  Without torch, libshk uses the system ROCm runtime."""
    import importlib.util
    import sys
    if "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if not spec or not spec.submodule_search_locations:
        return
    cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.exists(cand):
        try:
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
        except OSError:
            pass


FRONT_SYMBOLS = [
    "shk_fastq_open", "shk_fastq_open_ex", "shk_fastq_close", "shk_fastq_error", "shk_fastq_next_batch", "shk_fastq_next_batch_packed", "shk_fastq_stats",
    "shk_fastq_open_device", "shk_fastq_member_stats",
    "shk_write_histo", "shk_write_final_histo", "shk_write_stats_yaml", "shk_validate_args", "shk_run_error",
    "shk_packed_sizes", "shk_pack_reads",
    "shk_pcr_gene_defaults", "shk_pcr_parse_primers", "shk_pcr_validate_gene", "shk_pcr_validation_report", "shk_pcr_failure_reason",
    "shk_write_fasta", "shk_write_stats_yaml_pcr",
    "shk_pcr_check_depths", "shk_pcr_parse_depths", "shk_write_pcr_depths_tsv",
]


def _type_front(L):
    """The entry points of the plain-C++ host side (csrc/shk_front.cpp): FASTQ front-end, packer, writers."""
    vp, u64, u32 = C.c_void_p, C.c_uint64, C.c_uint32
    L.shk_packed_sizes.argtypes = [u64, C.POINTER(u64), C.POINTER(u64)]
    L.shk_packed_sizes.restype = None
    L.shk_pack_reads.argtypes = [vp, u64, vp, vp, u32]
    L.shk_fastq_open.argtypes = [C.POINTER(C.c_char_p), u32, u64, u64, C.POINTER(vp)]
    L.shk_fastq_open_ex.argtypes = [C.POINTER(C.c_char_p), u32, u64, u64, u32, C.POINTER(vp)]
    L.shk_fastq_close.argtypes = [vp]
    L.shk_fastq_close.restype = None
    L.shk_fastq_error.argtypes = [vp]
    L.shk_fastq_error.restype = C.c_char_p
    L.shk_fastq_next_batch.argtypes = [vp, vp, u64, vp, u64, C.POINTER(u64)]
    L.shk_fastq_next_batch_packed.argtypes = [vp, vp, vp, u64, vp, u64, C.POINTER(u64)]
    L.shk_fastq_stats.argtypes = [vp, C.POINTER(u64), C.POINTER(u64), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.shk_fastq_open_device.argtypes = [C.POINTER(C.c_char_p), u32, u64, u64, u32, C.c_int, C.POINTER(vp)]
    L.shk_fastq_member_stats.argtypes = [vp, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64)]
    L.shk_write_histo.argtypes = [C.c_char_p, C.c_char_p, u32, u32, u64, vp]
    L.shk_write_final_histo.argtypes = [C.c_char_p, C.c_char_p, u32, u32, u64, vp]
    L.shk_write_stats_yaml.argtypes = [C.c_char_p, C.POINTER(_RunStats)]
    L.shk_validate_args.argtypes = [u32, u64, C.c_char_p]
    L.shk_run_error.argtypes = []
    L.shk_run_error.restype = C.c_char_p
    L.shk_pcr_gene_defaults.argtypes = [C.POINTER(_PcrGene)]
    L.shk_pcr_gene_defaults.restype = None
    L.shk_pcr_parse_primers.argtypes = [C.c_char_p, C.POINTER(_PcrGene), C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t]
    L.shk_pcr_validate_gene.argtypes = [C.POINTER(_PcrGene), C.c_char_p, C.c_size_t]
    L.shk_pcr_validation_report.argtypes = [C.POINTER(_PcrGene), u32, C.POINTER(C.c_char_p), C.c_char_p, C.c_size_t]
    L.shk_pcr_failure_reason.argtypes = [u32]
    L.shk_pcr_failure_reason.restype = C.c_char_p
    L.shk_write_fasta.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(_PcrGene), C.POINTER(_PcrRecords), u64, u64]
    L.shk_write_stats_yaml_pcr.argtypes = [C.c_char_p, C.POINTER(_RunStats), C.POINTER(_PcrGeneStat), u32]
    L.shk_pcr_check_depths.argtypes = [vp, u64, u32, C.c_char_p, C.c_size_t]
    L.shk_pcr_parse_depths.argtypes = [C.c_char_p, u32, vp, u64, C.POINTER(u64), C.c_char_p, C.c_size_t]
    L.shk_write_pcr_depths_tsv.argtypes = [C.c_char_p, vp, u64]


_front = None


def load_front_library():
    """The library the host-side entry points are called in: libshk.so — or, with SHK_FRONT_LIB set, a build of
    csrc/shk_front.cpp + shk_inflate.cpp alone (the sanitizer builds of `make -C sharkmer_amd/csrc san`, which
    tests/test_host_san.py runs the CPU tests against)."""
    global _front
    if _front is not None:
        return _front
    alt = os.environ.get("SHK_FRONT_LIB")
    if not alt:
        _front = load_library()
        return _front
    L = C.CDLL(alt)
    _type_front(L)
    for name in FRONT_SYMBOLS:
        getattr(L, name)
    _front = L
    return L


def load_library():
    """dlopen libshk.so and type its entry points.  Raises if the HIP build is missing."""
    global _lib
    if _lib is not None:
        return _lib
    p = lib_path()
    if not os.path.exists(p):
        raise ShkError(-9, f"{p} not found: build it with __graft_entry__.build() "
                           f"(hipcc --offload-arch=gfx950); libshk has no CPU fallback")
    _share_hip_runtime_with_torch()
    L = C.CDLL(p)
    vp, u64, u32 = C.c_void_p, C.c_uint64, C.c_uint32
    L.shk_abi_version.restype = C.c_int
    L.shk_create.argtypes = [C.POINTER(_Config), C.POINTER(vp)]
    L.shk_create.restype = C.c_int
    L.shk_destroy.argtypes = [vp]
    L.shk_destroy.restype = None
    L.shk_reset.argtypes = [vp]
    L.shk_last_error.argtypes = [vp]
    L.shk_last_error.restype = C.c_char_p
    L.shk_ingest_batch.argtypes = [vp, u32, vp, vp, u64]
    L.shk_ingest_reads.argtypes = [vp, vp, vp, u64]
    L.shk_ingest_reads_device.argtypes = [vp, vp, vp, u64, u64]
    L.shk_fastq_parse_device.argtypes = [vp, vp, u64, C.POINTER(_FastqTextParams), vp, u64, vp, u64, C.POINTER(_FastqTextResult)]
    L.shk_crc32_members_device.argtypes = [vp, vp, vp, u32, vp]
    L.shk_fastq_parse_geometry.argtypes = [C.POINTER(u32)]
    L.shk_fastq_parse_geometry.restype = None
    L.shk_ingest_fastq_files_device.argtypes = [vp, C.POINTER(C.c_char_p), u32, u64, u64, C.POINTER(_FastqDeviceStats)]
    L.shk_fastq_device_totals.argtypes = [C.POINTER(u64)] * 6
    L.shk_insert_counts.argtypes = [vp, u32, vp, vp, u64]
    L.shk_sync.argtypes = [vp]
    L.shk_finalize.argtypes = [vp]
    L.shk_histograms.argtypes = [vp, vp]
    L.shk_get_counters.argtypes = [vp, C.POINTER(_Counters)]
    L.shk_get_timings.argtypes = [vp, C.POINTER(_Timings)]
    L.shk_reset_timings.argtypes = [vp]
    L.shk_get_lazy_table_timing.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
    L.shk_get_scatter_segments.argtypes = [vp, C.POINTER(C.c_uint32)]
    L.shk_export_table.argtypes = [vp, vp, vp, u64, C.POINTER(u64)]
    L.shk_lookup.argtypes = [vp, vp, vp, u64, C.c_int]
    L.shk_find_oligos.argtypes = [vp, vp, u32, u32, u32, vp, vp, u64, C.POINTER(u64)]
    L.shk_primer_compile.argtypes = [C.POINTER(_Primer), u32, C.POINTER(u32), C.POINTER(u32), vp, C.c_char_p,
                                     C.c_size_t]
    L.shk_primer_kmers.argtypes = [vp, vp, u32, vp, vp, vp, u64, vp, vp]
    L.shk_filter_reads.argtypes = [vp, vp, vp, u64, vp, u64, vp]
    L.shk_kmers_from_reads.argtypes = [vp, vp, vp, u64, vp, u64, vp, vp]
    L.shk_neighborhood.argtypes = [vp, vp, vp, u64, u32, u32, vp, vp, u64, C.POINTER(u64), vp, vp, u64, C.POINTER(u64),
                                   C.POINTER(u32)]
    L.shk_pcr_extend.argtypes = [vp, vp, vp, u64, vp, vp, u64, C.POINTER(_PcrExtendParams), vp, vp, u64, C.POINTER(u64),
                                 vp, vp, vp, u64, C.POINTER(u64), C.POINTER(u32), C.POINTER(u32), C.POINTER(u32)]
    L.shk_pcr_node_budget.argtypes = [u64]
    L.shk_neighborhood_panel.argtypes = [vp, vp, vp, vp, u32, vp, u32, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.shk_pcr_extend_panel.argtypes = [vp, vp, vp, vp, u32, vp, vp, vp, vp, u64, vp, vp, vp, vp, u64, vp, vp, vp]
    L.shk_pcr_prune_panel.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, u32, vp, C.POINTER(_PcrPruneOut)]
    L.shk_pcr_paths_panel.argtypes = [u32, C.POINTER(_PcrGraphs), vp, C.POINTER(_PcrRecords), C.c_char_p, C.c_size_t]
    L.shk_edit_within.argtypes = [C.c_char_p, u64, C.c_char_p, u64, u32]
    L.shk_pcr_dedup_panel.argtypes = [vp, vp, vp, vp, vp, vp, u32, C.POINTER(_PcrDedupOut)]
    L.shk_pcr_products_panel.argtypes = [vp, C.POINTER(_PcrGraphs), vp, vp, C.POINTER(_PcrRecords), vp, C.POINTER(C.c_double)]
    L.shk_thread_reads.argtypes = [vp, vp, u64, vp, vp, u64, vp, vp, u64, vp, vp, C.POINTER(_ThreadOut)]
    L.shk_thread_reads_device.argtypes = [vp, vp, u64, vp, vp, u64, vp, vp, u64, u64, vp, vp, C.POINTER(_ThreadOut)]
    L.shk_thread_reads_panel.argtypes = [vp, vp, vp, vp, vp, vp, u32, vp, vp, u64, vp, vp, vp, vp, C.POINTER(_ThreadPanelOut)]
    L.shk_thread_reads_panel_device.argtypes = [vp, vp, vp, vp, vp, vp, u32, vp, vp, u64, u64, vp, vp, vp, vp,
                                                C.POINTER(_ThreadPanelOut)]
    L.shk_filter_reads_panel.argtypes = [vp, vp, vp, u64, vp, vp, u32, vp, vp, u64, C.POINTER(u64)]
    L.shk_filter_reads_panel_device.argtypes = [vp, vp, vp, u64, u64, vp, vp, u32, vp, vp, u64, C.POINTER(u64)]
    L.shk_gather_reads_device.argtypes = [vp, vp, vp, u64, vp, u64, vp, u64, vp, C.POINTER(u64)]
    L.shk_retain_reads.argtypes = [vp, C.c_int, u64]
    L.shk_retained_info.argtypes = [vp, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64)]
    L.shk_retained_export.argtypes = [vp, u64, u64, vp, u64, vp, C.POINTER(u64)]
    L.shk_filter_reads_panel_retained.argtypes = [vp, vp, vp, u32, vp, vp, u64, C.POINTER(u64)]
    L.shk_thread_reads_panel_retained.argtypes = [vp, vp, vp, vp, vp, vp, u32, vp, vp, vp, vp, C.POINTER(_ThreadPanelOut)]
    L.shk_pcr_node_budget.restype = u64
    L.shk_owner_counts.argtypes = [vp, u32, vp]
    L.shk_compact_owners.argtypes = [vp, u32, vp, vp, vp, u64, C.c_int32]
    L.shk_merge_entries.argtypes = [vp, vp, vp, u64, u64]
    L.shk_compact_owners_packed.argtypes = [vp, u32, vp, vp, C.c_int32]
    L.shk_compact_owners_fixed.argtypes = [vp, u32, u64, vp, C.c_int32]
    L.shk_merge_pieces_max.argtypes = [vp, vp]
    L.shk_merge_pieces.argtypes = [vp, vp, u32, u64, C.c_int32]
    L.shk_set_owner_share.argtypes = [vp, u32, u32]
    L.shk_finalize_begin.argtypes = [vp, u64, C.POINTER(vp), C.POINTER(u64)]
    L.shk_finalize_end.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(u64)]
    L.shk_table_geometry.argtypes = [vp, C.POINTER(u64), C.POINTER(u32), C.POINTER(u32)]
    L.shk_table_reserve_pages.argtypes = [vp, u64]
    L.shk_table_device_ptrs.argtypes = [vp, C.POINTER(vp), C.POINTER(vp)]
    L.shk_merge_pages.argtypes = [vp, u64, u64, vp, vp, u64]
    L.shk_set_read_index.argtypes = [vp, u64]
    L.shk_xchg_scatter_device.argtypes = [vp, vp, vp, u64, u64, u64, C.POINTER(vp), C.POINTER(vp),
                                          C.POINTER(XchgLayout), C.POINTER(u64)]
    L.shk_xchg_scatter_begin.argtypes = [vp, vp, vp, u64, u64, u64, C.POINTER(vp), C.POINTER(vp), C.POINTER(XchgLayout)]
    L.shk_xchg_scatter_end.argtypes = [vp, C.POINTER(u64)]
    L.shk_xchg_absorb.argtypes = [vp, vp, vp, C.POINTER(XchgLayout)]
    L.shk_xchg_spill.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(u64)]
    L.shk_xchg_spill_clear.argtypes = [vp]
    L.shk_insert_device.argtypes = [vp, vp, vp, vp, u64]
    L.shk_release_cached_memory.argtypes = []
    L.shk_release_cached_memory.restype = None
    L.shk_xchg_wide_scatter_device.argtypes = [vp, vp, vp, u64, u64, C.POINTER(vp), C.POINTER(vp), C.POINTER(u64)]
    L.shk_xchg_feasible.argtypes = [vp]
    L.shk_stream.argtypes = [vp]
    L.shk_stream.restype = vp
    L.shk_ingest_packed.argtypes = [vp, vp, vp, vp, u64]
    L.shk_ingest_packed_device.argtypes = [vp, vp, vp, vp, u64, u64]
    L.shk_pack_reads_device.argtypes = [vp, vp, u64, vp, vp]
    L.shk_unpack_reads_device.argtypes = [vp, vp, vp, u64, vp]
    L.shk_set_owned_pages.argtypes = [vp, u64, u64]
    L.shk_alloc_pinned.argtypes = [C.c_size_t]
    L.shk_alloc_pinned.restype = vp
    L.shk_free_pinned.argtypes = [vp]
    L.shk_free_pinned.restype = None
    L.shk_alloc_device.argtypes = [vp, C.c_size_t]
    L.shk_alloc_device.restype = vp
    L.shk_free_device.argtypes = [vp, vp]
    L.shk_free_device.restype = None
    L.shk_synth_reads_device.argtypes = [vp, C.POINTER(_Synth), u64, u64, vp, vp]
    _type_front(L)
    L.shk_run_files.argtypes = [C.POINTER(_RunConfig), C.POINTER(_RunStats)]
    L.shk_run_files_pcr.argtypes = [C.POINTER(_RunConfig), C.POINTER(_PcrFileConfig), C.POINTER(_RunStats), C.POINTER(_PcrRunOut)]
    L.shk_pcr_run.argtypes = [vp, C.POINTER(_PcrGene), u32, C.POINTER(_PcrRunParams), C.POINTER(_PcrRunOut)]
    L.shk_chunk_bases.argtypes = [vp, vp]
    L.shk_lookup_depth.argtypes = [vp, vp, vp, u64, C.c_int, u32]
    L.shk_primer_kmers_depths.argtypes = [vp, vp, u32, vp, u32, vp, vp, vp, u64, vp, vp]
    L.shk_neighborhood_panel_depths.argtypes = [vp, vp, vp, vp, u32, vp, vp, u32, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.shk_pcr_extend_panel_depths.argtypes = [vp, vp, vp, vp, u32, vp, vp, vp, vp, vp, u64, vp, vp, vp, vp, u64, vp, vp, vp]
    L.shk_pcr_run_depths.argtypes = [vp, C.POINTER(_PcrGene), u32, C.POINTER(_PcrRunParams), vp, u32, C.POINTER(_PcrRunOut)]
    for name in ABI_SYMBOLS:
        getattr(L, name)  # AttributeError here = the .so is stale
    _lib = L
    return L


class KmerEngine:
    """One counting context on one GPU.

    k, chunks, histo_max: the reference's -k / --chunks / --histo-max
    (cli.rs:207-224; validated like cli.rs:659-677 except "k odd", which is the
    CLI's rule).  capacity_hint: expected number of distinct k-mers."""

    def __init__(self, k: int, chunks: int = 0, histo_max: int = 10000, device: int = 0,
                 capacity_hint: int = 0, flags: int = 0, n_owners: int = 0, owner_id: int = 0,
                 device_ids=None, reserve_cus: int = 0):
        """n_owners/owner_id: an OWNER SHARE — the context holds 1/n_owners of the key space
        (shk_config.n_owners).  device_ids: a multi-device context (shk_config.n_devices).
        reserve_cus: compute units the context's kernels leave free (shk_config.reserve_cus; 0 = the
        library's default, RESERVE_NONE = none)."""
        self._L = load_library()
        self.k, self.chunks, self.histo_max = k, chunks, histo_max
        self.n_owners, self.owner_id = max(n_owners, 1), owner_id
        self._tdev = f"cuda:{device}"  # torch tensors over this context's memory live on ITS device, whatever torch's current one is
        cfg = _Config(k=k, chunks=chunks, histo_max=histo_max, device=device, flags=flags,
                      table_capacity_hint=capacity_hint, n_owners=n_owners, owner_id=owner_id, reserve_cus=reserve_cus)
        if device_ids is not None:
            ids = (C.c_int32 * len(device_ids))(*device_ids)
            cfg.n_devices = len(device_ids)
            cfg.device_ids = C.cast(ids, C.POINTER(C.c_int32))
        h = C.c_void_p()
        rc = self._L.shk_create(C.byref(cfg), C.byref(h))
        if rc != 0:
            raise ShkError(rc, (self._L.shk_last_error(None) or b"").decode("utf-8", "replace"))
        self._h = h

    last_prune_device_ms = 0.0  # shk_pcr_prune_out.device_ms of the last pcr_prune_panel call
    prune_first_cap = 1 << 22   # pcr_prune_panel's first guess at the room the pruned panel needs, nodes and edges each

    # -- plumbing ------------------------------------------------------------------------
    def _check(self, rc: int):
        if rc != 0:
            raise ShkError(rc, (self._L.shk_last_error(self._h) or b"").decode("utf-8", "replace"))

    def close(self):
        if getattr(self, "_h", None):
            self._L.shk_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    @staticmethod
    def _pack(seqs):
        bs = [s.encode("latin-1") if isinstance(s, str) else bytes(s) for s in seqs]
        offsets = np.zeros(len(bs) + 1, dtype=np.uint64)
        if bs:
            offsets[1:] = np.cumsum([len(b) for b in bs])
        bases = np.frombuffer(b"".join(bs), dtype=np.uint8) if bs else np.zeros(0, dtype=np.uint8)
        return bases, offsets

    # -- ingest --------------------------------------------------------------------------
    def ingest_batch(self, chunk_id: int, bases: np.ndarray, offsets: np.ndarray):
        """drain_batch body (io.rs:356-358): all sequences to `chunk_id`."""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        self._check(self._L.shk_ingest_batch(self._h, chunk_id, bases.ctypes.data, offsets.ctypes.data,
                                             len(offsets) - 1))

    def ingest_reads(self, bases: np.ndarray, offsets: np.ndarray):
        """read_fastq cadence (io.rs:335-343,355-361): read i → chunk (i//1000) % n_chunks."""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        self._check(self._L.shk_ingest_reads(self._h, bases.ctypes.data, offsets.ctypes.data,
                                             len(offsets) - 1))

    def ingest_packed(self, pk: "PackedReads"):
        """shk_ingest_packed: a batch packed by pack_reads (2-bit stream + N mask + base offsets)."""
        self._check(self._L.shk_ingest_packed(self._h, pk.packed.ctypes.data, pk.nmask.ctypes.data,
                                              pk.offsets.ctypes.data, len(pk.offsets) - 1))

    def ingest_packed_slice(self, pk: "PackedReads", first_seq: int, n_seqs: int):
        """shk_ingest_packed over reads [first_seq, first_seq + n_seqs) of a packed batch: the offsets are positions in
        the batch's streams, so a slice is the same two streams and a window of the offsets."""
        assert 0 <= first_seq and first_seq + n_seqs <= len(pk.offsets) - 1
        self._check(self._L.shk_ingest_packed(self._h, pk.packed.ctypes.data, pk.nmask.ctypes.data,
                                              pk.offsets.ctypes.data + 8 * first_seq, n_seqs))

    def ingest_packed_device(self, d_packed: int, d_nmask: int, d_offsets: int, n_seqs: int, n_bases: int):
        self._check(self._L.shk_ingest_packed_device(self._h, d_packed, d_nmask, d_offsets, n_seqs, n_bases))

    def pack_reads_device(self, d_bases: int, n_bases: int, d_packed: int, d_nmask: int):
        self._check(self._L.shk_pack_reads_device(self._h, d_bases, n_bases, d_packed, d_nmask))

    def unpack_reads_device(self, d_packed: int, d_nmask: int, n_bases: int, d_bases: int):
        self._check(self._L.shk_unpack_reads_device(self._h, d_packed, d_nmask, n_bases, d_bases))

    def ingest_seqs(self, seqs):
        """Convenience: a list of str/bytes sequences in input order."""
        self.ingest_reads(*self._pack(seqs))

    def ingest_seq(self, seq, chunk_id: int = 0):
        """Chunk::ingest_seq (chunk.rs:25-30) for one sequence (launch-bound; tests only)."""
        self.ingest_batch(chunk_id, *self._pack([seq]))

    def ingest_reads_device(self, d_bases: int, d_offsets: int, n_seqs: int, n_bases: int):
        self._check(self._L.shk_ingest_reads_device(self._h, d_bases, d_offsets, n_seqs, n_bases))

    # -- FASTQ text on the device ------------------------------------------
    def parse_fastq_text(self, d_text: int, n_bytes: int, d_bases: int, bases_cap: int, d_offsets: int, offsets_cap: int,
                         first_record: int = 0, validate_every: int = 0, max_records: int = 0, last: bool = True) -> dict:
        """shk_fastq_parse_device: the records of n_bytes of FASTQ text at device pointer d_text (any alignment) framed
        into d_bases / d_offsets (what ingest_reads_device takes).  A capacity that is too small raises ShkError whose
        .needed says what the text needs."""
        p = _FastqTextParams(first_record, validate_every, max_records, 1 if last else 0, 0)
        r = _FastqTextResult()
        rc = self._L.shk_fastq_parse_device(self._h, d_text, n_bytes, C.byref(p), d_bases, bases_cap, d_offsets, offsets_cap, C.byref(r))
        out = {f: int(getattr(r, f)) for f, _ in _FastqTextResult._fields_ if f != "reserved"}
        if rc != 0:
            e = ShkError(rc, (self._L.shk_last_error(self._h) or b"").decode("utf-8", "replace"))
            e.needed = out
            raise e
        return out

    def crc32_members(self, d_text: int, d_jobs: int, n: int, d_crc: int):
        """shk_crc32_members_device: gzip's CRC-32 of n extents of d_text (d_jobs: n × (u64 offset, u32 len, u32 0)),
        one wave each, into d_crc[n] u32."""
        self._check(self._L.shk_crc32_members_device(self._h, d_text, d_jobs, n, d_crc))

    def ingest_fastq_files(self, paths, max_reads: int = 0, validate_every: int = 0) -> dict:
        """shk_ingest_fastq_files_device: bgzip'd FASTQ files into this (empty) engine with the text never leaving the
        device.  The dict is shk_fastq_device_stats; gave_up != 0: nothing of the files is in the engine (1: it has
        been reset) and the caller reads them through FastqReader."""
        arr = (C.c_char_p * max(len(paths), 1))(*[os.fsencode(p) for p in paths])
        st = _FastqDeviceStats()
        self._check(self._L.shk_ingest_fastq_files_device(self._h, arr, len(paths), max_reads, validate_every, C.byref(st)))
        return {f: int(getattr(st, f)) for f, _ in _FastqDeviceStats._fields_}

    @staticmethod
    def fastq_device_totals() -> dict:
        """shk_fastq_device_totals (process-wide): batches, records, give_ups, bytes_up, bytes_down, kernel_ns."""
        return fastq_device_totals()

    def insert(self, kmers, counts, chunk_id: int = 0):
        """KmerCounts::insert (counting.rs:152-154)."""
        kmers = np.ascontiguousarray(np.atleast_1d(kmers), dtype=np.uint64)
        counts = np.ascontiguousarray(np.atleast_1d(counts), dtype=np.uint32)
        assert len(kmers) == len(counts)
        self._check(self._L.shk_insert_counts(self._h, chunk_id, kmers.ctypes.data, counts.ctypes.data,
                                              len(kmers)))

    def sync(self):
        self._check(self._L.shk_sync(self._h))

    def reset(self):
        """Empty chunks and zero counters, keeping allocations (a fresh FastqReadState)."""
        self._check(self._L.shk_reset(self._h))

    # -- consolidate -------------------------------------------------------------------
    def finalize(self):
        self._check(self._L.shk_finalize(self._h))
        return self

    def finalize_begin(self, user_word: int = 0):
        """shk_finalize_begin: queues the scan; returns the int64 CUDA tensor (a view of the engine's control block)
        a reduction over the ranks may sum in place — on the engine's stream."""
        p, n = C.c_void_p(), C.c_uint64()
        self._check(self._L.shk_finalize_begin(self._h, user_word, C.byref(p), C.byref(n)))
        return self._raw_tensor(p.value, int(n.value), "<i8", self._tdev)

    def finalize_end(self):
        """shk_finalize_end → (again, Σ user_word)."""
        again, usum = C.c_int(0), C.c_uint64(0)
        self._check(self._L.shk_finalize_end(self._h, C.byref(again), C.byref(usum)))
        return bool(again.value), int(usum.value)

    def histograms(self, out: np.ndarray | None = None) -> np.ndarray:
        """histo_vecs (io.rs:1020-1028): (chunks, histo_max+2) u64.  out: a caller-owned array of that shape to
        fill (a job of a few hundred µs notices the allocation of a fresh one)."""
        if out is None:
            out = np.empty((self.chunks, self.histo_max + 2), dtype=np.uint64)
        else:
            assert out.shape == (self.chunks, self.histo_max + 2) and out.dtype == np.uint64 and out.flags.c_contiguous
        self._check(self._L.shk_histograms(self._h, out.ctypes.data))
        return out

    def counters(self) -> dict:
        c = _Counters()
        self._check(self._L.shk_get_counters(self._h, C.byref(c)))
        return {f: int(getattr(c, f)) for f, _ in _Counters._fields_}

    def timings(self) -> dict:
        t = _Timings()
        self._check(self._L.shk_get_timings(self._h, C.byref(t)))
        out = {KERNEL_NAMES[i]: (float(t.ms[i]), int(t.launches[i]))
               for i in range(len(KERNEL_NAMES)) if t.launches[i]}
        ms, n = C.c_double(0), C.c_uint64(0)   # the materialising pass of a lazily written table: beside shk_timings
        self._check(self._L.shk_get_lazy_table_timing(self._h, C.byref(ms), C.byref(n)))
        if n.value:
            out["materialise"] = (float(ms.value), int(n.value))
        return out

    def scatter_segments(self) -> int:
        """Cursor segments per page region of the last paged counting launch (0: none yet)."""
        s = C.c_uint32(0)
        self._check(self._L.shk_get_scatter_segments(self._h, C.byref(s)))
        return int(s.value)

    def reset_timings(self):
        self._check(self._L.shk_reset_timings(self._h))

    # -- merged-table read API ------------------------------------------------------
    def export_table(self):
        """KmerCounts::iter (counting.rs:239-241), sorted by k-mer for comparison."""
        n = C.c_uint64(0)
        self._check(self._L.shk_export_table(self._h, None, None, 0, C.byref(n)))
        cap = int(n.value)
        keys = np.zeros(cap, dtype=np.uint64)
        cnts = np.zeros(cap, dtype=np.uint32)
        if cap:
            self._check(self._L.shk_export_table(self._h, keys.ctypes.data, cnts.ctypes.data, cap,
                                                 C.byref(n)))
        o = np.argsort(keys, kind="stable")
        return keys[o], cnts[o]

    def chunk_bases(self) -> np.ndarray:
        """Chunk::n_bases of every chunk (u64[n_chunks]; counters()["n_bases_ingested"] is their sum): what a depth's
        node budget is computed from (pcr_run_depths)."""
        out = np.zeros(self.counters()["n_chunks"], dtype=np.uint64)
        self._check(self._L.shk_chunk_bases(self._h, out.ctypes.data))
        return out

    def lookup(self, kmers, canonical: bool = False, depth: int | None = None) -> np.ndarray:
        """get_count (counting.rs:224-226) / get_canonical_count (:205-209).  depth d (1..n_chunks): in the table of
        chunks 0..d-1 only (shk_lookup_depth); None: the merged table."""
        kmers = np.ascontiguousarray(np.atleast_1d(kmers), dtype=np.uint64)
        out = np.zeros(len(kmers), dtype=np.uint32)
        if depth is None:
            self._check(self._L.shk_lookup(self._h, kmers.ctypes.data, out.ctypes.data, len(kmers),
                                           1 if canonical else 0))
        else:
            self._check(self._L.shk_lookup_depth(self._h, kmers.ctypes.data, out.ctypes.data, len(kmers),
                                                 1 if canonical else 0, depth))
        return out

    def find_oligos(self, oligos, oligo_len: int, min_count: int = 1):
        """find_oligos_in_kmers (pcr/primers.rs:163-226): (kmers, counts) sorted by k-mer."""
        oligos = np.ascontiguousarray(np.atleast_1d(oligos), dtype=np.uint64)
        n = C.c_uint64(0)
        self._check(self._L.shk_find_oligos(self._h, oligos.ctypes.data, len(oligos), oligo_len, min_count,
                                            None, None, 0, C.byref(n)))
        cap = int(n.value)
        keys = np.zeros(cap, dtype=np.uint64)
        cnts = np.zeros(cap, dtype=np.uint32)
        if cap:
            self._check(self._L.shk_find_oligos(self._h, oligos.ctypes.data, len(oligos), oligo_len,
                                                min_count, keys.ctypes.data, cnts.ctypes.data, cap, C.byref(n)))
        o = np.argsort(keys, kind="stable")
        return keys[o], cnts[o]

    def primer_kmers(self, primers):
        """get_primer_kmers (pcr/primers.rs:234-480) for every primer direction in one pass over the table
        (shk_primer_kmers) → per primer (kmers u64, counts u32, levels u8, level_hits u64[PRIMER_LEVELS]), the
        k-mers in the reference's insertion order: level ascending, count descending, k-mer ascending."""
        (block,) = self._primer_blocks(list(primers), 1, lambda *a: self._L.shk_primer_kmers(self._h, *a))
        return block

    def primer_kmers_depths(self, primers, depths) -> list:
        """primer_kmers at every depth of `depths` (strictly ascending, at most PCR_MAX_DEPTHS) in one pass over the table
        (shk_primer_kmers_depths) → per depth what primer_kmers returns on a context that got the chunks below it only."""
        dep = np.ascontiguousarray(np.atleast_1d(depths), dtype=np.uint32)
        return self._primer_blocks(list(primers), len(dep),
                                   lambda arr, n, *a: self._L.shk_primer_kmers_depths(self._h, arr, n, dep.ctypes.data, len(dep), *a))

    def _primer_blocks(self, primers, n_blocks: int, call) -> list:
        """The arrays of a primer scan over n_blocks result blocks, call(primers, n, kmers, counts, levels, cap, offsets,
        level_hits) and its result sliced → per block, per primer (kmers, counts, levels, level_hits)."""
        n = len(primers)
        arr = (_Primer * max(n, 1))(*[p._c() for p in primers])
        cap = n_blocks * sum(p.max_kmers for p in primers)
        kmers = np.zeros(max(cap, 1), dtype=np.uint64)
        counts = np.zeros(max(cap, 1), dtype=np.uint32)
        levels = np.zeros(max(cap, 1), dtype=np.uint8)
        offsets = np.zeros(n * n_blocks + 1, dtype=np.uint64)
        hits = np.zeros((max(n * n_blocks, 1), PRIMER_LEVELS), dtype=np.uint64)
        self._check(call(C.cast(arr, C.c_void_p), n, kmers.ctypes.data, counts.ctypes.data, levels.ctypes.data, cap, offsets.ctypes.data,
                         hits.ctypes.data))
        out = []
        for j in range(n_blocks):
            block = []
            for i in range(j * n, j * n + n):
                a, b = int(offsets[i]), int(offsets[i + 1])
                block.append((kmers[a:b].copy(), counts[a:b].copy(), levels[a:b].copy(), hits[i].copy()))
            out.append(block)
        return out

    def primer_pair_kmers(self, forward: str, reverse: str, **params):
        """get_primer_kmers (pcr/primers.rs:440-480) for one PCRParams: (forward, reverse), each as primer_kmers
        returns it.  params: trim, mismatches, min_count, max_kmers (the reference's defaults otherwise)."""
        fwd, rev = self.primer_kmers([Primer(forward, **params), Primer(reverse, **params)])
        return fwd, rev

    def neighborhood(self, nodes, dirs, min_count: int, max_levels: int = 0, cap: int = 1 << 16,
                     fringe_cap: int = 1 << 16):
        """shk_neighborhood: the bulk neighbourhood of seed (node, dir) pairs in sPCR's extension graph (nodes are
        (k−1)-mers; dir 1 forward, 2 reverse, 3 both), expanded in whole levels while the accepted k-mers fit `cap` and a
        level fits `fringe_cap` → (kmers u64 ascending, counts u32, fringe_nodes u64, fringe_dirs u8, levels_done); an
        empty fringe says the neighbourhood is complete."""
        nodes = np.ascontiguousarray(np.atleast_1d(nodes), dtype=np.uint64)
        dirs = np.ascontiguousarray(np.atleast_1d(dirs), dtype=np.uint8)
        if len(nodes) != len(dirs):
            raise ValueError("nodes and dirs differ in length")
        kmers = np.zeros(max(cap, 1), dtype=np.uint64)
        counts = np.zeros(max(cap, 1), dtype=np.uint32)
        fn = np.zeros(max(fringe_cap, 1), dtype=np.uint64)
        fd = np.zeros(max(fringe_cap, 1), dtype=np.uint8)
        n_out, n_fr, lv = C.c_uint64(0), C.c_uint64(0), C.c_uint32(0)
        self._check(self._L.shk_neighborhood(self._h, nodes.ctypes.data, dirs.ctypes.data, len(nodes), min_count,
                                             max_levels, kmers.ctypes.data, counts.ctypes.data, cap, C.byref(n_out),
                                             fn.ctypes.data, fd.ctypes.data, fringe_cap, C.byref(n_fr), C.byref(lv)))
        a, b = int(n_out.value), int(n_fr.value)
        return kmers[:a].copy(), counts[:a].copy(), fn[:b].copy(), fd[:b].copy(), int(lv.value)

    def pcr_extend(self, fwd, rev, min_count: int = 2, table_min_count: int = 2, high_coverage_ratio: float = 10.0,
                   max_num_nodes: int | None = None, sweep: bool = True) -> PcrGraph:
        """create_seed_graph + extend_graph under do_pcr's threshold sweep (pcr/graph.rs:196-528, pcr/mod.rs:559-619)
        → PcrGraph.  fwd, rev: the two tuples of primer_pair_kmers (k-mers first, counts second).  max_num_nodes:
        None = compute_node_budget of the bases this context has ingested."""
        fk = np.ascontiguousarray(fwd[0], dtype=np.uint64)
        fc = np.ascontiguousarray(fwd[1], dtype=np.uint32)
        rk = np.ascontiguousarray(rev[0], dtype=np.uint64)
        rc = np.ascontiguousarray(rev[1], dtype=np.uint32)
        if max_num_nodes is None:
            max_num_nodes = pcr_node_budget(self.counters()["n_bases_ingested"])
        prm = _PcrExtendParams(min_count, table_min_count, high_coverage_ratio, max_num_nodes, 1 if sweep else 0, 0)
        node_cap, edge_cap = 4096, 8192
        while True:
            sub = np.zeros(node_cap, dtype=np.uint64)
            flags = np.zeros(node_cap, dtype=np.uint8)
            es, et, ec = (np.zeros(edge_cap, dtype=np.uint32) for _ in range(3))
            nn, ne = C.c_uint64(0), C.c_uint64(0)
            found, thr, steps = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
            rcode = self._L.shk_pcr_extend(self._h, fk.ctypes.data, fc.ctypes.data, len(fk), rk.ctypes.data,
                                           rc.ctypes.data, len(rk), C.byref(prm), sub.ctypes.data, flags.ctypes.data,
                                           node_cap, C.byref(nn), es.ctypes.data, et.ctypes.data, ec.ctypes.data, edge_cap,
                                           C.byref(ne), C.byref(found), C.byref(thr), C.byref(steps))
            n, e = int(nn.value), int(ne.value)
            if rcode == -2 and (n > node_cap or e > edge_cap):  # the buffers were too small: it says what it needs
                node_cap, edge_cap = max(node_cap, n), max(edge_cap, e)
                continue
            self._check(rcode)
            return PcrGraph(sub[:n].copy(), flags[:n].copy(), es[:e].copy(), et[:e].copy(), ec[:e].copy(),
                            bool(found.value), int(thr.value), int(steps.value))

    def neighborhood_panel(self, jobs, max_levels: int = 0, depths=None) -> list:
        """shk_neighborhood_panel: the neighbourhoods of many independent seed sets in one call.  jobs: a sequence of
        (nodes, dirs, min_count) or (nodes, dirs, min_count, cap, fringe_cap) — the arguments of `neighborhood`, the
        capacities 2^16 when left out; max_levels holds for all.  → per job the tuple `neighborhood` returns.
        depths: one depth per job (shk_neighborhood_panel_depths); None: the merged table."""
        jobs = [tuple(j) for j in jobs]
        nj = len(jobs)
        if depths is not None:
            depths = np.ascontiguousarray(np.atleast_1d(depths), dtype=np.uint32)
            if len(depths) != nj:
                raise ValueError("one depth per job")
        ns = [np.ascontiguousarray(np.atleast_1d(j[0]), dtype=np.uint64).reshape(-1) for j in jobs]
        ds = [np.ascontiguousarray(np.atleast_1d(j[1]), dtype=np.uint8).reshape(-1) for j in jobs]
        if any(len(a) != len(b) for a, b in zip(ns, ds)):
            raise ValueError("nodes and dirs differ in length")
        nodes = np.concatenate(ns) if ns else np.zeros(0, dtype=np.uint64)
        dirs = np.concatenate(ds) if ds else np.zeros(0, dtype=np.uint8)
        soff = np.zeros(nj + 1, dtype=np.uint64)
        if nj:
            soff[1:] = np.cumsum([len(a) for a in ns])
        mcs = np.array([j[2] for j in jobs], dtype=np.uint32)
        caps = np.array([j[3] if len(j) > 3 else 1 << 16 for j in jobs], dtype=np.uint64)
        fcaps = np.array([j[4] if len(j) > 4 else 1 << 16 for j in jobs], dtype=np.uint64)
        ka = np.concatenate([[0], np.cumsum(caps, dtype=np.uint64)]).astype(np.uint64)
        fa = np.concatenate([[0], np.cumsum(fcaps, dtype=np.uint64)]).astype(np.uint64)
        kmers = np.zeros(max(int(ka[-1]), 1), dtype=np.uint64)
        counts = np.zeros(max(int(ka[-1]), 1), dtype=np.uint32)
        fn = np.zeros(max(int(fa[-1]), 1), dtype=np.uint64)
        fd = np.zeros(max(int(fa[-1]), 1), dtype=np.uint8)
        n_out, n_fr = np.zeros(max(nj, 1), dtype=np.uint64), np.zeros(max(nj, 1), dtype=np.uint64)
        lv = np.zeros(max(nj, 1), dtype=np.uint32)
        if depths is None:
            self._check(self._L.shk_neighborhood_panel(self._h, nodes.ctypes.data, dirs.ctypes.data, soff.ctypes.data, nj,
                                                       mcs.ctypes.data, max_levels, caps.ctypes.data, fcaps.ctypes.data,
                                                       kmers.ctypes.data, counts.ctypes.data, n_out.ctypes.data, fn.ctypes.data,
                                                       fd.ctypes.data, n_fr.ctypes.data, lv.ctypes.data))
        else:
            self._check(self._L.shk_neighborhood_panel_depths(self._h, nodes.ctypes.data, dirs.ctypes.data, soff.ctypes.data, nj,
                                                              mcs.ctypes.data, depths.ctypes.data, max_levels, caps.ctypes.data,
                                                              fcaps.ctypes.data, kmers.ctypes.data, counts.ctypes.data,
                                                              n_out.ctypes.data, fn.ctypes.data, fd.ctypes.data, n_fr.ctypes.data,
                                                              lv.ctypes.data))
        out = []
        for j in range(nj):
            a, b, n, f = int(ka[j]), int(fa[j]), int(n_out[j]), int(n_fr[j])
            out.append((kmers[a:a + n].copy(), counts[a:a + n].copy(), fn[b:b + f].copy(), fd[b:b + f].copy(), int(lv[j])))
        return out

    def pcr_extend_panel(self, primer_results, params=None, depths=None) -> list:
        """shk_pcr_extend for every gene of a panel in one call (shk_pcr_extend_panel) → one PcrGraph per gene, a list
        thread_reads_panel takes as it is.  primer_results: what primer_kmers returns for primers ordered forward,
        reverse per gene (entry 2g gene g's forward set, 2g + 1 its reverse set; k-mers first, counts second), or the
        raw arrays (kmers, counts, offsets) of shk_primer_kmers.  params: one dict of pcr_extend's keyword arguments
        (min_count, table_min_count, high_coverage_ratio, max_num_nodes, sweep) per gene, or one for all;
        max_num_nodes None = compute_node_budget of the bases this context has ingested.  depths: one depth per gene
        (shk_pcr_extend_panel_depths; max_num_nodes None is still the whole context's budget); None: the merged table."""
        raw = len(primer_results) == 3 and all(isinstance(x, np.ndarray) and x.ndim == 1 for x in primer_results)
        if raw:
            pk = np.ascontiguousarray(primer_results[0], dtype=np.uint64)
            pc = np.ascontiguousarray(primer_results[1], dtype=np.uint32)
            po = np.ascontiguousarray(primer_results[2], dtype=np.uint64)
            if len(po) < 1 or len(po) % 2 != 1:
                raise ValueError("primer offsets take 2 * n_genes + 1 entries")
        else:
            sets = list(primer_results)
            if len(sets) % 2:
                raise ValueError("a forward and a reverse set per gene")
            ks = [np.ascontiguousarray(x[0], dtype=np.uint64).reshape(-1) for x in sets]
            cs = [np.ascontiguousarray(x[1], dtype=np.uint32).reshape(-1) for x in sets]
            if any(len(a) != len(b) for a, b in zip(ks, cs)):
                raise ValueError("k-mers and counts differ in length")
            pk = np.concatenate(ks) if ks else np.zeros(0, dtype=np.uint64)
            pc = np.concatenate(cs) if cs else np.zeros(0, dtype=np.uint32)
            po = np.zeros(len(sets) + 1, dtype=np.uint64)
            if sets:
                po[1:] = np.cumsum([len(a) for a in ks])
        ng = (len(po) - 1) // 2
        if params is None or isinstance(params, dict):
            params = [params or {}] * ng
        if len(params) != ng:
            raise ValueError("one set of parameters per gene")
        if depths is not None:
            depths = np.ascontiguousarray(np.atleast_1d(depths), dtype=np.uint32)
            if len(depths) != ng:
                raise ValueError("one depth per gene")
        budget = None
        prm = (_PcrExtendParams * max(ng, 1))()
        for g, p in enumerate(params):
            p = dict(p)
            mnn = p.get("max_num_nodes")
            if mnn is None:
                if budget is None:
                    budget = pcr_node_budget(self.counters()["n_bases_ingested"])
                mnn = budget
            prm[g] = _PcrExtendParams(p.get("min_count", 2), p.get("table_min_count", 2), p.get("high_coverage_ratio", 10.0),
                                      mnn, 1 if p.get("sweep", True) else 0, 0)
        noff, eoff = np.zeros(ng + 1, dtype=np.uint64), np.zeros(ng + 1, dtype=np.uint64)
        found, thr, steps = (np.zeros(max(ng, 1), dtype=np.uint32) for _ in range(3))
        node_cap, edge_cap = 4096 * max(ng, 1), 8192 * max(ng, 1)
        for attempt in (0, 1):
            sub = np.zeros(node_cap, dtype=np.uint64)
            flags = np.zeros(node_cap, dtype=np.uint8)
            es, et, ec = (np.zeros(edge_cap, dtype=np.uint32) for _ in range(3))
            if depths is None:
                rcode = self._L.shk_pcr_extend_panel(self._h, pk.ctypes.data, pc.ctypes.data, po.ctypes.data, ng, C.cast(prm, C.c_void_p),
                                                     sub.ctypes.data, flags.ctypes.data, noff.ctypes.data, node_cap, es.ctypes.data,
                                                     et.ctypes.data, ec.ctypes.data, eoff.ctypes.data, edge_cap, found.ctypes.data,
                                                     thr.ctypes.data, steps.ctypes.data)
            else:
                rcode = self._L.shk_pcr_extend_panel_depths(self._h, pk.ctypes.data, pc.ctypes.data, po.ctypes.data, ng,
                                                            C.cast(prm, C.c_void_p), depths.ctypes.data, sub.ctypes.data,
                                                            flags.ctypes.data, noff.ctypes.data, node_cap, es.ctypes.data,
                                                            et.ctypes.data, ec.ctypes.data, eoff.ctypes.data, edge_cap,
                                                            found.ctypes.data, thr.ctypes.data, steps.ctypes.data)
            n, e = int(noff[ng]), int(eoff[ng])
            if attempt == 0 and rcode == -2 and (n > node_cap or e > edge_cap):  # too small: the offsets say what it needs
                node_cap, edge_cap = max(node_cap, n), max(edge_cap, e)
                continue
            self._check(rcode)
            break
        out = []
        for g in range(ng):
            a, b, x, y = int(noff[g]), int(noff[g + 1]), int(eoff[g]), int(eoff[g + 1])
            out.append(PcrGraph(sub[a:b].copy(), flags[a:b].copy(), es[x:y].copy(), et[x:y].copy(), ec[x:y].copy(),
                                bool(found[g]), int(thr[g]), int(steps[g])))
        return out

    def pcr_prune_panel(self, graphs, tip_coverage_fraction=0.1, stages=3) -> list:
        """remove_low_coverage_tips, reachability_pruning and annotate_coverage_ratios for every gene of a panel in one
        call (shk_pcr_prune_panel) → one PrunedGraph per gene, a list thread_reads_panel takes as it is.  graphs: what
        pcr_extend_panel returns, or (node_sub_kmers, node_flags, edge_src, edge_tgt, edge_counts) tuples with endpoints
        local to the gene.  tip_coverage_fraction and stages (bit 0 the tips, bit 1 reachability): one value for all
        genes or one per gene."""
        gs = [(g.node_sub_kmers, g.node_flags, g.edge_src, g.edge_tgt, g.edge_counts) if isinstance(g, (PcrGraph, PrunedGraph)) else g
              for g in graphs]
        ng = len(gs)
        subs = [np.ascontiguousarray(g[0], dtype=np.uint64).reshape(-1) for g in gs]
        fls = [np.ascontiguousarray(g[1], dtype=np.uint8).reshape(-1) for g in gs]
        ess = [np.ascontiguousarray(g[2], dtype=np.uint32).reshape(-1) for g in gs]
        ets = [np.ascontiguousarray(g[3], dtype=np.uint32).reshape(-1) for g in gs]
        ecs = [np.ascontiguousarray(g[4], dtype=np.uint32).reshape(-1) for g in gs]
        if any(len(a) != len(b) for a, b in zip(subs, fls)):
            raise ValueError("node_sub_kmers and node_flags differ in length")
        if any(len(a) != len(b) or len(a) != len(c_) for a, b, c_ in zip(ess, ets, ecs)):
            raise ValueError("edge_src, edge_tgt and edge_counts differ in length")
        fracs = list(tip_coverage_fraction) if np.ndim(tip_coverage_fraction) else [tip_coverage_fraction] * ng
        stgs = list(stages) if np.ndim(stages) else [stages] * ng
        if len(fracs) != ng or len(stgs) != ng:
            raise ValueError("one tip_coverage_fraction and one stages value per gene")

        def cat(parts, dtype):
            off = np.zeros(ng + 1, dtype=np.uint64)
            if parts:
                off[1:] = np.cumsum([len(x) for x in parts])
            return (np.concatenate(parts) if parts else np.zeros(0, dtype=dtype)), off

        sub, noff = cat(subs, np.uint64)
        fl, _ = cat(fls, np.uint8)
        es, eoff = cat(ess, np.uint32)
        et, _ = cat(ets, np.uint32)
        ec, _ = cat(ecs, np.uint32)
        prm = (_PcrPruneParams * max(ng, 1))()
        for g in range(ng):
            prm[g] = _PcrPruneParams(float(fracs[g]), int(stgs[g]), 0)
        nn, ne = len(sub), len(es)
        keep = np.zeros(max(nn, 1), dtype=np.uint8)
        ono, oeo = np.zeros(ng + 1, dtype=np.uint64), np.zeros(ng + 1, dtype=np.uint64)
        med = np.zeros(max(ng, 1), dtype=np.float64)
        rounds, tips, unreach = (np.zeros(max(ng, 1), dtype=np.uint32) for _ in range(3))
        # a pruned graph is no larger than what went in: room for all of it (pages nothing writes to cost nothing), up to
        # prune_first_cap entries — a call that keeps more says so and is made again, which prunes a second time
        node_cap, edge_cap = max(min(nn, self.prune_first_cap), 1), max(min(ne, self.prune_first_cap), 1)
        for attempt in (0, 1):
            osub, ofl, oni = np.zeros(node_cap, dtype=np.uint64), np.zeros(node_cap, dtype=np.uint8), np.zeros(node_cap, dtype=np.uint32)
            oes, oet, oec, oei = (np.zeros(edge_cap, dtype=np.uint32) for _ in range(4))
            ratio = np.zeros(edge_cap, dtype=np.float64)
            out = _PcrPruneOut(keep.ctypes.data, ono.ctypes.data, oeo.ctypes.data, osub.ctypes.data, ofl.ctypes.data, oni.ctypes.data,
                               node_cap, oes.ctypes.data, oet.ctypes.data, oec.ctypes.data, oei.ctypes.data, ratio.ctypes.data, edge_cap,
                               med.ctypes.data, rounds.ctypes.data, tips.ctypes.data, unreach.ctypes.data, 0.0)
            rcode = self._L.shk_pcr_prune_panel(self._h, sub.ctypes.data, fl.ctypes.data, noff.ctypes.data, es.ctypes.data, et.ctypes.data,
                                                ec.ctypes.data, eoff.ctypes.data, ng, C.cast(prm, C.c_void_p), C.byref(out))
            n, e = int(ono[ng]), int(oeo[ng])
            if attempt == 0 and rcode == -2 and (n > node_cap or e > edge_cap):  # too small: the offsets say what it needs
                node_cap, edge_cap = max(node_cap, n), max(edge_cap, e)
                continue
            self._check(rcode)
            break
        self.last_prune_device_ms = float(out.device_ms)
        res = []
        for g in range(ng):
            a, b, x, y = (int(v) for v in (ono[g], ono[g + 1], oeo[g], oeo[g + 1]))
            v0, v1 = int(noff[g]), int(noff[g + 1])
            res.append(PrunedGraph(osub[a:b].copy(), ofl[a:b].copy(), oes[x:y].copy(), oet[x:y].copy(), oec[x:y].copy(), oni[a:b].copy(),
                                   oei[x:y].copy(), ratio[x:y].copy(), float(med[g]), keep[v0:v1].copy(), int(rounds[g]), int(tips[g]),
                                   int(unreach[g])))
        return res

    def pcr_dedup_panel(self, records, scores, dedup_edit_threshold=10, want_pairs: bool = False) -> list:
        """sort_and_deduplicate (pcr/paths.rs:360-427) for every gene of a panel (shk_pcr_dedup_panel): records is per
        gene a list of ACGT strings, scores per gene their composite scores, dedup_edit_threshold one value or one per
        gene → one DedupResult per gene.  want_pairs: also the within-threshold bit of every pair of the sorted order.
        How the pairs were decided and the kernel's time are left in self.last_dedup."""
        ng = len(records)
        if len(scores) != ng:
            raise ValueError("one score list per gene")
        thr = np.array(_per_gene(dedup_edit_threshold, ng, "dedup_edit_threshold"), dtype=np.uint32).reshape(-1)
        flat = [r.encode("ascii") if isinstance(r, str) else bytes(r) for g in records for r in g]
        roff = np.zeros(ng + 1, dtype=np.uint64)
        if ng:
            roff[1:] = np.cumsum([len(g) for g in records])
        soff = np.zeros(len(flat) + 1, dtype=np.uint64)
        if flat:
            soff[1:] = np.cumsum([len(r) for r in flat])
        seqs = np.frombuffer(b"".join(flat), dtype=np.uint8) if flat else np.zeros(0, dtype=np.uint8)
        sc = np.concatenate([np.asarray(x, dtype=np.float64).reshape(-1) for x in scores]) if ng else np.zeros(0)
        sc = np.ascontiguousarray(sc, dtype=np.float64)
        if len(sc) != len(flat):
            raise ValueError("one score per record")
        kept = np.zeros(PCR_MAX_AMPLICONS * max(ng, 1), dtype=np.uint32)
        gen, ret, rtd = (np.zeros(max(ng, 1), dtype=np.uint32) for _ in range(3))
        order = np.zeros(max(len(flat), 1), dtype=np.uint32)
        poff = np.zeros(ng + 1, dtype=np.uint64)
        n_words = sum((len(g) * (len(g) - 1) // 2 + 63) // 64 for g in records) if want_pairs else 0
        words = np.zeros(max(n_words, 1), dtype=np.uint64)
        out = _PcrDedupOut(kept.ctypes.data, gen.ctypes.data, ret.ctypes.data, rtd.ctypes.data, order.ctypes.data,
                           words.ctypes.data if want_pairs else None, poff.ctypes.data, n_words, 0, 0, 0, 0.0)
        rcode = self._L.shk_pcr_dedup_panel(self._h, seqs.ctypes.data, soff.ctypes.data, roff.ctypes.data, sc.ctypes.data,
                                            thr.ctypes.data, ng, C.byref(out))
        self._check(rcode)
        self.last_dedup = {"device_ms": float(out.device_ms), "pairs_device": int(out.pairs_device), "pairs_host": int(out.pairs_host),
                           "pairs_prefiltered": int(out.pairs_prefiltered)}
        res = []
        for g in range(ng):
            a, b, m = int(roff[g]), int(roff[g + 1]), len(records[g])
            bits = None
            if want_pairs:
                w = words[int(poff[g]):int(poff[g + 1])]
                bits = np.unpackbits(w.view(np.uint8), bitorder="little")[:m * (m - 1) // 2].astype(bool)
            res.append(DedupResult(kept[PCR_MAX_AMPLICONS * g:PCR_MAX_AMPLICONS * g + int(rtd[g])].copy(), int(gen[g]), int(ret[g]),
                                   order[a:b].copy(), bits))
        return res

    def pcr_products_panel(self, graphs, annotations=None, min_length=0, max_length=10000, max_dfs_states=100000,
                           max_paths_per_pair=20, max_node_visits=2, dedup_edit_threshold=10) -> list:
        """The last stage of do_pcr (pcr/mod.rs:699-813) for every gene of a panel in one call (shk_pcr_products_panel):
        bubble preferences, the path search, sequences and scores on the host, the dedup's pair matrix on the device,
        the products renumbered 0, 1, .. → one PcrProducts per gene.  graphs: the list pcr_prune_panel returns;
        annotations: the list thread_reads_panel returns, None entries allowed; each parameter one value for all genes
        or one per gene.  The kernel's time is left in self.last_products_device_ms."""
        G, keep = _pcr_graphs(graphs, annotations)
        ng = G.n_genes
        prm = _pcr_params(ng, min_length, max_length, max_dfs_states, max_paths_per_pair, max_node_visits)
        thr = np.array(_per_gene(dedup_edit_threshold, ng, "dedup_edit_threshold"), dtype=np.uint32).reshape(-1)
        if not ng:
            thr = np.zeros(1, dtype=np.uint32)
        retained = np.zeros(max(ng, 1), dtype=np.uint32)
        ms = C.c_double(0.0)
        res = _pcr_records_call(ng, lambda R: (self._L.shk_pcr_products_panel(self._h, C.byref(G), prm, thr.ctypes.data, C.byref(R),
                                                                              retained.ctypes.data, C.byref(ms)), self._check), retained)
        self.last_products_device_ms = float(ms.value)
        return res

    def pcr_prune(self, graph, tip_coverage_fraction: float = 0.1, stages: int = 3) -> PrunedGraph:
        """pcr_prune_panel for one gene."""
        return self.pcr_prune_panel([graph], tip_coverage_fraction, stages)[0]

    def thread_reads(self, graph, bases, offsets, read_index=None, mate=None, device: bool = False) -> ThreadingAnnotations:
        """thread_reads / thread_reads_paired (pcr/threading.rs:87-192) of a batch through `graph` — a PcrGraph or a
        (node_sub_kmers, edge_src, edge_tgt) tuple, any graph at all — on the device (shk_thread_reads).  read_index
        and mate (0 unpaired, 1 R1, 2 R2) together give the paired form.  device=True: bases and offsets are torch
        tensors on this context's device (shk_thread_reads_device)."""
        if isinstance(graph, (PcrGraph, PrunedGraph)):
            graph = (graph.node_sub_kmers, graph.edge_src, graph.edge_tgt)
        sub = np.ascontiguousarray(graph[0], dtype=np.uint64)
        es = np.ascontiguousarray(graph[1], dtype=np.uint32)
        et = np.ascontiguousarray(graph[2], dtype=np.uint32)
        if len(es) != len(et):
            raise ValueError("edge_src and edge_tgt differ in length")
        n = len(offsets) - 1
        ne = len(es)
        ri = None if read_index is None else np.ascontiguousarray(read_index, dtype=np.uint64)
        mt = None if mate is None else np.ascontiguousarray(mate, dtype=np.uint8)
        for a in (ri, mt):
            if a is not None and len(a) != n:
                raise ValueError("read_index and mate take one entry per read")
        tot, una = np.zeros(max(ne, 1), dtype=np.uint32), np.zeros(max(ne, 1), dtype=np.uint32)
        re = np.zeros(max(n, 1), dtype=np.uint32)
        if device:
            args = (bases.data_ptr(), offsets.data_ptr(), n, bases.numel())
            call = self._L.shk_thread_reads_device
        else:
            bases = np.ascontiguousarray(bases, dtype=np.uint8)
            offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
            args = (bases.ctypes.data, offsets.ctypes.data, n)
            call = self._L.shk_thread_reads
        # room for every link there can be: Σ in_deg · out_deg over the branch nodes (the retry is for graphs beyond 2^22)
        ind, outd = (np.bincount(a, minlength=len(sub) + 1).astype(np.int64) for a in (et, es))
        m = min(len(ind), len(outd))
        link_cap = max(1, min(int((ind[:m] * outd[:m])[(ind[:m] > 1) | (outd[:m] > 1)].sum()), 1 << 22))
        while True:
            li, lo, lc = (np.zeros(link_cap, dtype=np.uint32) for _ in range(3))
            out = _ThreadOut(tot.ctypes.data, una.ctypes.data, li.ctypes.data, lo.ctypes.data, lc.ctypes.data, link_cap, 0,
                             re.ctypes.data, 0)
            rcode = call(self._h, sub.ctypes.data, len(sub), es.ctypes.data, et.ctypes.data, ne, *args,
                         None if ri is None else ri.ctypes.data, None if mt is None else mt.ctypes.data, C.byref(out))
            m = int(out.n_links)
            if rcode == -2 and m > link_cap:  # the link arrays were too small: it says what it needs
                link_cap = m
                continue
            self._check(rcode)
            return ThreadingAnnotations(tot[:ne].copy(), una[:ne].copy(), np.stack([li[:m], lo[:m]], axis=1), lc[:m].copy(),
                                        re[:n].copy(), int(out.n_paired_links))

    def thread_reads_panel(self, graphs, bases, offsets, lists, read_index=None, mate=None, device: bool = False) -> list:
        """thread_reads of every gene of a panel in one call (shk_thread_reads_panel): graphs is a sequence of PcrGraph or
        (node_sub_kmers, edge_src, edge_tgt) tuples, one per gene, edge endpoints local to the gene; lists is what
        filter_reads_panel returns — per gene the indices of its reads in the batch (any order, repeats count).  The
        answer is one ThreadingAnnotations per gene: what thread_reads gives for that graph over its listed reads in
        list order.  read_index and mate (one entry per read of the BATCH) give the paired form.  device=True: bases
        and offsets are torch tensors on this context's device (shk_thread_reads_panel_device)."""
        n = len(offsets) - 1
        if device:
            args = (bases.data_ptr(), offsets.data_ptr(), n, bases.numel())
            call = self._L.shk_thread_reads_panel_device
        else:
            bases = np.ascontiguousarray(bases, dtype=np.uint8)
            offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
            args = (bases.ctypes.data, offsets.ctypes.data, n)
            call = self._L.shk_thread_reads_panel
        return self._thread_panel(call, args, n, graphs, lists, read_index, mate)

    def _thread_panel(self, call, args, n, graphs, lists, read_index, mate) -> list:
        """thread_reads_panel and thread_reads_retained behind their batch: `args` are the call's arguments between
        n_genes and list_offsets, n the reads of the batch."""
        gs = [(g.node_sub_kmers, g.edge_src, g.edge_tgt) if isinstance(g, (PcrGraph, PrunedGraph)) else g for g in graphs]
        ng = len(gs)
        if len(lists) != ng:
            raise ValueError("one read list per graph")
        subs = [np.ascontiguousarray(g[0], dtype=np.uint64).reshape(-1) for g in gs]
        ess = [np.ascontiguousarray(g[1], dtype=np.uint32).reshape(-1) for g in gs]
        ets = [np.ascontiguousarray(g[2], dtype=np.uint32).reshape(-1) for g in gs]
        lss = [np.ascontiguousarray(x, dtype=np.uint64).reshape(-1) for x in lists]
        if any(len(a) != len(b) for a, b in zip(ess, ets)):
            raise ValueError("edge_src and edge_tgt differ in length")

        def cat(parts, dtype):
            off = np.zeros(ng + 1, dtype=np.uint64)
            if parts:
                off[1:] = np.cumsum([len(x) for x in parts])
            return (np.concatenate(parts) if parts else np.zeros(0, dtype=dtype)), off

        sub, noff = cat(subs, np.uint64)
        es, eoff = cat(ess, np.uint32)
        et, _ = cat(ets, np.uint32)
        lr, loff = cat(lss, np.uint64)
        ne, nl = len(es), len(lr)
        ri = None if read_index is None else np.ascontiguousarray(read_index, dtype=np.uint64)
        mt = None if mate is None else np.ascontiguousarray(mate, dtype=np.uint8)
        for a in (ri, mt):
            if a is not None and len(a) != n:
                raise ValueError("read_index and mate take one entry per read of the batch")
        tot, una = np.zeros(max(ne, 1), dtype=np.uint32), np.zeros(max(ne, 1), dtype=np.uint32)
        re = np.zeros(max(nl, 1), dtype=np.uint32)
        koff = np.zeros(ng + 1, dtype=np.uint64)
        npl = np.zeros(max(ng, 1), dtype=np.uint64)
        # room for every link there can be, per gene as thread_reads sizes it (the retry is for panels beyond 2^22)
        link_cap = 0
        for s_, a, b in zip(subs, ess, ets):
            ind, outd = (np.bincount(x, minlength=len(s_) + 1).astype(np.int64) for x in (b, a))
            m = min(len(ind), len(outd))
            link_cap += int((ind[:m] * outd[:m])[(ind[:m] > 1) | (outd[:m] > 1)].sum())
        link_cap = max(1, min(link_cap, 1 << 22))
        while True:
            li, lo, lc = (np.zeros(link_cap, dtype=np.uint32) for _ in range(3))
            out = _ThreadPanelOut(tot.ctypes.data, una.ctypes.data, koff.ctypes.data, li.ctypes.data, lo.ctypes.data, lc.ctypes.data,
                                  link_cap, 0, re.ctypes.data, npl.ctypes.data)
            rcode = call(self._h, sub.ctypes.data, noff.ctypes.data, es.ctypes.data, et.ctypes.data, eoff.ctypes.data, ng, *args,
                         loff.ctypes.data, lr.ctypes.data, None if ri is None else ri.ctypes.data,
                         None if mt is None else mt.ctypes.data, C.byref(out))
            if rcode == -2 and int(out.n_links) > link_cap:  # the link arrays were too small: it says what it needs
                link_cap = int(out.n_links)
                continue
            self._check(rcode)
            anns = []
            for g in range(ng):
                e0, e1, k0, k1, l0, l1 = (int(x) for x in (eoff[g], eoff[g + 1], koff[g], koff[g + 1], loff[g], loff[g + 1]))
                anns.append(ThreadingAnnotations(tot[e0:e1].copy(), una[e0:e1].copy(), np.stack([li[k0:k1], lo[k0:k1]], axis=1),
                                                 lc[k0:k1].copy(), re[l0:l1].copy(), int(npl[g])))
            return anns

    def filter_reads(self, bases: np.ndarray, offsets: np.ndarray, primer_kmers) -> np.ndarray:
        """PrimerReadFilter::matches per read (pcr/read_filter.rs:43-55) → bool array."""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        pk = np.ascontiguousarray(np.atleast_1d(primer_kmers), dtype=np.uint64)
        n = len(offsets) - 1
        out = np.zeros(max(n, 1), dtype=np.uint8)
        self._check(self._L.shk_filter_reads(self._h, bases.ctypes.data, offsets.ctypes.data, n,
                                             pk.ctypes.data, len(pk), out.ctypes.data))
        return out[:n].astype(bool)

    def filter_reads_panel(self, bases, offsets, gene_kmers, device: bool = False) -> list:
        """PrimerReadFilter::filter_reads (pcr/read_filter.rs:24-55) of one batch against every gene of a panel in one
        pass (shk_filter_reads_panel): gene_kmers is a sequence of arrays of canonical primer k-mers, one per gene; the
        answer is one uint64 array per gene, the indices of the reads that match it, ascending.  device=True: bases
        and offsets are torch tensors on this context's device (shk_filter_reads_panel_device)."""
        n = len(offsets) - 1
        if device:
            args = (bases.data_ptr(), offsets.data_ptr(), n, bases.numel())
            call = self._L.shk_filter_reads_panel_device
        else:
            bases = np.ascontiguousarray(bases, dtype=np.uint8)
            offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
            args = (bases.ctypes.data, offsets.ctypes.data, n)
            call = self._L.shk_filter_reads_panel
        return self._filter_panel(call, args, n, gene_kmers)

    def _filter_panel(self, call, args, n, gene_kmers) -> list:
        """filter_reads_panel and filter_reads_retained behind their batch: `args` are the call's arguments in front of
        primer_kmers, n the reads of the batch."""
        genes = [np.ascontiguousarray(np.atleast_1d(g), dtype=np.uint64).reshape(-1) for g in gene_kmers]
        goff = np.zeros(len(genes) + 1, dtype=np.uint64)
        if genes:
            goff[1:] = np.cumsum([len(g) for g in genes])
        pk = np.concatenate(genes) if genes else np.zeros(0, dtype=np.uint64)
        moff = np.zeros(len(genes) + 1, dtype=np.uint64)
        # room for every read in up to four genes: a call that finds more says so and is made again, which walks the
        # reads a second time
        cap = max(n, 1) * min(max(len(genes), 1), 4)
        while True:
            reads = np.zeros(cap, dtype=np.uint64)
            need = C.c_uint64(0)
            rcode = call(self._h, *args, pk.ctypes.data, goff.ctypes.data, len(genes), moff.ctypes.data, reads.ctypes.data, cap,
                         C.byref(need))
            if rcode == -2 and need.value > cap:  # the list was too small: it says what it needs
                cap = int(need.value)
                continue
            self._check(rcode)
            return [reads[int(moff[g]):int(moff[g + 1])].copy() for g in range(len(genes))]

    # ---- retained reads: the job's reads kept in device memory at ingest (shk_retain_reads) ------------------------------
    def retain_reads(self, on: bool = True, capacity_bases: int = 0):
        """Keep every read ingested from now on in device memory (three bit planes, 0.375 bytes per base) for
        filter_reads_retained and thread_reads_retained.  Switching on takes a context that holds no reads (new, or
        after reset); capacity_bases sizes the first allocation.  on=False frees the store."""
        self._check(self._L.shk_retain_reads(self._h, 1 if on else 0, int(capacity_bases)))

    def retained_info(self) -> dict:
        """→ {"reads", "bases", "device_bytes"} of the retained store."""
        r, b, d = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        self._check(self._L.shk_retained_info(self._h, C.byref(r), C.byref(b), C.byref(d)))
        return {"reads": int(r.value), "bases": int(b.value), "device_bytes": int(d.value)}

    def retained_reads(self, first: int = 0, n: int | None = None):
        """Retained reads first .. first + n (n=None: to the last) back as ASCII → (bases uint8, offsets uint64 from 0)."""
        if n is None:
            n = max(self.retained_info()["reads"] - first, 0)
        offsets = np.zeros(n + 1, dtype=np.uint64)
        cap = 150 * n  # (a guess; the retry is for longer reads)
        while True:
            bases = np.zeros(max(cap, 1), dtype=np.uint8)
            need = C.c_uint64(0)
            rcode = self._L.shk_retained_export(self._h, first, n, bases.ctypes.data, cap, offsets.ctypes.data, C.byref(need))
            if rcode == -2 and need.value > cap:  # nothing was written: it says what it needs
                cap = int(need.value)
                continue
            self._check(rcode)
            return bases[:int(need.value)].copy(), offsets

    def filter_reads_retained(self, gene_kmers) -> list:
        """filter_reads_panel with the batch being every read retained so far, in retention order
        (shk_filter_reads_panel_retained): no batch crosses anything, the walk reads the store's planes."""
        n = self.retained_info()["reads"]
        return self._filter_panel(self._L.shk_filter_reads_panel_retained, (), n, gene_kmers)

    def thread_reads_retained(self, graphs, lists, read_index=None, mate=None) -> list:
        """thread_reads_panel over the retained reads (shk_thread_reads_panel_retained): lists name retained reads — what
        filter_reads_retained returns — and read_index / mate take one entry per retained read."""
        n = self.retained_info()["reads"]
        return self._thread_panel(self._L.shk_thread_reads_panel_retained, (), n, graphs, lists, read_index, mate)

    def pcr_run(self, genes, reads=None, paired: bool = False, min_kmer_count: int = 2, max_num_nodes: int = 0,
                record_cap: int | None = None, seq_cap: int | None = None) -> list:
        """do_pcr for every gene of a panel in one call (shk_pcr_run; pcr/mod.rs:431-819 under stats.rs:84-98) → one
        PcrOutcome per gene.  genes: PcrGene or specification strings.  reads: None (k-mer-only scoring), "retained"
        (every read retained so far) or (bases, offsets[, read_index, mate]), a host batch as ingest_reads takes it.
        paired: without read_index / mate the reads alternate R1, R2.  max_num_nodes 0: compute_node_budget of the bases
        ingested.  record_cap / seq_cap: fixed capacities (no second call when they are too small)."""
        genes = [g if isinstance(g, PcrGene) else parse_pcr_primers(g) for g in genes]
        ng = len(genes)
        arr = _pcr_genes(genes)
        prm = _PcrRunParams(min_kmer_count, PCR_READS_NONE, 1 if paired else 0, 0, max_num_nodes, None, None, 0, None, None)
        keep = []
        if isinstance(reads, str):
            if reads != "retained":
                raise ValueError('reads: None, "retained" or (bases, offsets[, read_index, mate])')
            prm.reads = PCR_READS_RETAINED
        elif reads is not None:
            bases = np.ascontiguousarray(reads[0], dtype=np.uint8)
            offsets = np.ascontiguousarray(reads[1], dtype=np.uint64)
            keep += [bases, offsets]
            prm.reads, prm.bases, prm.offsets, prm.n_seqs = PCR_READS_HOST, bases.ctypes.data, offsets.ctypes.data, len(offsets) - 1
            if len(reads) > 2 and (reads[2] is not None or reads[3] is not None):
                ri = None if reads[2] is None else np.ascontiguousarray(reads[2], dtype=np.uint64)
                mt = None if reads[3] is None else np.ascontiguousarray(reads[3], dtype=np.uint8)
                if any(x is not None and len(x) != prm.n_seqs for x in (ri, mt)):
                    raise ValueError("read_index and mate take one entry per read")
                keep += [ri, mt]
                prm.read_index = None if ri is None else ri.ctypes.data
                prm.mate = None if mt is None else mt.ctypes.data
        O = _PcrRunOut()
        cols = _pcr_out_columns(O, ng)

        def call(R):
            R.record_cap = R.record_cap if record_cap is None else record_cap
            R.seq_cap = R.seq_cap if seq_cap is None else seq_cap
            O.records = R
            rc = self._L.shk_pcr_run(self._h, arr, ng, C.byref(prm), C.byref(O))
            R.n_records, R.n_seq_bytes = O.records.n_records, O.records.n_seq_bytes
            if rc != 0 and (record_cap is not None or seq_cap is not None):  # (no second call with room)
                try:
                    self._check(rc)
                except ShkError as e:  # what the call left: the needs and the per-gene arrays, which are complete
                    e.needs = (int(R.n_records), int(R.n_seq_bytes))
                    e.per_gene = {f: a[:ng].copy() for f, a in cols.items()}
                    raise
            return rc, self._check

        return _pcr_outcomes(genes, cols, _pcr_records_call(ng, call))

    def pcr_run_depths(self, genes, depths, min_kmer_count: int = 2, max_num_nodes: int = 0, record_cap: int | None = None,
                       seq_cap: int | None = None) -> list:
        """pcr_run(reads=None) of the panel at every depth of `depths` (strictly ascending, at most PCR_MAX_DEPTHS) as one
        pipeline over the (gene, depth) pairs (shk_pcr_run_depths) → per depth the list pcr_run returns on a context that got
        the chunks below it only.  max_num_nodes 0: compute_node_budget of the bases of the chunks below the depth.
        record_cap / seq_cap: fixed capacities per depth (no second call when they are too small)."""
        genes = [g if isinstance(g, PcrGene) else parse_pcr_primers(g) for g in genes]
        dep = np.ascontiguousarray(np.atleast_1d(depths), dtype=np.uint32)
        ng, nd = len(genes), len(dep)
        arr = _pcr_genes(genes)
        prm = _PcrRunParams(min_kmer_count, PCR_READS_NONE, 0, 0, max_num_nodes, None, None, 0, None, None)
        O = (_PcrRunOut * max(nd, 1))()
        cols = [_pcr_out_columns(O[j], ng) for j in range(nd)]
        fixed = record_cap is not None or seq_cap is not None
        bufs = [_PcrRecordBuf(ng, max(64 * ng, 1) if record_cap is None else record_cap, 1 << 16 if seq_cap is None else seq_cap)
                for _ in range(nd)]
        for attempt in (0, 1):
            for j in range(nd):
                O[j].records = bufs[j].struct()
            rc = self._L.shk_pcr_run_depths(self._h, arr, ng, C.byref(prm), dep.ctypes.data, nd, O)
            for j in range(nd):
                bufs[j].take(O[j].records)
            if rc == -2 and any(b.short() for b in bufs):
                if attempt == 0 and not fixed:  # too small: every depth says what it needs
                    bufs = [_PcrRecordBuf(ng, max(b.rcap, b.n_records), max(b.scap, b.n_seq_bytes)) for b in bufs]
                    continue
                try:
                    self._check(rc)
                except ShkError as e:  # what the call left: every depth's needs and per-gene arrays, which are complete
                    e.needs = [(b.n_records, b.n_seq_bytes) for b in bufs]
                    e.per_gene = [{f: a[:ng].copy() for f, a in c.items()} for c in cols]
                    raise
            self._check(rc)
            break
        return [_pcr_outcomes(genes, cols[j], bufs[j].products()) for j in range(nd)]

    def gather_reads(self, bases_t, offsets_t, read_ids):
        """The reads read_ids (any order, repeats allowed) of a batch that lies on this context's device, as a batch of
        their own on the same device (shk_gather_reads_device) → (bases uint8 tensor, offsets int64 tensor): what takes a
        gene's list from filter_reads_panel to thread_reads(device=True)."""
        import torch
        ids = np.ascontiguousarray(read_ids, dtype=np.uint64).reshape(-1)
        n = offsets_t.numel() - 1
        out_off = torch.empty(len(ids) + 1, dtype=torch.int64, device=self._tdev)
        cap = len(ids) * (bases_t.numel() // max(n, 1) + 1)  # the mean read length each; the retry is for longer picks
        while True:
            out = torch.empty(max(cap, 1), dtype=torch.uint8, device=self._tdev)
            need = C.c_uint64(0)
            rcode = self._L.shk_gather_reads_device(self._h, bases_t.data_ptr(), offsets_t.data_ptr(), n, ids.ctypes.data, len(ids),
                                                    out.data_ptr(), cap, out_off.data_ptr(), C.byref(need))
            if rcode == -2 and need.value > cap:  # nothing was written: it says what it needs
                cap = int(need.value)
                continue
            self._check(rcode)
            return out[:int(need.value)], out_off

    def kmers_from_reads(self, bases: np.ndarray, offsets: np.ndarray):
        """Batched kmers_from_ascii (kmer/encoding.rs:332-371) in the form thread_reads uses it
        (pcr/threading.rs:97-101) → (list of per-read uint64 arrays, bad_byte uint8 array).  A read with
        a byte outside ACGTN has bad_byte != 0 and no k-mers."""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = len(offsets) - 1
        lens = np.diff(offsets.astype(np.int64))
        room = np.maximum(lens - self.k + 1, 0)
        koff = np.concatenate([[0], np.cumsum(room)]).astype(np.int64)
        kmers = np.empty(max(int(koff[-1]), 1), dtype=np.uint64)
        n_k = np.zeros(max(n, 1), dtype=np.uint32)
        bad = np.zeros(max(n, 1), dtype=np.uint8)
        self._check(self._L.shk_kmers_from_reads(self._h, bases.ctypes.data, offsets.ctypes.data, n,
                                                 kmers.ctypes.data, int(koff[-1]), n_k.ctypes.data,
                                                 bad.ctypes.data))
        return [kmers[koff[i]:koff[i] + int(n_k[i])] for i in range(n)], bad[:n]

    def kmers_from_ascii(self, seq) -> np.ndarray:
        """kmers_from_ascii(seq, k) (kmer/encoding.rs:332-371) for one sequence; raises with the
        reference's message on a byte outside ACGTN (encoding.rs:353-356)."""
        b = np.frombuffer(seq.encode() if isinstance(seq, str) else bytes(seq), dtype=np.uint8)
        out, bad = self.kmers_from_reads(b, np.array([0, len(b)], dtype=np.uint64))
        if bad[0]:
            raise ShkError(-1, "Invalid character '%s' in sequence. Only ACGTN allowed." % chr(int(bad[0])))
        return out[0]

    # -- multi-GPU hooks ---------------------------------------------------------------
    def table_geometry(self):
        p, s, l = C.c_uint64(0), C.c_uint32(0), C.c_uint32(0)
        self._check(self._L.shk_table_geometry(self._h, C.byref(p), C.byref(s), C.byref(l)))
        return int(p.value), int(s.value), int(l.value)

    def reserve_pages(self, n_pages: int):
        self._check(self._L.shk_table_reserve_pages(self._h, n_pages))

    def table_device_ptrs(self):
        k, v = C.c_void_p(), C.c_void_p()
        self._check(self._L.shk_table_device_ptrs(self._h, C.byref(k), C.byref(v)))
        return int(k.value), int(v.value)

    def merge_pages(self, p0: int, p1: int, d_keys: int, d_vals: int, lane_stride: int):
        self._check(self._L.shk_merge_pages(self._h, p0, p1, d_keys, d_vals, lane_stride))

    # -- exchange rounds between owner shares (include/shk.h, shk_xchg_*) ---------------------
    def stream(self) -> int:
        return int(self._L.shk_stream(self._h) or 0)

    def xchg_scatter_device(self, d_bases: int, d_offsets: int, n_seqs: int, n_bases: int, layout_bases: int = 0):
        """→ (d_records, d_cursors, XchgLayout, n_foreign_spilled)."""
        rec, cur, lay, nf = C.c_void_p(), C.c_void_p(), XchgLayout(), C.c_uint64(0)
        self._check(self._L.shk_xchg_scatter_device(self._h, d_bases, d_offsets, n_seqs, n_bases, layout_bases,
                                                    C.byref(rec), C.byref(cur), C.byref(lay), C.byref(nf)))
        return int(rec.value or 0), int(cur.value or 0), lay, int(nf.value)

    def xchg_scatter_begin(self, d_bases: int, d_offsets: int, n_seqs: int, n_bases: int, layout_bases: int = 0):
        """The scatter launched, not waited for → (d_records, d_cursors, XchgLayout); xchg_scatter_end() → n_foreign_spilled."""
        rec, cur, lay = C.c_void_p(), C.c_void_p(), XchgLayout()
        self._check(self._L.shk_xchg_scatter_begin(self._h, d_bases, d_offsets, n_seqs, n_bases, layout_bases,
                                                   C.byref(rec), C.byref(cur), C.byref(lay)))
        return int(rec.value or 0), int(cur.value or 0), lay

    def xchg_scatter_end(self) -> int:
        nf = C.c_uint64(0)
        self._check(self._L.shk_xchg_scatter_end(self._h, C.byref(nf)))
        return int(nf.value)

    def xchg_absorb(self, d_records: int, d_cursors: int, lay):
        self._check(self._L.shk_xchg_absorb(self._h, d_records, d_cursors, C.byref(lay)))

    def xchg_spill(self):
        """→ (d_kmers, d_lanes, d_counts, n): the foreign spill list."""
        k, l, c, n = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_uint64(0)
        self._check(self._L.shk_xchg_spill(self._h, C.byref(k), C.byref(l), C.byref(c), C.byref(n)))
        return int(k.value or 0), int(l.value or 0), int(c.value or 0), int(n.value)

    def xchg_spill_clear(self):
        self._check(self._L.shk_xchg_spill_clear(self._h))

    def xchg_feasible(self) -> bool:
        """Does this share's key width fit the owner layout's 4-byte records (shk_xchg_scatter_device)?  If not
        (k > 21 at the default fan-out), rounds go through xchg_wide_scatter_device + insert_device."""
        return bool(self._L.shk_xchg_feasible(self._h))

    def xchg_wide_scatter_device(self, d_bases: int, d_offsets: int, n_seqs: int, n_bases: int):
        """→ (d_kmers, d_lanes, counts[n_owners]): the batch's k-mers as whole 64-bit values grouped by owner."""
        km, ln = C.c_void_p(), C.c_void_p()
        counts = (C.c_uint64 * 64)()
        self._check(self._L.shk_xchg_wide_scatter_device(self._h, d_bases, d_offsets, n_seqs, n_bases, C.byref(km), C.byref(ln), counts))
        return int(km.value or 0), int(ln.value or 0), [int(counts[i]) for i in range(max(self.n_owners, 1))]

    def insert_device(self, d_kmers: int, d_lanes: int, d_counts: int, n: int):
        self._check(self._L.shk_insert_device(self._h, d_kmers, d_lanes, d_counts, n))

    def set_read_index(self, next_read_index: int):
        """Global index of the next read (chunk striping of a sharded stream)."""
        self._check(self._L.shk_set_read_index(self._h, next_read_index))

    # -- torch views for the multi-GPU driver (sharkmer_amd/dist.py) ---------------------
    def table_tensors(self):
        """(keys int64[capacity], vals int32[n_lanes, capacity]) as zero-copy CUDA tensors over
        the live table (valid until the table grows)."""
        import torch
        n_pages, page_slots, n_lanes = self.table_geometry()
        cap = n_pages * page_slots
        dk, dv = self.table_device_ptrs()

        class _Raw:  # minimal __cuda_array_interface__ carrier
            def __init__(self, ptr, shape, typestr):
                self.__cuda_array_interface__ = {"shape": shape, "typestr": typestr,
                                                 "data": (ptr, False), "version": 2}

        keys = torch.as_tensor(_Raw(dk, (cap,), "<i8"), device=self._tdev)
        vals = torch.as_tensor(_Raw(dv, (n_lanes, cap), "<i4"), device=self._tdev)
        return keys, vals

    def merge_page_tensors(self, p0: int, p1: int, keys_t, vals_t):
        """KmerCounts::extend of a peer's page range held in torch tensors
        (keys_t int64[(p1-p0)*page_slots], vals_t int32[n_lanes, same])."""
        assert keys_t.is_contiguous() and vals_t.stride(-1) == 1
        self.merge_pages(p0, p1, keys_t.data_ptr(), vals_t.data_ptr(),
                         vals_t.stride(0) if vals_t.dim() == 2 else keys_t.numel())

    def set_owned_pages(self, p0: int, p1: int):
        self._check(self._L.shk_set_owned_pages(self._h, p0, p1))

    def set_owner_share(self, n_owners: int, owner: int):
        self._check(self._L.shk_set_owner_share(self._h, n_owners, owner))

    def owner_counts(self, n_owners: int) -> np.ndarray:
        """Occupied slots in each of n_owners equal page ranges."""
        out = np.zeros(n_owners, dtype=np.uint64)
        self._check(self._L.shk_owner_counts(self._h, n_owners, out.ctypes.data))
        return out

    def compact_owner_tensors(self, counts, skip_owner: int = -1):
        """The occupied entries, owner after owner: (keys int64[n], vals int32[n_lanes, n]) as new
        CUDA tensors, n = sum(counts) (counts from owner_counts with the same number of owners;
        skip_owner's count must be 0: its range is left out)."""
        import torch
        counts = np.asarray(counts, dtype=np.uint64)
        n = int(counts.sum())
        _, _, n_lanes = self.table_geometry()
        keys = torch.empty(max(n, 1), dtype=torch.int64, device=self._tdev)
        vals = torch.empty((n_lanes, max(n, 1)), dtype=torch.int32, device=self._tdev)
        off = np.zeros(len(counts), dtype=np.uint64)
        off[1:] = np.cumsum(counts)[:-1]
        self._check(self._L.shk_compact_owners(self._h, len(counts), off.ctypes.data, keys.data_ptr(),
                                               vals.data_ptr(), vals.stride(0), skip_owner))
        return keys[:n], vals[:, :n]

    def compact_owner_packed(self, counts, skip_owner: int = -1):
        """Every owner's occupied entries as one self-contained piece of ONE int32 CUDA tensor (include/shk.h,
        shk_compact_owners_packed): piece o = [k-mers 2·c ints][lane 0 counts c ints]…, c = counts[o].
        Queued on the engine's stream."""
        import torch
        counts = np.ascontiguousarray(counts, dtype=np.uint64)
        _, _, n_lanes = self.table_geometry()
        n = int(counts.sum())
        buf = torch.empty(max(n * (2 + n_lanes), 1), dtype=torch.int32, device=self._tdev)
        self._check(self._L.shk_compact_owners_packed(self._h, len(counts), counts.ctypes.data, buf.data_ptr(), skip_owner))
        return buf[:n * (2 + n_lanes)], n_lanes

    def compact_owner_fixed(self, n_owners: int, capacity: int, skip_owner: int = -1):
        """The same with pieces of a fixed capacity at fixed places (include/shk.h, shk_compact_owners_fixed):
        piece o = [header 2 ints][k-mers 2·capacity][lane counts capacity each], unused places EMPTY."""
        import torch
        n_lanes = max(1, self.chunks)  # (not table_geometry(): that waits for the counting launches)
        buf = torch.empty(n_owners * (2 + capacity * (2 + n_lanes)), dtype=torch.int32, device=self._tdev)
        self._check(self._L.shk_compact_owners_fixed(self._h, n_owners, capacity, buf.data_ptr(), skip_owner))
        return buf, n_lanes

    def merge_fixed_pieces(self, buf_t, n_pieces: int, capacity: int, skip_piece: int = -1):
        """KmerCounts::extend of all received fixed-capacity pieces in one launch — or of none, if any sender had
        more entries than a piece holds (shk_merge_pieces)."""
        assert buf_t.is_contiguous()
        self._check(self._L.shk_merge_pieces(self._h, buf_t.data_ptr(), n_pieces, capacity, skip_piece))

    def merge_pieces_max(self) -> int:
        """Largest piece header the last merge_fixed_pieces saw (valid after finalize): > capacity ⇒ not merged."""
        v = C.c_uint64(0)
        self._check(self._L.shk_merge_pieces_max(self._h, C.byref(v)))
        return int(v.value)

    def merge_packed_piece(self, piece_t, c: int, n_lanes: int):
        """KmerCounts::extend of one received piece (c entries: k-mers, then each lane's counts)."""
        if c:
            assert piece_t.is_contiguous() and piece_t.numel() == c * (2 + n_lanes)
            p = piece_t.data_ptr()
            self._check(self._L.shk_merge_entries(self._h, p, p + 8 * c, c, c))

    def merge_entry_tensors(self, keys_t, vals_t):
        """KmerCounts::extend of received entries (keys_t int64[n], vals_t int32[n_lanes, n], unit stride)."""
        n = keys_t.numel()
        if n == 0:
            return
        assert keys_t.is_contiguous() and vals_t.stride(-1) == 1
        self._check(self._L.shk_merge_entries(self._h, keys_t.data_ptr(), vals_t.data_ptr(), n, vals_t.stride(0)))

    # -- exchange rounds as torch tensors (sharkmer_amd/dist.py: OwnerCounter) -----------------------
    @staticmethod
    def _raw_tensor(ptr: int, n: int, typestr: str, device: str = "cuda"):
        import torch

        class _Raw:  # minimal __cuda_array_interface__ carrier
            def __init__(self, ptr, shape, typestr):
                self.__cuda_array_interface__ = {"shape": shape, "typestr": typestr,
                                                 "data": (ptr, False), "version": 2}
        if n == 0 or not ptr:
            return torch.empty(0, dtype={"<i4": torch.int32, "<i8": torch.int64, "|u1": torch.uint8}[typestr], device=device)
        return torch.as_tensor(_Raw(ptr, (n,), typestr), device=device)

    def xchg_scatter_tensors(self, d_bases: int, d_offsets: int, n_seqs: int, n_bases: int, layout_bases: int = 0):
        """One round's level-1 scatter → (records int32 or int64 [W·segment_records], cursors int32[W·regions],
        layout, n_foreign_spilled) as zero-copy views of the context's exchange buffer."""
        rec, cur, lay, nf = self.xchg_scatter_device(d_bases, d_offsets, n_seqs, n_bases, layout_bases)
        W = lay.n_owners
        # (a tensor element is one record: int32 for the 4-byte layout, int64 for the 8-byte one — layout.record_bytes)
        return (self._raw_tensor(rec, W * lay.segment_records, "<i8" if lay.record_bytes == 8 else "<i4", self._tdev),
                self._raw_tensor(cur, W * lay.regions, "<i4", self._tdev), lay, nf)

    def xchg_scatter_begin_tensors(self, d_bases: int, d_offsets: int, n_seqs: int, n_bases: int, layout_bases: int = 0):
        """xchg_scatter_tensors without the wait: (records, cursors, layout) — views that are complete once
        xchg_scatter_end() has returned (stream-ordered users on the engine's stream need not wait for that)."""
        rec, cur, lay = self.xchg_scatter_begin(d_bases, d_offsets, n_seqs, n_bases, layout_bases)
        W = lay.n_owners
        return (self._raw_tensor(rec, W * lay.segment_records, "<i8" if lay.record_bytes == 8 else "<i4", self._tdev),
                self._raw_tensor(cur, W * lay.regions, "<i4", self._tdev), lay)

    def xchg_absorb_tensors(self, rec_t, cur_t, lay):
        assert rec_t.is_contiguous() and cur_t.is_contiguous()
        assert rec_t.numel() == lay.segment_records and cur_t.numel() == lay.regions
        self.xchg_absorb(rec_t.data_ptr(), cur_t.data_ptr(), lay)

    def xchg_spill_tensors(self):
        """(kmers int64[n], lanes int32[n], counts int32[n]) views of the foreign spill list."""
        k, l, c, n = self.xchg_spill()
        return self._raw_tensor(k, n, "<i8", self._tdev), self._raw_tensor(l, n, "<i4", self._tdev), self._raw_tensor(c, n, "<i4", self._tdev)

    def insert_tensors(self, kmers_t, lanes_t, counts_t=None):
        """counts_t None: every record counts once."""
        n = kmers_t.numel()
        if n:
            assert kmers_t.is_contiguous() and lanes_t.is_contiguous() and (counts_t is None or counts_t.is_contiguous())
            self.insert_device(kmers_t.data_ptr(), lanes_t.data_ptr(), counts_t.data_ptr() if counts_t is not None else None, n)

    def xchg_wide_scatter_tensors(self, d_bases: int, d_offsets: int, n_seqs: int, n_bases: int):
        """→ (kmers int64[n], lanes int32[n], counts list[n_owners]) — views of the context's buffers, valid until the
        next scatter."""
        km, ln, counts = self.xchg_wide_scatter_device(d_bases, d_offsets, n_seqs, n_bases)
        n = sum(counts)
        return self._raw_tensor(km, n, "<i8", self._tdev), self._raw_tensor(ln, n, "<i4", self._tdev), counts

    # -- device memory + synthetic input ---------------------------------------------
    def alloc_device(self, nbytes: int) -> int:
        p = self._L.shk_alloc_device(self._h, nbytes)
        if not p:
            raise ShkError(-4, f"device allocation of {nbytes} bytes failed")
        return int(p)

    def free_device(self, p: int):
        self._L.shk_free_device(self._h, p)

    def synth_reads_device(self, spec, first_read: int, n_reads: int, d_bases: int, d_offsets: int):
        s = _Synth(seed_genome=spec.seed_genome, seed_reads=spec.seed_reads,
                   genome_len=spec.genome_len, read_len=spec.read_len,
                   sub_per_64k=spec.sub_per_64k, n_per_64k=spec.n_per_64k)
        self._check(self._L.shk_synth_reads_device(self._h, C.byref(s), first_read, n_reads,
                                                   d_bases, d_offsets))


# ---- 2-bit packed batches (include/shk.h: the reference's Read::from_str layout + an N mask) --------------

class PackedReads:
    """A batch as shk_pack_reads leaves it: packed u8[(n+3)//4] (4 bases per byte, first base on top),
    nmask u32[(n+31)//32] (bit p%32 of word p//32 ⇔ base p is N), offsets u64[n_seqs+1] in bases."""

    def __init__(self, packed, nmask, offsets, n_bases, _pinned=None):
        self.packed, self.nmask, self.offsets, self.n_bases = packed, nmask, offsets, n_bases
        self._pinned = _pinned  # (library, [pointers]) when the arrays are views over shk_alloc_pinned memory

    def close(self):
        """Give pinned arrays back (shk_free_pinned); the numpy views must not be used afterwards."""
        if self._pinned:
            L, ptrs = self._pinned
            self._pinned = None
            self.packed = self.nmask = self.offsets = None
            for q in ptrs:
                L.shk_free_pinned(q)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def nbytes(self):
        return self.packed.nbytes + self.nmask.nbytes + self.offsets.nbytes

    def wire_bytes(self) -> int:
        """What shk_ingest_packed moves over PCIe for this batch: the 2-bit stream, the offsets, and the N mask —
        as (index, word) pairs of its non-zero words when those are at most 1/16 of it (per slice in the engine;
        estimated here over the whole batch)."""
        nz = int(np.count_nonzero(self.nmask))
        mask = 8 * nz if nz <= self.nmask.size // 16 else self.nmask.nbytes
        return self.packed.nbytes + self.offsets.nbytes + mask


def release_cached_memory():
    """shk_release_cached_memory: device and pinned blocks the process keeps for the next context go back to the driver."""
    load_library().shk_release_cached_memory()


def pack_reads(bases: np.ndarray, offsets: np.ndarray, threads: int = 0, pinned: bool = False, out: "PackedReads" = None) -> PackedReads:
    """shk_pack_reads over a batch of concatenated ASCII reads (host, multi-threaded).  pinned: the
    output arrays live in pinned host memory (shk_alloc_pinned), owned by the PackedReads: close() — or dropping the
    object — gives them back.  out: a PackedReads of the same shape (a batch packed before) whose arrays are written
    again — a caller that streams batches pins its buffers once."""
    L = load_library() if (pinned or (out is not None and out._pinned)) else load_front_library()
    bases = np.ascontiguousarray(bases, dtype=np.uint8)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    n = int(offsets[-1]) if len(offsets) else 0
    assert len(offsets) == 0 or int(offsets[0]) == 0
    nb, nw = (n + 3) // 4, (n + 31) // 32
    if out is not None:
        assert out.packed.size == nb and out.nmask.size == nw and out.offsets.size == len(offsets), "out: another batch shape"
        out.offsets[:] = offsets
        rc = L.shk_pack_reads(bases.ctypes.data, n, out.packed.ctypes.data, out.nmask.ctypes.data, threads)
        if rc != 0:
            raise ShkError(rc, (L.shk_run_error() or b"").decode("utf-8", "replace"))
        out.n_bases = n
        return out
    if pinned:
        pp = L.shk_alloc_pinned(max(nb, 1) + 16)
        pm = L.shk_alloc_pinned(max(nw, 1) * 4 + 16)
        po = L.shk_alloc_pinned(offsets.nbytes + 16)
        packed = np.ctypeslib.as_array(C.cast(pp, C.POINTER(C.c_uint8)), shape=(nb,))
        nmask = np.ctypeslib.as_array(C.cast(pm, C.POINTER(C.c_uint32)), shape=(nw,))
        offs = np.ctypeslib.as_array(C.cast(po, C.POINTER(C.c_uint64)), shape=(len(offsets),))
        offs[:] = offsets
    else:
        packed, nmask, offs = np.zeros(nb, dtype=np.uint8), np.zeros(nw, dtype=np.uint32), offsets
    rc = L.shk_pack_reads(bases.ctypes.data, n, packed.ctypes.data, nmask.ctypes.data, threads)
    if rc != 0:
        raise ShkError(rc, (L.shk_run_error() or b"").decode("utf-8", "replace"))
    return PackedReads(packed, nmask, offs, n, _pinned=(L, [pp, pm, po]) if pinned else None)


# ---- host side either side of the path: FASTQ front-end, writers, whole-run driver -----------------

class FastqReader:
    """read_fastq / open_fastq_reader (io.rs:271-352, 598-625) through libshk's C++ host.
    Parses only (no GPU needed)."""

    def __init__(self, paths, max_reads: int = 0, validate_every: int = 0, gzip_all_members: bool = False, bgzf=None, device: int = 0):
        """gzip_all_members: NOT the reference (a gzip file is read up to the end of its first member, io.rs:606-617) —
        every member (bgzip, concatenated files), shk_fastq_open_ex's SHK_FASTQ_GZIP_ALL_MEMBERS.
        bgzf: "host" or "device" — every member too, BGZF members decoded in batches on the reader's threads or on HIP
        device `device` (SHK_FASTQ_BGZF_BATCH / SHK_FASTQ_BGZF_DEVICE, shk_fastq_open_device); the same reads and errors."""
        self._L = load_front_library()
        arr = (C.c_char_p * max(len(paths), 1))(*[os.fsencode(p) for p in paths])
        h = C.c_void_p()
        flags = (FASTQ_GZIP_ALL_MEMBERS if gzip_all_members else 0) | _bgzf_flags(bgzf)
        rc = self._L.shk_fastq_open_device(arr, len(paths), max_reads, validate_every, flags, device, C.byref(h))
        if rc != 0 and flags & FASTQ_BGZF_DEVICE:
            raise ShkError(rc, (self._L.shk_run_error() or b"").decode("utf-8", "replace"))
        if rc != 0:
            raise ShkError(rc, "shk_fastq_open failed")
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._L.shk_fastq_close(self._h)
            self._h = None

    __del__ = close

    def next_batch(self, max_seqs: int = 1_000_000, max_bases: int = 64 << 20):
        bases = np.empty(max_bases, dtype=np.uint8)
        offsets = np.zeros(max_seqs + 1, dtype=np.uint64)
        n = C.c_uint64(0)
        rc = self._L.shk_fastq_next_batch(self._h, bases.ctypes.data, max_bases, offsets.ctypes.data,
                                          max_seqs, C.byref(n))
        if rc != 0:
            raise ShkError(rc, (self._L.shk_fastq_error(self._h) or b"").decode("utf-8", "replace"))
        n = int(n.value)
        return bases[:int(offsets[n])].copy(), offsets[:n + 1].copy()

    def next_batch_packed(self, max_seqs: int = 1_000_000, max_bases: int = 64 << 20) -> "PackedReads":
        """The next batch in the 2-bit packed input format (shk_fastq_next_batch_packed): what pack_reads would make
        of next_batch's output, without the ASCII batch in between."""
        packed = np.zeros(((max_bases + 3) // 4 + 7) // 8 * 8, dtype=np.uint8)
        nmask = np.zeros((max_bases + 31) // 32, dtype=np.uint32)
        offsets = np.zeros(max_seqs + 1, dtype=np.uint64)
        n = C.c_uint64(0)
        rc = self._L.shk_fastq_next_batch_packed(self._h, packed.ctypes.data, nmask.ctypes.data, max_bases,
                                                 offsets.ctypes.data, max_seqs, C.byref(n))
        if rc != 0:
            raise ShkError(rc, (self._L.shk_fastq_error(self._h) or b"").decode("utf-8", "replace"))
        n = int(n.value)
        nb = int(offsets[n])
        return PackedReads(packed[:(nb + 3) // 4].copy(), nmask[:(nb + 31) // 32].copy(), offsets[:n + 1].copy(), nb)

    def stats(self) -> dict:
        a, b, m, d = C.c_uint64(0), C.c_uint64(0), C.c_int(0), C.c_int(0)
        self._L.shk_fastq_stats(self._h, C.byref(a), C.byref(b), C.byref(m), C.byref(d))
        return {"n_reads_read": int(a.value), "n_bases_read": int(b.value),
                "reached_max": bool(m.value), "done": bool(d.value)}

    def member_stats(self) -> dict:
        """gzip members decoded so far, by route (shk_fastq_member_stats): on the device, in host batches, one after the
        other.  The decoders run ahead of what has been handed out."""
        a, b, c = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        self._L.shk_fastq_member_stats(self._h, C.byref(a), C.byref(b), C.byref(c))
        return {"device": int(a.value), "host_batch": int(b.value), "sequential": int(c.value)}


def write_histo(path: str, histo: np.ndarray, k: int, histo_max: int, version: str = "3.1.0"):
    h = np.ascontiguousarray(histo, dtype=np.uint64)
    rc = load_front_library().shk_write_histo(os.fsencode(path), version.encode(), k, h.shape[0], histo_max,
                                        h.ctypes.data)
    if rc != 0:
        raise ShkError(rc, "shk_write_histo failed")


def write_final_histo(path: str, histo: np.ndarray, k: int, histo_max: int, version: str = "3.1.0"):
    h = np.ascontiguousarray(histo, dtype=np.uint64)
    rc = load_front_library().shk_write_final_histo(os.fsencode(path), version.encode(), k, h.shape[0],
                                              histo_max, h.ctypes.data)
    if rc != 0:
        raise ShkError(rc, "shk_write_final_histo failed")


def write_stats_yaml(path: str, **f):
    st = _RunStats(sharkmer_version=f.get("sharkmer_version", "3.1.0").encode(),
                   command=f.get("command", "").encode(), sample=f.get("sample", "").encode(),
                   kmer_length=f["kmer_length"], chunks=f["chunks"], n_reads_read=f["n_reads_read"],
                   n_bases_read=f["n_bases_read"], n_subreads_ingested=f["n_subreads_ingested"],
                   n_bases_ingested=f["n_bases_ingested"], n_kmers=f["n_kmers"],
                   n_multi_kmers=f.get("n_multi_kmers", 0), n_singleton_kmers=f.get("n_singleton_kmers", 0),
                   peak_memory_bytes=f.get("peak_memory_bytes", 0),
                   has_histogram=1 if f.get("has_histogram", f["chunks"] > 0) else 0)
    results = f.get("pcr_results")  # [(gene_name, status, product_lengths)]: stats.rs:11-23, 43-44
    if results is None:
        rc = load_front_library().shk_write_stats_yaml(os.fsencode(path), C.byref(st))
    else:
        arr, keep = (_PcrGeneStat * max(len(results), 1))(), []
        for i, (name, status, lengths) in enumerate(results):
            ln = np.asarray(list(lengths), dtype=np.uint64)
            keep.append(ln)
            arr[i] = _PcrGeneStat(name.encode(), int(status), len(ln), ln.ctypes.data if len(ln) else None)
        rc = load_front_library().shk_write_stats_yaml_pcr(os.fsencode(path), C.byref(st), arr, len(results))
    if rc != 0:
        raise ShkError(rc, "shk_write_stats_yaml failed")


def fastq_parse_geometry() -> int:
    """The bytes of text one wave takes in the framing passes (shk_fastq_parse_geometry)."""
    t = C.c_uint32(0)
    load_library().shk_fastq_parse_geometry(C.byref(t))
    return int(t.value)


def fastq_device_totals() -> dict:
    """shk_fastq_device_totals: process-wide, since the library was loaded."""
    v = [C.c_uint64(0) for _ in range(6)]
    load_library().shk_fastq_device_totals(*[C.byref(x) for x in v])
    return dict(zip(("batches", "records", "give_ups", "bytes_up", "bytes_down", "kernel_ns"), (int(x.value) for x in v)))


def validate_args(k: int, histo_max: int, sample):
    """cli.rs:659-673 + 645-652; raises ShkError with the reference's message."""
    L = load_front_library()
    rc = L.shk_validate_args(k, histo_max, None if sample is None else sample.encode())
    if rc != 0:
        raise ShkError(rc, (L.shk_run_error() or b"").decode("utf-8", "replace"))


def run_files(inputs, k: int, chunks: int, sample: str, outdir: str = "./", histo_max: int = 10000,
              max_reads: int = 0, validate_every: int = 0, device: int = 0, capacity_hint: int = 0,
              command: str = "", batch_reads: int = 0, batch_bases: int = 0, device_ids=None, gzip_all_members: bool = False,
              bgzf=None, parse=None, pcr_primers=None, read_threading: bool = False, min_kmer_count: int = 2, node_budget_global: int = 0,
              group_graph: bool = False, group_reads: bool = False, pcr_depths=None, **tuning) -> dict:
    """main.rs:112-199: FASTQ files → counts → .histo/.final.histo/.stats.yaml, and with pcr_primers (specification
    strings or PcrGene) sPCR's {sample}_{gene}.fasta files and pcr_results in the stats file (shk_run_files_pcr).
    tuning: the six global flags of main.rs:49-56 (max_dfs_states, max_paths_per_pair, max_node_visits,
    max_primer_kmers, high_coverage_ratio, tip_coverage_fraction), which overwrite every gene's values.
    device_ids: run on one multi-device context (shk_run_config.n_devices); with pcr_primers that needs group_graph=True
    (SHK_FLAG_GROUP_GRAPH), and read_threading there needs group_reads=True (SHK_FLAG_GROUP_READS).  gzip_all_members, bgzf: see FastqReader
    (bgzf="device" decodes on the context's first device).  parse="device" (with bgzf="device" only): the decoded text
    stays on the device and is framed there (SHK_FASTQ_DEVICE_PARSE); a file the route gives up on is read the
    bgzf="device" way from its start.  pcr_depths: "all" or a list of depths (chunks >= 1, one device, no read_threading):
    after the panel, pcr_run_depths with {sample}_{gene}.depth{d}.fasta and {sample}.pcr_depths.tsv (shk_count --pcr-depths)."""
    if parse not in (None, "device"):
        raise ValueError(f"parse must be None or 'device', not {parse!r}")
    known = ("max_dfs_states", "max_paths_per_pair", "max_node_visits", "max_primer_kmers", "high_coverage_ratio", "tip_coverage_fraction")
    if set(tuning) - set(known):
        raise TypeError(f"unexpected arguments {sorted(set(tuning) - set(known))}")
    L = load_library()
    arr = (C.c_char_p * max(len(inputs), 1))(*[os.fsencode(p) for p in inputs])
    cfg = _RunConfig(inputs=arr, n_inputs=len(inputs), k=k, chunks=chunks, device=device,
                     histo_max=histo_max, max_reads=max_reads, validate_every=validate_every,
                     sample=None if sample is None else sample.encode(), outdir=os.fsencode(outdir),
                     command=command.encode(), version=None, table_capacity_hint=capacity_hint,
                     batch_reads=batch_reads, batch_bases=batch_bases, fastq_flags=(FASTQ_GZIP_ALL_MEMBERS if gzip_all_members else 0) | _bgzf_flags(bgzf) | (FASTQ_DEVICE_PARSE if parse else 0))
    if device_ids is not None:
        ids = (C.c_int32 * len(device_ids))(*device_ids)
        cfg.n_devices = len(device_ids)
        cfg.device_ids = C.cast(ids, C.POINTER(C.c_int32))
    st = _RunStats()
    if pcr_primers:
        genes = []
        for spec in pcr_primers:
            try:
                g = spec if isinstance(spec, PcrGene) else parse_pcr_primers(spec)
            except ShkError as e:
                raise ShkError(e.code, f'Could not parse primer specification: "{spec}"\n\nCaused by:\n    {e.msg}') from None
            for name, value in tuning.items():
                setattr(g, name, value)
            genes.append(g)
        if min_kmer_count < 1:
            raise ShkError(-2, "min-kmer-count must be at least 1")
        arr = _pcr_genes(genes)
        pcfg = _PcrFileConfig(arr, len(genes), min_kmer_count, 1 if read_threading else 0, 0, node_budget_global,
                              (FLAG_GROUP_GRAPH if group_graph else 0) | (FLAG_GROUP_READS if group_reads else 0))
        if pcr_depths is not None:
            dep = np.arange(1, chunks + 1, dtype=np.uint32) if isinstance(pcr_depths, str) and pcr_depths == "all" else \
                np.ascontiguousarray(np.atleast_1d(pcr_depths), dtype=np.uint32)
            dep = dep if len(dep) else np.zeros(1, dtype=np.uint32)  # (an empty list is refused as depth 0 is)
            pcfg.depths, pcfg.n_depths = dep.ctypes.data, len(dep)
        rc = L.shk_run_files_pcr(C.byref(cfg), C.byref(pcfg), C.byref(st), None)
    elif pcr_depths is not None:
        raise ShkError(-2, "--pcr-depths needs --pcr-primers")
    else:
        rc = L.shk_run_files(C.byref(cfg), C.byref(st))
    if rc != 0:
        raise ShkError(rc, (L.shk_run_error() or b"").decode("utf-8", "replace"))
    return {f: int(getattr(st, f)) for f, t in _RunStats._fields_ if t in (C.c_uint32, C.c_uint64)}
