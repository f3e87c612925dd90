"""The reference's data model of a counting run, call by call — the expected answer of the call-sequence sweep
(tests/test_gpu_sequences.py).  CPU only, oracle only.

A context is n_lanes = max(chunks, 1) `KmerCounts` (one per Chunk, io.rs:378-379), a running read index and the
read/base counters of FastqReadState.  Nothing is merged until somebody looks: an observation builds a fresh merged
`KmerCounts` and a fresh `Histogram` and extends them lane after lane, taking `get_vector()` after each — literally
io.rs:1020-1028 — so the model has no state of its own that a call order could leave stale.  What the engine keeps
between calls (a merged table, lazily cleared blocks, a histogram left behind by a page pass) has no counterpart
here: that is the point."""
from __future__ import annotations

import numpy as np

import pcr_ref
import primer_ref
import products_ref
import prune_ref
import thread_ref

U32_MAX = 0xFFFFFFFF
SHK_ERR_BAD_ARG, SHK_ERR_STATE = -2, -11  # include/shk.h
_VALID = np.zeros(256, dtype=bool)
_VALID[list(b"ACGTN")] = True

NO_READS = "No reads were ingested. Check that input files contain valid FASTQ records."  # io.rs:578-580


class ModelError(Exception):
    """The reference's anyhow error, with its text — or, where the reference has no such call and include/shk.h states
    the error, the ABI's code."""

    def __init__(self, text, code=None):
        super().__init__(text)
        self.code = code


class Observation:
    """What consolidate_and_histogram leaves (io.rs:1020-1047): the merged table, one histogram column per lane,
    the saturation warning and the totals."""

    def __init__(self, merged, columns, any_saturated, lane_sum):
        self.merged, self.columns, self.any_saturated, self.lane_sum = merged, columns, any_saturated, lane_sum
        self.keys, self.counts = merged.export()
        self.n_unique = len(merged)
        self.n_hashed = merged.get_n_kmers()


class MergedView:
    """The merged table read key by key, as much of a {k-mer: count} dict as tests/pcr_ref.py asks for: a key inserted
    with count 0 is there with 0, an absent one gives the default."""

    def __init__(self, merged):
        self.merged = merged

    def get(self, kmer, default=None):
        return self.merged.get_count(kmer) if self.merged.contains(kmer) else default


class LaneModel:
    def __init__(self, orc, k: int, chunks: int, histo_max: int, multi_device: bool = False, group_graph: bool = False):
        self.orc, self.k, self.chunks, self.histo_max = orc, k, chunks, histo_max
        self.multi_device = multi_device  # (the same data model: only what the ABI refuses on such a context differs)
        self.group_graph = group_graph    # SHK_FLAG_GROUP_GRAPH: a multi-device context answers the graph calls, merged
        self.n_lanes = max(chunks, 1)  # io.rs:378
        self.retain = False  # shk_retain_reads: the switch outlives a reset, what is retained does not
        self.reset()

    # ---- operations ------------------------------------------------------------------------------
    def reset(self):
        """A fresh FastqReadState (io.rs:381-387)."""
        self.lanes = [self.orc.KmerCounts(self.k) for _ in range(self.n_lanes)]
        self.read_index = 0
        self.n_reads = self.n_bases_read = self.n_bases_ingested = self.n_inserted = 0
        self.retained = []  # the reads of every ingest since, in arrival order, as bytes
        self._obs = None

    def set_read_index(self, i: int):
        self.read_index = int(i)

    @staticmethod
    def first_bad_byte(bases, offsets):
        """The first byte outside ACGTN in input order (encoding.rs:353-356), or None."""
        lo, hi = int(offsets[0]), int(offsets[-1])
        bad = np.flatnonzero(~_VALID[np.asarray(bases[lo:hi], dtype=np.uint8)])
        return int(bases[lo + int(bad[0])]) if len(bad) else None

    @staticmethod
    def bad_byte_message(b: int) -> str:
        return "Invalid character '%s' in sequence. Only ACGTN allowed." % chr(b)

    def _ingest(self, bases, offsets, lane_of):
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        off = [int(x) for x in offsets]
        bad = self.first_bad_byte(bases, off)
        if bad is not None:
            raise ModelError(self.bad_byte_message(bad))
        self._obs = None
        raw = bases.tobytes()
        for i in range(len(off) - 1):
            self.lanes[lane_of(i)].ingest_seq(raw[off[i]:off[i + 1]])  # Chunk::ingest_seq, chunk.rs:25-30
        n = len(off) - 1
        if self.retain:  # whatever the lane and the read index: the store is one list
            self.retained += [raw[off[i]:off[i + 1]] for i in range(n)]
        self.n_reads += n
        self.n_bases_read += off[-1] - off[0]
        self.n_bases_ingested += int((bases[off[0]:off[-1]] != ord("N")).sum())  # chunk.rs:28
        return n

    def ingest_reads(self, bases, offsets):
        """read_fastq's cadence: read i goes to lane (i // 1000) % n_lanes (io.rs:340-361)."""
        first = self.read_index
        n = self._ingest(bases, offsets, lambda i: ((first + i) // 1000) % self.n_lanes)
        self.read_index = first + n

    def ingest_batch(self, chunk_id: int, bases, offsets):
        """drain_batch's body with an explicit chunk (io.rs:356-358); the striping index stays."""
        assert 0 <= chunk_id < self.n_lanes
        self._ingest(bases, offsets, lambda i: chunk_id)

    def insert(self, chunk_id: int, kmers, counts):
        """KmerCounts::insert (counting.rs:152-154): the entry is created whatever the count, the add saturates."""
        assert 0 <= chunk_id < self.n_lanes
        self._obs = None
        for key, c in zip(np.atleast_1d(kmers).tolist(), np.atleast_1d(counts).tolist()):
            self.lanes[chunk_id].insert(int(key), int(c))
            self.n_inserted += 1

    # ---- observations ----------------------------------------------------------------------------
    def is_empty(self) -> bool:
        return self.n_reads == 0 and self.n_inserted == 0

    def observe(self) -> Observation:
        if self._obs is None:
            est = sum(len(l) for l in self.lanes)  # io.rs:1005-1006
            merged, histo = self.orc.KmerCounts(self.k, est), self.orc.Histogram(self.histo_max)
            cols, sat = [], False
            for lane in self.lanes:  # io.rs:1023-1028
                sat |= merged.extend_with_histogram(lane, histo)
                cols.append(histo.get_vector())
            self._obs = Observation(merged, np.stack(cols), sat, sum(l.get_n_kmers() for l in self.lanes))
        return self._obs

    def columns(self) -> np.ndarray:
        """histo_vecs: (chunks, histo_max + 2); chunks = 0 has none (io.rs:1133-1158)."""
        return self.observe().columns[:self.chunks]

    def totals(self) -> dict:
        o = self.observe()
        t = dict(n_reads_ingested=self.n_reads, n_bases_read=self.n_bases_read, n_bases_ingested=self.n_bases_ingested,
                 n_kmers_ingested=o.lane_sum, n_unique_kmers=o.n_unique, n_hashed_kmers=o.n_hashed,
                 any_saturated=int(o.any_saturated))
        if self.chunks > 0:
            t["n_singleton_kmers"] = int(o.columns[-1][1])  # io.rs:1096-1099
        return t

    def finalize(self) -> Observation:
        """consolidate_and_histogram's checks in the reference's order; the observation is computed by then."""
        if self.is_empty():
            raise ModelError(NO_READS)
        o = self.observe()
        if o.n_hashed != o.lane_sum:  # io.rs:1042-1047
            raise ModelError("The total count of hashed kmers (%d) does not equal the number of ingested kmers (%d)"
                             % (o.n_hashed, o.lane_sum))
        if self.chunks > 0:
            nu = int(o.columns[-1][1:].sum())
            if nu != o.n_unique:  # io.rs:1127-1132: a key with merged count 0 sits in no bin
                raise ModelError("The total count of unique kmers in the histogram (%d) does not equal the total "
                                 "count of hashed kmers (%d)" % (nu, o.n_unique))
        return o

    def export(self):
        o = self.observe()
        return o.keys, o.counts

    def get_count(self, kmers, canonical: bool = False) -> np.ndarray:
        m = self.observe().merged
        f = m.get_canonical_count if canonical else m.get_count
        return np.array([f(int(x)) for x in np.atleast_1d(kmers).tolist()], dtype=np.uint32)

    def find_oligos(self, oligos, oligo_len: int, min_count: int = 1):
        return self.observe().merged.find_oligos(oligos, oligo_len, min_count)

    def primer_kmers(self, primers):
        """get_primer_kmers per direction over the merged table (tests/primer_ref.py)."""
        keys, counts = self.export()
        for p in primers:
            primer_ref.check_variant_limit(p.seq, p.trim, self.k)
        return [primer_ref.get_primer_kmers(p.seq, keys, counts, self.k, p.trim, p.mismatches, p.min_count,
                                            p.max_kmers, check_variants=False) for p in primers]

    # ---- sPCR's graph extension (tests/pcr_ref.py) -----------------------------------------------
    def graph_table(self, what: str) -> MergedView:
        """The merged table as shk_lookup(canonical = 1) sees it — the saturating sum over the lanes, a key inserted
        with count 0 present with 0 — or the refusal include/shk.h states for `what`."""
        if self.multi_device and not self.group_graph:
            raise ModelError("%s needs the whole table on one device: this is a multi-device context (n_devices > 1)" % what,
                             SHK_ERR_STATE)
        if self.k < 2:
            raise ModelError("%s needs k >= 2 (a node is a (k-1)-mer), got k=%d" % (what, self.k), SHK_ERR_BAD_ARG)
        return MergedView(self.observe().merged)

    def neighborhood(self, nodes, dirs, min_count: int, max_levels: int = 0, cap: int = 1 << 16, fringe_cap: int = 1 << 16):
        """shk_neighborhood → (kmers, counts, fringe_nodes, fringe_dirs, levels_done) as lists."""
        table = self.graph_table("shk_neighborhood")
        mask = (1 << (2 * (self.k - 1))) - 1
        for i, (n, d) in enumerate(zip(nodes, dirs)):
            if not 1 <= int(d) <= 3 or int(n) > mask:
                raise ModelError("seed %d: (node 0x%x, dir %d) is no (k-1)-mer with a dir of 1, 2 or 3" % (i, int(n), int(d)),
                                 SHK_ERR_BAD_ARG)
        try:
            return pcr_ref.neighborhood(nodes, dirs, table, self.k, min_count, max_levels, cap, fringe_cap)
        except ValueError as e:  # more distinct seeds than fringe_cap
            raise ModelError(str(e), SHK_ERR_BAD_ARG) from e

    def pcr_extend(self, fwd, rev, **params):
        """shk_pcr_extend → (pcr_ref.Graph of the last step run, threshold used, steps run).  fwd, rev: (k-mers,
        counts); params: pcr_ref.pcr_extend's (min_count, table_min_count, high_coverage_ratio, max_num_nodes, sweep)."""
        table = self.graph_table("shk_pcr_extend")
        return pcr_ref.pcr_extend(fwd, rev, table, self.k, **params)

    def neighborhood_panel(self, jobs, max_levels: int = 0):
        """shk_neighborhood_panel: `neighborhood` per job (nodes, dirs, min_count, cap, fringe_cap), one max_levels."""
        return [self.neighborhood(n, d, mc, max_levels, cap, fcap) for n, d, mc, cap, fcap in jobs]

    # ---- retained reads (shk_retain_api.hip.h) ---------------------------------------------------
    def _single_device(self):
        if self.multi_device:
            raise ModelError("not available on a multi-device context", SHK_ERR_STATE)

    def retain_reads(self, on: bool = True):
        """shk_retain_reads: on takes a context that holds no reads; off drops the store."""
        self._single_device()
        if not on:
            self.retain, self.retained = False, []
        elif not self.retain:
            if self.n_reads or self.n_bases_read:
                raise ModelError("shk_retain_reads: the context holds reads already; switch retention on after shk_create or shk_reset",
                                 SHK_ERR_STATE)
            self.retain = True
        elif self.retained:
            raise ModelError("reads are being retained already", SHK_ERR_STATE)

    def _retaining(self, who: str):
        self._single_device()
        if not self.retain:
            raise ModelError("%s: reads are not retained (shk_retain_reads)" % who, SHK_ERR_STATE)

    def retained_info(self) -> dict:
        self._single_device()
        return dict(reads=len(self.retained), bases=sum(len(r) for r in self.retained))

    def retained_export(self, first: int, n: int):
        """shk_retained_export → (bases, offsets from 0) of retained reads first .. first + n."""
        self._retaining("shk_retained_export")
        if first > len(self.retained) or n > len(self.retained) - first:
            raise ModelError("reads %d to %d are outside the %d retained reads" % (first, first + n, len(self.retained)), SHK_ERR_BAD_ARG)
        part = self.retained[first:first + n]
        offsets = np.zeros(n + 1, dtype=np.uint64)
        offsets[1:] = np.cumsum([len(r) for r in part])
        return np.frombuffer(b"".join(part), dtype=np.uint8), offsets

    def filter_reads_panel(self, reads, genes) -> list:
        """PrimerReadFilter::filter_reads per gene (read_filter.rs:24-55), as panel_cases.expected: the oracle's
        KmerCounts.filter_matches per gene and read → ascending indices into `reads` (a list of bytes) per gene."""
        rows = []
        for gene in genes:
            kc = self.orc.KmerCounts(self.k)
            for x in np.atleast_1d(gene).tolist():
                kc.insert(int(x), 1)
            rows.append([i for i, r in enumerate(reads) if kc.filter_matches(r)])
        return rows

    def filter_retained(self, genes) -> list:
        self._retaining("shk_filter_reads_panel_retained")
        return self.filter_reads_panel(self.retained, genes)

    def thread_reads_panel(self, reads, graphs, lists, read_index=None, mate=None) -> list:
        """thread_reads[_paired] per gene over its listed reads in list order (tests/thread_ref.py, as
        thread_panel_cases.expected).  graphs: (sub_kmers, [(source, target)]) per gene; reads: a list of bytes, or a
        {index: bytes} of the listed ones → per gene (support_total, support_unambiguous, links, link_counts,
        read_edges, n_paired_links)."""
        if self.k < 2:
            raise ModelError("shk_thread_reads needs k >= 2 (a node is a (k-1)-mer), got k=%d" % self.k, SHK_ERR_BAD_ARG)
        out = []
        for (sub, edges), ids in zip(graphs, lists):
            g = thread_ref.Graph([int(x) for x in sub], [(int(s), int(t)) for s, t in edges])
            seqs = [reads[int(i)] for i in ids]
            if mate is None:
                ann = thread_ref.thread_reads(g, seqs, self.k)
            else:
                ann = thread_ref.thread_reads_paired(g, seqs, [int(read_index[int(i)]) for i in ids], [int(mate[int(i)]) for i in ids], self.k)
            out.append(tuple(thread_ref.as_arrays(ann, len(g.edges))) + (ann.n_paired_links,))
        return out

    def thread_retained(self, graphs, lists, read_index=None, mate=None) -> list:
        self._retaining("shk_thread_reads_panel_retained")
        return self.thread_reads_panel(self.retained, graphs, lists, read_index, mate)

    # ---- the calls that need no table: the context's k is all they take ------------------------
    def prune_panel(self, graphs, fractions, stages) -> list:
        """shk_pcr_prune_panel → one prune_ref.Pruned per gene; graphs: (flags, edge_src, edge_tgt, edge_counts)."""
        return [prune_ref.prune(*g, self.k, f, s) for g, f, s in zip(graphs, fractions, stages)]

    @staticmethod
    def dedup_panel(records, scores, thresholds) -> list:
        """shk_pcr_dedup_panel → per gene (order, pair bits of the sorted order, kept, generated, retained) by
        tests/products_ref.py's sort_and_deduplicate and its full-matrix edit distance."""
        out = []
        for seqs, sc, t in zip(records, scores, thresholds):
            dist = products_ref.distance_matrix(seqs)
            order = products_ref.sort_order(seqs, sc)
            kept, retained = products_ref.sort_and_deduplicate(seqs, sc, t, dist)
            out.append((order, products_ref.pair_matrix(seqs, order, t, dist), kept, len(seqs), retained))
        return out
