"""do_pcr (src/pcr/mod.rs:431-819) as run_pcr drives it (src/stats.rs:84-98), composed from the models of its stages:
primer_ref (get_primer_kmers), pcr_ref (seed graph, extension, threshold sweep), prune_ref, thread_ref, products_ref.
Nothing here calls the library: the expected answers of shk_pcr_run come from this file."""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

import pcr_ref
import primer_ref
import products_ref
import prune_ref
import thread_ref

SUCCESS, NO_FORWARD, NO_REVERSE, NO_PRIMERS, NO_PATH, NODE_BUDGET = range(6)
REASONS = {SUCCESS: None, NO_FORWARD: "forward primer not found", NO_REVERSE: "reverse primer not found",
           NO_PRIMERS: "forward and reverse primers not found", NO_PATH: "no path found", NODE_BUDGET: "node budget exceeded"}


@dataclass
class Outcome:
    status: int = NO_PATH
    reason: str | None = None
    products: list = field(default_factory=list)   # products_ref.Record, in product order
    n_fwd_kmers: int = 0
    n_rev_kmers: int = 0
    max_fwd_count: int = 0
    max_rev_count: int = 0
    median_primer_count: int = 0
    threshold_used: int = 0
    steps_run: int = 0
    found_path: bool = False
    n_nodes: int = 0
    n_edges: int = 0
    n_pruned_nodes: int = 0
    n_pruned_edges: int = 0
    n_reads_matched: int = 0
    matched: list = field(default_factory=list)
    threaded: bool = False
    n_paired_links: int = 0
    low_primer_counts: bool = False
    generated: int = 0
    paths_found: int = 0


def median_count(counts) -> int:
    """KmerCounts::get_median_count (counting.rs:275-298)."""
    v = sorted(int(c) for c in counts)
    if not v:
        return 0
    mid = len(v) // 2
    return v[mid - 1] // 2 + v[mid] // 2 if len(v) % 2 == 0 else v[mid]


def read_kmer_sets(reads, k):
    """Per read the set of its kmers_from_ascii k-mers, None for a read with a byte outside ACGTN (read_filter.rs:43-49)."""
    out = []
    for s in reads:
        try:
            kmers, _ = thread_ref.kmers_from_ascii(s, k)
            out.append(set(int(x) for x in kmers))
        except thread_ref.InvalidChar:
            out.append(None)
    return out


def primer_sets(gene, keys, counts, k, min_count):
    """primers::get_primer_kmers (primers.rs:440-478): both variant checks first, then forward, then reverse."""
    primer_ref.check_variant_limit(gene.forward_seq, gene.trim, k)
    primer_ref.check_variant_limit(gene.reverse_seq, gene.trim, k)
    args = (keys, counts, k, gene.trim, gene.mismatches, min_count, gene.max_primer_kmers, False)
    return primer_ref.get_primer_kmers(gene.forward_seq, *args), primer_ref.get_primer_kmers(gene.reverse_seq, *args)


def do_pcr(gene, keys, counts, table, k, reads, kmer_sets, read_index, mate, min_kmer_count, max_num_nodes) -> Outcome:
    o = Outcome()
    min_count = max(gene.min_count, min_kmer_count)  # collect_pcr_params, cli.rs:556-570
    f, r = primer_sets(gene, keys, counts, k, min_count)
    o.n_fwd_kmers, o.n_rev_kmers = len(f[0]), len(r[0])
    o.max_fwd_count = max((int(c) for c in f[1]), default=0)
    o.max_rev_count = max((int(c) for c in r[1]), default=0)
    if not o.n_fwd_kmers or not o.n_rev_kmers:  # mod.rs:446-468
        o.status = NO_PRIMERS if not o.n_fwd_kmers and not o.n_rev_kmers else NO_FORWARD if not o.n_fwd_kmers else NO_REVERSE
        o.reason = REASONS[o.status]
        return o
    o.median_primer_count = min(median_count(f[1]), median_count(r[1]))
    o.low_primer_counts = o.max_fwd_count < 5 or o.max_rev_count < 5
    gene_reads = None
    if reads is not None:  # from_primer_kmers + filter_reads (read_filter.rs:24-55)
        want = {min(int(x), pcr_ref.revcomp(int(x), k)) for x in list(f[0]) + list(r[0])}
        gene_reads = [i for i, ks in enumerate(kmer_sets) if ks is not None and ks & want]
        o.matched, o.n_reads_matched = gene_reads, len(gene_reads)
    graph, o.threshold_used, o.steps_run = pcr_ref.pcr_extend(f[:2], r[:2], table, k, min_count, min_kmer_count, gene.high_coverage_ratio,
                                                              max_num_nodes, True)
    o.found_path, o.n_nodes, o.n_edges = bool(graph.found_path), len(graph.sub_kmer), len(graph.edges)
    o.status = NODE_BUDGET if o.n_nodes >= max_num_nodes else NO_PATH  # mod.rs:567, 621-623
    if graph.found_path:
        es, et, ec = ([e[i] for e in graph.edges] for i in range(3))
        pr = prune_ref.prune(graph.flags(), es, et, ec, k, gene.tip_coverage_fraction)
        sub = [graph.sub_kmer[v] for v in pr.node_index]
        o.n_pruned_nodes, o.n_pruned_edges = len(sub), len(pr.edge_src)
        ann = None
        if gene_reads:  # mod.rs:664-697
            tg = thread_ref.Graph(sub, list(zip(pr.edge_src, pr.edge_tgt)))
            seqs = [reads[i] for i in gene_reads]
            if mate is not None and any(mate[i] != 0 for i in gene_reads):
                a = thread_ref.thread_reads_paired(tg, seqs, [int(read_index[i]) for i in gene_reads], [int(mate[i]) for i in gene_reads], k)
            else:
                a = thread_ref.thread_reads(tg, seqs, k)
            tot, una, links, link_counts, _ = thread_ref.as_arrays(a, len(pr.edge_src))
            ann = products_ref.Annotations(tot, una, {tuple(l): c for l, c in zip(links, link_counts)})
            o.threaded, o.n_paired_links = True, a.n_paired_links
        res = products_ref.run_gene(k, sub, pr.node_flags, pr.edge_src, pr.edge_tgt, pr.edge_counts, pr.coverage_ratio, ann,
                                    products_ref.Params(gene.min_length, gene.max_length, gene.max_dfs_states, gene.max_paths_per_pair,
                                                        gene.max_node_visits, gene.dedup_edit_threshold))
        o.generated, o.paths_found = len(res.records), res.paths_found
        if res.records:  # mod.rs:735-743
            o.status, o.products = SUCCESS, res.products
    o.reason = REASONS[o.status]
    return o


def run_pcr(keys, counts, k, genes, reads=None, read_index=None, mate=None, paired=False, min_kmer_count=2, max_num_nodes=100_000):
    """One Outcome per gene.  keys / counts: the merged table; reads: byte strings or None; read_index / mate per read, or
    paired=True for interleaved pairs (reread_sequences, io.rs:831-898: R1, R2, R1, … with index = ordinal)."""
    table = pcr_ref.table_dict(keys, counts)
    kmer_sets = None
    if reads is not None:
        reads = [bytes(s) for s in reads]
        kmer_sets = read_kmer_sets(reads, k)
        if mate is None and paired:
            read_index, mate = list(range(len(reads))), [1 + (i & 1) for i in range(len(reads))]
    return [do_pcr(g, keys, counts, table, k, reads, kmer_sets, read_index, mate, min_kmer_count, max_num_nodes) for g in genes]


def split_reads(bases: np.ndarray, offsets: np.ndarray) -> list:
    return [bases[int(offsets[i]):int(offsets[i + 1])].tobytes() for i in range(len(offsets) - 1)]


def fasta_text(sample, gene_name, products, width=80) -> str:
    """run_pcr's file for a gene (stats.rs:106-116): write_fasta_record (io.rs:144-158) per product."""
    out = []
    for i, r in enumerate(products):
        out.append(f">{sample}_{gene_name}_{i} {r.desc(sample, gene_name, i)}\n")
        out += [r.sequence[a:a + width] + "\n" for a in range(0, len(r.sequence), width)]
    return "".join(out)
