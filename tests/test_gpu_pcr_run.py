"""GPU tests of shk_pcr_run, shk_run_files_pcr and shk_count's sPCR flags against tests/pcr_run_ref.py (do_pcr / run_pcr
composed from the stage models) and against the six stage calls chained by hand on the same context: the mixed panel
(every status) without reads, with a host batch, with retained reads, as interleaved pairs by rule and by arrays; a batch
that matches nothing; the padded 18S; the error order; states and capacities; the command line and run_files.  The
expected answers are computed once (pcr_run_cases) and shared."""
import os
import subprocess

import numpy as np
import pytest
import yaml

import pcr_panel_cases as pc
import pcr_run_cases as cases
import pcr_run_ref as ref
import sharkmer_amd as sa
from test_products_ref_cpu import assert_records

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "sharkmer_amd", "csrc", "shk_count")
DIAGNOSTICS = ("n_fwd_kmers", "n_rev_kmers", "max_fwd_count", "max_rev_count", "median_primer_count", "threshold_used", "steps_run",
               "found_path", "n_nodes", "n_edges", "n_pruned_nodes", "n_pruned_edges", "n_reads_matched", "threaded", "n_paired_links",
               "low_primer_counts")


def assert_outcomes(got, want, what):
    assert len(got) == len(want), what
    for i, (g, w) in enumerate(zip(got, want)):
        at = f"{what}: gene {i} '{g.gene_name}'"
        assert (g.status, g.failure_reason) == (w.status, w.reason), at
        assert [getattr(g, f) for f in DIAGNOSTICS] == [getattr(w, f) for f in DIAGNOSTICS], at
        assert (g.products.paths_found, g.products.generated) == (w.paths_found, w.generated), at
        assert_records(g.products, w.products, at)


def same_outcomes(a, b, what):
    for x, y in zip(a, b):
        assert (x.status, [getattr(x, f) for f in DIAGNOSTICS]) == (y.status, [getattr(y, f) for f in DIAGNOSTICS]), (what, x.gene_name)
        assert x.products.sequences == y.products.sequences, (what, x.gene_name)
        for f in ("start_node", "path_nodes", "count_mean", "count_median", "count_min", "count_max", "score", "score_fields"):
            assert getattr(x.products, f).tobytes() == getattr(y.products, f).tobytes(), (what, x.gene_name, f)


def canonical(kmers, k):
    return np.array(sorted({min(int(x), ref.pcr_ref.revcomp(int(x), k)) for x in kmers}), dtype=np.uint64)


def hand_chain(e, k, genes, reads=None, min_kmer_count=2, max_num_nodes=100_000):
    """The six stage calls as a caller had to chain them before shk_pcr_run → per gene None (no primer set) or
    (PcrGraph, PcrProducts or None)."""
    mc = [max(g.min_count, min_kmer_count) for g in genes]
    prim = e.primer_kmers([sa.Primer(s, g.trim, g.mismatches, m, g.max_primer_kmers) for g, m in zip(genes, mc) for s in (g.forward_seq, g.reverse_seq)])
    alive = [i for i in range(len(genes)) if len(prim[2 * i][0]) and len(prim[2 * i + 1][0])]
    graphs = e.pcr_extend_panel([prim[2 * i + d] for i in alive for d in (0, 1)],
                                [dict(min_count=mc[i], table_min_count=min_kmer_count, high_coverage_ratio=genes[i].high_coverage_ratio,
                                      max_num_nodes=max_num_nodes) for i in alive])
    out = [None] * len(genes)
    found = [(i, gr) for i, gr in zip(alive, graphs) if gr.found_path]
    for i, gr in zip(alive, graphs):
        out[i] = (gr, None)
    if found:
        pruned = e.pcr_prune_panel([gr for _, gr in found], tip_coverage_fraction=[genes[i].tip_coverage_fraction for i, _ in found])
        anns = None
        if reads is not None:
            lists = e.filter_reads_panel(reads[0], reads[1], [canonical(np.concatenate([prim[2 * i][0], prim[2 * i + 1][0]]), k) for i, _ in found])
            anns = e.thread_reads_panel(pruned, reads[0], reads[1], lists)
            anns = [a if len(l) else None for a, l in zip(anns, lists)]
        gs = [genes[i] for i, _ in found]
        prods = e.pcr_products_panel(pruned, anns, min_length=[g.min_length for g in gs], max_length=[g.max_length for g in gs],
                                     max_dfs_states=[g.max_dfs_states for g in gs], max_paths_per_pair=[g.max_paths_per_pair for g in gs],
                                     max_node_visits=[g.max_node_visits for g in gs], dedup_edit_threshold=[g.dedup_edit_threshold for g in gs])
        for (i, gr), p in zip(found, prods):
            out[i] = (gr, p)
    return out


def assert_equals_chain(got, chain, what):
    for o, c in zip(got, chain):
        at = (what, o.gene_name)
        if c is None:
            assert o.status in (sa.PCR_NO_FORWARD, sa.PCR_NO_REVERSE, sa.PCR_NO_PRIMERS) and o.n_nodes == 0, at
            continue
        gr, p = c
        assert (o.threshold_used, o.steps_run, o.found_path, o.n_nodes, o.n_edges) == (gr.threshold_used, gr.steps_run, gr.found_path,
                                                                                      len(gr.node_sub_kmers), len(gr.edge_src)), at
        if p is None:
            assert not o.products.sequences, at
            continue
        assert o.products.sequences == p.sequences, at
        for f in ("start_node", "path_nodes", "count_mean", "count_median", "count_min", "count_max", "score", "score_fields"):
            assert getattr(o.products, f).tobytes() == getattr(p, f).tobytes(), at + (f,)


@pytest.fixture(scope="module")
def mixed(orc):
    p = pc.mixed_panel(orc)
    with sa.KmerEngine(p.k, 1, 100) as e:
        e.retain_reads(True)
        e.ingest_reads(p.bases, p.offsets)
        e.finalize()
        yield e, p, cases.mixed_genes(orc)


def test_mixed_panel_without_reads(mixed, orc):
    e, p, genes = mixed
    got = e.pcr_run(genes, max_num_nodes=pc.MIXED_BUDGET)
    assert_outcomes(got, cases.mixed_expected(orc, "none"), "no reads")
    assert {o.status for o in got} == {0, 1, 3, 4, 5}
    assert_equals_chain(got, hand_chain(e, p.k, genes, max_num_nodes=pc.MIXED_BUDGET), "no reads")
    assert all(np.isnan(o.products.score_fields[:, 3:]).all() for o in got)


def test_mixed_panel_with_a_host_batch_and_with_retained_reads(mixed, orc):
    e, p, genes = mixed
    want = cases.mixed_expected(orc, "reads")
    host = e.pcr_run(genes, reads=(p.bases, p.offsets), max_num_nodes=pc.MIXED_BUDGET)
    kept = e.pcr_run(genes, reads="retained", max_num_nodes=pc.MIXED_BUDGET)
    assert_outcomes(host, want, "host batch")
    assert_outcomes(kept, want, "retained")
    same_outcomes(host, kept, "host batch and retained")
    assert_equals_chain(host, hand_chain(e, p.k, genes, (p.bases, p.offsets), max_num_nodes=pc.MIXED_BUDGET), "host batch")
    assert any(o.threaded for o in host)
    for o in host:
        assert o.threaded == (o.found_path and o.n_reads_matched > 0), o.gene_name
        if len(o.products.sequences):
            assert np.isnan(o.products.score_fields[:, 3:]).all() == (not o.threaded), o.gene_name  # NaN exactly where unthreaded

def test_pairs_by_rule_and_by_arrays(mixed, orc):
    e, p, genes = mixed
    n = len(p.offsets) - 1
    index, mate = np.arange(n, dtype=np.uint64), (1 + (np.arange(n) & 1)).astype(np.uint8)
    want = cases.mixed_expected(orc, "paired")
    for what, got in (("rule, host", e.pcr_run(genes, reads=(p.bases, p.offsets), paired=True, max_num_nodes=pc.MIXED_BUDGET)),
                      ("rule, retained", e.pcr_run(genes, reads="retained", paired=True, max_num_nodes=pc.MIXED_BUDGET)),
                      ("arrays", e.pcr_run(genes, reads=(p.bases, p.offsets, index, mate), max_num_nodes=pc.MIXED_BUDGET))):
        assert_outcomes(got, want, what)
    odd = e.pcr_run(genes, reads=(p.bases[:int(p.offsets[n - 1])], p.offsets[:n]), paired=True, max_num_nodes=pc.MIXED_BUDGET)
    assert_outcomes(odd, cases.mixed_expected(orc, "odd"), "599 reads as pairs")
    unpaired = e.pcr_run(genes, reads="retained", paired=False, max_num_nodes=pc.MIXED_BUDGET)
    assert all(o.n_paired_links == 0 for o in unpaired)


def test_pairs_that_link_on_the_18s_reads(orc):
    """Ten identical reads that all map: five pairs by rule and by arrays, four of nine reads, none unpaired."""
    seq, bases, offsets, gene, keys, counts = cases.case_18s(orc)
    with sa.KmerEngine(21, 1, 100) as e:
        e.retain_reads(True)
        e.ingest_reads(bases, offsets)
        e.finalize()
        want = cases.expected_18s(orc, True, paired=True)
        assert want.n_paired_links == 5
        index, mate = np.arange(10, dtype=np.uint64), (1 + (np.arange(10) & 1)).astype(np.uint8)
        for what, got in (("rule, retained", e.pcr_run([gene], reads="retained", paired=True, max_num_nodes=500_000)),
                          ("rule, host", e.pcr_run([gene], reads=(bases, offsets), paired=True, max_num_nodes=500_000)),
                          ("arrays", e.pcr_run([gene], reads=(bases, offsets, index, mate), max_num_nodes=500_000))):
            assert_outcomes(got, [want], what)
        nine = e.pcr_run([gene], reads=(bases[:int(offsets[9])], offsets[:10]), paired=True, max_num_nodes=500_000)
        assert_outcomes(nine, [cases.expected_18s(orc, True, paired=True, n_reads=9)], "nine reads")
        assert nine[0].n_paired_links == 4
        assert e.pcr_run([gene], reads="retained", max_num_nodes=500_000)[0].n_paired_links == 0


def test_reads_that_match_nothing_thread_nothing(mixed, orc):
    e, p, genes = mixed
    other = np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.default_rng(977).integers(0, 4, 50 * 150)]
    ooff = np.arange(51, dtype=np.uint64) * np.uint64(150)
    table = set(p.keys.tolist())  # no k-mer of these reads is in the table, so none is a primer k-mer of any gene
    assert not any(ks & table for ks in ref.read_kmer_sets(ref.split_reads(other, ooff), p.k))
    got = e.pcr_run(genes, reads=(other, ooff), max_num_nodes=pc.MIXED_BUDGET)
    assert all(o.n_reads_matched == 0 and not o.threaded for o in got)
    bare = e.pcr_run(genes, max_num_nodes=pc.MIXED_BUDGET)
    same_outcomes(got, bare, "another genome's reads")
    empty = e.pcr_run(genes, reads=(np.zeros(0, np.uint8), np.zeros(1, np.uint64)), max_num_nodes=pc.MIXED_BUDGET)
    same_outcomes(empty, bare, "zero reads")


def test_18s_yields_the_amplicon(orc):
    seq, bases, offsets, gene, keys, counts = cases.case_18s(orc)
    with sa.KmerEngine(21, 1, 100) as e:
        e.ingest_reads(bases, offsets)
        e.finalize()
        got = e.pcr_run([gene], reads=(bases, offsets), max_num_nodes=500_000)
        assert_outcomes(got, [cases.expected_18s(orc, True)], "18S")
        assert_equals_chain(got, hand_chain(e, 21, [gene], (bases, offsets), max_num_nodes=500_000), "18S")
        (product,) = got[0].products.sequences
        assert product in seq and len(product) > 1700 and got[0].n_reads_matched == 10 and got[0].threaded
        bare = e.pcr_run([gene])  # the node budget of the bases ingested
        assert_outcomes(bare, [cases.expected_18s(orc, False)], "18S, no reads")
        clamped = e.pcr_run([sa.PcrGene("18s", gene.forward_seq, gene.reverse_seq, max_length=2500)], min_kmer_count=11)
        assert clamped[0].status == sa.PCR_NO_PRIMERS  # min_count 2 runs as 11: every k-mer has count 10


def test_error_order_and_no_launch_before_it(orc):
    p = pc.mixed_panel(orc)
    genes = cases.mixed_genes(orc)
    ok = genes[0]
    bad_char = sa.PcrGene("bad char", "ACGTACGTAXGTACGTACGTA", ok.reverse_seq)
    variants = sa.PcrGene("variants", "ACGTACGTA" + "N" * 15, ok.reverse_seq)
    with sa.KmerEngine(p.k, 1, 100, flags=sa.FLAG_TIMING) as e:
        e.ingest_reads(p.bases, p.offsets)
        e.finalize()
        e.reset_timings()
        for panel, code, texts in (([ok, bad_char, variants], -2, ("gene 1 'bad char'", "Invalid nucleotide(s) X in forward primer")),
                                   ([ok, variants, bad_char], -2, ("gene 1 'variants'", "variants")),
                                   ([ok, genes[1], sa.PcrGene(ok.gene_name, genes[1].forward_seq, genes[1].reverse_seq)], -2,
                                    (f"Duplicate gene name '{ok.gene_name}'",)),
                                   ([ok, sa.PcrGene("low", ok.forward_seq, ok.reverse_seq, min_count=1)], -2,
                                    ("gene 1 'low'", "min-count is 1, must be at least 2"))):
            with pytest.raises(sa.ShkError) as err:
                e.pcr_run(panel, max_num_nodes=pc.MIXED_BUDGET)
            assert err.value.code == code and all(t in err.value.msg for t in texts), err.value.msg
        want_variants = None
        try:
            ref.primer_ref.check_variant_limit(variants.forward_seq, 15, p.k)
        except ref.primer_ref.RefError as x:
            want_variants = str(x)
        with pytest.raises(sa.ShkError) as err:
            e.pcr_run([ok, variants])
        assert want_variants and want_variants in err.value.msg
        assert e.timings() == {}  # nothing was launched
        assert e.pcr_run([]) == []
        assert e.timings() == {}


def test_states_and_capacities(mixed, orc):
    e, p, genes = mixed
    with sa.KmerEngine(p.k, 1, 100) as plain:
        plain.ingest_reads(p.bases, p.offsets)
        plain.finalize()
        with pytest.raises(sa.ShkError) as err:
            plain.pcr_run(genes[:2], reads="retained")
        assert err.value.code == -11 and "reads are not retained" in err.value.msg
    with sa.KmerEngine(p.k, 1, 100, device_ids=[0, 0]) as multi:
        multi.ingest_reads(p.bases, p.offsets)
        multi.finalize()
        with pytest.raises(sa.ShkError) as err:
            multi.pcr_run(genes[:2])
        assert err.value.code == -11 and "multi-device context" in err.value.msg
    with sa.KmerEngine(p.k, 1, 100, n_owners=2, owner_id=1) as share:
        share.ingest_reads(p.bases, p.offsets)
        share.finalize()
        with pytest.raises(sa.ShkError) as err:
            share.pcr_run(genes[:2])
        assert err.value.code == -11 and "owner share" in err.value.msg
    want = cases.mixed_expected(orc, "none")
    with pytest.raises(sa.ShkError) as err:
        e.pcr_run(genes, max_num_nodes=pc.MIXED_BUDGET, record_cap=1)
    assert err.value.code == -2
    assert err.value.needs == (sum(len(w.products) for w in want), sum(len(r.sequence) for w in want for r in w.products))
    assert err.value.per_gene["status"].tolist() == [w.status for w in want]
    assert err.value.per_gene["n_nodes"].tolist() == [w.n_nodes for w in want]
    assert err.value.per_gene["n_pruned_edges"].tolist() == [w.n_pruned_edges for w in want]
    with pytest.raises(sa.ShkError) as err:
        e.pcr_run(genes, max_num_nodes=pc.MIXED_BUDGET, seq_cap=10)
    assert err.value.code == -2 and err.value.needs[1] > 10 and err.value.per_gene["status"].tolist() == [w.status for w in want]


def test_record_cap_one_short_on_the_plain_call(mixed, orc):
    """The plain call writes its records straight into the caller's arrays: one record of room too few is that call's own
    refusal, with the same needs as any short call and every per-gene figure of an unconstrained run."""
    # (this file's own mixed fixture, the same panel on one chunk: test_gpu_pcr_depths.py, whose fixture has four, imports
    # from this file, and no depth enters the plain call)
    e, p, genes = mixed
    free = e.pcr_run(genes, max_num_nodes=pc.MIXED_BUDGET)
    with pytest.raises(sa.ShkError) as first:
        e.pcr_run(genes, max_num_nodes=pc.MIXED_BUDGET, record_cap=1)
    need_records, need_bases = first.value.needs
    assert need_records == sum(len(o.products.sequences) for o in free) > 1
    with pytest.raises(sa.ShkError) as err:
        e.pcr_run(genes, max_num_nodes=pc.MIXED_BUDGET, record_cap=need_records - 1)
    assert err.value.code == -2
    assert f"{need_records} records of {need_bases} bases do not fit record_cap {need_records - 1}" in err.value.msg
    assert err.value.needs == first.value.needs
    for f in ("status", "n_nodes", "n_pruned_edges"):
        assert err.value.per_gene[f].tolist() == [getattr(o, f) for o in free], f
    same_outcomes(e.pcr_run(genes, max_num_nodes=pc.MIXED_BUDGET, record_cap=need_records, seq_cap=need_bases), free, "exactly what it needs")


# ---- the command line and run_files ---------------------------------------------------------------------------------------

def write_fastq(path, bases, offsets):
    with open(path, "w") as f:
        for i, s in enumerate(ref.split_reads(bases, offsets)):
            f.write(f"@r{i}\n{s.decode()}\n+\n{'I' * len(s)}\n")


COUNTING_KEYS = ("sharkmer_version", "sample", "kmer_length", "chunks", "n_reads_read", "n_bases_read", "n_subreads_ingested",
                 "n_bases_ingested", "n_kmers", "n_multi_kmers", "n_singleton_kmers")


def test_shk_count_writes_the_amplicon_and_pcr_results(tmp_path, orc):
    seq, bases, offsets, gene, keys, counts = cases.case_18s(orc)
    fq = tmp_path / "reads.fastq"
    write_fastq(fq, bases, offsets)
    spec = f"forward={cases.FWD_18S.lower()},reverse={cases.REV_18S},name=18s,max-length=2500,min-count=3"
    absent = sa.PcrGene("absent", pc.ABSENT, cases.REV_18S)
    (want_absent,) = ref.run_pcr(keys, counts, 21, [absent], ref.split_reads(bases, offsets))
    assert want_absent.status == ref.NO_FORWARD
    want = cases.expected_18s(orc, True)
    base = ["-k", "21", "--chunks", "2", "--histo-max", "50", "-s", "s"]
    for d in ("cli", "plain"):
        (tmp_path / d).mkdir()
    r = subprocess.run([EXE] + base + ["-o", str(tmp_path / "cli"), "--pcr-primers", spec, "--pcr-primers",
                                       f"forward={pc.ABSENT},reverse={cases.REV_18S},name=absent", "--read-threading", str(fq)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "cli" / "s_18s.fasta").read_text() == ref.fasta_text("s", "18s", want.products)
    assert max(len(x) for x in (tmp_path / "cli" / "s_18s.fasta").read_text().split("\n")[1:]) == 80
    assert not (tmp_path / "cli" / "s_absent.fasta").exists()
    doc = yaml.safe_load((tmp_path / "cli" / "s.stats.yaml").read_text())
    assert doc["pcr_results"] == [dict(gene_name="18s", status="success", n_products=1, product_lengths=[len(want.products[0].sequence)]),
                                  dict(gene_name="absent", status="fail", n_products=0, failure_reason="forward primer not found")]
    r = subprocess.run([EXE] + base + ["-o", str(tmp_path / "plain"), str(fq)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    plain = yaml.safe_load((tmp_path / "plain" / "s.stats.yaml").read_text())
    assert "pcr_results" not in plain and [doc[f] for f in COUNTING_KEYS] == [plain[f] for f in COUNTING_KEYS]
    assert (tmp_path / "cli" / "s.histo").read_bytes() == (tmp_path / "plain" / "s.histo").read_bytes()
    # run_files gives the same files
    (tmp_path / "py").mkdir()
    sa.run_files([str(fq)], k=21, chunks=2, histo_max=50, sample="s", outdir=str(tmp_path / "py"), read_threading=True,
                 pcr_primers=[spec, f"forward={pc.ABSENT},reverse={cases.REV_18S},name=absent"])
    assert (tmp_path / "py" / "s_18s.fasta").read_bytes() == (tmp_path / "cli" / "s_18s.fasta").read_bytes()
    assert yaml.safe_load((tmp_path / "py" / "s.stats.yaml").read_text())["pcr_results"] == doc["pcr_results"]
    assert not (tmp_path / "py" / "s_absent.fasta").exists()


def test_shk_count_refuses_bad_specifications(tmp_path):
    r = subprocess.run([EXE, "-k", "21", "-s", "s", "-o", str(tmp_path), "--pcr-primers", "forward=ACGT,colour=red", "nothing.fastq"],
                       capture_output=True, text=True)
    assert r.returncode != 0
    assert r.stderr.startswith('Error: Could not parse primer specification: "forward=ACGT,colour=red"\n\nCaused by:\n    Unexpected parameter: colour')
    r = subprocess.run([EXE, "-k", "21", "-s", "s", "-o", str(tmp_path), "--pcr-primers", "forward=ACGT,reverse=ACGT,name=x,min-count=1",
                        "nothing.fastq"], capture_output=True, text=True)
    assert r.returncode != 0 and r.stderr.startswith("Error: Primer validation failed (2 errors):\n\n  x (--pcr-primers):\n    - min-count is 1")
    r = subprocess.run([EXE, "-k", "21", "-s", "s", "-o", str(tmp_path), "--min-kmer-count", "0", "--pcr-primers",
                        "forward=ACGT,reverse=ACGA,name=x", "nothing.fastq"], capture_output=True, text=True)
    assert r.returncode != 0 and "min-kmer-count must be at least 1" in r.stderr
    assert not list(tmp_path.iterdir())
