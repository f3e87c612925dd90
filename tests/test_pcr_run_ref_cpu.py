"""CPU checks around shk_pcr_run: the model of do_pcr / run_pcr (tests/pcr_run_ref.py) on the cases the GPU test uses —
so that test cannot pass on a panel that exercises nothing — and the host helpers of the library (the primer
specification's parser, the validator, the FASTA and stats writers), which need no device.  No GPU.

The layout of pcr_results in the stats file is taken from reading serde_yaml_ng's emitter (block sequences with the dash
at the parent key's indentation, plain scalars where they read back as strings): no reference binary can be built here
(no Rust toolchain), so the expected bytes below are written by hand, not recorded."""
import numpy as np
import pytest
import yaml

import pcr_run_cases as cases
import pcr_run_ref as ref
import sharkmer_amd as sa


# ---- the model on the shared cases ------------------------------------------------------------------------------------

def test_mixed_panel_yields_every_status(orc):
    genes = cases.mixed_genes(orc)
    out = cases.mixed_expected(orc, "none")
    by = {g.gene_name: o for g, o in zip(genes, out)}
    assert all(sa.validate_pcr_gene(g) == [] for g in genes) and len({g.gene_name for g in genes}) == len(genes)
    assert {o.status for o in out} == {ref.SUCCESS, ref.NO_FORWARD, ref.NO_PRIMERS, ref.NO_PATH, ref.NODE_BUDGET}
    assert by["no forward set"].status == ref.NO_FORWARD and by["no set at all"].status == ref.NO_PRIMERS
    assert by["budget"].status == ref.NODE_BUDGET and not by["budget"].found_path
    assert [by[n].steps_run for n in ("first threshold", "second step", "third step")] == [1, 2, 3]
    assert all(by[n].status == ref.SUCCESS and by[n].products for n in ("first threshold", "second step", "third step", "twin a", "twin b"))
    # a found path that yields nothing: NO_PATH after found_path (mod.rs:723-744 leaves the reason of mod.rs:567)
    long_ = by["too long"]
    assert long_.found_path and long_.status == ref.NO_PATH and long_.reason == "no path found" and not long_.products
    assert long_.n_pruned_nodes > 100 and by["first threshold"].products[0].sequence and len(by["first threshold"].products[0].sequence) > 100
    assert all(o.reason == ref.REASONS[o.status] for o in out)
    assert all(not o.threaded and o.n_reads_matched == 0 for o in out)


def test_mixed_panel_with_reads_threads_the_found_genes(orc):
    out = cases.mixed_expected(orc, "reads")
    bare = cases.mixed_expected(orc, "none")
    assert [o.status for o in out] == [o.status for o in bare]
    assert any(o.threaded for o in out) and any(o.found_path and o.threaded for o in out)
    assert all(o.threaded == (o.found_path and o.n_reads_matched > 0) for o in out)
    assert all(o.n_paired_links == 0 for o in out)
    paired = cases.mixed_expected(orc, "paired")  # (random reads: two neighbours seldom both reach a gene's graph)
    assert [o.n_reads_matched for o in paired] == [o.n_reads_matched for o in out]
    # pairs that do link: the ten identical 18S reads as five pairs, nine of them as four pairs and a single R1
    assert cases.expected_18s(orc, True, paired=True).n_paired_links == 5
    assert cases.expected_18s(orc, True, paired=True, n_reads=9).n_paired_links == 4
    assert cases.expected_18s(orc, True).n_paired_links == 0


def test_18s_model_yields_the_amplicon(orc):
    seq = cases.case_18s(orc)[0]
    for with_reads in (False, True):
        o = cases.expected_18s(orc, with_reads)
        assert o.status == ref.SUCCESS and len(o.products) == 1 and o.threaded == with_reads
        assert o.products[0].sequence in seq and len(o.products[0].sequence) > 1700
    assert cases.expected_18s(orc, True).n_reads_matched == 10


def test_min_count_is_clamped_to_min_kmer_count(orc):
    """collect_pcr_params (cli.rs:556-570): min-count 2 under --min-kmer-count 4 runs as 4 — the primer scan's and the
    sweep's lowest threshold."""
    seq, bases, offsets, gene, keys, counts = cases.case_18s(orc)
    g2 = sa.PcrGene("18s", gene.forward_seq, gene.reverse_seq, max_length=2500, min_count=2)
    g4 = sa.PcrGene("18s", gene.forward_seq, gene.reverse_seq, max_length=2500, min_count=4)
    (a,) = ref.run_pcr(keys, counts, 21, [g2], min_kmer_count=4, max_num_nodes=500_000)
    (b,) = ref.run_pcr(keys, counts, 21, [g4], min_kmer_count=4, max_num_nodes=500_000)
    assert (a.status, a.threshold_used, a.steps_run, a.n_nodes) == (b.status, b.threshold_used, b.steps_run, b.n_nodes)
    (hi,) = ref.run_pcr(keys, counts, 21, [g2], min_kmer_count=11, max_num_nodes=500_000)  # every k-mer has count 10
    assert hi.status == ref.NO_PRIMERS


# ---- the parser (cli.rs:12-140) ---------------------------------------------------------------------------------------

def test_parser_takes_every_key_and_the_defaults():
    g = sa.parse_pcr_primers("forward=grctgtttaccaaaaacata,reverse=AATTCAACATMGAGG,name=16s")
    assert g == sa.PcrGene("16s", "GRCTGTTTACCAAAAACATA", "AATTCAACATMGAGG")
    assert (g.min_length, g.max_length, g.min_count, g.mismatches, g.trim, g.dedup_edit_threshold) == (0, 10000, 2, 2, 15, 10)
    assert (g.max_dfs_states, g.max_paths_per_pair, g.max_node_visits, g.max_primer_kmers) == (100000, 20, 2, 40)
    assert (g.high_coverage_ratio, g.tip_coverage_fraction) == (10.0, 0.1)
    g = sa.parse_pcr_primers("NAME=x,Forward=ac,REVERSE=gt,max-length=700,min-length=500,min-count=3,mismatches=1,trim=12,"
                             "dedup-edit-threshold=4,citation=doi:10.1/x?a=b,notes=a=b=c")
    assert g == sa.PcrGene("x", "AC", "GT", 500, 700, 3, 1, 12, 4)
    assert sa.parse_pcr_primers("name=a=b,forward=AC,reverse=GT").gene_name == "a=b"  # split_once: '=' stays in the value
    assert sa.parse_pcr_primers("name=,forward=,reverse=") == sa.PcrGene()


@pytest.mark.parametrize("spec, text", [
    ("", "Invalid empty primer specification"),
    ("forward=AC,reverse", "Invalid parameter (should be key=value): 'reverse'\nCommas are not allowed in field values. "
                           "Use --pcr-panel-file with a YAML panel for complex metadata."),
    ("forward=AC,,name=x", "Invalid parameter (should be key=value): ''\nCommas are not allowed in field values. "
                           "Use --pcr-panel-file with a YAML panel for complex metadata."),
    ("name=x,Name=y", "Duplicate parameter 'name' in primer specification 'name=x,Name=y'. Each key may appear at most once."),
    ("name=x,colour=red", "Unexpected parameter: colour"),
    ("name=x,max-length=7k", "Invalid value for max-length: 7k"),
    ("name=x,min-count=-1", "Invalid value for min-count: -1"),
    ("name=x,trim=", "Invalid value for trim: "),
    ("name=x,mismatches=4294967296", "Invalid value for mismatches: 4294967296"),
    ("name=x,min-length= 5", "Invalid value for min-length:  5"),
])
def test_parser_errors_carry_the_reference_texts(spec, text):
    with pytest.raises(sa.ShkError) as e:
        sa.parse_pcr_primers(spec)
    assert e.value.code == -2 and e.value.msg == text


# ---- the validator (mod.rs:295-399, cli.rs:528-554) -------------------------------------------------------------------

OK = dict(gene_name="g", forward_seq="ACGTAC", reverse_seq="TTGCA")


@pytest.mark.parametrize("change, error, suggestion", [
    (dict(forward_seq="A"), "Forward primer sequence is too short: 'A'", "Primer sequences must be at least 2 bases"),
    (dict(reverse_seq=""), "Reverse primer sequence is too short: ''", "Primer sequences must be at least 2 bases"),
    (dict(forward_seq="ACXGTZ"), "Invalid nucleotide(s) X, Z in forward primer ACXGTZ", "Valid characters: A C G T R Y W S M K B D H V N"),
    (dict(reverse_seq="acGT"), "Invalid nucleotide(s) a, c in reverse primer acGT", "Valid characters: A C G T R Y W S M K B D H V N"),
    (dict(min_length=11, max_length=10), "min-length (11) is greater than max-length (10)", "Swap the values or adjust the range"),
    (dict(min_count=1), "min-count is 1, must be at least 2", "Set min-count to at least 2"),
    (dict(max_length=0), "max-length is 0", "Set max-length to a positive value"),
    (dict(gene_name=""), "Gene name is empty", "Provide a unique name for the primer pair via the 'name' field"),
    (dict(reverse_seq="ACGTAC"), "Forward and reverse primers are identical: ACGTAC", "Check that forward and reverse sequences are not swapped"),
])
def test_validator_reports_each_check(change, error, suggestion):
    assert sa.validate_pcr_gene(sa.PcrGene(**OK)) == []
    assert sa.validate_pcr_gene(sa.PcrGene(**dict(OK, **change))) == [(error, suggestion)]


def test_validator_keeps_the_reference_order_and_the_report_text():
    bad = sa.PcrGene("", "A", "A", min_length=5, max_length=0, min_count=0)
    assert [e for e, _ in sa.validate_pcr_gene(bad)] == [
        "Forward primer sequence is too short: 'A'", "Reverse primer sequence is too short: 'A'",
        "min-length (5) is greater than max-length (0)", "min-count is 0, must be at least 2", "max-length is 0", "Gene name is empty"]
    assert sa.pcr_validation_report([sa.PcrGene(**OK)]) == ""
    one = sa.pcr_validation_report([sa.PcrGene(**OK), sa.PcrGene(**dict(OK, gene_name="b", min_count=1))])
    assert one == ("Primer validation failed (1 error):\n\n  b (--pcr-primers):\n    - min-count is 1, must be at least 2\n"
                   "      Suggestion: Set min-count to at least 2\n")
    two = sa.pcr_validation_report([sa.PcrGene(**dict(OK, max_length=0)), sa.PcrGene(**OK), sa.PcrGene(**dict(OK, gene_name="c", forward_seq="AX"))],
                                   sources=["panel file 'p.yaml'", None, None])
    assert two == ("Primer validation failed (2 errors):\n\n  g (panel file 'p.yaml'):\n    - max-length is 0\n"
                   "      Suggestion: Set max-length to a positive value\n\n  c (--pcr-primers):\n"
                   "    - Invalid nucleotide(s) X in forward primer AX\n      Suggestion: Valid characters: A C G T R Y W S M K B D H V N\n")


def test_failure_reasons():
    assert [sa.pcr_failure_reason(s) for s in range(7)] == [ref.REASONS[s] for s in range(6)] + [None]


# ---- the writers ------------------------------------------------------------------------------------------------------

STATS = dict(command="shk_count -k 21 -s x", sample="x", kmer_length=21, chunks=2, n_reads_read=10, n_bases_read=1500,
             n_subreads_ingested=10, n_bases_ingested=1490, n_kmers=1300, n_multi_kmers=900, n_singleton_kmers=400, peak_memory_bytes=7)


def test_stats_yaml_without_genes_is_todays_file(tmp_path):
    sa.write_stats_yaml(str(tmp_path / "a.yaml"), **STATS)
    sa.write_stats_yaml(str(tmp_path / "b.yaml"), pcr_results=[], **STATS)
    assert (tmp_path / "a.yaml").read_bytes() == (tmp_path / "b.yaml").read_bytes()
    assert "pcr_results" not in yaml.safe_load((tmp_path / "b.yaml").read_text())


def test_stats_yaml_with_pcr_results(tmp_path):
    results = [("18s", sa.PCR_SUCCESS, [1780, 1779]), ("co1", sa.PCR_NO_FORWARD, []), ("16s: v2", sa.PCR_NODE_BUDGET, []), ("123", sa.PCR_NO_PATH, [])]
    sa.write_stats_yaml(str(tmp_path / "s.yaml"), pcr_results=results, **STATS)
    text = (tmp_path / "s.yaml").read_text()
    sa.write_stats_yaml(str(tmp_path / "a.yaml"), **STATS)
    head = (tmp_path / "a.yaml").read_text()
    assert text == head + ("pcr_results:\n"
                           "- gene_name: 18s\n  status: success\n  n_products: 2\n  product_lengths:\n  - 1780\n  - 1779\n"
                           "- gene_name: co1\n  status: fail\n  n_products: 0\n  failure_reason: forward primer not found\n"
                           "- gene_name: '16s: v2'\n  status: fail\n  n_products: 0\n  failure_reason: node budget exceeded\n"
                           "- gene_name: '123'\n  status: fail\n  n_products: 0\n  failure_reason: no path found\n")
    doc = yaml.safe_load(text)
    assert doc["n_kmers"] == 1300 and doc["pcr_results"] == [
        dict(gene_name="18s", status="success", n_products=2, product_lengths=[1780, 1779]),
        dict(gene_name="co1", status="fail", n_products=0, failure_reason="forward primer not found"),
        dict(gene_name="16s: v2", status="fail", n_products=0, failure_reason="node budget exceeded"),
        dict(gene_name="123", status="fail", n_products=0, failure_reason="no path found")]


def products_of(seqs):
    n = len(seqs)
    return sa.PcrProducts(list(seqs), np.zeros(n, np.uint32), np.zeros(n, np.uint64), np.array([12.345 + i for i in range(n)]),
                          np.array([12.0 if i % 2 == 0 else 12.5 for i in range(n)]), np.arange(n, dtype=np.uint64) + 3,
                          np.arange(n, dtype=np.uint64) + 30, np.array([0.125 * (i + 1) for i in range(n)]),
                          np.full((n, 6), np.nan), 0, n, 0)


def test_fasta_writer_wraps_at_80_columns(tmp_path):
    """write_fasta_record (io.rs:144-158): seq.chunks(80), a line feed after each; the headers are PcrProducts.fasta's."""
    seqs = [("ACGT" * 50)[:n] for n in (79, 80, 81, 160, 161)]
    p = products_of(seqs)
    sa.write_fasta(str(tmp_path / "x.fasta"), "s1", "18s", p)
    got = (tmp_path / "x.fasta").read_text()
    flat = p.fasta("s1", "18s").split("\n")  # header, sequence, header, sequence, …
    want = []
    for i, s in enumerate(seqs):
        want.append(flat[2 * i])
        want += [s[a:a + 80] for a in range(0, len(s), 80)]
    assert got == "\n".join(want) + "\n"
    lines = got.split("\n")
    assert lines[0] == ">s1_18s_0 sample=s1 gene=18s product=0 length=79 kmer_count_mean=12.35 kmer_count_median=12 kmer_count_min=3 kmer_count_max=30 score=0.12"
    assert "kmer_count_median=12.5 " in lines[2] and " product=1 length=80 " in lines[2]
    assert [len(x) for x in lines if x and not x.startswith(">")] == [79, 80, 80, 1, 80, 80, 80, 80, 1]
    sa.write_fasta(str(tmp_path / "e.fasta"), "s1", "18s", products_of([]))
    assert (tmp_path / "e.fasta").read_bytes() == b""
