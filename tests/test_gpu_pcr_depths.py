"""GPU tests of the sPCR depth sweep: shk_chunk_bases, shk_lookup_depth, shk_primer_kmers_depths
(k_primer_scan_depths), shk_neighborhood_panel_depths / shk_pcr_extend_panel_depths (the lane-bounded probe) and
shk_pcr_run_depths.  Every depth result is compared with the models over the oracle's table of the reads below the depth
(depth_cases) AND with today's call on a second context that was fed only those reads, under the same chunk ids."""
import numpy as np
import pytest

import depth_cases as dc
import nb_cases
import pcr_panel_cases as pc
import pcr_ref
import pcr_run_cases as cases
import primer_ref
import sharkmer_amd as sa
from test_gpu_pcr_run import assert_outcomes, same_outcomes

pytestmark = pytest.mark.gpu

BAD_ARG, STATE = -2, -11


def engine_below(k, bases, offsets, n_chunks, depth, **kw):
    e = sa.KmerEngine(k, n_chunks, 100, **kw)
    dc.ingest_below(e, bases, offsets, n_chunks, depth)
    return e


@pytest.fixture(scope="module")
def mixed(orc):
    """(panel, genes, the context with all 4 chunks, [the context that got only the chunks < d for d = 1..4])."""
    p = pc.mixed_panel(orc)
    full = engine_below(p.k, p.bases, p.offsets, dc.CHUNKS_MIXED, dc.CHUNKS_MIXED, flags=sa.FLAG_TIMING)
    subs = [engine_below(p.k, p.bases, p.offsets, dc.CHUNKS_MIXED, d) for d in range(1, dc.CHUNKS_MIXED + 1)]
    yield p, cases.mixed_genes(orc), full, subs
    for e in [full] + subs:
        e.close()


def mixed_primers(genes, min_count=2):
    return [sa.Primer(s, g.trim, g.mismatches, max(g.min_count, min_count), g.max_primer_kmers) for g in genes
            for s in (g.forward_seq, g.reverse_seq)]


def same_primer_results(a, b, what):
    assert len(a) == len(b), what
    for i, (x, y) in enumerate(zip(a, b)):
        for f, (u, v) in enumerate(zip(x, y)):
            assert np.array_equal(u, v), (what, "primer", i, "field", f)


# ---- 1. lookup at a depth --------------------------------------------------------------------------------------------------

def test_lookup_depth_against_the_oracle_of_the_subset(mixed, orc):
    p, genes, full, subs = mixed
    probe = np.concatenate([p.keys, np.array([0, 1, (1 << 42) - 1], dtype=np.uint64)])
    assert full.counters()["n_chunks"] == dc.CHUNKS_MIXED
    for d in range(1, dc.CHUNKS_MIXED + 1):
        table = dc.mixed_table(orc, d)
        want = np.array([table.get(int(x), 0) for x in probe], dtype=np.uint32)
        got = full.lookup(probe, depth=d)
        assert np.array_equal(got, want), d
        assert np.array_equal(got, subs[d - 1].lookup(probe)), d
        assert np.array_equal(full.lookup(probe, canonical=True, depth=d), subs[d - 1].lookup(probe, canonical=True)), d
    assert (full.lookup(p.keys, depth=1) == 0).sum() > 100  # keys that only deeper chunks hold: not in the depth-1 table
    assert np.array_equal(full.lookup(probe, depth=dc.CHUNKS_MIXED), full.lookup(probe))
    assert np.array_equal(full.chunk_bases(), np.array(dc.chunk_bases(orc, p.bases, p.offsets, p.k, dc.CHUNKS_MIXED), dtype=np.uint64))
    assert int(full.chunk_bases().sum()) == full.counters()["n_bases_ingested"]


def test_lookup_depth_saturates_in_lane_order_and_one_chunk():
    key = nb_cases.canonical(0b0110110001, 5)
    with sa.KmerEngine(5, 3, 10) as e:
        for lane, c in enumerate((0xFFFFFFFE, 5, 7)):
            e.insert([key], [c], chunk_id=lane)
        assert [int(e.lookup([key], depth=d)[0]) for d in (1, 2, 3)] == [0xFFFFFFFE, 0xFFFFFFFF, 0xFFFFFFFF]
        assert int(e.lookup([key])[0]) == 0xFFFFFFFF
    with sa.KmerEngine(5, 1, 10) as e:
        e.insert([key], [9])
        assert int(e.lookup([key], depth=1)[0]) == 9 and int(e.lookup([key ^ 1], depth=1)[0]) == 0
        (block,) = e.primer_kmers_depths([sa.Primer("ACGTA", 4, 0, 1, 10)], [1])
        same_primer_results(block, e.primer_kmers([sa.Primer("ACGTA", 4, 0, 1, 10)]), "one chunk")


# ---- 2. the fused primer scan ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("depths", [[1, 2, 3, 4], [1, 3]])
def test_primer_kmers_depths_equal_the_subset_contexts(mixed, orc, depths):
    p, genes, full, subs = mixed
    primers = mixed_primers(genes)
    got = full.primer_kmers_depths(primers, depths)
    assert len(got) == len(depths)
    for block, d in zip(got, depths):
        same_primer_results(block, subs[d - 1].primer_kmers(primers), f"depth {d}")
        keys, counts = dc.depth_table(orc, p.bases, p.offsets, p.k, dc.CHUNKS_MIXED, d)
        for i in (0, 1, 4):  # and the model, for a few of them
            pr = primers[i]
            wk, wc, wl = primer_ref.get_primer_kmers(pr.seq, keys, counts, p.k, pr.trim, pr.mismatches, pr.min_count, pr.max_kmers, False)[:3]
            assert [list(block[i][0]), list(block[i][1]), list(block[i][2])] == [list(wk), list(wc), list(wl)], (d, i)
    if depths[-1] == dc.CHUNKS_MIXED:
        same_primer_results(got[-1], full.primer_kmers(primers), "the last depth is the merged table")
    assert any(len(a[0]) != len(b[0]) for a, b in zip(got[0], got[-1]))  # the answer moves with the depth


def test_primer_min_count_zero_reports_nothing_of_later_chunks(mixed):
    p, genes, full, subs = mixed
    primers = [sa.Primer(pr.seq, pr.trim, pr.mismatches, 0, 4000) for pr in mixed_primers(genes)[:6]]
    got = full.primer_kmers_depths(primers, [1, 2, 4])
    for block, d in zip(got, (1, 2, 4)):
        same_primer_results(block, subs[d - 1].primer_kmers(primers), f"min_count 0, depth {d}")
        for kmers, counts, _, _ in block:
            assert (counts > 0).all()
            canon = [min(int(x), pcr_ref.revcomp(int(x), p.k)) for x in kmers]
            assert (subs[d - 1].lookup(canon) > 0).all()


def test_primer_candidates_overflow_reruns_with_a_cut_per_depth(mixed, monkeypatch):
    p, genes, full, subs = mixed
    primers = mixed_primers(genes)
    depths = [1, 2, 3, 4]
    want = full.primer_kmers_depths(primers, depths)
    full.reset_timings()
    full.primer_kmers_depths(primers, depths)
    once = full.timings()["lookup"][1]
    full.reset_timings()
    full.primer_kmers_depths(primers, [3])
    assert full.timings()["lookup"][1] == once  # D depths launch the scan as often as one depth
    monkeypatch.setenv("SHK_PRIMER_CANDIDATES", "16")
    full.reset_timings()
    got = full.primer_kmers_depths(primers, depths)
    assert full.timings()["lookup"][1] == 2 * once  # the rerun
    for a, b, d in zip(got, want, depths):
        same_primer_results(a, b, f"rerun, depth {d}")


# ---- 3. neighbourhoods at a depth -----------------------------------------------------------------------------------------

def test_neighborhood_panel_depths_wide_and_narrow():
    """pcr_panel_cases.wide_narrow_panel's chains dealt over 3 lanes (insert i → lane i % 3): a job at depth d sees the
    inserts of the lanes below d only; flat1025's level takes k_nb_wide with the bound."""
    p = pc.wide_narrow_panel()
    lanes = 3
    dealt = [(i % lanes, keys, counts) for i, (_, keys, counts) in enumerate(p.inserts)]
    depths = [(j % lanes) + 1 for j in range(len(p.jobs))]
    depths[2] = lanes  # flat1025 whole: its 1025-entry level is there
    jobs = [(n, d, mc, 1 << 14, 1 << 12) for n, d, mc in p.jobs]
    with sa.KmerEngine(p.k, lanes, 10) as eng:
        for lane, keys, counts in dealt:
            eng.insert(keys, counts, chunk_id=lane)
        got = eng.neighborhood_panel(jobs, depths=depths)
        whole = eng.neighborhood_panel(jobs)
        same = eng.neighborhood_panel(jobs, depths=[lanes] * len(jobs))
    for j, (a, b) in enumerate(zip(whole, same)):
        assert all(np.array_equal(x, y) for x, y in zip(a[:4], b[:4])) and a[4] == b[4], j
    assert max(len(g[0]) for g in got) > 1024
    for d in range(1, lanes + 1):
        below = [ins for ins in dealt if ins[0] < d]
        table = nb_cases.merged_table(below)
        with sa.KmerEngine(p.k, lanes, 10) as sub:
            for lane, keys, counts in below:
                sub.insert(keys, counts, chunk_id=lane)
            mine = [j for j in range(len(jobs)) if depths[j] == d]
            alone = sub.neighborhood_panel([jobs[j] for j in mine])
        for j, a in zip(mine, alone):
            g = got[j]
            assert all(np.array_equal(x, y) for x, y in zip(g[:4], a[:4])) and g[4] == a[4], (d, j)
            want = pcr_ref.neighborhood(jobs[j][0], jobs[j][1], table, p.k, jobs[j][2], cap=jobs[j][3], fringe_cap=jobs[j][4])
            assert [list(g[0]), list(g[1]), list(g[2]), list(g[3]), g[4]] == list(want), (d, j)
    assert any(len(got[j][0]) != len(whole[j][0]) for j in range(len(jobs)))


# ---- 4. the extension and the whole run -------------------------------------------------------------------------------------

def same_graphs(a, b, what):
    for f in ("node_sub_kmers", "node_flags", "edge_src", "edge_tgt", "edge_counts"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), (what, f)
    assert (a.found_path, a.threshold_used, a.steps_run) == (b.found_path, b.threshold_used, b.steps_run), what


def test_pcr_extend_panel_depths(mixed):
    p, genes, full, subs = mixed
    primers = mixed_primers(genes)
    depths = [1, 2, 3, 4]
    prim = full.primer_kmers_depths(primers, depths)
    sets, gene_depths, params = [], [], []
    for block, d in zip(prim, depths):
        for g in range(len(genes)):
            if len(block[2 * g][0]) and len(block[2 * g + 1][0]):
                sets += [block[2 * g], block[2 * g + 1]]
                gene_depths.append(d)
                params.append(dict(min_count=2, table_min_count=2, high_coverage_ratio=genes[g].high_coverage_ratio, max_num_nodes=pc.MIXED_BUDGET))
    assert len(set(gene_depths)) == 4
    got = full.pcr_extend_panel(sets, params, depths=gene_depths)
    for d in depths:
        mine = [i for i, x in enumerate(gene_depths) if x == d]
        alone = subs[d - 1].pcr_extend_panel([sets[2 * i + s] for i in mine for s in (0, 1)], [params[i] for i in mine])
        for i, a in zip(mine, alone):
            same_graphs(got[i], a, (d, i))


def test_pcr_run_depths_mixed_panel(mixed, orc):
    p, genes, full, subs = mixed
    depths = [1, 2, 3, 4]
    got = full.pcr_run_depths(genes, depths, max_num_nodes=pc.MIXED_BUDGET)
    assert len(got) == 4
    for block, d in zip(got, depths):
        assert_outcomes(block, dc.mixed_expected(orc, d), f"depth {d}")
        same_outcomes(block, subs[d - 1].pcr_run(genes, max_num_nodes=pc.MIXED_BUDGET), f"depth {d} and the subset context")
    same_outcomes(got[-1], full.pcr_run(genes, max_num_nodes=pc.MIXED_BUDGET), "the last depth and shk_pcr_run")
    assert [o.status for o in got[0]] != [o.status for o in got[2]]
    (gapped,) = full.pcr_run_depths(genes, [3], max_num_nodes=pc.MIXED_BUDGET)
    same_outcomes(gapped, got[2], "one depth alone")
    # max_num_nodes 0: the budget of the bases below the depth, per depth
    bases = full.chunk_bases()
    auto = full.pcr_run_depths(genes[:3], [2, 4])
    for block, d in zip(auto, (2, 4)):
        budget = sa.pcr_node_budget(int(bases[:d].sum()))
        (explicit,) = full.pcr_run_depths(genes[:3], [d], max_num_nodes=budget)
        same_outcomes(block, explicit, f"budget of depth {d}")
        same_outcomes(block, subs[d - 1].pcr_run(genes[:3]), f"budget of depth {d}, subset context")


def test_pcr_run_depths_record_capacities(mixed, orc):
    p, genes, full, subs = mixed
    depths = [1, 2, 3, 4]
    want = [dc.mixed_expected(orc, d) for d in depths]
    with pytest.raises(sa.ShkError) as err:
        full.pcr_run_depths(genes, depths, max_num_nodes=pc.MIXED_BUDGET, record_cap=1)
    assert err.value.code == BAD_ARG
    assert err.value.needs == [(sum(len(w.products) for w in ws), sum(len(r.sequence) for w in ws for r in w.products)) for ws in want]
    for j, ws in enumerate(want):
        assert err.value.per_gene[j]["status"].tolist() == [w.status for w in ws], j
        assert err.value.per_gene[j]["n_nodes"].tolist() == [w.n_nodes for w in ws], j
        assert err.value.per_gene[j]["n_pruned_edges"].tolist() == [w.n_pruned_edges for w in ws], j
    assert max(n for n, _ in err.value.needs) > 1 and err.value.needs[0] == (0, 0)
    needs = err.value.needs
    retry = full.pcr_run_depths(genes, depths, max_num_nodes=pc.MIXED_BUDGET, record_cap=max(n for n, _ in needs),
                                seq_cap=max(b for _, b in needs))
    for block, ws, d in zip(retry, want, depths):
        assert_outcomes(block, ws, f"retry, depth {d}")


# Launches per timing slot of one call over the mixed panel on the 4-chunk context, read from commit 38af4a5 ("sPCR depth
# sweep: a panel at every cumulative chunk from one count"), where the plain call and the sweep were two pipelines: the
# one pipeline launches what each of them launched.  Counts, not times: equal or wrong.
LAUNCHES_PCR_RUN = {"lookup": 1, "extend": 11}
LAUNCHES_PCR_RUN_DEPTHS_4 = {"lookup": 1, "extend": 11}


def launches(e, call):
    e.reset_timings()
    call()
    return {slot: n for slot, (_, n) in e.timings().items()}


def test_launches_per_timing_slot(mixed):
    p, genes, full, subs = mixed
    plain = launches(full, lambda: full.pcr_run(genes))
    sweep = launches(full, lambda: full.pcr_run_depths(genes, [4]))
    print("launches pcr_run:", plain)
    print("launches pcr_run_depths [4]:", sweep)
    assert plain == LAUNCHES_PCR_RUN
    assert sweep == LAUNCHES_PCR_RUN_DEPTHS_4


def test_pcr_run_depths_18s(orc):
    seq, bases, offsets, gene, _, _ = cases.case_18s(orc)
    n = dc.CHUNKS_18S
    with engine_below(21, bases, offsets, n, n) as e:
        assert np.array_equal(e.chunk_bases(), np.array(dc.chunk_bases(orc, bases, offsets, 21, n), dtype=np.uint64))
        got = e.pcr_run_depths([gene], list(range(1, n + 1)), max_num_nodes=500_000)
        for d, (o,) in enumerate(got, start=1):
            assert_outcomes([o], [dc.expected_18s(orc, d)], f"18S, depth {d}")
            with engine_below(21, bases, offsets, n, d) as sub:
                same_outcomes([o], sub.pcr_run([gene], max_num_nodes=500_000), f"18S, depth {d}, subset context")
        assert got[0][0].status == sa.PCR_NO_PRIMERS
        assert all(o.status == sa.PCR_SUCCESS and len(o.products.sequences) == 1 and o.products.sequences[0] in seq for (o,) in got[1:])
        same_outcomes([got[-1][0]], e.pcr_run([gene], max_num_nodes=500_000), "18S, the last depth")


# ---- 5. errors, all before the device is touched ------------------------------------------------------------------------------

def refused(call, code, text=None):
    with pytest.raises(sa.ShkError) as err:
        call()
    assert err.value.code == code, err.value.msg
    if text:
        assert text in err.value.msg, err.value.msg


def test_errors_launch_nothing(mixed):
    p, genes, full, subs = mixed
    primers = mixed_primers(genes)[:2]
    job = [([1, 2], [1, 2], 2, 64, 64)]
    prim = full.primer_kmers(primers)
    full.reset_timings()
    for bad in ([], list(range(1, 18)), [0, 1], [2, 5], [2, 2], [3, 2]):
        refused(lambda: full.primer_kmers_depths(primers, bad), BAD_ARG)
        refused(lambda: full.pcr_run_depths(genes[:1], bad), BAD_ARG)
    for d in (0, 5):
        refused(lambda: full.lookup([1], depth=d), BAD_ARG, "depth")
        refused(lambda: full.neighborhood_panel(job, depths=[d]), BAD_ARG, "depth")
        refused(lambda: full.pcr_extend_panel(prim, depths=[d]), BAD_ARG, "depth")
    refused(lambda: full.pcr_run_depths([sa.PcrGene(f"g{i}", genes[0].forward_seq, genes[0].reverse_seq) for i in range(1025)], [1, 2, 3, 4]),
            BAD_ARG, "SHK_PCR_MAX_GENES")
    prm_reads = full._L.shk_pcr_run_depths  # (the Python mirror offers no reads: the C entry point with reads = RETAINED)
    import ctypes as C
    from sharkmer_amd.engine import _PcrRunOut, _PcrRunParams, _pcr_genes
    arr = _pcr_genes(genes[:1])
    status, roff = np.zeros(1, np.uint32), np.zeros(2, np.uint64)
    out = (_PcrRunOut * 1)()
    out[0].status, out[0].records.record_offsets = status.ctypes.data, roff.ctypes.data
    dep = np.array([1], dtype=np.uint32)
    prm = _PcrRunParams(2, 1, 0, 0, 0, None, None, 0, None, None)
    assert prm_reads(full._h, arr, 1, C.byref(prm), dep.ctypes.data, 1, out) == BAD_ARG
    assert "a depth sweep takes no reads" in full._L.shk_last_error(full._h).decode()
    dup = [genes[0], sa.PcrGene(genes[0].gene_name, genes[1].forward_seq, genes[1].reverse_seq)]
    refused(lambda: full.pcr_run_depths(dup, [1, 2]), BAD_ARG, "Duplicate gene name")
    assert full.timings() == {}  # nothing was launched
    assert full.pcr_run_depths([], [1, 2]) == [[], []]
    assert full.timings() == {}


def test_states(orc):
    p = pc.mixed_panel(orc)
    genes = cases.mixed_genes(orc)[:2]
    primers = mixed_primers(genes)
    job = [([1, 2], [1, 2], 2, 64, 64)]

    def all_refuse(e, text):
        e.reset_timings()
        refused(lambda: e.lookup([1], depth=1), STATE, text)
        refused(lambda: e.primer_kmers_depths(primers, [1]), STATE, text)
        refused(lambda: e.neighborhood_panel(job, depths=[1]), STATE, text)
        refused(lambda: e.pcr_extend_panel([(np.zeros(0, np.uint64), np.zeros(0, np.uint32))] * 2, dict(max_num_nodes=100), depths=[1]), STATE, text)
        refused(lambda: e.pcr_run_depths(genes, [1]), STATE, text)
        assert e.timings() == {}

    for flags in (0, sa.FLAG_GROUP_GRAPH):
        with sa.KmerEngine(p.k, 2, 100, flags=flags | sa.FLAG_TIMING, device_ids=[0, 0]) as multi:
            multi.ingest_reads(p.bases, p.offsets)
            multi.finalize()
            all_refuse(multi, "multi-device context")
    with sa.KmerEngine(p.k, 2, 100, flags=sa.FLAG_TIMING, n_owners=2, owner_id=1) as share:
        share.ingest_reads(p.bases, p.offsets)
        share.finalize()
        all_refuse(share, "owner share")


def test_between_scatter_begin_and_end():
    import torch
    bases, offsets = sa.synth_reads(sa.SynthSpec(genome_len=5_000), 0, 200)
    with sa.KmerEngine(21, 1, 100, n_owners=1, owner_id=0) as e:
        d_b = torch.from_numpy(bases.copy()).cuda()
        d_o = torch.from_numpy(offsets.astype(np.int64)).cuda()
        torch.cuda.synchronize()
        rec, cur, lay = e.xchg_scatter_begin_tensors(d_b.data_ptr(), d_o.data_ptr(), 200, len(bases))
        text = "an exchange scatter is begun and not ended"
        refused(lambda: e.lookup([1], depth=1), STATE, text)
        refused(lambda: e.primer_kmers_depths([sa.Primer("ACGTACGTACGTACGTACGTA")], [1]), STATE, text)
        refused(lambda: e.neighborhood_panel([([1], [1], 2, 64, 64)], depths=[1]), STATE, text)
        refused(lambda: e.pcr_run_depths([sa.PcrGene("g", "ACGTACGTACGTACGTACGTA", "ACGTACGTACGTACGTACGTT")], [1]), STATE, text)
        with pytest.raises(sa.ShkError):
            e.chunk_bases()
        assert e.xchg_scatter_end() == 0
        e.xchg_absorb_tensors(rec, cur, lay)
        e.finalize()
        assert int(e.chunk_bases().sum()) == e.counters()["n_bases_ingested"]
        keys, counts = e.export_table()
        assert len(keys) and np.array_equal(e.lookup(keys, depth=1), counts)  # the share of a world of one takes depths


# ---- 6. the table is not written ---------------------------------------------------------------------------------------------

def test_a_sweep_leaves_the_table_alone(mixed):
    p, genes, full, subs = mixed
    before = (full.histograms().copy(), full.export_table(), full.pcr_run(genes, max_num_nodes=pc.MIXED_BUDGET), full.counters())
    full.pcr_run_depths(genes, [1, 2, 3, 4], max_num_nodes=pc.MIXED_BUDGET)
    full.primer_kmers_depths(mixed_primers(genes), [2, 4])
    full.lookup(p.keys, depth=2)
    assert np.array_equal(full.histograms(), before[0])
    keys, counts = full.export_table()
    assert np.array_equal(keys, before[1][0]) and np.array_equal(counts, before[1][1])
    same_outcomes(full.pcr_run(genes, max_num_nodes=pc.MIXED_BUDGET), before[2], "pcr_run after a sweep")
    assert full.counters() == before[3]


def test_not_finalized_is_as_shk_primer_kmers(orc):
    """The depth calls open as their plain forms do: on a context that was fed and not finalized, the same answer — or
    the same refusal, code and text."""
    p = pc.mixed_panel(orc)
    primers = mixed_primers(cases.mixed_genes(orc))[:4]

    def outcome(call):
        try:
            return ("ok", call())
        except sa.ShkError as e:
            return ("refused", e.code, e.msg)

    with sa.KmerEngine(p.k, 2, 100) as e:
        for c, b, o in dc.chunk_batches(p.bases, p.offsets, 2):
            e.ingest_batch(c, b, o)
        plain = outcome(lambda: e.primer_kmers(primers))
        deep = outcome(lambda: e.primer_kmers_depths(primers, [2])[0])
        assert plain[0] == deep[0]
        if plain[0] == "ok":
            same_primer_results(deep[1], plain[1], "not finalized")
        else:
            assert plain[1:] == deep[1:]
        a, b = outcome(lambda: e.lookup(p.keys[:50])), outcome(lambda: e.lookup(p.keys[:50], depth=2))
        assert a[0] == b[0] and (np.array_equal(a[1], b[1]) if a[0] == "ok" else a[1:] == b[1:])


def test_pcr_extend_panel_depths_18s(orc):
    """18S on 5 chunks, all 5 depths, through pcr_extend_panel(depths=) itself: the pairs with both primer sets."""
    seq, bases, offsets, gene, _, _ = cases.case_18s(orc)
    n = dc.CHUNKS_18S
    primers = [sa.Primer(s, gene.trim, gene.mismatches, gene.min_count, gene.max_primer_kmers) for s in (gene.forward_seq, gene.reverse_seq)]
    params = dict(min_count=gene.min_count, table_min_count=2, high_coverage_ratio=gene.high_coverage_ratio, max_num_nodes=500_000)
    with engine_below(21, bases, offsets, n, n) as e:
        prim = e.primer_kmers_depths(primers, list(range(1, n + 1)))
        assert len(prim[0][0][0]) == 0 and all(len(b[0][0]) and len(b[1][0]) for b in prim[1:])  # nothing at depth 1
        alive = list(range(2, n + 1))
        got = e.pcr_extend_panel([prim[d - 1][s] for d in alive for s in (0, 1)], params, depths=alive)
        for d, g in zip(alive, got):
            with engine_below(21, bases, offsets, n, d) as sub:
                (alone,) = sub.pcr_extend_panel(sub.primer_kmers(primers), params)
            same_graphs(g, alone, f"18S, depth {d}")
            want = dc.expected_18s(orc, d)
            assert (g.found_path, len(g.node_sub_kmers), len(g.edge_src), g.threshold_used) == (want.found_path, want.n_nodes, want.n_edges,
                                                                                              want.threshold_used), d


# ---- 7. the command line -----------------------------------------------------------------------------------------------------

import os  # noqa: E402
import subprocess  # noqa: E402

import pcr_run_ref as run_ref  # noqa: E402

EXE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sharkmer_amd", "csrc", "shk_count")
SPEC_18S = f"forward={cases.FWD_18S},reverse={cases.REV_18S},name=18s,max-length=2500,min-count=3"
TSV_HEADER = "depth\tn_bases_ingested\tgene\tstatus\tfailure_reason\tn_products\tproduct_lengths\n"


def cli_reads(seq):
    """2001 reads: the padded 18S at 0, 1, 1000, 1001 and 2000, every other read ACGT (no k-mers) — at --chunks 3 the
    1000-read cadence puts two copies in chunks 0 and 1 and one in chunk 2."""
    return [seq if i in (0, 1, 1000, 1001, 2000) else "ACGT" for i in range(2001)]


def without_run_lines(text):
    """A stats file without the two lines that name the run: the command line and the device memory in use."""
    return [ln for ln in text.split("\n") if not ln.startswith(("command:", "peak_memory_bytes:"))]


def test_shk_count_pcr_depths(tmp_path, orc):
    seq, _, _, gene, _, _ = cases.case_18s(orc)
    reads = cli_reads(seq)
    fq = tmp_path / "reads.fastq"
    fq.write_text("".join(f"@r{i}\n{s}\n+\n{'I' * len(s)}\n" for i, s in enumerate(reads)))
    want, bases_below = [], []
    for d in (1, 2, 3):
        sub = reads[:1000 * d]
        b = np.frombuffer("".join(sub).encode(), dtype=np.uint8).copy()
        o = np.concatenate([[0], np.cumsum([len(s) for s in sub])]).astype(np.uint64)
        bases_below.append(int(orc.run_batch(b, o, 21, 1, 50).stats["n_bases_ingested"]))
        keys, counts = pc.oracle_table(orc, b, o, 21)
        (w,) = run_ref.run_pcr(keys, counts, 21, [gene], None, max_num_nodes=pcr_ref.compute_node_budget(bases_below[-1]))
        want.append(w)
    assert [w.status for w in want] == [run_ref.NO_PRIMERS, run_ref.SUCCESS, run_ref.SUCCESS]
    base = ["-k", "21", "--chunks", "3", "--histo-max", "50", "-s", "s", "--pcr-primers", SPEC_18S]
    for d in ("sweep", "plain", "py"):
        (tmp_path / d).mkdir()
    r = subprocess.run([EXE] + base + ["-o", str(tmp_path / "sweep"), "--pcr-depths", "all", str(fq)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([EXE] + base + ["-o", str(tmp_path / "plain"), str(fq)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    sweep, plain = tmp_path / "sweep", tmp_path / "plain"
    assert not (sweep / "s_18s.depth1.fasta").exists()
    for d in (2, 3):
        assert (sweep / f"s_18s.depth{d}.fasta").read_text() == run_ref.fasta_text("s", "18s", want[d - 1].products), d
    rows = [f"{d}\t{bases_below[d - 1]}\t18s\t{'success' if w.status == 0 else 'fail'}\t{w.reason or ''}\t{len(w.products)}\t"
            f"{','.join(str(len(x.sequence)) for x in w.products)}\n" for d, w in zip((1, 2, 3), want)]
    assert (sweep / "s.pcr_depths.tsv").read_text() == TSV_HEADER + "".join(rows)
    assert rows[0].split("\t")[4] == "forward and reverse primers not found"
    # every other file is the run's without the flag
    assert sorted(x.name for x in sweep.iterdir()) == sorted([x.name for x in plain.iterdir()] + ["s_18s.depth2.fasta", "s_18s.depth3.fasta",
                                                                                                "s.pcr_depths.tsv"])
    for name in ("s_18s.fasta", "s.histo", "s.final.histo"):
        assert (sweep / name).read_bytes() == (plain / name).read_bytes(), name
    assert without_run_lines((sweep / "s.stats.yaml").read_text()) == without_run_lines((plain / "s.stats.yaml").read_text())
    # a gapped list, and run_files
    sa.run_files([str(fq)], k=21, chunks=3, histo_max=50, sample="s", outdir=str(tmp_path / "py"), pcr_primers=[SPEC_18S], pcr_depths=[1, 3])
    assert (tmp_path / "py" / "s.pcr_depths.tsv").read_text() == TSV_HEADER + rows[0] + rows[2]
    assert (tmp_path / "py" / "s_18s.depth3.fasta").read_bytes() == (sweep / "s_18s.depth3.fasta").read_bytes()
    assert not (tmp_path / "py" / "s_18s.depth2.fasta").exists()


def test_shk_count_pcr_depths_refusals(tmp_path):
    out = tmp_path / "out"
    base = [EXE, "-k", "21", "-s", "s", "-o", str(out)]
    with_gene = base + ["--pcr-primers", SPEC_18S]
    for args, text in ((with_gene + ["--chunks", "3", "--pcr-depths", "all", "--read-threading"], "--pcr-depths takes no --read-threading"),
                       (with_gene + ["--chunks", "3", "--pcr-depths", "all", "--devices", "0,0", "--group-graph"], "--pcr-depths needs one device"),
                       (base + ["--chunks", "3", "--pcr-depths", "all"], "--pcr-depths needs --pcr-primers"),
                       (with_gene + ["--chunks", "3", "--pcr-depths", "2,4"], "depth 4 is not in 1..3"),
                       (with_gene + ["--chunks", "3", "--pcr-depths", "0"], "depth 0 is not in 1..3"),
                       (with_gene + ["--chunks", "3", "--pcr-depths", "2,1"], "strictly ascending"),
                       (with_gene + ["--chunks", "3", "--pcr-depths", "some"], "neither 'all' nor a list"),
                       (with_gene + ["--pcr-depths", "all"], "--chunks of at least 1")):
        r = subprocess.run(args + ["nothing.fastq"], capture_output=True, text=True)
        assert r.returncode == 1 and r.stderr.startswith("Error: ") and text in r.stderr, (args, r.stderr)
    assert not out.exists()  # before a read is read, and before the output directory is made
    for kw, text in ((dict(pcr_primers=[SPEC_18S], pcr_depths="all", read_threading=True), "--read-threading"),
                     (dict(pcr_primers=[SPEC_18S], pcr_depths="all", device_ids=[0, 0], group_graph=True), "one device"),
                     (dict(pcr_depths="all"), "--pcr-primers"),
                     (dict(pcr_primers=[SPEC_18S], pcr_depths=[4]), "depth 4 is not in 1..3")):
        refused(lambda: sa.run_files(["nothing.fastq"], k=21, chunks=3, sample="s", outdir=str(out), **kw), BAD_ARG, text)
    assert not out.exists()
