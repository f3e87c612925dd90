"""GPU tests of sPCR's graph extension over the device-resident table: shk_neighborhood (k_nb_narrow_panel, k_nb_wide) and
shk_pcr_extend against tests/pcr_ref.py — the reference's create_seed_graph / extend_graph / threshold sweep and the
level-by-level definition of the neighbourhood, restated literally over the CPU oracle's merged table.  Everything is
compared as arrays, order included."""
import os
import random

import numpy as np
import pytest

import sharkmer_amd as sa
import pcr_ref as ref
import primer_ref

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FWD_18S, REV_18S = "AACCTGGTTGATCCTGCCAGT", "TGATCCTTCTGCAGGTTCACCTAC"
_cache = {}


def oracle_table(orc, bases, offsets, k, chunks):
    run = orc.run_batch(bases, offsets, k, chunks, 100)
    return run.merged().export()  # (copies: run may go)


def reads_of(seq, copies):
    b = np.frombuffer(seq.encode() * copies, dtype=np.uint8).copy()
    return b, np.arange(copies + 1, dtype=np.uint64) * np.uint64(len(seq))


def rc_str(s):
    return s[::-1].translate(str.maketrans("ACGTN", "TGCAN"))


def assert_graph(got, want, used, steps, what=None):
    g = want
    assert list(got.node_sub_kmers) == g.sub_kmer, what
    assert list(got.node_flags) == g.flags(), what
    assert list(got.edge_src) == [e[0] for e in g.edges], what
    assert list(got.edge_tgt) == [e[1] for e in g.edges], what
    assert list(got.edge_counts) == [e[2] for e in g.edges], what
    assert (got.found_path, got.threshold_used, got.steps_run) == (g.found_path, used, steps), what


def assert_neighborhood(got, want, what=None):
    gk, gc, gn, gd, gl = got
    wk, wc, wn, wd, wl = want
    assert gl == wl, (what, gl, wl)
    assert list(gk) == wk and list(gc) == wc, (what, len(gk), len(wk))
    assert list(gn) == wn and list(gd) == wd, (what, len(gn), len(wn))


# ---- 1. the 18S case --------------------------------------------------------------------------------------------

def case_18s(orc):
    if "18s" not in _cache:
        seq = open(os.path.join(G, "pcr_18s_padded.txt")).read().strip()
        bases, offsets = reads_of(seq, 10)
        keys, counts = oracle_table(orc, bases, offsets, 21, 1)
        _cache["18s"] = (bases, offsets, ref.table_dict(keys, counts))
    return _cache["18s"]


@pytest.mark.parametrize("min_count,sweep", [(5, False), (3, True)])
def test_18s_end_to_end(orc, min_count, sweep):
    """primer_pair_kmers → pcr_extend on the padded 18S ×10 at k 21 (mod.rs:1331-1371): a chain about 1800 levels
    deep, the narrow kernel's case."""
    bases, offsets, table = case_18s(orc)
    with sa.KmerEngine(21, 1, 100) as eng:
        eng.ingest_reads(bases, offsets)
        eng.finalize()
        fwd, rev = eng.primer_pair_kmers(FWD_18S, REV_18S, trim=15, mismatches=2, min_count=3)
        got = eng.pcr_extend(fwd, rev, min_count=min_count, table_min_count=1, sweep=sweep,
                             max_num_nodes=ref.DEFAULT_MAX_NUM_NODES)
        nb = eng.neighborhood(got.node_sub_kmers[:2], [1, 2], 5, cap=1 << 14, fringe_cap=64)
    want, used, steps = ref.pcr_extend(fwd[:2], rev[:2], table, 21, min_count, 1, 10.0, ref.DEFAULT_MAX_NUM_NODES, sweep)
    assert want.found_path and len(want.sub_kmer) > 1700
    assert_graph(got, want, used, steps)
    assert_neighborhood(nb, ref.neighborhood(want.sub_kmer[:2], [1, 2], table, 21, 5))
    assert nb[4] > 1700 and len(nb[2]) == 0


def test_18s_single_call_under_the_fetch_caps(orc, monkeypatch):
    """shk_pcr_extend is shk_pcr_extend_panel's replay with one gene: SHK_PCR_FETCH_CAP sizes its fetches as it sizes the
    panel's, the panel-only SHK_PCR_PANEL_FETCH_CAP does not touch it, and either way its graph is the model's and the
    one pcr_extend_panel gives for that gene."""
    bases, offsets, table = case_18s(orc)
    a = dict(min_count=5, table_min_count=1, sweep=False, max_num_nodes=ref.DEFAULT_MAX_NUM_NODES)
    for name in ("SHK_PCR_FETCH_CAP", "SHK_PCR_PANEL_FETCH_CAP", "SHK_PCR_PANEL_THREADS"):
        monkeypatch.delenv(name, raising=False)
    with sa.KmerEngine(21, 1, 100) as eng:
        eng.ingest_reads(bases, offsets)
        eng.finalize()
        fwd, rev = eng.primer_pair_kmers(FWD_18S, REV_18S, trim=15, mismatches=2, min_count=3)
        want, used, steps = ref.pcr_extend(fwd[:2], rev[:2], table, 21, 5, 1, 10.0, ref.DEFAULT_MAX_NUM_NODES, False)
        assert want.found_path and len(want.sub_kmer) > 1700
        for fetch_cap in (None, "64"):
            for panel_cap in (None, "64"):
                for env, value in (("SHK_PCR_FETCH_CAP", fetch_cap), ("SHK_PCR_PANEL_FETCH_CAP", panel_cap)):
                    if value is None:
                        monkeypatch.delenv(env, raising=False)
                    else:
                        monkeypatch.setenv(env, value)
                what = (fetch_cap, panel_cap)
                assert_graph(eng.pcr_extend(fwd, rev, **a), want, used, steps, what)
                (one,) = eng.pcr_extend_panel([fwd, rev], a)
                assert_graph(one, want, used, steps, what + ("panel",))


# ---- 2. neighborhood on synthetic reads ---------------------------------------------------------------------------

SPEC = dict(genome_len=40_000, sub_per_64k=400, n_per_64k=30)


def synth_case(orc, k, chunks):
    """Reads, the oracle's table as a dict, 35 seeds (30 cut from reads with random dirs, 5 that occur nowhere) and the
    model's levels per min_count — computed once per (k, chunks)."""
    key = ("synth", k, chunks)
    if key in _cache:
        return _cache[key]
    rng = random.Random(7000 + k)
    bases, offsets = sa.synth_reads(sa.SynthSpec(seed_genome=k, **SPEC), 0, 1200)
    nodes, dirs = [], []
    if k % 2 == 0:  # a random genome this size holds no palindromic k-mer: two more reads with one in the middle
        clean, _ = sa.synth_reads(sa.SynthSpec(genome_len=SPEC["genome_len"], seed_genome=k), 0, 1)
        s = clean.tobytes().decode()
        pal = s[65:65 + k // 2] + rc_str(s[65:65 + k // 2])
        extra = np.frombuffer((s[:65] + pal + s[65 + k:150]).encode() * 2, dtype=np.uint8)
        bases = np.concatenate([bases, extra])
        offsets = np.arange(1202 + 1, dtype=np.uint64) * np.uint64(150)
        nodes.append(primer_ref.string_to_oligo(pal[:k - 1]))  # the node in front of the palindrome, both ways
        dirs.append(3)
    keys, counts = oracle_table(orc, bases, offsets, k, chunks)
    table = ref.table_dict(keys, counts)
    while len(nodes) < 30:
        r = rng.randrange(len(offsets) - 1)
        s = bases[int(offsets[r]):int(offsets[r + 1])].tobytes().decode()
        at = rng.randrange(0, len(s) - (k - 1))
        p = s[at:at + k - 1]
        if "N" in p:
            continue
        nodes.append(primer_ref.string_to_oligo(p))
        dirs.append(rng.randint(1, 3))
    mask = (1 << (2 * (k - 1))) - 1
    present = set()
    for x in table:
        for y in (x, ref.revcomp(x, k)):
            present.add(y >> 2)
            present.add(y & mask)
    while len(nodes) < 35:
        n = rng.randrange(mask + 1)
        if n not in present:
            nodes.append(n)
            dirs.append(rng.randint(1, 3))
    levels = {mc: ref.neighborhood_levels(nodes, dirs, table, k, mc) for mc in (1, 2, 3)}
    _cache[key] = (bases, offsets, table, nodes, dirs, levels)
    return _cache[key]


@pytest.mark.parametrize("k,chunks", [(21, 1), (21, 3), (31, 1), (20, 1), (9, 1)])
def test_neighborhood_against_model(orc, k, chunks):
    """Complete neighbourhoods at min_count 1, 2, 3: lanes summed (3 chunks), a 60-bit node (k 31), an even k with
    palindromic k-mers (k 20), and k 9, where the graph branches at every node, the frontier outgrows a workgroup
    within a few levels (the wide kernel) and thins out again at the end (the way back to the narrow one)."""
    bases, offsets, table, nodes, dirs, levels = synth_case(orc, k, chunks)
    n_all = len(table)
    with sa.KmerEngine(k, chunks, 100) as eng:
        eng.ingest_reads(bases, offsets)
        eng.finalize()
        for mc in (1, 2, 3):
            want = ref.neighborhood(nodes, dirs, table, k, mc, levels=levels[mc])
            got = eng.neighborhood(nodes, dirs, mc, cap=n_all + 1, fringe_cap=n_all * 2 + 64)
            assert_neighborhood(got, want, (k, mc))
            assert len(got[2]) == 0 and len(want[0]) > 0
        if k == 20:
            assert any(x == ref.revcomp(x, k) for x in table)
        # mid-stream too: what shk_lookup sees (no finalize since the ingest)
        eng.reset()
        eng.ingest_reads(bases, offsets)
        assert_neighborhood(eng.neighborhood(nodes, dirs, 1, cap=n_all + 1, fringe_cap=n_all * 2 + 64),
                            ref.neighborhood(nodes, dirs, table, k, 1, levels=levels[1]), (k, "mid-stream"))
    sizes = [len(e) for e, _ in levels[1]]
    if k == 9:  # otherwise the wide kernel was not taken, or never left again
        assert max(sizes) > 1024 and sizes[-1] <= 1024 and sizes[0] <= 1024
    if k == 21:
        assert len(levels[1]) > 50  # many levels in one narrow launch


# ---- 3. truncation ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [21, 9])
def test_truncation_and_resume(orc, k):
    """max_levels, cap and fringe_cap cut at whole levels exactly as the model's rule says, at the capacities where the
    rule turns (|K_L| and |K_L| − 1, a level's size and one less); resuming from the fringe reaches the whole
    neighbourhood."""
    bases, offsets, table, nodes, dirs, levels = synth_case(orc, k, 1)
    lv = levels[1]
    n_seeds = len(lv[0][0])
    big_k, big_f = len(table) + 1, 2 * len(table) + 64
    ksz = np.cumsum([len(nk) for _, nk in lv])  # |K_L| for L = 1, 2, …
    L = max(range(1, len(lv)), key=lambda i: len(lv[i][0]))  # the widest level: wider than the seeds, so that
    some_level = len(lv[L][0])                              # a fringe_cap of one less still takes them
    assert some_level - 1 >= n_seeds and 1 <= L < len(lv) - 1
    cases = [dict(max_levels=m) for m in (1, 2, 3)]
    cases += [dict(cap=c) for c in (0, 1, 7, int(ksz[L]), int(ksz[L]) - 1)]
    cases += [dict(fringe_cap=f) for f in (n_seeds, some_level, some_level - 1)]
    with sa.KmerEngine(k, 1, 100) as eng:
        eng.ingest_reads(bases, offsets)
        eng.finalize()
        for kw in cases:
            a = dict(max_levels=0, cap=big_k, fringe_cap=big_f)
            a.update(kw)
            want = ref.neighborhood(nodes, dirs, table, k, 1, levels=lv, **a)
            got = eng.neighborhood(nodes, dirs, 1, **a)
            assert_neighborhood(got, want, kw)
            if kw.get("cap") == 0:
                assert got[4] == 0 and len(got[2]) == n_seeds
        # resume: a fresh call knows nothing of the earlier ones, so the caller leaves out what it has already sent
        whole = ref.neighborhood(nodes, dirs, table, k, 1, levels=lv)
        for step in (dict(max_levels=3 if k == 9 else 40), dict(cap=200 if k == 21 else 3000)):
            union, sent = {}, set()
            fn, fd = list(nodes), list(dirs)
            calls = 0
            while fn:
                for n, d in zip(fn, fd):
                    sent.update((n, b) for b in (1, 2) if d & b)
                n = 2 * len(fn)
                a = dict(max_levels=0, cap=big_k, fringe_cap=big_f)
                a.update(step)
                a["cap"] = max(a["cap"], 4 * n)  # (level 0 always fits then: every call gets further)
                gk, gc, gn, gd, gl = eng.neighborhood(fn, fd, 1, **a)
                assert gl >= 1
                union.update(zip(gk.tolist(), gc.tolist()))
                keep = [(x, y) for x, y in zip(gn.tolist(), gd.tolist()) if (x, y) not in sent]
                fn, fd = [x for x, _ in keep], [y for _, y in keep]
                calls += 1
            assert calls >= 2
            assert sorted(union) == whole[0] and [union[x] for x in whole[0]] == whole[1], step


# ---- 4. pcr_extend on random primer pairs -------------------------------------------------------------------------

PCR_SPEC = dict(genome_len=6000, sub_per_64k=400, n_per_64k=30)
PCR_READS = 600
# (min_count, table_min_count, high_coverage_ratio, max_num_nodes (None: the default budget), sweep)
PCR_PARAMS = [(2, 2, 10.0, None, True), (2, 1, 10.0, None, False), (2, 2, 1.5, None, True), (8, 2, 1.5, None, False),
              (2, 2, 10.0, 50, True), (2, 1, 10.0, 50, False), (2, 2, 10.0, 1200, True), (16, 1, 1.5, 1200, False),
              (12, 1, 1.5, None, False), (3, 2, 10.0, 1200, False), (24, 2, 1.5, 50, True)]


def pcr_case(orc, k, doubled):
    key = ("pcr", k, doubled)
    if key in _cache:
        return _cache[key]
    bases, offsets = sa.synth_reads(sa.SynthSpec(seed_genome=100 + k, **PCR_SPEC), 0, PCR_READS)
    if doubled:
        bases = np.tile(bases, 2)
        offsets = np.arange(2 * PCR_READS + 1, dtype=np.uint64) * np.uint64(150)
    keys, counts = oracle_table(orc, bases, offsets, k, 1)
    # both primers from one strand of the genome, 300-900 bases apart: error-free stretches of 1000 bases
    long_, _ = sa.synth_reads(sa.SynthSpec(genome_len=6000, read_len=1000, seed_genome=100 + k), 0, 4)
    rng = random.Random(k)
    pairs = []
    for r in range(2):
        s = long_[r * 1000:(r + 1) * 1000].tobytes().decode()
        a, d = rng.randrange(0, 60), rng.randrange(300, 900)
        pairs.append((s[a:a + 24], rc_str(s[a + d:a + d + 24])))
    _cache[key] = (bases, offsets, keys, counts, ref.table_dict(keys, counts), pairs)
    return _cache[key]


@pytest.mark.parametrize("k,doubled", [(15, False), (15, True), (21, False), (21, True)])
def test_pcr_extend_random_pairs(orc, k, doubled, monkeypatch):
    """Budgets that break mid-queue (50, 1200), both ratios, both table floors, both sweep values; with the reads
    doubled a k 15 graph passes 1000 nodes and the median is refreshed (graph.rs:400-405).  Every case twice: with the
    library's own fetch size and with SHK_PCR_FETCH_CAP = 8, which makes the replay fetch again every few nodes.  (On
    these reads no run at ratio 1.5 grows to 1000 nodes: a skip at 1.5 cuts the chain long before.)"""
    bases, offsets, keys, counts, table, pairs = pcr_case(orc, k, doubled)
    default_budget = ref.compute_node_budget(int((bases != ord("N")).sum()))
    refreshes = breaks = skips_differ = 0
    monkeypatch.delenv("SHK_PCR_FETCH_CAP", raising=False)
    with sa.KmerEngine(k, 1, 100) as eng:
        eng.ingest_reads(bases, offsets)
        eng.finalize()
        for fp, rp in pairs:
            fwd, rev = eng.primer_pair_kmers(fp, rp, trim=15, mismatches=2, min_count=2)
            wf = primer_ref.get_primer_kmers(fp, keys, counts, k, 15, 2, 2)
            assert list(fwd[0]) == list(wf[0]) and len(fwd[0]) and len(rev[0])
            for mc, tmc, ratio, budget, sweep in PCR_PARAMS:
                mc = mc * 2 if doubled and mc > 3 else mc
                want, used, steps = ref.pcr_extend(fwd[:2], rev[:2], table, k, mc, tmc, ratio, budget or default_budget, sweep)
                refreshes += want.median_refreshes
                breaks += want.budget_break
                what = (fp, rp, mc, tmc, ratio, budget, sweep)
                got = eng.pcr_extend(fwd, rev, min_count=mc, table_min_count=tmc, high_coverage_ratio=ratio,
                                     max_num_nodes=budget, sweep=sweep)
                assert_graph(got, want, used, steps, what)
                monkeypatch.setenv("SHK_PCR_FETCH_CAP", "8")
                forced = eng.pcr_extend(fwd, rev, min_count=mc, table_min_count=tmc, high_coverage_ratio=ratio,
                                        max_num_nodes=budget, sweep=sweep)
                monkeypatch.delenv("SHK_PCR_FETCH_CAP")
                assert_graph(forced, want, used, steps, what + ("forced",))
                other = ref.pcr_extend(fwd[:2], rev[:2], table, k, mc, tmc, 10.0 if ratio == 1.5 else 1.5,
                                       budget or default_budget, sweep)[0]
                skips_differ += other.sub_kmer != want.sub_kmer
    assert breaks > 0 and skips_differ > 0
    if k == 15 and doubled:
        assert refreshes > 0


# ---- 5. errors ------------------------------------------------------------------------------------------------------

def test_errors_and_empty_sets(orc):
    bases, offsets, table = case_18s(orc)
    k = 21
    mask = (1 << (2 * (k - 1))) - 1
    with sa.KmerEngine(k, 1, 100) as eng:
        eng.ingest_reads(bases, offsets)
        eng.finalize()
        for nodes, dirs in (([5], [0]), ([5], [4]), ([5, 6], [1, 255]), ([mask + 1], [1])):
            with pytest.raises(sa.ShkError) as e:
                eng.neighborhood(nodes, dirs, 1)
            assert e.value.code == -2, (nodes, dirs)
        with pytest.raises(sa.ShkError) as e:
            eng.neighborhood([1, 2, 3], [1, 1, 3], 1, fringe_cap=3)  # four distinct entries
        assert e.value.code == -2 and "fringe_cap" in e.value.msg
        assert_neighborhood(eng.neighborhood([1, 2, 2], [1, 3, 2], 1, fringe_cap=3),
                            ref.neighborhood([1, 2, 2], [1, 3, 2], table, k, 1))
        assert eng.neighborhood([], [], 1)[4] == 0
        assert_neighborhood(eng.neighborhood([mask], [3], 0, cap=0, fringe_cap=2),
                            ref.neighborhood([mask], [3], table, k, 0, cap=0, fringe_cap=2))  # min_count 0 reads as 1
        # an empty primer set: the other set's seeds alone, extended; no path
        fwd, rev = eng.primer_pair_kmers(FWD_18S, REV_18S, trim=15, mismatches=2, min_count=3)
        none = (np.zeros(0, np.uint64), np.zeros(0, np.uint32))
        for f, r in ((fwd, none), (none, rev), (none, none)):
            for sweep in (False, True):
                got = eng.pcr_extend(f, r, min_count=3, table_min_count=1, sweep=sweep, max_num_nodes=100_000)
                want, used, steps = ref.pcr_extend(f[:2], r[:2], table, k, 3, 1, 10.0, 100_000, sweep)
                assert_graph(got, want, used, steps)
                assert not got.found_path and len(got.node_sub_kmers) >= len(f[0]) + len(r[0])
    with sa.KmerEngine(k, 1, 100, device_ids=[0, 0]) as eng:
        eng.ingest_reads(bases, offsets)
        eng.finalize()
        with pytest.raises(sa.ShkError) as e:
            eng.neighborhood([5], [1], 1)
        assert e.value.code == -11 and "multi-device context" in e.value.msg
        with pytest.raises(sa.ShkError) as e:
            eng.pcr_extend(fwd, rev, max_num_nodes=1000)
        assert e.value.code == -11 and "multi-device context" in e.value.msg
    with sa.KmerEngine(k, 1, 100, n_owners=2, owner_id=1) as eng:
        eng.ingest_reads(bases, offsets)
        eng.finalize()
        with pytest.raises(sa.ShkError) as e:
            eng.neighborhood([5], [1], 1)
        assert e.value.code == -11 and "owner share" in e.value.msg
