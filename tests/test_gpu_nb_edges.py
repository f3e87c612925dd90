"""shk_neighborhood and shk_pcr_extend on the crafted tables of tests/nb_cases.py: levels of exactly 1023, 1024, 1025 and
2049 entries and the cuts (max_levels, cap, fringe_cap) on the level where k_nb_narrow_panel and k_nb_wide hand over, complete
de Bruijn graphs at k 2..7, thresholds met only by the saturating sum over lanes, a table grown under the graph.  Every
table goes in through `insert` — no reads, no finalize — and every answer is compared with tests/pcr_ref.py over the
same inserts merged in Python, arrays and order included.  tests/test_pcr_ref_cpu.py checks without a GPU that each
table has the level sizes it was designed to have; the sizes are asserted here again from the model's levels."""
import numpy as np
import pytest

import sharkmer_amd as sa
import nb_cases
import pcr_ref as ref
from test_gpu_pcr_extend import assert_graph, assert_neighborhood

pytestmark = pytest.mark.gpu


def engine_for(case, hint=0):
    eng = sa.KmerEngine(case.k, case.chunks, 10, capacity_hint=hint)
    for lane, keys, counts in case.inserts:
        eng.insert(keys, counts, chunk_id=lane)
    return eng


class Walk:
    """One (table, seeds, min_count): the model's levels once, then any number of calls compared."""

    def __init__(self, eng, case, table, min_count=None):
        self.eng, self.case, self.table = eng, case, table
        self.mc = case.min_count if min_count is None else min_count
        self.lv = ref.neighborhood_levels(case.seeds, case.dirs, table, case.k, self.mc)
        self.sizes = [len(e) for e, _ in self.lv]
        self.ksz = [0] + [int(x) for x in np.cumsum([len(nk) for _, nk in self.lv])]  # |K_L| for L = 0, 1, …
        self.big = dict(max_levels=0, cap=len(table) + 1, fringe_cap=2 * len(table) + len(self.lv[0][0]) + 64)

    def check(self, **kw):
        a = dict(self.big)
        a.update(kw)
        c = self.case
        what = (c.name, self.mc, kw)
        try:
            want = ref.neighborhood(c.seeds, c.dirs, self.table, c.k, self.mc, levels=self.lv, **a)
        except ValueError:  # more distinct seeds than fringe_cap
            with pytest.raises(sa.ShkError) as e:
                self.eng.neighborhood(c.seeds, c.dirs, self.mc, **a)
            assert e.value.code == -2 and "fringe_cap" in e.value.msg, what
            return None
        assert_neighborhood(self.eng.neighborhood(c.seeds, c.dirs, self.mc, **a), want, what)
        return want

    def resume(self, **step):
        """Call after call from the fringe (a fresh call knows nothing of the earlier ones: the caller leaves out what it
        has sent) until nothing is left: the union is the whole neighbourhood."""
        whole = ref.neighborhood(self.case.seeds, self.case.dirs, self.table, self.case.k, self.mc, levels=self.lv)
        union, sent, calls = {}, set(), 0
        fn, fd = list(self.case.seeds), list(self.case.dirs)
        while fn:
            for n, d in zip(fn, fd):
                sent.update((n, b) for b in (1, 2) if d & b)
            a = dict(self.big)
            a.update(step)
            gk, gc, gn, gd, gl = self.eng.neighborhood(fn, fd, self.mc, **a)
            assert gl >= 1
            union.update(zip(gk.tolist(), gc.tolist()))
            keep = [(x, y) for x, y in zip(gn.tolist(), gd.tolist()) if (x, y) not in sent]
            fn, fd = [x for x, _ in keep], [y for _, y in keep]
            calls += 1
        assert sorted(union) == whole[0] and [union[x] for x in whole[0]] == whole[1], (self.case.name, step)
        return calls


# ---- 1. the hand-over sizes -------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["flat1023", "flat1024", "flat1025", "flat2049", "falling", "rising", "zigzag"])
def test_levels_at_the_hand_over_sizes(name):
    """Levels of exactly NB_NARROW − 1, NB_NARROW, NB_NARROW + 1 entries (and two workgroups' worth), flat, falling
    through the hand-over, rising through it, and wide → narrow → wide → narrow (zigzag: the one-workgroup kernel launched
    on the single job from the host's level loop, and handing back to it); fringe_cap at the three sizes (fewer than the seeds: refused), and on
    the hand-over level L every cut there is: max_levels L − 1, L, L + 1, cap |K_L| and |K_{L+1}| and one less each."""
    case = nb_cases.CASES[name]()
    table = nb_cases.merged_table(case.inserts)
    with engine_for(case) as eng:
        w = Walk(eng, case, table)
        assert w.sizes == case.sizes
        whole = w.check()
        assert whole[4] == len(case.sizes) and not whole[2] and len(whole[0]) == len(table)
        for f in (1023, 1024, 1025):
            w.check(fringe_cap=f)
        L = case.hand_over or 3
        for m in (L - 1, L, L + 1):
            w.check(max_levels=m)
            w.check(max_levels=m, fringe_cap=1024)
        for cap in (w.ksz[L], w.ksz[L] - 1, w.ksz[L + 1], w.ksz[L + 1] - 1):
            cut = w.check(cap=cap)
            assert cut[4] == (L + 1 if cap == w.ksz[L + 1] else L if cap >= w.ksz[L] else L - 1)
        assert w.resume(max_levels=2) == (len(case.sizes) + 1) // 2


@pytest.mark.parametrize("name", ["rising", "zigzag", "dense5_one", "dense7_one"])
def test_single_calls_around_a_panel_call(name):
    """shk_neighborhood lays its scratch out as the panel does (it is the panel's one-job case): on one context a single
    call, a panel of three jobs with other seeds and capacities, and the single call again with a smaller cap — each
    against the model, so nothing of the layout before shows in the call after."""
    case = nb_cases.CASES[name]()
    table = nb_cases.merged_table(case.inserts)
    with engine_for(case) as eng:
        w = Walk(eng, case, table)
        whole = w.check()
        assert len(whole[0]) == len(table)
        last = case.seeds[-1:]
        jobs = [(case.seeds, case.dirs, w.mc, w.big["cap"], w.big["fringe_cap"]),   # the same job inside a panel
                (last, [3], w.mc, 8, 64),                                           # one seed both ways, cut by its cap
                (case.seeds[:7], case.dirs[:7], w.mc + 1, w.ksz[2], w.big["fringe_cap"])]
        got = eng.neighborhood_panel(jobs, max_levels=3)
        for j, (job, g) in enumerate(zip(jobs, got)):
            want = ref.neighborhood(job[0], job[1], table, case.k, job[2], max_levels=3, cap=job[3], fringe_cap=job[4])
            assert_neighborhood(g, want, (name, "job", j))
        cut = w.check(cap=w.ksz[2] - 1)
        assert cut[4] == 1 and len(cut[0]) < len(whole[0])
        w.check(max_levels=2, cap=w.ksz[2])
        w.check()


# ---- 2. complete de Bruijn graphs -------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [2, 3, 4, 5, 6, 7])
def test_complete_de_bruijn_graphs(k):
    """Every canonical k-mer is there, so every successor is met again from four sides (the worst case for the two
    device sets); k ≤ 5 has one- to four-base nodes and homopolymer self-loops, k 6 palindromes, and at k 7 one seed
    grows to a level of 3072 entries (the wide kernel) while every node both ways is 8192 seeds and nothing after.
    Thresholds 1..4 over counts 1..4, cap at the number of canonical k-mers and one less, and resumed two levels a call."""
    one, every = nb_cases.dense(k, False), nb_cases.dense(k, True)
    table = nb_cases.merged_table(one.inserts)
    n = len(table)
    assert n == len(nb_cases.canonical_kmers(k)) and (k != 6 or any(x == ref.revcomp(x, k) for x in table))
    with engine_for(one) as eng:
        for case in (one, every):
            for mc in (1, 2, 3, 4):
                w = Walk(eng, case, table, mc)
                whole = w.check()
                assert not whole[2]
                full = w.check(cap=n)
                w.check(cap=n - 1)
                if mc == 1:
                    assert w.sizes == case.sizes and len(whole[0]) == n and full == whole
                    assert w.check(cap=n - 1)[4] < whole[4]
                if whole[0]:
                    w.check(cap=len(whole[0]))
                    w.check(cap=len(whole[0]) - 1)
                calls = w.resume(max_levels=2)
                assert calls >= 2 or len(w.sizes) <= 2


# ---- 3. thresholds over lanes -----------------------------------------------------------------------------------

def test_thresholds_met_over_lanes():
    """3 lanes: a count that meets min_count only as the sum over lanes is taken and one a unit short is not; a sum past
    2^32 − 1 is reported as 2^32 − 1 and accepted at min_count 2^32 − 1, where 2^32 − 2 is refused; a key inserted with
    count 0 is in the table and stops the walk."""
    cases = nb_cases.lanes()
    table = nb_cases.merged_table(cases[0].inserts)
    with engine_for(cases[0]) as eng:
        keys = np.array(sorted(table), dtype=np.uint64)
        assert eng.lookup(keys, canonical=True).tolist() == [table[int(x)] for x in keys]
        for case in cases:
            w = Walk(eng, case, table)
            assert w.sizes == case.sizes, case.name
            whole = w.check()
            assert len(whole[0]) == sum(case.sizes[1:]) and not whole[2], case.name
            if case.min_count == nb_cases.U32_MAX:
                assert whole[1] == [nb_cases.U32_MAX] * 2
            if case.min_count == nb_cases.U32_MAX - 1:
                assert sorted(whole[1]) == [nb_cases.U32_MAX - 1, nb_cases.U32_MAX, nb_cases.U32_MAX]
            w.check(max_levels=2)
            w.check(cap=1)


# ---- 4. the same graph in a table that grew -----------------------------------------------------------------------

def test_complete_graph_in_a_table_that_grew():
    """The k 7 graph on a context made with the smallest capacity hint; 300 000 inserts of keys no canonical lookup
    reaches grow the table (n_grows > 0), and the neighbourhood over the union is what it was."""
    one, every = nb_cases.dense(7, False), nb_cases.dense(7, True)
    more = nb_cases.growth_inserts()
    union = nb_cases.merged_table(one.inserts + [more])
    assert len(union) > len(nb_cases.merged_table(one.inserts))
    with engine_for(one, hint=1) as eng:
        before = eng.counters()["n_grows"]
        first = eng.neighborhood(one.seeds, one.dirs, 1, cap=len(union), fringe_cap=1 << 14)
        eng.insert(more[1], more[2], chunk_id=more[0])
        assert eng.counters()["n_grows"] > before and eng.counters()["n_grows"] > 0
        for case in (one, every):
            for mc in (1, 3):
                w = Walk(eng, case, union, mc)
                whole = w.check()
                if mc == 1:
                    assert w.sizes == case.sizes
                    if case is one:
                        assert_neighborhood(first, whole, "before the growth")
            w.resume(max_levels=2)
        keys, counts = eng.export_table()
        assert dict(zip(keys.tolist(), counts.tolist())) == union


# ---- 5. pcr_extend over the chains --------------------------------------------------------------------------------

# (min_count, table_min_count, high_coverage_ratio, max_num_nodes, sweep)
EXTEND_PARAMS = [(1, 1, 10.0, 100_000, True), (1, 1, 10.0, 100_000, False), (2, 1, 1.5, 100_000, True), (1, 2, 10.0, 2500, True),
                 (1, 1, 1.5, 50, False), (3, 1, 10.0, 100_000, False)]


@pytest.mark.parametrize("name", ["falling", "rising"])
def test_pcr_extend_over_the_chains(name, monkeypatch):
    """The chain heads as the forward primer set and the reverse complements of the chain tails as the reverse one:
    the replay's first fetch is a level of some 2050 entries and the ones after it fall or rise through the hand-over.
    With the library's own fetch size and with SHK_PCR_FETCH_CAP = 8."""
    case = nb_cases.CASES[name]()
    k = case.k
    table = nb_cases.merged_table(case.inserts)
    fk = sorted(case.heads)
    rk = sorted(ref.revcomp(x, k) for x in case.tails)
    fwd = (fk, [ref.canonical_count(table, x, k) for x in fk])
    rev = (rk, [ref.canonical_count(table, x, k) for x in rk])
    monkeypatch.delenv("SHK_PCR_FETCH_CAP", raising=False)
    found = 0
    with engine_for(case) as eng:
        for mc, tmc, ratio, budget, sweep in EXTEND_PARAMS:
            want, used, steps = ref.pcr_extend(fwd, rev, table, k, mc, tmc, ratio, budget, sweep)
            found += want.found_path
            what = (name, mc, tmc, ratio, budget, sweep)
            a = dict(min_count=mc, table_min_count=tmc, high_coverage_ratio=ratio, max_num_nodes=budget, sweep=sweep)
            assert_graph(eng.pcr_extend(fwd, rev, **a), want, used, steps, what)
            monkeypatch.setenv("SHK_PCR_FETCH_CAP", "8")
            forced = eng.pcr_extend(fwd, rev, **a)
            monkeypatch.delenv("SHK_PCR_FETCH_CAP")
            assert_graph(forced, want, used, steps, what + ("forced",))
    assert found > 0
