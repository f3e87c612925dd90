"""GPU tests of shk_neighborhood_panel (k_nb_seed_panel, k_nb_narrow_panel and the wide continuation): every job of a
panel call against the same job alone through shk_neighborhood and against tests/pcr_ref.py's level-by-level model, on
the panels of tests/pcr_panel_cases.py.  Everything is compared as arrays, order included."""
import numpy as np
import pytest

import sharkmer_amd as sa
import pcr_panel_cases as pc
import pcr_ref as ref

pytestmark = pytest.mark.gpu


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a[:4], b[:4])) and a[4] == b[4]


def as_model(t):
    return [list(t[0]), list(t[1]), list(t[2]), list(t[3]), t[4]]


def check_jobs(eng, table, k, jobs, max_levels=0, what=None):
    """jobs: (nodes, dirs, min_count, cap, fringe_cap).  The panel call against each job alone and the model."""
    got = eng.neighborhood_panel(jobs, max_levels=max_levels)
    assert len(got) == len(jobs)
    for j, (job, g) in enumerate(zip(jobs, got)):
        nodes, dirs, mc, cap, fcap = job
        alone = eng.neighborhood(nodes, dirs, mc, max_levels=max_levels, cap=cap, fringe_cap=fcap)
        assert same(g, alone), (what, j, g[4], alone[4], len(g[0]), len(alone[0]))
        want = ref.neighborhood(nodes, dirs, table, k, mc, max_levels=max_levels, cap=cap, fringe_cap=fcap)
        assert as_model(g) == list(want), (what, j, g[4], want[4])
    return got


@pytest.fixture(scope="module")
def mixed(orc):
    p = pc.mixed_panel(orc)
    eng = sa.KmerEngine(p.k, 1, 100)
    eng.ingest_reads(p.bases, p.offsets)
    eng.finalize()
    yield p, eng
    eng.close()


def mixed_jobs(p, cap=1 << 14):
    """A job per gene of the mixed panel: the gene's seed graph as seeds (start nodes forward, end nodes backward) at the
    gene's lowest threshold — the first fetch of its last sweep step."""
    jobs = []
    for i, g in enumerate(p.genes):
        seed = ref.create_seed_graph(p.sets[2 * i][0], p.sets[2 * i + 1][0], p.k)
        jobs.append((seed.sub_kmer, seed.flags(), max(g.params["min_count"], g.params["table_min_count"]), cap, cap))
    return jobs


def test_mixed_panel_jobs(mixed):
    p, eng = mixed
    jobs = mixed_jobs(p)
    got = check_jobs(eng, p.table, p.k, jobs, what="mixed")
    assert sum(len(g[0]) > 800 for g in got) >= 6 and max(g[4] for g in got) > 1000  # chains, one workgroup each
    empty = pc.gene_index(p, "no set at all")
    assert len(jobs[empty][0]) == 0 and got[empty][4] == 0 and len(got[empty][0]) == 0
    a, b = pc.gene_index(p, "twin a"), pc.gene_index(p, "twin b")
    assert same(got[a], got[b])


def test_one_job_is_shk_neighborhood(mixed):
    p, eng = mixed
    for job in (mixed_jobs(p)[0], mixed_jobs(p, cap=300)[1]):
        (got,) = eng.neighborhood_panel([job])
        assert same(got, eng.neighborhood(job[0], job[1], job[2], cap=job[3], fringe_cap=job[4]))
        assert got[4] > 0
    assert eng.neighborhood_panel([]) == []


def test_wide_and_narrow_jobs():
    p = pc.wide_narrow_panel()
    with sa.KmerEngine(p.k, p.chunks, 10) as eng:
        for lane, keys, counts in p.inserts:
            eng.insert(keys, counts, chunk_id=lane)
        jobs = [(n, d, mc, 1 << 14, 1 << 12) for n, d, mc in p.jobs]
        got = check_jobs(eng, p.table, p.k, jobs, what="wide and narrow")
        assert all(len(g[2]) == 0 for g in got)  # every job complete
        check_jobs(eng, p.table, p.k, jobs, max_levels=3, what="wide and narrow, 3 levels")
        # a fringe_cap that rising's last level (1025) does not fit and flat1024's levels just do
        tight = [(n, d, mc, 1 << 14, 1024) for n, d, mc in p.jobs if len(n) <= 1024]
        check_jobs(eng, p.table, p.k, tight, what="fringe_cap 1024")


def test_many_jobs(orc):
    p = pc.many_jobs_panel(orc)
    with sa.KmerEngine(p.k, 1, 100) as eng:
        eng.ingest_reads(p.bases, p.offsets)
        eng.finalize()
        jobs = [(n, d, mc, 1024, 1024) for n, d, mc in p.jobs]
        got = check_jobs(eng, p.table, p.k, jobs, max_levels=p.max_levels, what="many")
        assert len(got) == 600 and sum(g[4] == p.max_levels for g in got) > 300


def test_capacities_limits_and_odd_seeds(mixed):
    p, eng = mixed
    jobs = mixed_jobs(p)
    ia, ib, ic = (pc.gene_index(p, n) for n in ("first threshold", "third step", "twin a"))
    A, B, C = jobs[ia], jobs[ib], jobs[ic]
    lv = ref.neighborhood_levels(A[0], A[1], p.table, p.k, A[2])
    need2 = len(lv[0][1]) + len(lv[1][1])  # |K_2|: what the second level's expansion brings the k-mers to
    assert len(lv) > 3 and len(lv[1][1]) > 0
    none = ([], [], 1, 64, 64)
    tight = (A[0], A[1], A[2], need2 - 1, A[4])
    got = check_jobs(eng, p.table, p.k, [tight, B, none, C], what="cap one short")
    assert got[0][4] == 1 and len(got[0][2]) > 0                    # A: dropped to level 1, fringe = level 1
    assert len(got[1][2]) == 0 and len(got[3][2]) == 0 and got[1][4] > 800 and got[3][4] > 800  # B, C complete
    assert got[2][4] == 0 and len(got[2][0]) == 0 and len(got[2][2]) == 0
    exact = (A[0], A[1], A[2], need2, A[4])
    assert check_jobs(eng, p.table, p.k, [exact, none, B], max_levels=2, what="cap exact")[0][4] == 2
    for ml in (1, 3):
        got = check_jobs(eng, p.table, p.k, [A, none, B, C], max_levels=ml, what=("max_levels", ml))
        assert [g[4] for g in got] == [ml, 0, ml, ml]
    # duplicate seeds, dir 3, and a zero capacity (level 0 comes back as the fringe)
    n0 = A[0][0]
    odd = ([n0, n0, n0], [1, 3, 2], A[2], 1 << 12, 1 << 12)
    zero = (B[0], B[1], B[2], 0, 64)
    got = check_jobs(eng, p.table, p.k, [odd, zero, C], what="odd seeds")
    assert got[1][4] == 0 and len(got[1][2]) == len(set(zip(B[0], B[1]))) > 0


def test_resume_from_the_fringe(mixed):
    """The pattern of test_truncation_and_resume: a panel call cut by its capacities, each job's fringe fed back as its
    seeds, until every job is complete — the union is the whole neighbourhood of the single call."""
    p, eng = mixed
    picks = [pc.gene_index(p, n) for n in ("first threshold", "second step", "twin b")]
    start = [mixed_jobs(p)[i] for i in picks]
    whole = [ref.neighborhood(j[0], j[1], p.table, p.k, j[2]) for j in start]
    union = [dict() for _ in start]
    sent = [set() for _ in start]
    seeds = [(list(j[0]), list(j[1])) for j in start]
    calls = 0
    while any(len(s[0]) for s in seeds):
        jobs = []
        for i, (fn, fd) in enumerate(seeds):
            for n, d in zip(fn, fd):
                sent[i].update((n, b) for b in (1, 2) if d & b)
            cap = max(200 + 50 * i, 8 * len(fn))  # (level 0 always fits then: every call gets further)
            jobs.append((fn, fd, start[i][2], cap, cap))
        got = eng.neighborhood_panel(jobs)
        for i, (gk, gc, gn, gd, gl) in enumerate(got):
            assert gl >= 1 or not len(jobs[i][0])
            union[i].update(zip(gk.tolist(), gc.tolist()))
            keep = [(x, y) for x, y in zip(gn.tolist(), gd.tolist()) if (x, y) not in sent[i]]
            seeds[i] = ([x for x, _ in keep], [y for _, y in keep])
        calls += 1
    assert calls >= 3
    for u, w in zip(union, whole):
        assert sorted(u) == w[0] and [u[x] for x in w[0]] == w[1]


def test_errors_name_the_job_and_leave_the_table_alone(mixed):
    p, eng = mixed
    mask = (1 << (2 * (p.k - 1))) - 1
    ok = ([5], [1], 1, 64, 64)
    before = (eng.export_table(), eng.histograms().copy())
    for bad, word in ((([5], [0], 1, 64, 64), "dir"), (([5], [4], 1, 64, 64), "dir"), (([mask + 1], [1], 1, 64, 64), "node"),
                      (([1, 2, 3], [1, 1, 3], 1, 64, 3), "fringe_cap")):
        with pytest.raises(sa.ShkError) as e:
            eng.neighborhood_panel([ok, ok, bad, ok])
        assert e.value.code == -2 and "job 2" in e.value.msg and word in e.value.msg, e.value.msg
    # decreasing seed_offsets and too many jobs: below the wrapper
    L, u64 = eng._L, np.uint64
    z8, z4, z1 = np.zeros(8, u64), np.zeros(8, np.uint32), np.zeros(8, np.uint8)
    off = np.array([0, 2, 1, 2], dtype=u64)
    caps = np.full(3, 2, dtype=u64)
    ones = z1 + 1
    rc = L.shk_neighborhood_panel(eng._h, z8.ctypes.data, ones.ctypes.data, off.ctypes.data, 3, z4.ctypes.data, 0,
                                  caps.ctypes.data, caps.ctypes.data, z8.ctypes.data, z4.ctypes.data, z8.ctypes.data,
                                  z8.ctypes.data, z1.ctypes.data, z8.ctypes.data, z4.ctypes.data)
    assert rc == -2 and "job 1" in eng._L.shk_last_error(eng._h).decode() and "seed_offsets" in eng._L.shk_last_error(eng._h).decode()
    rc = L.shk_neighborhood_panel(eng._h, None, None, None, 4097, None, 0, None, None, None, None, None, None, None, None, None)
    assert rc == -2 and "4097" in eng._L.shk_last_error(eng._h).decode()
    after = (eng.export_table(), eng.histograms())
    assert all(np.array_equal(np.sort(a), np.sort(b)) for a, b in zip(before[0], after[0])) and np.array_equal(before[1], after[1])
    assert same(eng.neighborhood_panel([ok])[0], eng.neighborhood(ok[0], ok[1], 1, cap=64, fringe_cap=64))  # still usable
    with sa.KmerEngine(p.k, 1, 100, n_owners=2, owner_id=1) as share:
        share.ingest_reads(p.bases, p.offsets)
        share.finalize()
        with pytest.raises(sa.ShkError) as e:
            share.neighborhood_panel([ok])
        assert e.value.code == -11 and "owner share" in e.value.msg
