"""The world of owner shares of tests/share_model.py and the plan of tests/test_gpu_share_sequences.py, pinned before
they judge the engine: the model's owner function is the library's, its shares together are the one-context LaneModel
of the same job at every observation of every default seed, a round that nobody absorbs leaves nothing but read
counters, the plan is a function of the seed and meets every position twice, and the refusals' texts are the ones the
sources print.  No GPU."""
import ctypes
import hashlib
import os

import numpy as np
import pytest

import share_model
from lane_model import LaneModel
from share_model import ShareWorld, owner_of
from test_gpu_fuzz import draw_reads

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAN_HASH = "e4f44673720138f7746d4d3654e4ba9a914cb6cc40f87af05289ecee538635c6"
DEFAULT_SEEDS_PINNED, N_POSITIONS_PINNED = 40, 17


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from sharkmer_amd.engine import lib_path
    L = ctypes.CDLL(lib_path())
    L.shk_key_owner.restype = ctypes.c_uint32
    L.shk_key_owner.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint64]
    return L


_dry = []


def dry_sequences(orc):
    """The default seeds' sequences applied to the model alone, once for the tests that read them."""
    import test_gpu_share_sequences as seq
    if not _dry:
        for seed in range(seq.DEFAULT_SEEDS):
            s = seq.dry_sequence(orc, seed)   # (every observation in it ran ShareWorld.check_union)
            s.model = None
            _dry.append(s)
    return _dry


@pytest.mark.parametrize("W", [1, 2, 4, 8])
def test_the_model_s_owner_is_shk_key_owner(lib, W):
    """On random keys for every k the sweep draws (and the two ends of the key space)."""
    import test_gpu_share_sequences as seq
    ks = sorted({seq.draw_plan(seed)[0]["k"] for seed in range(200)})
    assert ks == [9, 15, 17, 19, 21, 22, 23, 27, 31]
    for k in ks:
        rng = np.random.default_rng([20261021, k, W])
        keys = np.concatenate([rng.integers(0, 1 << (2 * k), size=3000, dtype=np.uint64), np.array([0, (1 << (2 * k)) - 1], dtype=np.uint64)])
        want = np.array([lib.shk_key_owner(k, W, x) for x in keys.tolist()], dtype=np.int64)
        assert np.array_equal(owner_of(k, W, keys), want), (k, W)
        assert W == 1 or len(set(want.tolist())) == W


def test_the_plan_is_a_function_of_the_seed():
    """Drawn twice, the same; and the default seeds' plans are the ones pinned here, so that a later change of the
    generator is deliberate (the hash is of the plans' repr)."""
    import test_gpu_share_sequences as seq
    h = hashlib.sha256()
    for seed in range(seq.DEFAULT_SEEDS):
        plan = seq.draw_plan(seed)
        assert plan == seq.draw_plan(seed)
        assert 6 <= len(plan[2]) <= 20 + 2   # (a poisoned round brings its reset's job with it)
        h.update(repr(plan).encode())
    assert (seq.DEFAULT_SEEDS, h.hexdigest()) == (DEFAULT_SEEDS_PINNED, PLAN_HASH)


def test_every_position_is_met_by_two_default_seeds(orc):
    """The positions follow from the draw alone.  Also a run of the sweep's own code: a draw the model refuses, or a
    world whose shares do not add up to the one-context model, fails here first."""
    import test_gpu_share_sequences as seq
    met = {}
    for seed, s in enumerate(dry_sequences(orc)):
        for item in s.met_here:
            met.setdefault(item, []).append(seed)
    assert len(seq.POSITIONS) == N_POSITIONS_PINNED
    missing = [p for p in seq.POSITIONS if len(met.get(p, ())) < 2]
    assert not missing, (missing, met)


def test_the_mutation_seeds_last_round_survives(orc):
    """The two harness-mutation tests of the GPU file change one segment of their seed's last round: it has records to
    lose (the model alone says so) and nothing resets after it."""
    import test_gpu_share_sequences as seq
    forms = set()
    for seed in seq.MUTATION_SEEDS:
        assert seq.mutation_survives(seed)
        s = seq.dry_sequence(orc, seed, mutate="withhold")
        assert s.mutated
        forms.add("wide" if not s.geom["record_bytes"] or s.ops[s.last_round][1]["form"] == "wide" else "owner")
    assert forms == {"wide", "owner"}


def test_the_union_of_the_shares_was_held_against_the_one_context_model(orc):
    """check_union ran at every observation of every dry run (it raises where the shares' summed histogram columns, the
    union of their exports or their summed totals differ from the LaneModel of the whole job); here: that it had the
    one-context model to compare with — a reset of one share alone takes it away until the next reset of all — on most
    seeds and at several observations each, in worlds of every size."""
    runs = dry_sequences(orc)
    checked = [s for s in runs if s.n_union_checks >= 2]
    assert 4 * len(checked) >= 3 * len(runs), [s.n_union_checks for s in runs]
    assert {s.W for s in checked} == {1, 2, 4, 8}


@pytest.mark.parametrize("W,k,chunks", [(1, 21, 3), (2, 9, 0), (4, 22, 10), (8, 31, 40)])
def test_a_world_of_shares_is_the_one_context_model(orc, W, k, chunks):
    """By hand, without the plan: two delivered rounds with a moved read index, a round nobody absorbs, a drop-mode
    ingest, inserts with foreign keys, count 0 and a count near saturation.  The shares add up; the dropped round left
    its reads in the scattering share's counters and nothing in any table; a foreign key looks up as 0."""
    rng = np.random.default_rng([7, W, k])
    world = ShareWorld(orc, k, chunks, 50, W)
    whole = LaneModel(orc, k, chunks, 50)
    batches = [draw_reads(np.random.default_rng([11, W, i]))[1:] for i in range(4)]
    batches = [(b[:int(o[min(len(o) - 1, 400)])], o[:min(len(o) - 1, 400) + 1]) for b, o in batches]
    for i, first in ((0, 0), (1, 12_345)):
        parcels = [world.scatter(s, *batches[i], first + 1000 * s) for s in range(W)]
        for p in parcels:
            world.deliver(p)
        for s in range(W):
            whole.set_read_index(first + 1000 * s)
            whole.ingest_reads(*batches[i])
    before = [s.export() for s in world.shares]
    world.scatter(W - 1, *batches[2], 5000)   # scattered and never absorbed
    for s, b in zip(world.shares, before):
        assert np.array_equal(s.export()[0], b[0]) and np.array_equal(s.export()[1], b[1])
    n = len(batches[0][1]) + len(batches[1][1]) - 2
    assert world.shares[W - 1].n_reads == n + len(batches[2][1]) - 1 and (W == 1 or world.shares[0].n_reads == n)
    world.drop_ingest(*batches[3], 999)
    whole.set_read_index(999)
    whole.ingest_reads(*batches[3])
    keys = rng.integers(0, 1 << (2 * k), size=200, dtype=np.uint64)
    counts = rng.integers(1, 9, size=200).astype(np.uint32)
    counts[0], counts[1] = 0, (1 << 31) + 5 if chunks <= 1 else 1 << 20
    world.insert(0, keys, counts)
    whole.insert(0, keys, counts)
    assert world.check_union()
    cols, uk, uc, tot, sat = world.union()
    w = whole.observe()
    assert np.array_equal(uk, w.keys) and np.array_equal(uc, w.counts) and np.array_equal(cols, w.columns.astype(object))
    assert tot == {f: whole.totals()[f] for f in share_model.KMER_TOTALS}
    own = owner_of(k, W, keys)
    for o, s in enumerate(world.shares):
        got = s.get_count(keys)
        assert not got[own != o].any() and np.array_equal(got[own == o], whole.get_count(keys[own == o]))
        s.finalize() if chunks == 0 or counts[0] else None   # (a share without reads of its own finalizes: no NO_READS)
    world.reset(0)
    assert len(world.shares[0].export()[0]) == 0 and world.shares[0].n_reads == 0
    assert world.whole_valid == (W == 1)
    ShareWorld(orc, k, chunks, 50, W).shares[0].finalize()   # an empty share does not fail with the no-reads text


def test_the_exchange_geometry_restated(orc):
    """xchg_geometry at the configurations tests/test_gpu_owner.py pins on the engine
    (test_exchange_feasibility_is_a_function_of_the_configuration): 4-byte records up to k = 21, 8-byte ones beyond, the
    wide round alone with more than 32 lanes at k > 21 or with SHK_XL64=0, and a level-1 fan-out that is the hook's."""
    g = lambda k, chunks, hooks={}, flags=0, W=4, hint=4_200_000: share_model.xchg_geometry(k, chunks, W, hint, flags, hooks)
    assert [g(k, 3)["record_bytes"] for k in (15, 21, 22, 31)] == [4, 4, 8, 8]
    assert g(31, 40)["record_bytes"] == 0
    assert [g(k, 3, {"SHK_XL64": "0"})["record_bytes"] for k in (21, 22, 31)] == [4, 0, 0]
    assert g(21, 3, flags=share_model.FLAG_FORCE_DIRECT)["record_bytes"] == 0
    for lvl1 in (5, 6, 8, 10):   # a share starts with the fan-out's pages: the layout does not follow the table's size
        for hint in (0, 20_000, 4_200_000):
            assert g(19, 3, {"SHK_LEVEL1_LOG": str(lvl1)}, hint=hint)["log_p1"] == lvl1
    assert g(21, 1)["region_cap"](1 << 17) == 2048 and g(21, 1, {"SHK_LEVEL1_LOG": "5"})["region_cap"](1 << 17) == 6144


def test_the_refusals_texts_are_the_ones_the_code_prints():
    src = "".join(open(os.path.join(ROOT, "sharkmer_amd", "csrc", f)).read() for f in ("shk_engine.hip", "shk_table_api.hip.h"))
    for text in share_model.REFUSAL_TEXTS:
        assert text in src, text
    hdr = open(os.path.join(ROOT, "include", "shk.h")).read()
    assert "take the wide round" in hdr

