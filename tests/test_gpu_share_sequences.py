"""A randomized sweep of CALL SEQUENCES on a world of OWNER SHARES against tests/share_model.py.

tests/test_gpu_sequences.py sweeps the calls of one context; tests/test_gpu_owner.py and tests/test_dist_gloo.py draw
configurations of the owner exchange and drive every one of them in the one order sharkmer_amd.dist.OwnerCounter uses
(rounds, one finalize, destroy).  The exchange entry points carry more state from call to call than anything else in
the engine — two exchange buffers taken in turn, a foreign spill list that stays between rounds, absorbed records
waiting for a page pass, a scatter launched in front of the previous absorb's outcome, a statistics copy pending
between shk_xchg_scatter_begin and _end, a table that may grow under an absorb — so here a seed draws a world of W
shares (W contexts on one card, one thread; the test is the transport) and 6-20 operations: rounds in the three forms
(the owner layout in one call or in two, the wide round) delivered at once or DEFERRED behind the next round's scatter,
skewed rounds that overflow a region, rounds that nobody absorbs, rounds with an invalid byte, drop-mode ingests,
inserts from host and device lists (foreign k-mers, count 0, near-saturating counts), resets of all shares or of one,
and between them every observation a share answers.  Each is applied to the engine and to the model in lockstep; every
comparison is integer equality, share by share, and after each observation the shares together — summed histogram
columns, the union of the tables, the summed k-mer totals — are held against the one-context LaneModel of the same job.

The transport: after a scatter has returned (the two-call form: after _end) every segment and its cursors, every wide
piece and every foreign spill list is CLONED into tensors of the test's own, which live until the absorbing context has
been finalized; absorbs and inserts read the clones.  A deferred round is absorbed behind the next round's scatter —
with the two-call form between _begin and _end, where OwnerCounter puts it — never later.

Between shk_xchg_scatter_begin and _end the transport launches the previous round's absorbs, as the header allows; where
the draw says so it also makes every other call there — each must be refused with SHK_ERR_STATE and the one text, and the
round behind it must come out exact.

SHK_SHARE_SEQ_SEEDS: how many seeds; SHK_SHARE_SEQ_FIRST: the first one.  A failing case prints its seed, its world,
its hooks and the operations applied so far: SHK_SHARE_SEQ_FIRST=<seed> SHK_SHARE_SEQ_SEEDS=1 replays it.
`dry_run(orc, seed)` runs the draw and the model without an engine (tests/test_share_model_cpu.py).

40 seeds from 0.  Positions follow from the draw alone and are checked without an engine
(tests/test_share_model_cpu.py: every one by at least two default seeds); the rarest are "zero-count insert_device"
(seeds 15, 25, 34, 35, 37), "reset between a scatter and its absorb" (0, 3, 4, 6, 19, 33) and "near-saturating count"
(3, 9, 20, 30, 31, 37, 38); "refused call between begin and end" is met by 0, 13, 14, 25, 28, 29, 30, 34 and 36.
The routes need the engine; on an MI355X: `grow` and `grew_alone` by seeds 2, 4 and 5 — the small worlds, which the
draw opens with one share handed more keys than its table takes — `insert_list` by 33 and 39, `absorb_spill` by 30, 31
and 39, `rec4` by 10 seeds, `rec8` by 12, `foreign_spill` by 21, `wide` by 33.  `late_settle` (14, 26, 30, 31, 34) is
the route's PRECONDITION, seen from outside — an owner-layout scatter on a context whose last call was an absorb, the
hook not 0 — since the engine reports nowhere whether it took the route: those seeds show that sequences which should
take it come out exact, not that it ran.  The file (40 sequences, the four harness mutations and the fixed tests)
takes 26.0 s there, tests/test_gpu_sequences.py 74.4 s on the same machine in the same session; a sequence takes 0.1
to 1.5 s."""
import os

import numpy as np
import pytest

import sharkmer_amd as sa
from lane_model import LaneModel, ModelError, SHK_ERR_STATE
from share_model import (IS_A_SHARE, KMER_TOTALS, NO_SCATTER_BEGUN, NOT_A_SHARE, SCATTER_BEGUN, TAKE_THE_WIDE_ROUND, ShareWorld, owner_of, xchg_geometry)
from test_gpu_fuzz import draw_reads
from test_gpu_sequences import PANEL, random_kmers, revcomp, _brief

pytestmark = pytest.mark.gpu

DEFAULT_SEEDS = 40
OVERRIDDEN = "SHK_SHARE_SEQ_SEEDS" in os.environ or "SHK_SHARE_SEQ_FIRST" in os.environ
N_SEEDS = int(os.environ.get("SHK_SHARE_SEQ_SEEDS", str(DEFAULT_SEEDS)))
FIRST = int(os.environ.get("SHK_SHARE_SEQ_FIRST", "0"))

SHK_ERR_INVALID_CHAR = -1
MAX_READS, MAX_BASES, ROUND_BASES = 800, 60_000, 1 << 17   # per rank and round; what every round's layout is sized for
SHARE_HOOKS = {"SHK_LEVEL1_LOG": ["5", "6", "8", "10"], "SHK_XL64": ["0"], "SHK_XCHG_LATE_SETTLE": ["0"], "SHK_ACC_MAX_MRECORDS": ["1"],
               "SHK_INSERT_PAGED_MIN": ["1"], "SHK_INSERT_PAGED": ["0"], "SHK_DEFER_BUDGET": ["20000", "300000"],
               "SHK_FUSED_HIST": ["0", "2"]}
HOOK_RATE, LEVEL1_RATE = 0.35, 0.6   # (a small level-1 fan-out is what lets a small hint's table grow at these sizes)
POSITIONS = ("observation between two rounds", "observation between a round's scatter and its deferred absorb",
             "reset between a scatter and its absorb", "absorb after the next scatter", "owner round after a wide round",
             "wide round after an owner round", "drop-mode ingest between two rounds", "insert_device with foreign keys",
             "zero-count insert_device", "near-saturating count", "dropped round followed by finalize",
             "poisoned round followed by reset and a job", "reset_one", "finalize twice", "round after finalize", "W = 1",
             "refused call between begin and end")
# foreign_spill: a scatter reported n_foreign_spilled > 0; absorb_spill: counters()["n_spilled"] rose over a stretch with an
# absorb in it; grow: n_grows > 0 on a share; grew_alone: the shares' table_capacity differed at a look and a round was delivered
# after it; rec4 / rec8 / wide: the records of a delivered round; late_settle: an owner-layout scatter on a context whose
# last call was an absorb, SHK_XCHG_LATE_SETTLE not 0 (the engine does not report the route: this is its precondition);
# insert_list: a wide round's piece on a FLAG_TIMING seed whose insert_device launched no k_insert (timings() before and after)
ROUTES = ("foreign_spill", "absorb_spill", "grow", "grew_alone", "rec4", "rec8", "wide", "late_settle", "insert_list")
RECORD = {"positions": {}, "routes": {}, "seeds": set()}
NAMES = ["round", "skewed_round", "dropped_round", "poisoned_round", "drop_ingest", "insert", "insert_device", "set_read_index",
         "reset_all", "reset_one", "finalize", "finalize_twice", "lookup", "export", "counters", "sync", "refusal", "find_oligos", "primer_kmers"]
WEIGHTS = np.array([5.0, 0.9, 0.8, 0.5, 1.2, 0.8, 1.2, 0.4, 0.6, 0.6, 2.5, 0.7, 1.2, 1.0, 0.8, 0.5, 0.7, 0.8, 0.6])
FORMS = ("owner", "owner2", "wide")


# ---- the draw: a pure function of the seed ---------------------------------------------------------------------

def draw_plan(seed):
    """→ (world, hooks, operations).  Operations are (name, parameters); data comes from the sub-seeds in the parameters
    when the operation is applied."""
    rng = np.random.default_rng(40_000 + seed)
    W = int(rng.choice([1, 2, 4, 8]))
    world = dict(W=W, k=int(rng.choice([9, 15, 17, 19, 21, 21, 22, 23, 27, 31])), chunks=int(rng.choice([0, 1, 3, 10, 16, 32, 40])),
                 histo_max=int(rng.choice([1, 5, 50, 300])), hint=int(rng.choice([0, 20_000, 600_000, 1_100_000, 4_200_000])),
                 flags=int(rng.choice([0, 0, sa.FLAG_FORCE_DIRECT, sa.FLAG_TIMING])))
    hooks = {}
    for name, values in SHARE_HOOKS.items():
        v = values[int(rng.integers(0, len(values)))]
        if rng.random() < (HOOK_RATE if name != "SHK_LEVEL1_LOG" else 1.0 if world["hint"] == 20_000 else LEVEL1_RATE):
            hooks[name] = v
    n_lanes = max(world["chunks"], 1)
    sub = lambda: int(rng.integers(1, 1 << 30))
    ops, queue = [], ["round"] if rng.random() < 0.7 else []
    # A small world — the smallest hint under a fan-out of 2^5 or 2^6: shares of 2^18 slots and fewer all told — opens with
    # the route "a share grew while a peer had not": a round, one share alone handed more keys of its own than its table
    # takes, a look at the counters, and a round between the grown share and the others.
    if W > 1 and world["hint"] == 20_000 and hooks.get("SHK_LEVEL1_LOG") in ("5", "6"):
        queue = ["round", "grow_one", "counters", "round"]
    for _ in range(int(rng.integers(6, 21))):
        name = queue.pop(0) if queue else NAMES[int(rng.choice(len(NAMES), p=WEIGHTS / WEIGHTS.sum()))]
        if name == "grow_one":
            ops.append(("insert_device", dict(r=sub(), lane=int(rng.integers(0, n_lanes)), n=200_000, zero=False, high=False,
                                              ranks=[int(rng.integers(0, W))], counted=bool(rng.random() < 0.5))))
            continue
        if name in ("round", "dropped_round", "poisoned_round"):
            empty = sorted(int(x) for x in rng.choice(W, size=int(rng.integers(1, max(W, 2))), replace=False)) if rng.random() < 0.3 else []
            p = dict(r=sub(), form=FORMS[int(rng.integers(0, 3))], first=int(rng.choice([0, 999, 1000, 12_345, 1_000_000_001])), empty=empty)
            if name != "poisoned_round":
                p["between"] = bool(rng.random() < 0.4)   # the two-call form: every refused call between _begin and _end
            if name == "round":
                p["defer"] = bool(rng.random() < 0.45)
            if name == "poisoned_round":
                p.update(rank=int(rng.integers(0, W)), byte=int(rng.choice(list(b"xRn-*@"))), then=str(rng.choice(["reset_one", "reset_all"])))
                p["empty"] = [x for x in empty if x != p["rank"]]
                queue = ["round", "finalize"]
        elif name == "skewed_round":
            p = dict(r=sub(), form=FORMS[int(rng.integers(0, 2))], first=int(rng.choice([0, 1000, 1_000_000_000])), rank=int(rng.integers(0, W)))
        elif name == "drop_ingest":
            p = dict(r=sub(), first=int(rng.choice([0, 999, 12_345])), route=str(rng.choice(["host", "device"])))
        elif name in ("insert", "insert_device"):
            p = dict(r=sub(), lane=int(rng.integers(0, n_lanes)), n=int(rng.choice([1, 7, 300, 5000])), zero=bool(rng.random() < 0.3),
                     high=bool(rng.random() < 0.3), ranks=None if rng.random() < 0.7 else [int(rng.integers(0, W))])
            if name == "insert_device":
                p["counted"] = bool(rng.random() < 0.75)   # False: d_counts = NULL, one occurrence each
                if p["ranks"] is not None and rng.random() < 0.6:
                    p["n"] = 60_000   # one share alone is handed a table's worth of keys: it grows, its peers do not
        elif name == "set_read_index":
            p = dict(index=int(rng.choice([0, 999, 1000, 12_345, 1_000_000_001])))
        elif name == "reset_one":
            p = dict(rank=int(rng.integers(0, W)))
        elif name in ("lookup", "refusal", "find_oligos", "primer_kmers"):
            p = dict(r=sub())
        else:
            p = {}
        ops.append((name, p))
    return world, hooks, ops


def rank_batch(r, rank):
    """Rank `rank`'s batch of the round with sub-seed r: a test_gpu_fuzz.py draw cut down to MAX_READS and MAX_BASES."""
    _, bases, offsets = draw_reads(np.random.default_rng([r, rank]))
    n = min(len(offsets) - 1, MAX_READS, int(np.searchsorted(offsets, MAX_BASES, side="right")) - 1)
    return np.ascontiguousarray(bases[:int(offsets[n])]), offsets[:n + 1].copy()


def skewed_batch(k, region_cap):
    """150-base reads of a two-base repeat: two canonical k-mers, each more often than a region holds (one lane: the
    batch lies inside one 1000-read block)."""
    per_read = (150 - k + 1) // 2
    n = min(-(-region_cap * 5 // 4 // per_read) + 4, 1000)
    bases = np.frombuffer(b"AC" * 75 * n, dtype=np.uint8)
    return bases, np.arange(n + 1, dtype=np.uint64) * np.uint64(150)


# ---- one sequence, applied to the engines and the model in lockstep ---------------------------------------------

class Sequence:
    def __init__(self, orc, seed, engine=True, mutate=None, plan=None):
        """mutate: ("withhold" | "twice") — the transport loses or repeats one segment of the plan's last round.
        plan: a (world, hooks, operations) written by hand instead of the seed's draw (the fixed tests)."""
        self.orc, self.seed, self.live, self.mutate = orc, seed, engine, mutate
        self.world, self.hooks, self.ops = plan or draw_plan(seed)
        self.W, self.k = self.world["W"], self.world["k"]
        self.n_lanes = max(self.world["chunks"], 1)
        self.geom = xchg_geometry(self.k, self.world["chunks"], self.W, self.world["hint"], self.world["flags"], self.hooks)
        self.done, self.met_here, self.routes = [], set(), set()
        self.n_union_checks = 0
        self.mutated = False
        self.last_round = max([i for i, (name, _) in enumerate(self.ops) if name in ("round", "skewed_round")], default=-1)
        self.model = ShareWorld(orc, self.k, self.world["chunks"], self.world["histo_max"], self.W)
        self.engs, self.keep = [], []
        self.pending = None       # a deferred round: (parcels, per destination rank the engine-side deliveries)
        self.trail = ""           # R: a delivered round (W wide, O owner layout beside it), o: observation, d: drop-mode ingest, f: finalize, x: dropped round
        self.after_poison = ""    # "", "reset", "job"
        self.last_call = [""] * self.W   # per context: "absorb" if that was its last engine call
        self.grows_differed = False
        self.spilled_seen = [0] * self.W
        self.absorbed_since_look = False
        self.nf = {}              # per rank: n_foreign_spilled of its last owner-layout scatter
        if self.W == 1:
            self.met_here.add("W = 1")

    def report(self, what=""):
        return "%s\nseed %d  hooks %s\nworld %s\noperations so far:\n  %s" % (
            what, self.seed, self.hooks, self.world, "\n  ".join("%s %s" % o for o in self.done))

    def same(self, got, want, what):
        if self.live:
            assert np.array_equal(got, want), self.report("%s: engine %s, model %s" % (what, _brief(got), _brief(want)))

    def refused(self, code, text, call, what, exact=False):
        if not self.live:
            return
        try:
            call()
        except sa.ShkError as e:
            assert e.code == code and (e.msg == text if exact else text in e.msg), self.report(
                "%s: [%d] %r, expected [%d] %r" % (what, e.code, e.msg, code, text))
        else:
            raise AssertionError(self.report("%s did not fail; expected [%d] %r" % (what, code, text)))

    def open(self):
        if self.live:
            w = self.world
            self.engs = [sa.KmerEngine(w["k"], w["chunks"], w["histo_max"], capacity_hint=w["hint"], flags=w["flags"], n_owners=self.W, owner_id=o)
                         for o in range(self.W)]
            for o, e in enumerate(self.engs):   # a function of the configuration: the model's restatement against the engine's answer
                assert e.xchg_feasible() == bool(self.geom["record_bytes"]), self.report(
                    "share %d: shk_xchg_feasible %s, the model's geometry %s" % (o, e.xchg_feasible(), self.geom))

    def close(self):
        if self.live:
            for e in self.engs:
                e.close()
            self.engs, self.keep = [], []

    def run(self):
        try:
            self.open()
            for i, (name, p) in enumerate(self.ops):
                self.at = i
                self.done.append((name, p))
                getattr(self, "op_" + name)(**p)
            self.at = len(self.ops)
            self.flush_pending()
            self.done.append(("finalize", {}))
            self.op_finalize()
        except ModelError as e:   # the draw asked the model for something it refuses: the test's own fault
            raise AssertionError(self.report("the model refused: %s" % e)) from e
        except sa.ShkError as e:
            raise AssertionError(self.report("the engine refused: %s" % e)) from e
        finally:
            self.close()

    # ---- the transport ------------------------------------------------------------------------------
    def device_batch(self, bases, offsets):
        import torch
        lo, hi = int(offsets[0]), int(offsets[-1])
        db = torch.from_numpy(bases[lo:hi].copy()).cuda() if hi > lo else torch.zeros(1, dtype=torch.uint8).cuda()
        do = torch.from_numpy((np.asarray(offsets) - offsets[0]).astype(np.int64)).cuda()
        self.keep += [db, do]
        return db.data_ptr(), do.data_ptr(), len(offsets) - 1, hi - lo

    def effective_form(self, form):
        """The owner layout where the geometry cannot take it: the refusal is checked, the round goes the wide way."""
        if form != "wide" and not self.geom["record_bytes"]:
            if self.live:
                self.refused(SHK_ERR_STATE, TAKE_THE_WIDE_ROUND, lambda: self.engs[0].xchg_scatter_tensors(0, 0, 0, 0, ROUND_BASES),
                             "owner-layout scatter on a geometry that cannot take it")
            return "wide"
        return form

    def scatter_round(self, form, batches, firsts, poisoned=None, between=False):
        """Every rank scatters its batch (None: it has none) → (parcels, deliveries): the model's side and, per
        destination rank, what the transport holds for it — ("seg", records, cursors, layout) or ("list", k-mers, lanes,
        counts) clones.  A deferred round from before is absorbed behind these scatters.  poisoned: (rank, text)."""
        import torch
        form = self.effective_form(form)
        if between and form == "owner2":
            self.met_here.add("refused call between begin and end")
        parcels, deliveries = [], [[] for _ in range(self.W)]
        before, self.pending = self.pending, None
        if before is not None:
            self.met_here.add("absorb after the next scatter")
        for s in range(self.W):
            b = batches[s]
            ok = poisoned is None or poisoned[0] != s
            if b is not None and ok:
                parcels.append(self.model.scatter(s, b[0], b[1], firsts[s]))
            if not self.live:
                continue
            eng = self.engs[s]
            args = (0, 0, 0, 0)
            if b is not None:
                eng.set_read_index(firsts[s])
                args = self.device_batch(*b)
            if form == "wide":
                if b is None:
                    continue
                if not ok:
                    self.refused(SHK_ERR_INVALID_CHAR, poisoned[1], lambda: eng.xchg_wide_scatter_tensors(*args), "wide scatter of a batch with an invalid byte", exact=True)
                    continue
                km, ln, counts = eng.xchg_wide_scatter_tensors(*args)
                self.last_call[s] = "scatter"
                at = 0
                for d in range(self.W):
                    if counts[d]:
                        deliveries[d].append(("list", km[at:at + counts[d]].clone(), ln[at:at + counts[d]].clone(), None, s))
                    at += counts[d]
                self.same(sum(counts), sum(parcels[-1].occurrences(d) for d in range(self.W)), "wide scatter of rank %d: k-mers" % s)
                continue
            if self.last_call[s] == "absorb" and self.hooks.get("SHK_XCHG_LATE_SETTLE") != "0":
                self.routes.add("late_settle")
            if form == "owner":
                if not ok:
                    self.refused(SHK_ERR_INVALID_CHAR, poisoned[1], lambda: eng.xchg_scatter_tensors(*args, ROUND_BASES), "scatter of a batch with an invalid byte", exact=True)
                    continue
                rec, cur, lay, nf = eng.xchg_scatter_tensors(*args, ROUND_BASES)
            else:
                rec, cur, lay = eng.xchg_scatter_begin_tensors(*args, ROUND_BASES)
                if before is not None:   # where OwnerCounter puts the previous round's absorbs (lists go through insert_device: after _end)
                    self.deliver_to(s, [it for it in before[1][s] if it[0] == "seg"])
                if between:
                    self.refused_between(s, b)
                if not ok:
                    self.refused(SHK_ERR_INVALID_CHAR, poisoned[1], eng.xchg_scatter_end, "the end of a scatter of a batch with an invalid byte", exact=True)
                    continue
                nf = eng.xchg_scatter_end()
                if before is not None:
                    self.deliver_to(s, [it for it in before[1][s] if it[0] != "seg"])
            self.last_call[s] = "scatter"
            self.same((lay.log_p1, lay.record_bytes or 4, lay.region_cap), (self.geom["log_p1"], self.geom["record_bytes"], self.geom["region_cap"](ROUND_BASES)),
                      "layout of rank %d (level-1 bits, record bytes, region capacity)" % s)
            S, G = lay.segment_records, lay.regions
            for d in range(self.W):
                deliveries[d].append(("seg", rec[d * S:(d + 1) * S].clone(), cur[d * G:(d + 1) * G].clone(), lay, s))
            if nf:   # the foreign spill list: to every rank, the scattering one included (it may own what overflowed)
                self.routes.add("foreign_spill")
                lists = [t.clone() for t in eng.xchg_spill_tensors()]
                self.same(lists[0].numel(), nf, "foreign spill list of rank %d: entries" % s)
                eng.xchg_spill_clear()
                for d in range(self.W):
                    deliveries[d].append(("list", lists[0], lists[1], lists[2], s))
            self.nf[s] = nf
        if self.live:
            torch.cuda.synchronize()   # the clones are complete before any context's stream reads them
            if before is not None and form != "owner2":
                for d in range(self.W):
                    self.deliver_to(d, before[1][d])
        if before is not None:
            self.land(before[0])
        return form, parcels, deliveries

    def refused_between(self, s, b):
        """Every call but the allowed ones (include/shk.h) between shk_xchg_scatter_begin and _end: SHK_ERR_STATE with the
        one text, the context as it was — the _end that follows and the round behind it are checked like any other."""
        import torch
        eng = self.engs[s]
        tiny = (np.frombuffer(b"ACGTACGTACGTACGTACGTACGTACGTACGTACGT", dtype=np.uint8), np.array([0, 36], dtype=np.uint64))
        one, lane = torch.ones(1, dtype=torch.int64).cuda(), torch.zeros(1, dtype=torch.int32).cuda()
        self.keep += [one, lane]
        calls = (("finalize", eng.finalize), ("sync", eng.sync), ("histograms", eng.histograms), ("counters", eng.counters),
                 ("lookup", lambda: eng.lookup(np.array([1], dtype=np.uint64))), ("export_table", eng.export_table),
                 ("ingest_reads", lambda: eng.ingest_reads(*tiny)), ("ingest_reads_device", lambda: eng.ingest_reads_device(*self.device_batch(*tiny))),
                 ("insert", lambda: eng.insert(np.array([1], dtype=np.uint64), np.array([1], dtype=np.uint32))),
                 ("insert_device", lambda: eng.insert_tensors(one, lane, None)), ("xchg_spill", eng.xchg_spill), ("xchg_spill_clear", eng.xchg_spill_clear),
                 ("xchg_wide_scatter_device", lambda: eng.xchg_wide_scatter_device(0, 0, 0, 0)),
                 ("xchg_scatter_begin", lambda: eng.xchg_scatter_begin(0, 0, 0, 0, ROUND_BASES)),
                 ("xchg_scatter_device", lambda: eng.xchg_scatter_device(0, 0, 0, 0, ROUND_BASES)),
                 ("set_read_index", lambda: eng.set_read_index(5)), ("find_oligos", lambda: eng.find_oligos(np.array([1], dtype=np.uint64), 3)),
                 ("table_geometry", eng.table_geometry), ("timings", eng.timings), ("retained_info", eng.retained_info))
        for what, call in calls:
            self.refused(SHK_ERR_STATE, SCATTER_BEGUN, call, "%s between xchg_scatter_begin and _end on share %d" % (what, s), exact=True)
        assert eng.xchg_feasible() and eng.stream()   # (two of the calls that stay allowed)

    def deliver_to(self, d, items):
        """Rank d absorbs what the transport holds for it (poisoned contexts are not handed anything: the round is dropped)."""
        eng = self.engs[d]
        for item in items:
            self.keep.append(item)
            if item[0] == "seg":
                eng.xchg_absorb_tensors(item[1], item[2], item[3])
                self.last_call[d] = "absorb"
                self.absorbed_since_look = True
                self.routes.add("rec%d" % (item[3].record_bytes or 4))
            else:
                timed = item[3] is None and self.world["flags"] & sa.FLAG_TIMING
                before = eng.timings().get("insert", (0, 0))[1] if timed else 0
                eng.insert_tensors(item[1], item[2], item[3])
                self.last_call[d] = "insert"
                if item[3] is None:
                    self.routes.add("wide")
                if timed and eng.timings().get("insert", (0, 0))[1] == before:
                    self.routes.add("insert_list")

    def land(self, parcels):
        """The model's side of a delivery, and where in the world's life it fell."""
        for p in parcels:
            self.model.deliver(p)
        if "f" in self.trail:
            self.met_here.add("round after finalize")
        last = self.trail.rfind("R")
        if last >= 0 and "o" in self.trail[last:]:
            self.met_here.add("observation between two rounds")
        if last >= 0 and "d" in self.trail[last:]:
            self.met_here.add("drop-mode ingest between two rounds")
        if self.grows_differed:
            self.routes.add("grew_alone")
        if self.after_poison == "reset":
            self.after_poison = "job"
        self.trail += "R"

    def deliver_round(self, form, parcels, deliveries, defer):
        kind = "W" if form == "wide" else "O"
        prev = [c for c in self.trail if c in "WO"]
        if prev and prev[-1] != kind:
            self.met_here.add("owner round after a wide round" if kind == "O" else "wide round after an owner round")
        if self.mutate and self.at == self.last_round:   # the harness's own mutation: the segment with the most records
            by_rank = {p.rank: p for p in parcels}
            src, dst = max(((r, d) for r in by_rank for d in range(self.W)), key=lambda sd: by_rank[sd[0]].occurrences(sd[1]), default=(-1, -1))
            assert src >= 0 and by_rank[src].occurrences(dst) > 0, self.report("nothing to mutate in the last round")
            self.mutated = True
            if self.live:   # the ENGINE's side is mutated; the model delivers the round as it was scattered
                items = [it for it in deliveries[dst] if it[4] == src]
                deliveries[dst] = [it for it in deliveries[dst] if it[4] != src] + (items * 2 if self.mutate == "twice" else [])
        if defer:
            self.pending = (parcels, deliveries)
            self.trail += kind
            return
        if self.live:
            for d in range(self.W):
                self.deliver_to(d, deliveries[d])
        self.trail += kind
        self.land(parcels)

    def flush_pending(self):
        if self.pending is not None:
            parcels, deliveries = self.pending
            self.pending = None
            if self.live:
                for d in range(self.W):
                    self.deliver_to(d, deliveries[d])
            self.land(parcels)

    # ---- rounds -----------------------------------------------------------------------------------
    def round_batches(self, r, empty):
        batches = [None if s in empty else rank_batch(r, s) for s in range(self.W)]
        return [None if b is None or len(b[1]) < 2 else b for b in batches]

    def op_round(self, r, form, first, empty, defer, between=False):
        firsts = [first + 1000 * s for s in range(self.W)]
        form, parcels, deliveries = self.scatter_round(form, self.round_batches(r, empty), firsts, between=between)
        self.deliver_round(form, parcels, deliveries, defer)

    def op_skewed_round(self, r, form, first, rank):
        cap = self.geom["region_cap"](ROUND_BASES)
        batches = self.round_batches(r, [])
        batches[rank] = skewed_batch(self.k, cap)
        form, parcels, deliveries = self.scatter_round(form, batches, [first + 1000 * s for s in range(self.W)])
        hot = max(int(c.max()) for p in parcels if p.rank == rank for part in p.per_owner for _, _, c in part)
        if form != "wide":   # the precondition, then the route
            assert hot > cap, self.report("the skewed batch's hottest k-mer occurs %d times, a region holds %d" % (hot, cap))
            if self.live:
                assert self.nf[rank] > 0, self.report("a k-mer with %d occurrences in one lane did not overflow its region of %d" % (hot, cap))
        self.deliver_round(form, parcels, deliveries, False)

    def op_dropped_round(self, r, form, first, empty, between=False):
        """Every rank scatters and nobody absorbs — what a caller is left with when a peer failed: the read and base
        counters of the scattering shares are all that remains (the spill lists were cleared with the round)."""
        self.scatter_round(form, self.round_batches(r, empty), [first + 1000 * s for s in range(self.W)], between=between)
        self.trail += "x"

    def op_poisoned_round(self, r, form, first, empty, rank, byte, then):
        self.flush_pending()   # (a poisoned context absorbs nothing: the round before is delivered first)
        batches = self.round_batches(r, empty)
        b = batches[rank] if batches[rank] is not None else (np.frombuffer(b"ACGTACGTACGTACGTACGTACGTACGTACGTACGT", dtype=np.uint8), np.array([0, 36], dtype=np.uint64))
        bases = b[0].copy()
        bases[int(np.random.default_rng(r).integers(int(b[1][0]), int(b[1][-1])))] = byte
        batches[rank] = (bases, b[1])
        text = LaneModel.bad_byte_message(byte)
        assert LaneModel.first_bad_byte(bases, [int(x) for x in b[1]]) == byte
        form = self.scatter_round(form, batches, [first + 1000 * s for s in range(self.W)], poisoned=(rank, text))[0]
        if self.live:   # the same code and text from every later call, until its reset
            import torch
            eng = self.engs[rank]
            one = torch.ones(1, dtype=torch.int64).cuda()
            lane = torch.zeros(1, dtype=torch.int32).cuda()
            for what, call in (("finalize", eng.finalize), ("sync", eng.sync), ("insert_device", lambda: eng.insert_tensors(one, lane, None)),
                               ("ingest_reads", lambda: eng.ingest_reads(*b)), ("scatter", lambda: eng.xchg_scatter_tensors(0, 0, 0, 0, ROUND_BASES) if form != "wide"
                                                                               else eng.xchg_wide_scatter_tensors(*self.device_batch(*b))), ("finalize", eng.finalize)):
                self.refused(SHK_ERR_INVALID_CHAR, text, call, "%s on a poisoned share" % what, exact=True)
        self.trail += "x"
        self.done.append((then, dict(rank=rank) if then == "reset_one" else {}))
        if then == "reset_one":
            self.op_reset_one(rank)
        else:
            self.op_reset_all()
        self.after_poison = "reset"

    # ---- other mutations ------------------------------------------------------------------------------
    def op_drop_ingest(self, r, first, route):
        bases, offsets = rank_batch(r, 0)
        self.model.drop_ingest(bases, offsets, first)
        if self.live:
            for s, eng in enumerate(self.engs):
                eng.set_read_index(first)
                if route == "host":
                    eng.ingest_reads(bases, offsets)
                else:
                    eng.ingest_reads_device(*self.device_batch(bases, offsets))
                self.last_call[s] = "ingest"
        self.trail += "d"

    def insert_list(self, r, n, zero, high):
        rng = np.random.default_rng(r)
        have = self.model.union()[1]
        new = random_kmers(rng, self.k, n)
        new = np.minimum(new, revcomp(new, self.k))
        keys = np.concatenate([new, have[rng.integers(0, len(have), size=n // 2)]]) if len(have) else new
        keys = keys[rng.permutation(len(keys))]
        counts = np.ones(len(keys), dtype=np.uint32)
        some = rng.random(len(keys)) < 0.5
        counts[some] = rng.integers(2, 50, size=int(some.sum()))
        if high:   # (more than one lane: counts that the sequence's inserts cannot carry to u32::MAX — Σ lane counts would
            counts[rng.random(len(keys)) < 0.1] = (1 << 31) + 5 if self.n_lanes == 1 else 1 << 20   # differ from Σ merged counts, io.rs:1042-1047)
            counts[0] = (1 << 31) + 5 if self.n_lanes == 1 else 1 << 20
            self.met_here.add("near-saturating count")
        if zero:
            counts[-1:] = 0
        return keys, counts

    def op_insert(self, r, lane, n, zero, high, ranks):
        keys, counts = self.insert_list(r, n, zero, high)
        self.model.insert(lane, keys, counts, ranks)
        if self.live:
            for s in range(self.W) if ranks is None else ranks:
                self.engs[s].insert(keys, counts, chunk_id=lane)
                self.last_call[s] = "insert"

    def op_insert_device(self, r, lane, n, zero, high, ranks, counted):
        keys, counts = self.insert_list(r, n, zero and counted, high and counted)
        if not counted:
            counts = np.ones(len(keys), dtype=np.uint32)
        self.model.insert(lane, keys, counts, ranks)
        if self.W > 1 and (self.model.owner_of(keys) != (0 if ranks is None else ranks[0])).any():
            self.met_here.add("insert_device with foreign keys")
        if zero and counted:
            self.met_here.add("zero-count insert_device")
        if self.live:
            import torch
            dk = torch.from_numpy(keys.view(np.int64).copy()).cuda()
            dl = torch.full((len(keys),), lane, dtype=torch.int32).cuda()
            dc = torch.from_numpy(counts.view(np.int32).copy()).cuda() if counted else None
            self.keep += [dk, dl, dc]
            for s in range(self.W) if ranks is None else ranks:
                self.engs[s].insert_tensors(dk, dl, dc)
                self.last_call[s] = "insert"

    def op_set_read_index(self, index):
        for s in self.model.shares:
            s.set_read_index(index)
        if self.live:
            for eng in self.engs:
                eng.set_read_index(index)

    def op_reset_all(self):
        if self.pending is not None:
            self.met_here.add("reset between a scatter and its absorb")
        self.model.reset()
        if self.live:
            for s, eng in enumerate(self.engs):
                eng.reset()
                self.last_call[s] = "reset"
            self.spilled_seen = [0] * self.W
        self.trail, self.grows_differed = "", False

    def op_reset_one(self, rank):
        if self.pending is not None:
            self.met_here.add("reset between a scatter and its absorb")
        self.model.reset(rank)
        if self.live:
            self.engs[rank].reset()
            self.last_call[rank] = "reset"
            self.spilled_seen[rank] = 0
        self.met_here.add("reset_one")

    # ---- observations -----------------------------------------------------------------------------------
    def observed(self):
        if self.pending is not None:
            self.met_here.add("observation between a round's scatter and its deferred absorb")
        self.trail += "o"
        try:
            if self.model.check_union():
                self.n_union_checks += 1
        except AssertionError as e:
            raise AssertionError(self.report("the model's shares against the one-context model: %s" % e)) from e

    def look_at_counters(self, s, c):
        if c["n_grows"]:
            self.routes.add("grow")
        if c["n_spilled"] > self.spilled_seen[s] and self.absorbed_since_look:
            self.routes.add("absorb_spill")
        self.spilled_seen[s] = c["n_spilled"]

    def op_counters(self):
        if self.live:
            grows = []
            for s, (eng, m) in enumerate(zip(self.engs, self.model.shares)):
                c = eng.counters()
                for f, v in (("n_reads_ingested", m.n_reads), ("n_bases_read", m.n_bases_read), ("n_bases_ingested", m.n_bases_ingested)):
                    assert c[f] == v, self.report("share %d counter %s: engine %d, model %d" % (s, f, c[f], v))
                self.look_at_counters(s, c)
                grows.append(c["table_capacity"])
            self.grows_differed |= len(set(grows)) > 1
            self.absorbed_since_look = False
        self.observed()

    def op_finalize(self):
        all_fine, hist_sum, tot_sum = True, None, dict.fromkeys(KMER_TOTALS, 0)
        grows = []
        for s, m in enumerate(self.model.shares):
            try:
                m.finalize()
                expected = None
            except ModelError as e:   # a key with merged count 0 (io.rs:1127-1132): the share reports its own numbers
                expected = str(e)
                assert "unique kmers in the histogram" in expected and self.world["chunks"] > 0, self.report("the draw led to: " + expected)
            all_fine &= expected is None
            if not self.live:
                continue
            eng = self.engs[s]
            if expected is None:
                eng.finalize()
            else:
                self.raises_text(expected, eng.finalize, s)
            self.last_call[s] = "finalize"
            h = eng.histograms()
            self.same(h, m.columns(), "histograms of share %d" % s)
            c, want = eng.counters(), m.totals()
            for f, v in want.items():
                assert c[f] == v, self.report("share %d counter %s: engine %d, model %d" % (s, f, c[f], v))
            self.look_at_counters(s, c)
            grows.append(c["table_capacity"])
            hist_sum = h.astype(object) if hist_sum is None else hist_sum + h.astype(object)
            for f in KMER_TOTALS:
                tot_sum[f] += c[f]
        if self.live:
            self.grows_differed |= len(set(grows)) > 1
            self.absorbed_since_look = False
            if self.pending is None:
                self.keep = []   # every context has been waited for: nothing reads the clones any more
            if self.model.whole_valid:   # the engines' shares together against the one-context model
                self.same(hist_sum, self.model.whole.columns().astype(object), "Σ shares' histograms against the one-context model")
                wt = self.model.whole.totals()
                self.same([tot_sum[f] for f in KMER_TOTALS], [wt[f] for f in KMER_TOTALS], "Σ shares' k-mer totals against the one-context model")
        self.observed()
        if all_fine:
            if "x" in self.trail and self.trail.rstrip("of").endswith("x"):
                self.met_here.add("dropped round followed by finalize")
            if self.after_poison == "job":
                self.met_here.add("poisoned round followed by reset and a job")
                self.after_poison = ""
            self.trail += "f"
        return all_fine

    def raises_text(self, text, call, s):
        try:
            call()
        except sa.ShkError as e:
            assert e.msg == text, self.report("finalize of share %d: message %r, expected %r" % (s, e.msg, text))
        else:
            raise AssertionError(self.report("finalize of share %d did not fail; expected %r" % (s, text)))

    def op_finalize_twice(self):
        if self.op_finalize() & self.op_finalize():
            self.met_here.add("finalize twice")

    def op_lookup(self, r):
        """Own and foreign keys: an owned key gives its count, a foreign one 0."""
        rng = np.random.default_rng(r)
        have = self.model.union()[1]
        keys = [random_kmers(rng, self.k, 40), np.array([0, (1 << (2 * self.k)) - 1], dtype=np.uint64)]
        if len(have):
            some = have[rng.integers(0, len(have), size=300)]
            keys += [some, revcomp(some[:100], self.k)]
        keys = np.concatenate(keys)
        for s, m in enumerate(self.model.shares):
            for canonical in (False, True):
                want = m.get_count(keys, canonical)
                if self.live:
                    self.same(self.engs[s].lookup(keys, canonical), want, "lookup on share %d, canonical=%s" % (s, canonical))
                    self.last_call[s] = "lookup"
        self.observed()

    def op_export(self):
        got = []
        for s, m in enumerate(self.model.shares):
            if self.live:
                got.append(self.engs[s].export_table())
                self.same(got[-1], m.export(), "export of share %d" % s)
                self.last_call[s] = "export"
        if self.live and self.model.whole_valid:
            keys, counts = np.concatenate([g[0] for g in got]), np.concatenate([g[1] for g in got])
            order = np.argsort(keys, kind="stable")
            self.same((keys[order], counts[order]), self.model.whole.export(), "the union of the shares' exports against the one-context model")
        self.observed()

    def op_find_oligos(self, r):
        """shk_find_oligos on every share: the k-mers of ITS table that begin or end with an oligo."""
        rng = np.random.default_rng(r)
        k = self.k
        L = int(rng.integers(1, k))
        have = self.model.union()[1]
        oligos = [random_kmers(rng, L, 2)]
        if len(have):
            some = have[rng.integers(0, len(have), size=4)]
            oligos += [some[:2] >> np.uint64(2 * (k - L)), revcomp(some[2:] & np.uint64((1 << (2 * L)) - 1), L)]
        oligos = np.unique(np.concatenate(oligos))
        min_count = int(rng.integers(1, 4))
        for s, m in enumerate(self.model.shares):
            wk, wc = m.find_oligos(oligos, L, min_count)
            if self.live:
                got = self.engs[s].find_oligos(oligos, L, min_count)
                order, worder = np.lexsort((got[1], got[0])), np.lexsort((wc, wk))
                self.same((got[0][order], got[1][order]), (wk[worder], wc[worder]), "find_oligos on share %d" % s)
                self.last_call[s] = "find_oligos"
        self.observed()

    def op_primer_kmers(self, r):
        """shk_primer_kmers on every share: get_primer_kmers over the k-mers it owns."""
        rng = np.random.default_rng(r)
        pair = PANEL[int(rng.integers(0, len(PANEL)))]
        params = dict(trim=int(rng.choice([0, 10, 12, 15, max(self.k - 1, 0), self.k + 3])), mismatches=int(rng.integers(0, 3)),
                      min_count=int(rng.integers(1, 3)), max_kmers=int(rng.choice([1, 40])))
        primers = [sa.Primer(s, **params) for s in pair[:int(rng.integers(1, 3))]]
        for s, m in enumerate(self.model.shares):
            want = m.primer_kmers(primers)
            if self.live:
                got = self.engs[s].primer_kmers(primers)
                self.same(len(got), len(want), "primer_kmers on share %d: primers" % s)
                for g, w, p in zip(got, want, primers):
                    for what, a, b in zip(("k-mers", "counts", "levels", "level hits"), g, w):
                        self.same(a, b, "primer_kmers %s of %s on share %d" % (what, p, s))
                self.last_call[s] = "primer_kmers"
        self.observed()

    def op_sync(self):
        if self.live:
            for s, eng in enumerate(self.engs):
                eng.sync()
                self.last_call[s] = "sync"

    def op_refusal(self, r):
        """One of the calls a share refuses, or that is refused for not being one; the sequence goes on as if it had not been made."""
        rng = np.random.default_rng(r)
        which, s = int(rng.integers(0, 3)), int(rng.integers(0, self.W))
        if not self.live:
            return
        if which == 0 and self.W > 1:
            for name, call in (("shk_neighborhood", lambda: self.engs[s].neighborhood([1], [1], 1)),
                               ("shk_pcr_extend", lambda: self.engs[s].pcr_extend((np.array([1], dtype=np.uint64), np.array([1], dtype=np.uint32)),
                                                                                  (np.array([2], dtype=np.uint64), np.array([1], dtype=np.uint32)), max_num_nodes=100))):
                self.refused(SHK_ERR_STATE, IS_A_SHARE % name, call, "%s on share %d" % (name, s), exact=True)
            gene = sa.PcrGene(gene_name="g", forward_seq=PANEL[0][0], reverse_seq=PANEL[0][1])
            # (shk_pcr_run is refused where its graph step opens: the text names that step)
            self.refused(SHK_ERR_STATE, IS_A_SHARE % "shk_pcr_extend_panel", lambda: self.engs[s].pcr_run([gene]), "shk_pcr_run on share %d" % s, exact=True)
        elif which == 1:
            self.refused(SHK_ERR_STATE, NO_SCATTER_BEGUN, self.engs[s].xchg_scatter_end, "xchg_scatter_end without a begin on share %d" % s, exact=True)
        else:
            with sa.KmerEngine(self.k, 1, 10) as plain:
                self.refused(SHK_ERR_STATE, NOT_A_SHARE, lambda: plain.xchg_wide_scatter_device(0, 0, 0, 0), "xchg_wide_scatter_device on a context that is no share", exact=True)
                assert not plain.xchg_feasible()


def dry_sequence(orc, seed, mutate=None):
    s = Sequence(orc, seed, engine=False, mutate=mutate)
    s.run()
    return s


def dry_run(orc, seed):
    """The draw and the model alone → the positions the seed meets (the routes need the engine)."""
    return dry_sequence(orc, seed).met_here


# ---- the sweep ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", range(FIRST, FIRST + N_SEEDS))
def test_random_call_sequence_on_a_world_of_shares(orc, monkeypatch, seed):
    s = Sequence(orc, seed)
    for name, v in s.hooks.items():
        monkeypatch.setenv(name, v)
    s.run()
    RECORD["seeds"].add(seed)
    for item in s.met_here:
        RECORD["positions"].setdefault(item, []).append(seed)
    for name in s.routes:
        RECORD["routes"].setdefault(name, []).append(seed)


# ---- the comparison bites: the transport itself goes wrong, no kernel does -----------------------------------------

MUTATION_SEEDS = (36, 39)   # the last round: owner-layout segments (two-call scatter, deferred) / the wide round's pieces; nothing resets after it


def mutation_survives(seed):
    """The plan's last round is there and no later operation takes its records away again."""
    ops = draw_plan(seed)[2]
    last = max([i for i, (name, _) in enumerate(ops) if name in ("round", "skewed_round")], default=-1)
    return last >= 0 and not any(name in ("reset_all", "reset_one", "poisoned_round") for name, _ in ops[last + 1:])


@pytest.mark.parametrize("seed", MUTATION_SEEDS)
@pytest.mark.parametrize("how", ["withhold", "twice"])
def test_a_segment_the_transport_loses_or_repeats_fails_the_comparison(orc, monkeypatch, how, seed):
    """The harness withholds one segment of the seed's last round, or delivers it twice: only counts change, and the
    sweep's own assertion (engine against model) must fail."""
    assert mutation_survives(seed)
    s = Sequence(orc, seed, mutate=how)
    for name, v in s.hooks.items():
        monkeypatch.setenv(name, v)
    with pytest.raises(AssertionError, match=r"engine .*, model ") as err:
        s.run()
    assert s.mutated and "seed %d" % seed in str(err.value)


# ---- fixed sequences: what the sweep found ------------------------------------------------------------------------

@pytest.mark.parametrize("n_owners", [0, 1, 2])
def test_insert_device_with_a_count_of_zero_creates_the_entry_seed_25(orc, n_owners):
    """Found by the sweep (seed 25: a world of one share, 40 lanes, a job and then insert_device with one count of 0,
    finalize): shk_insert_counts notes that a key may sit in the table with count 0, so that finalize takes occupancy from
    the keys and fails as io.rs:1127-1132 does; shk_insert_device created the same entry and noted nothing — its finalize
    took occupancy from the counts, reported one unique k-mer fewer than the table holds and succeeded.  Any context, share
    or not."""
    import torch
    keys = np.array([5, 9, 77, 9], dtype=np.uint64)
    if n_owners == 2:
        mine = np.arange(200, dtype=np.uint64)
        mine = mine[owner_of(21, 2, mine) == 0]   # (share 0's own keys: a foreign one is dropped, whatever its count)
        keys = mine[[0, 1, 2, 1]]
    counts = np.array([3, 0, 1, 0], dtype=np.uint32)
    model = LaneModel(orc, 21, 2, 5)
    model.insert(1, keys, counts)
    with sa.KmerEngine(21, 2, 5, n_owners=n_owners) as eng:
        eng.insert_tensors(torch.from_numpy(keys.view(np.int64)).cuda(), torch.ones(4, dtype=torch.int32).cuda(), torch.from_numpy(counts.view(np.int32)).cuda())
        with pytest.raises(ModelError) as want:
            model.finalize()
        with pytest.raises(sa.ShkError) as got:
            eng.finalize()
        assert got.value.msg == str(want.value) == "The total count of unique kmers in the histogram (2) does not equal the total count of hashed kmers (3)"
        assert np.array_equal(eng.histograms(), model.columns())
        c, t = eng.counters(), model.totals()
        assert {f: c[f] for f in KMER_TOTALS} == {f: t[f] for f in KMER_TOTALS}
        assert all(np.array_equal(a, b) for a, b in zip(eng.export_table(), model.export()))
        assert list(eng.lookup(keys[:3])) == [3, 0, 1]


@pytest.mark.parametrize("k", [17, 21])
def test_a_share_that_grew_alone_takes_its_peers_rounds(orc, monkeypatch, k):
    """The route of the sweep's small worlds (seeds 2, 4 and 5 there), fixed: a hint of 20 000 and a fan-out of 2^5 leave
    two shares with 2^17 slots each, share 0 alone is handed 10^5 keys of its own and grows, and then rounds in all three
    forms — at once and deferred — go between the grown share and the one that did
    not grow, 4-byte records (k = 17) and 8-byte ones (k = 21).  shk_xchg_absorb refuses a layout whose log_p1 is not
    the receiver's: it is the fan-out on both from shk_create on (include/shk.h), so nothing is refused and the result
    is the model's."""
    world = dict(W=2, k=k, chunks=3, histo_max=50, hint=20_000, flags=0)
    rounds = [("round", dict(r=101 + i, form=form, first=first, empty=[], defer=defer))
              for i, (form, first, defer) in enumerate((("owner", 0, False), ("owner2", 999, True), ("wide", 12_345, True), ("owner2", 1000, False)))]
    ops = [("insert_device", dict(r=5, lane=1, n=200_000, zero=False, high=False, ranks=[0], counted=True)), ("counters", {})] + rounds + [("finalize", {}), ("export", {})]
    s = Sequence(orc, -1, plan=(world, {"SHK_LEVEL1_LOG": "5"}, ops))
    monkeypatch.setenv("SHK_LEVEL1_LOG", "5")
    s.run()
    assert {"grow", "grew_alone", "rec%d" % (4 if k == 17 else 8), "wide"} <= s.routes, s.routes


# ---- what the default seed set has to have met (last in the file: after the sweep) -----------------------------

def test_the_default_seeds_cover_every_position_and_route():
    if OVERRIDDEN:
        pytest.skip("SHK_SHARE_SEQ_SEEDS / SHK_SHARE_SEQ_FIRST are set: the coverage is a property of the default seed set")
    assert RECORD["seeds"] == set(range(DEFAULT_SEEDS)), "the sweep did not run (or not pass) on every default seed"
    missing = [p for p in POSITIONS if p not in RECORD["positions"]] + ["route " + r for r in ROUTES if r not in RECORD["routes"]]
    print("\n".join("%s: seeds %s" % kv for part in ("positions", "routes") for kv in sorted(RECORD[part].items())))
    assert not missing, (missing, RECORD)
