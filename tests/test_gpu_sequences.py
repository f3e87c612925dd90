"""A randomized sweep of CALL SEQUENCES on one context against the per-lane model of tests/lane_model.py.

test_gpu_fuzz.py draws the configuration and the input; every case there is create, ingest, finalize once, read,
destroy.  The engine is not a function of its input, though: it carries lazy state from call to call (a table that
whoever comes first after a reset has to clear, records still waiting for their page pass, the histogram a fresh page
pass left behind, a dirty control block, keys inserted with count 0, the process-wide cache that hands a destroyed
context's blocks to the next one), and include/shk.h promises that none of it shows: finalize is idempotent and an
ingest re-opens the context, shk_reset gives the state right after shk_create, the sPCR read helpers leave the table
alone.  Here a seed draws the context (as test_gpu_fuzz.py does, plus SHK_FUSED_HIST, the multi-device context and a
life of two contexts) and 10-30 operations — ingests by every route, explicit chunks, a moved read index, inserts
(count 0 and near-saturating ones too), resets, and between them every observation the ABI has — which are applied
to the engine and to the model in lockstep.  Every comparison is integer equality.

shk_neighborhood and shk_pcr_extend are drawn by a second generator and interleaved, about one to five operations
(the first draw is what it was before they existed: tests/test_lane_model_cpu.py holds a hash of it).  They are
observations that settle, clear and may grow the table on their way (shk.h: "the table is not touched"): what is checked
is their own answer and, since the sequence goes on over a model they did not touch, every finalize, histogram column,
counter and export after them.

SHK_SEQ_SEEDS: how many seeds; SHK_SEQ_FIRST: the first one.  A failing case prints its seed, its context and the
operations applied so far (name + parameters): SHK_SEQ_FIRST=<seed> SHK_SEQ_SEEDS=1 replays it.  `dry_run(seed)`
runs the draw and the model without an engine (tests/test_lane_model_cpu.py checks the default set's coverage so)."""
import os

import numpy as np
import pytest

import sharkmer_amd as sa
from lane_model import LaneModel, ModelError, NO_READS, SHK_ERR_STATE, U32_MAX
from test_gpu_fuzz import HOOKS, draw_reads

pytestmark = pytest.mark.gpu

# 96 seeds from 0.  Positions and kinds follow from the draw alone and are checked without an engine
# (tests/test_lane_model_cpu.py): the rarest, "neighborhood after a zero-count insert", is met by seeds 17, 47 and 55,
# "neighborhood on a saturated count" by 12, 19, 24, 49, 73 and 93, the poison step and the saturated count by 8 seeds
# each.  The routes need the engine: on an MI355X the rarest, `histo_rows` (a job whose one fresh page pass is
# finalized as it is, on a FLAG_TIMING seed), was met by no seed of the first 48 and is met by seeds 25, 75 and 94 —
# a neighborhood call in front of such a finalize drops the fused histogram on purpose (seed 25's first job has one),
# and the three seeds still meet the route; `grow` by 11 seeds, `extend` by 16.
# The 96 sequences (and the fixed ones below) take 59.3 s there with the two graph observations, 53.9 s without them
# (the parent of the change that added them, same machine, same day), against 430 s for the rest of the GPU suite.
DEFAULT_SEEDS = 96
OVERRIDDEN = "SHK_SEQ_SEEDS" in os.environ or "SHK_SEQ_FIRST" in os.environ
N_SEEDS = int(os.environ.get("SHK_SEQ_SEEDS", str(DEFAULT_SEEDS)))
FIRST = int(os.environ.get("SHK_SEQ_FIRST", "0"))

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PANEL = [l.split("\t")[1:3] for l in open(os.path.join(G, "primer_panel_cnidaria.tsv")).read().splitlines()
         if l and not l.startswith("#")]
MAX_BASES = 2_000_000
PRE_FINALIZE = ("n_reads_ingested", "n_bases_read", "n_bases_ingested")
POSITIONS = ("observation before the first finalize", "observation between two ingests",
             "ingest after finalize, then a second finalize", "reset followed by a job", "finalize twice",
             "poison step", "two-context life", "zero-count insert", "saturated count",
             "neighborhood between two ingests", "neighborhood before the first finalize",
             "neighborhood after a zero-count insert", "neighborhood on a saturated count", "pcr_extend after a reset",
             "neighborhood refused on a multi-device context")
ROUTES = ("direct", "scatter", "pages", "histo", "histo_rows", "grow", "insert", "lookup", "export", "extend")
GRAPH_OPS = ("neighborhood", "pcr_extend")
GRAPH_SEED = 7_000_000   # the second generator: GRAPH_SEED + the sequence seed
GRAPH_RATE = 0.2
RECORD = {"positions": {}, "routes": {}, "kinds": {}, "seeds": set()}   # item → the seeds that met it


# ---- the draw: a pure function of the seed ---------------------------------------------------------------------

def draw_context(rng, kind=None):
    k = int(rng.choice([1, 2, 5, 9, 11, 13, 15, 16, 17, 19, 21, 21, 21, 22, 23, 25, 27, 29, 31, 31]))
    chunks = int(rng.choice([0, 1, 1, 2, 3, 7, 10, 16, 17, 40, 100, 129]))
    histo_max = int(rng.choice([1, 5, 50, 300]))
    flags = int(rng.choice([0, 0, 0, sa.FLAG_FORCE_DIRECT, sa.FLAG_FORCE_PAGED, sa.FLAG_DEFER_ERRORS]))
    hint = int(rng.choice([0, 0, 0, 20_000, 400_000, 1_100_000]))   # small or none: the table grows mid-life
    if kind is None:
        kind = str(rng.choice(["plain", "plain", "plain", "plain", "multi2", "multi4"]))
    return dict(k=k, chunks=chunks, histo_max=histo_max, flags=flags, hint=hint, kind=kind)


def draw_plan(seed):
    """→ (contexts, hooks, operations): draw_base_plan's, with the graph observations of the second generator after
    about every fifth operation (name + sub-seed: nodes and parameters come from the model's table when applied)."""
    contexts, hooks, base = draw_base_plan(seed)
    rng = np.random.default_rng(GRAPH_SEED + seed)
    ops = []
    for op in base:
        ops.append(op)
        if rng.random() < GRAPH_RATE:
            ops.append((GRAPH_OPS[int(rng.random() < 0.3)], dict(r=int(rng.integers(1, 1 << 30)))))
    return contexts, hooks, ops


def draw_base_plan(seed):
    """→ (contexts, hooks, operations).  Operations are (name, parameters); data comes from the sub-seeds in the
    parameters when the operation is applied.  What a context kind does not take is left out HERE: packed and device
    buffers on a multi-device context, near-saturating counts on more than one lane (Σ lane counts would differ from
    Σ merged counts: io.rs:1042-1047, a fourth expected error), oligos at k = 1."""
    rng = np.random.default_rng(20_000 + seed)
    ctx = draw_context(rng)
    if rng.random() < 1 / 3:
        ctx["flags"] |= sa.FLAG_TIMING
    hooks = {}
    for name, values in HOOKS.items():
        v = values[int(rng.integers(0, len(values)))]
        if v is not None and rng.random() < 0.6:   # a subset of a test_gpu_fuzz.py draw
            hooks[name] = v
    fused = [None, "0", "2"][int(rng.integers(0, 3))]
    if fused is not None:
        hooks["SHK_FUSED_HIST"] = fused
    contexts = [ctx]
    n_ops = int(rng.integers(10, 31))
    second_at = -1
    if rng.random() < 1 / 6:
        while True:
            c2 = draw_context(rng, kind=ctx["kind"])
            if (c2["k"], c2["chunks"], c2["hint"]) != (ctx["k"], ctx["chunks"], ctx["hint"]):
                break
        c2["flags"] |= ctx["flags"] & sa.FLAG_TIMING
        contexts.append(c2)
        second_at = int(rng.integers(3, n_ops - 2))
    poison_at = int(rng.integers(1, n_ops)) if rng.random() < 1 / 8 else -1
    pool = [int(x) for x in rng.integers(1, 1 << 30, size=3)]   # batches come back: later ingests meet earlier keys
    names = ["ingest", "ingest_batch", "set_read_index", "insert", "saturate", "reset", "finalize", "finalize_twice",
             "lookup", "export", "find_oligos", "primer_kmers", "filter_reads", "kmers_from_reads", "sync"]
    weight = np.array([5.0, 1.5, 0.7, 1.5, 0.8, 1.2, 3.0, 1.0, 1.5, 1.0, 1.0, 0.7, 0.5, 0.5, 0.7])
    ops = []
    job = lambda: ["ingest", "finalize"] if rng.random() < 0.5 else []   # a plain job first: one ingest, finalized as it is
    queue = job()
    for i in range(n_ops):
        if i == second_at:
            ctx = contexts[1]
            ops.append(("second_context", {}))
            queue = job()
        multi = ctx["kind"] != "plain"
        n_lanes = max(ctx["chunks"], 1)
        sub = lambda: int(rng.integers(1, 1 << 30))
        if i == poison_at:
            ops.append(("poison", dict(r=sub(), route="host" if multi else str(rng.choice(["host", "device"])),
                                       byte=int(rng.choice(list(b"xRn-*@"))), repeats=int(rng.integers(1, 3)))))
            continue
        w = weight.copy()
        if n_lanes != 1:
            w[names.index("saturate")] = 0
        if ctx["k"] < 2:
            w[names.index("find_oligos")] = 0
        name = queue.pop(0) if queue else names[int(rng.choice(len(names), p=w / w.sum()))]
        if name == "reset":
            queue = job()
        if name == "ingest":
            p = dict(r=pool[int(rng.integers(0, 3))] if rng.random() < 0.6 else sub(),
                     route="host" if multi else str(rng.choice(["host", "host", "packed", "device"])),
                     window=bool(rng.random() < 0.5))
        elif name == "ingest_batch":
            p = dict(r=pool[int(rng.integers(0, 3))] if rng.random() < 0.5 else sub(), chunk_id=int(rng.integers(0, n_lanes)))
        elif name == "set_read_index":
            p = dict(index=int(rng.choice([0, 999, 1000, 12_345, 1_000_000_001])))
        elif name == "insert":
            p = dict(r=sub(), chunk_id=int(rng.integers(0, n_lanes)), n=int(rng.choice([1, 7, 300, 5000])),
                     zero=bool(rng.random() < 0.12))
        elif name == "saturate":
            p = dict(r=sub(), short=int(rng.integers(0, 3)))
        elif name in ("lookup", "find_oligos", "primer_kmers", "filter_reads", "kmers_from_reads"):
            p = dict(r=sub())
        else:
            p = {}
        ops.append((name, p))
    return contexts, hooks, ops


def batch(r):
    shape, bases, offsets = draw_reads(np.random.default_rng(r))
    if int(offsets[-1]) > MAX_BASES:   # (the long reads)
        n = max(int(np.searchsorted(offsets, MAX_BASES, side="right")) - 1, 1)
        offsets = offsets[:n + 1]
        bases = bases[:int(offsets[-1])]
    return bases, offsets


def small_batch(r, n_max=60):
    bases, offsets = batch(r)
    n = min(len(offsets) - 1, n_max)
    return bases[:int(offsets[n])], offsets[:n + 1]


def revcomp(x, k):
    a = np.asarray(x, dtype=np.uint64)
    out = np.zeros_like(a)
    for _ in range(k):
        out = (out << np.uint64(2)) | (np.uint64(3) - (a & np.uint64(3)))
        a = a >> np.uint64(2)
    return out


def random_kmers(rng, k, n):
    return rng.integers(0, 1 << (2 * k), size=n, dtype=np.uint64)


# ---- where in a context's life things happened ----------------------------------------------------------------

class Positions:
    def __init__(self, met):
        self.met = met
        self.fresh()

    def fresh(self, after_reset=False):
        self.n_final = 0          # successful finalizes since create / reset
        self.nonempty = False
        self.trail = ""           # i: ingest, o: observation, n: a neighborhood call, f: finalize — since create / reset
        self.after_reset = after_reset

    def ingest(self):
        self.nonempty = True
        last = self.trail.rfind("i")
        if last >= 0 and ("o" in self.trail[last + 1:] or "n" in self.trail[last + 1:]):
            self.met("observation between two ingests")
        if last >= 0 and "n" in self.trail[last + 1:]:
            self.met("neighborhood between two ingests")
        self.trail += "i"

    def mutate(self):
        self.nonempty = True

    def observe(self, neighborhood=False):
        if self.nonempty and self.n_final == 0:
            self.met("observation before the first finalize")
            if neighborhood:
                self.met("neighborhood before the first finalize")
        self.trail += "n" if neighborhood else "o"

    def finalized(self):
        self.n_final += 1
        if "f" in self.trail and "i" in self.trail[self.trail.rfind("f"):]:
            self.met("ingest after finalize, then a second finalize")
        if self.after_reset and "i" in self.trail:
            self.met("reset followed by a job")
        self.trail += "f"


# ---- one sequence, applied to the engine and the model in lockstep --------------------------------------------

class Sequence:
    def __init__(self, orc, seed, engine=True):
        self.orc, self.seed, self.live = orc, seed, engine
        self.contexts, self.hooks, self.ops = draw_plan(seed)
        self.done = []
        self.met_here = set()
        self.routes = set()
        self.pos = Positions(self.met_here.add)
        self.keep = []   # device buffers of asynchronous ingests
        self.eng = None

    def report(self, what=""):
        return "%s\nseed %d  hooks %s\ncontexts %s\noperations so far:\n  %s" % (
            what, self.seed, self.hooks, self.contexts, "\n  ".join("%s %s" % o for o in self.done))

    # the engine's side of every step: nothing on a dry run
    def call(self, name, *a, **kw):
        return getattr(self.eng, name)(*a, **kw) if self.live else None

    def same(self, got, want, what):
        if self.live:
            assert np.array_equal(got, want), self.report("%s: engine %s, model %s" % (what, _brief(got), _brief(want)))

    def raises(self, text, name, *a, exact=True):
        """The call must fail, with this message (exact=False: with this text in it)."""
        if not self.live:
            return
        try:
            getattr(self, name)(*a) if name == "hand_over" else getattr(self.eng, name)(*a)
        except sa.ShkError as e:
            assert e.msg == text if exact else text in e.msg, self.report("%s: message %r, expected %r" % (name, e.msg, text))
        else:
            raise AssertionError(self.report("%s did not fail; expected %r" % (name, text)))

    def refused(self, e, name, *a, **kw):
        """The model refused with one of the ABI's codes (include/shk.h): so must the engine."""
        assert e.code is not None, self.report("the model refused: %s" % e)
        if not self.live:
            return
        try:
            getattr(self.eng, name)(*a, **kw)
        except sa.ShkError as got:
            assert got.code == e.code, self.report("%s: code %d (%s), expected %d" % (name, got.code, got.msg, e.code))
        else:
            raise AssertionError(self.report("%s did not fail; expected code %d" % (name, e.code)))

    def open(self, ctx):
        self.ctx, self.multi = ctx, ctx["kind"] != "plain"
        self.model = LaneModel(self.orc, ctx["k"], ctx["chunks"], ctx["histo_max"], multi_device=self.multi)
        self.pos.fresh()
        self.met_here.add("kind " + ("multi-device" if self.multi else "plain"))
        if self.live:
            devs = {"plain": None, "multi2": [0, 0], "multi4": [0, 0, 0, 0]}[ctx["kind"]]
            self.eng = sa.KmerEngine(ctx["k"], ctx["chunks"], ctx["histo_max"], capacity_hint=ctx["hint"], flags=ctx["flags"], device_ids=devs)

    def close(self):
        if self.live and self.eng is not None:
            if self.ctx["flags"] & sa.FLAG_TIMING:
                self.routes |= {name for name, (_, launches) in self.eng.timings().items() if launches}
            self.eng.close()
            self.eng = None
            self.keep = []

    def run(self):
        try:
            self.open(self.contexts[0])
            for name, p in self.ops:
                self.done.append((name, p))
                getattr(self, "op_" + name)(**p)
            if self.model.is_empty():
                self.done.append(("ingest", dict(r=7, route="host", window=False)))
                self.op_ingest(r=7, route="host", window=False)
            self.done.append(("finalize", {}))
            self.op_finalize()
        except ModelError as e:   # the draw asked the reference for something it refuses: the test's own fault
            raise AssertionError(self.report("the model refused: %s" % e)) from e
        except sa.ShkError as e:
            raise AssertionError(self.report("the engine refused: %s" % e)) from e
        finally:
            self.close()

    # ---- mutating operations ------------------------------------------------------------------
    def hand_over(self, route, bases, offsets, window):
        if not self.live:
            return
        lo, hi = int(offsets[0]), int(offsets[-1])
        if route == "host":
            if window:
                self.call("ingest_reads", bases, offsets)
            else:
                self.call("ingest_reads", bases[lo:hi], offsets - offsets[0])
        elif route == "packed":
            self.call("ingest_packed", sa.pack_reads(bases[lo:hi], offsets - offsets[0]))
        else:
            import torch
            db = torch.from_numpy(bases[lo:hi].copy()).cuda() if hi > lo else torch.zeros(1, dtype=torch.uint8).cuda()
            do = torch.from_numpy((offsets - offsets[0]).astype(np.int64)).cuda()
            self.keep += [db, do]
            self.eng.ingest_reads_device(db.data_ptr(), do.data_ptr(), len(offsets) - 1, hi - lo)

    def op_ingest(self, r, route, window):
        bases, offsets = batch(r)
        if window and len(offsets) > 3:   # a run of reads out of the middle of the caller's arrays
            offsets = offsets[1:-1]
        self.model.ingest_reads(bases, offsets)
        self.hand_over(route, bases, offsets, window)
        self.pos.ingest()

    def op_ingest_batch(self, r, chunk_id):
        bases, offsets = small_batch(r, 1500)
        self.model.ingest_batch(chunk_id, bases, offsets)
        self.call("ingest_batch", chunk_id, bases, offsets)
        self.pos.ingest()

    def op_set_read_index(self, index):
        self.model.set_read_index(index)
        self.call("set_read_index", index)

    def op_insert(self, r, chunk_id, n, zero):
        """Canonical keys only, as every table of the reference holds them (shk_primer_kmers relies on it): some that
        are there, some that are not.  More than one lane: counts that 30 inserts cannot carry to u32::MAX."""
        rng = np.random.default_rng(r)
        k = self.ctx["k"]
        have = self.model.export()[0]
        new = random_kmers(rng, k, n)
        new = np.minimum(new, revcomp(new, k))
        keys = np.concatenate([new, have[rng.integers(0, len(have), size=n // 2)]]) if len(have) else new
        keys = keys[rng.permutation(len(keys))]
        counts = rng.integers(1, 50, size=len(keys)).astype(np.uint32)
        counts[rng.random(len(keys)) < 0.05] = (1 << 31) + 5 if self.model.n_lanes == 1 else 1 << 20
        if zero:
            counts[:2] = 0
            self.met_here.add("zero-count insert")
        self.model.insert(chunk_id, keys, counts)
        self.call("insert", keys, counts, chunk_id=chunk_id)
        self.pos.mutate()

    def op_saturate(self, r, short):
        """One lane: an insert leaves a key `short` below u32::MAX, an ingest that holds it three times follows."""
        rng = np.random.default_rng(r)
        k = self.ctx["k"]
        seq = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=k + 40)]
        key = self.orc.kmers_from_ascii(seq.tobytes(), k)[0]
        self.model.insert(0, [key], [U32_MAX - short])
        self.call("insert", [key], [U32_MAX - short], chunk_id=0)
        bases = np.tile(seq, 3)
        offsets = np.arange(4, dtype=np.uint64) * np.uint64(len(seq))
        self.model.ingest_batch(0, bases, offsets)
        self.call("ingest_batch", 0, bases, offsets)
        assert self.model.get_count([key])[0] == U32_MAX
        self.pos.ingest()

    def op_reset(self):
        self.model.reset()
        self.call("reset")
        self.pos.fresh(after_reset=True)

    def op_second_context(self):
        """The first context goes, the second is made of its blocks (the process-wide cache hands them on as they are)."""
        self.close()
        self.open(self.contexts[1])
        self.met_here.add("two-context life")

    def op_poison(self, r, route, byte, repeats):
        """One byte outside ACGTN: the call fails with the reference's text (encoding.rs:353-356) — or, where the
        ingest only queues (FLAG_DEFER_ERRORS, device buffers), the next synchronising call does — and finalize keeps
        failing until shk_reset, after which the context is an empty one."""
        bases, offsets = batch(r)
        if int(offsets[-1]) == int(offsets[0]):
            bases, offsets = np.frombuffer(b"ACGTACGT", dtype=np.uint8), np.array([0, 8], dtype=np.uint64)
        bases = bases.copy()
        at = int(np.random.default_rng(r).integers(int(offsets[0]), int(offsets[-1])))
        bases[at] = byte
        text = LaneModel.bad_byte_message(byte)
        assert LaneModel.first_bad_byte(bases, offsets) == byte
        exact = not self.multi
        if self.live:
            queued = bool(self.ctx["flags"] & sa.FLAG_DEFER_ERRORS) or route == "device"
            if queued:
                try:   # (it may also have looked already)
                    self.hand_over(route, bases, offsets, False)
                    early = None
                except sa.ShkError as e:
                    early = e
                if early is None:
                    self.raises(text, "sync", exact=exact)
                else:
                    assert early.msg == text if exact else text in early.msg, self.report("poison: message %r" % early.msg)
            else:
                self.raises(text, "hand_over", route, bases, offsets, False, exact=exact)
        for _ in range(repeats + 1):
            self.raises(text, "finalize", exact=exact)
        self.done.append(("reset", {}))
        self.op_reset()
        self.same(self.call("export_table"), self.model.export(), "export after the poisoned context's reset")
        self.check_pre_finalize_counters()
        self.raises(NO_READS, "finalize")
        self.met_here.add("poison step")

    # ---- observations -------------------------------------------------------------------------------
    def check_pre_finalize_counters(self):
        if self.live:
            c, t = self.eng.counters(), self.model.totals()
            for f in PRE_FINALIZE:
                assert c[f] == t[f], self.report("counter %s: engine %d, model %d" % (f, c[f], t[f]))

    def op_finalize(self):
        try:
            self.model.finalize()
            expected = None
        except ModelError as e:
            expected = str(e)
        if expected == NO_READS:
            self.raises(NO_READS, "finalize")
            return
        if expected is not None:   # a key with merged count 0 (io.rs:1127-1132); a share reports its own numbers
            assert "unique kmers in the histogram" in expected and self.ctx["chunks"] > 0, self.report("the draw led to: " + expected)
            self.raises(expected if not self.multi else "unique kmers in the histogram", "finalize", exact=not self.multi)
            if self.multi:   # (the shares' histograms were not summed)
                return
        else:
            self.call("finalize")
        # io.rs:1020-1028 precede the checks: the columns and the totals are there either way
        self.same(self.call("histograms"), self.model.columns(), "histograms")
        want = self.model.totals()
        if self.live:
            got = self.eng.counters()
            for f, v in want.items():
                assert got[f] == v, self.report("counter %s: engine %d, model %d" % (f, got[f], v))
        if expected is None:
            self.pos.finalized()
            if want["any_saturated"]:
                self.met_here.add("saturated count")
        else:
            self.pos.observe()

    def op_finalize_twice(self):
        before = self.pos.n_final
        self.op_finalize()
        self.op_finalize()
        if self.pos.n_final == before + 2:
            self.met_here.add("finalize twice")

    def op_lookup(self, r):
        rng = np.random.default_rng(r)
        k = self.ctx["k"]
        have = self.model.export()[0]
        keys = [random_kmers(rng, k, 40), np.array([0, (1 << (2 * k)) - 1], dtype=np.uint64)]
        if len(have):
            some = have[rng.integers(0, len(have), size=300)]
            keys += [some, revcomp(some[:100], k)]
        keys = np.concatenate(keys)
        for canonical in (False, True):
            self.same(self.call("lookup", keys, canonical), self.model.get_count(keys, canonical), "lookup canonical=%s" % canonical)
        self.pos.observe()

    def op_export(self):
        self.same(self.call("export_table"), self.model.export(), "export_table")   # (both sorted by k-mer)
        self.pos.observe()

    def op_find_oligos(self, r):
        rng = np.random.default_rng(r)
        k = self.ctx["k"]
        L = int(rng.integers(1, k))
        have = self.model.export()[0]
        oligos = [random_kmers(rng, L, 2)]
        if len(have):
            some = have[rng.integers(0, len(have), size=4)]
            oligos += [some[:2] >> np.uint64(2 * (k - L)), revcomp(some[2:] & np.uint64((1 << (2 * L)) - 1), L)]
        oligos = np.unique(np.concatenate(oligos))
        min_count = int(rng.integers(1, 4))
        got = self.call("find_oligos", oligos, L, min_count)
        wk, wc = self.model.find_oligos(oligos, L, min_count)
        if self.live:
            order = np.lexsort((got[1], got[0]))
            worder = np.lexsort((wc, wk))
            self.same((got[0][order], got[1][order]), (wk[worder], wc[worder]), "find_oligos")
        self.pos.observe()

    def op_primer_kmers(self, r):
        rng = np.random.default_rng(r)
        k = self.ctx["k"]
        pair = PANEL[int(rng.integers(0, len(PANEL)))]
        params = dict(trim=int(rng.choice([0, 10, 12, 15, max(k - 1, 0), k + 3])), mismatches=int(rng.integers(0, 3)),
                      min_count=int(rng.integers(1, 3)), max_kmers=int(rng.choice([1, 40])))
        primers = [sa.Primer(s, **params) for s in pair[:int(rng.integers(1, 3))]]
        want = self.model.primer_kmers(primers)
        got = self.call("primer_kmers", primers)
        if self.live:
            assert len(got) == len(want)
            for g, w, p in zip(got, want, primers):
                for what, a, b in zip(("k-mers", "counts", "levels", "level hits"), g, w):
                    self.same(a, b, "primer_kmers %s of %s" % (what, p))
        self.pos.observe()

    def graph_seeds(self, rng):
        """(node, dir) seeds cut from k-mers the model holds — a zero-count key and a saturated one among them when
        there are any — as the prefix or the suffix of either orientation, and a few nodes from nowhere."""
        k = self.ctx["k"]
        keys, counts = self.model.export()
        mask = (1 << (2 * (k - 1))) - 1
        picked, marks = [], []
        if len(keys):
            picked += keys[rng.integers(0, len(keys), size=5)].tolist()
            for special, where in ((0, "neighborhood after a zero-count insert"), (U32_MAX, "neighborhood on a saturated count")):
                at = np.flatnonzero(counts == special)
                if len(at):
                    picked.append(int(keys[at[int(rng.integers(0, len(at)))]]))
                    marks.append(where)
        nodes = []
        for x in picked:
            if rng.random() < 0.5:
                x = int(revcomp(np.array([x], dtype=np.uint64), k)[0])
            nodes.append(x >> 2 if rng.random() < 0.5 else x & mask)
        nodes += [int(x) for x in rng.integers(0, mask + 1, size=2, dtype=np.uint64)]
        dirs = [int(d) for d in rng.integers(1, 4, size=len(nodes))]
        return nodes, dirs, counts, marks

    def op_neighborhood(self, r):
        """shk_neighborhood in the middle of a job, bounded so that the model stays cheap: at most 6 levels, 4096 k-mers
        and a level of 4096.  The model is not touched; the sequence goes on."""
        rng = np.random.default_rng(r)
        nodes, dirs, counts, marks = self.graph_seeds(rng) if self.ctx["k"] >= 2 else ([0], [1], np.zeros(0, np.uint32), [])
        n_distinct = len({(n, b) for n, d in zip(nodes, dirs) for b in (1, 2) if d & b})
        a = dict(min_count=int(rng.choice([0, 1, 2, int(counts[int(rng.integers(0, len(counts)))]) if len(counts) else 3, U32_MAX])),
                 max_levels=int(rng.integers(1, 7)), cap=int(rng.choice([0, 1, 64, 4096])),
                 fringe_cap=int(rng.choice([n_distinct, 64, 4096])))
        self.done[-1] = ("neighborhood", dict(r=r, nodes=nodes, dirs=dirs, **a))
        try:
            want = self.model.neighborhood(nodes, dirs, **a)
        except ModelError as e:   # a multi-device context (SHK_ERR_STATE), k = 1 (SHK_ERR_BAD_ARG)
            self.refused(e, "neighborhood", nodes, dirs, **a)
            if e.code == SHK_ERR_STATE:
                self.met_here.add("neighborhood refused on a multi-device context")
            return
        got = self.call("neighborhood", nodes, dirs, **a)
        if self.live:
            for what, g, w in zip(("k-mers", "counts", "fringe nodes", "fringe dirs", "levels done"), got, want):
                self.same(g, w, "neighborhood %s" % what)
        self.met_here.update(marks)
        self.pos.observe(neighborhood=True)

    def op_pcr_extend(self, r):
        """shk_pcr_extend from the model's top-count k-mers in both orientations, the node budget small."""
        rng = np.random.default_rng(r)
        k = self.ctx["k"]
        keys, counts = self.model.export()
        top = np.argsort(counts, kind="stable")[::-1][:8]
        sets = []
        for part in (top[0::2], top[1::2]):
            ks, cs = keys[part].copy(), counts[part].copy()
            flip = rng.random(len(ks)) < 0.5
            if k >= 2:
                ks[flip] = revcomp(ks[flip], k)
            sets.append((ks, cs))
        a = dict(min_count=int(rng.integers(1, 4)), table_min_count=int(rng.choice([1, 2])),
                 high_coverage_ratio=float(rng.choice([1.5, 10.0])), max_num_nodes=int(rng.choice([50, 1200])),
                 sweep=bool(rng.random() < 0.5))
        self.done[-1] = ("pcr_extend", dict(r=r, fwd=sets[0][0].tolist(), rev=sets[1][0].tolist(), **a))
        try:
            want, used, steps = self.model.pcr_extend(sets[0], sets[1], **a)
        except ModelError as e:
            self.refused(e, "pcr_extend", sets[0], sets[1], **a)
            return
        got = self.call("pcr_extend", sets[0], sets[1], **a)
        if self.live:
            self.same(got.node_sub_kmers, want.sub_kmer, "pcr_extend nodes")
            self.same(got.node_flags, want.flags(), "pcr_extend node flags")
            for i, (what, g) in enumerate((("sources", got.edge_src), ("targets", got.edge_tgt), ("counts", got.edge_counts))):
                self.same(g, np.array([e[i] for e in want.edges], dtype=np.uint32), "pcr_extend edge %s" % what)
            self.same((got.found_path, got.threshold_used, got.steps_run), (want.found_path, used, steps), "pcr_extend outcome")
        if self.pos.after_reset and self.pos.nonempty:
            self.met_here.add("pcr_extend after a reset")
        self.pos.observe()

    def op_filter_reads(self, r):
        """PrimerReadFilter::matches per read with a few of the table's k-mers as the primer set; the table stays."""
        rng = np.random.default_rng(r)
        k = self.ctx["k"]
        bases, offsets = small_batch(r)
        have = self.model.export()[0]
        pk = np.concatenate([random_kmers(rng, k, 3)] + ([have[rng.integers(0, len(have), size=20)]] if len(have) else []))
        pset = self.orc.KmerCounts(k)
        for x in pk.tolist():
            pset.insert(int(x), 1)
        raw = bases.tobytes()
        want = np.array([pset.filter_matches(raw[int(a):int(b)]) for a, b in zip(offsets[:-1], offsets[1:])], dtype=bool)
        self.same(self.call("filter_reads", bases, offsets, pk), want, "filter_reads")
        self.op_export()

    def op_kmers_from_reads(self, r):
        """Batched kmers_from_ascii; one read may hold a byte outside ACGTN (no k-mers, no poison); the table stays."""
        rng = np.random.default_rng(r)
        k = self.ctx["k"]
        bases, offsets = small_batch(r)
        bases = bases.copy()
        if len(bases) and rng.random() < 0.4:
            bases[int(rng.integers(0, len(bases)))] = ord("x")
        raw = bases.tobytes()
        if self.live:
            got, bad = self.eng.kmers_from_reads(bases, offsets)
            for i, (a, b) in enumerate(zip(offsets[:-1], offsets[1:])):
                read = raw[int(a):int(b)]
                if b"x" in read:
                    assert bad[i] == ord("x") and len(got[i]) == 0, self.report("kmers_from_reads: read %d" % i)
                else:
                    self.same(got[i], np.array(self.orc.kmers_from_ascii(read, k), dtype=np.uint64), "kmers_from_reads: read %d" % i)
                    assert bad[i] == 0, self.report("kmers_from_reads: bad byte of read %d" % i)
        self.op_export()

    def op_sync(self):
        self.call("sync")
        self.check_pre_finalize_counters()
        self.pos.observe()


def _brief(x):
    if isinstance(x, tuple):
        return "(" + ", ".join(_brief(y) for y in x) + ")"
    a = np.asarray(x)
    return "%s%s %s%s" % (a.dtype, list(a.shape), a.ravel()[:8].tolist(), "…" if a.size > 8 else "")


def dry_run(orc, seed):
    """The draw and the model alone → what the seed covers (positions and kinds; the routes need the engine)."""
    s = Sequence(orc, seed, engine=False)
    s.run()
    return s.met_here


# ---- the sweep ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", range(FIRST, FIRST + N_SEEDS))
def test_random_call_sequence_against_the_lane_model(orc, monkeypatch, seed):
    s = Sequence(orc, seed)
    for name, v in s.hooks.items():
        monkeypatch.setenv(name, v)
    s.run()
    RECORD["seeds"].add(seed)
    for item in s.met_here:
        RECORD["kinds" if item.startswith("kind ") else "positions"].setdefault(item, []).append(seed)
    for name in s.routes:
        RECORD["routes"].setdefault(name, []).append(seed)


# ---- fixed sequences: what the sweep found ----------------------------------------------------------------

def test_multi_device_insert_only_job_finalizes(orc):
    """Found by the sweep (insert, finalize on device_ids=[0,0]): a job of inserts alone finalizes on a one-device
    context (n_inserted counts as input) and was refused with "No reads were ingested" on a multi-device one,
    whose finalize looked at the summed read count alone.  Empty contexts of either kind are still refused."""
    for devs in (None, [0, 0]):
        model = LaneModel(orc, 11, 2, 10)
        with sa.KmerEngine(11, 2, 10, device_ids=devs) as eng:
            with pytest.raises(sa.ShkError) as ei:
                eng.finalize()
            assert ei.value.msg == NO_READS
            for m in (model, eng):
                m.insert(kmers=[1, 20, 2, 11], counts=[3, 5, 5, 11], chunk_id=1)
            eng.finalize()
            model.finalize()
            assert np.array_equal(eng.histograms(), model.columns())
            c, t = eng.counters(), model.totals()
            assert {f: c[f] for f in t} == t
            eng.reset()
            with pytest.raises(sa.ShkError) as ei:
                eng.finalize()
            assert ei.value.msg == NO_READS


@pytest.mark.parametrize("k,chunks,hooks", [(15, 17, {}), (29, 16, {"SHK_REC32": "0", "SHK_DEFER_BUDGET": "150000"})])
def test_multi_device_table_grows_between_two_absorbs_of_a_round(orc, monkeypatch, k, chunks, hooks):
    """Found by the sweep (seeds 86 and 87: device_ids=[0,0], a hint of 20 000, ingest — 4-byte and 8-byte exchange
    records): a share's table of fewer pages than the level-1 fan-out has an exchange layout that follows its size,
    and the flush in front of a round's second absorb grew it: "segment has 68 regions, this context expects 272".
    A share now starts with the fan-out's pages, so the layout is one for all shares and for good."""
    for name, v in hooks.items():
        monkeypatch.setenv(name, v)
    model = LaneModel(orc, k, chunks, 5)
    with sa.KmerEngine(k, chunks, 5, capacity_hint=20_000, flags=sa.FLAG_TIMING, device_ids=[0, 0]) as eng:
        for r in (24312679, 544142001, 931922698):
            bases, offsets = batch(r)
            model.ingest_reads(bases, offsets)
            eng.ingest_reads(bases, offsets)
        eng.finalize()
        model.finalize()
        assert np.array_equal(eng.histograms(), model.columns())
        c, t = eng.counters(), model.totals()
        assert {f: c[f] for f in t} == t
        assert all(np.array_equal(a, b) for a, b in zip(eng.export_table(), model.export()))


# ---- what the default seed set has to have met (last in the file: after the sweep) --------------------------

def test_the_default_seeds_cover_every_position_route_and_kind():
    if OVERRIDDEN:
        pytest.skip("SHK_SEQ_SEEDS / SHK_SEQ_FIRST are set: the coverage is a property of the default seed set")
    assert RECORD["seeds"] == set(range(DEFAULT_SEEDS)), "the sweep did not run (or not pass) on every default seed"
    missing = [p for p in POSITIONS if p not in RECORD["positions"]]
    missing += [k for k in ("kind plain", "kind multi-device") if k not in RECORD["kinds"]]
    missing += ["route " + r for r in ROUTES if r not in RECORD["routes"]]
    print("\n".join("%s: seeds %s" % kv for part in ("positions", "kinds", "routes") for kv in sorted(RECORD[part].items())))
    assert not missing, (missing, RECORD)
