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

A third generator decides what lies beside the contexts — whether a one-device context retains its reads
(shk_retain_reads, the first allocation 0, 64 or 1000 bases so that the store moves under queued appends) and whether
a multi-device one is made with SHK_FLAG_GROUP_GRAPH, which then answers the graph calls as the merged view — and
interleaves about two to six more operations: the retained store read back over drawn ranges, the panel filter and
the panel threading over it, and the panel calls that share the context's scratch (thread_reads_panel as host and
device batch, neighborhood_panel, pcr_prune_panel, pcr_dedup_panel).  Their expected answers are the lane model's —
the oracle's filter_matches, tests/thread_ref.py, prune_ref.py, products_ref.py, pcr_ref.py — and each is followed by
an export, so the table and everything later is checked against a model they did not touch.  Without the third
generator's operations the plan is the one drawn before them (tests/test_lane_model_cpu.py holds that hash too).

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
# (tests/test_lane_model_cpu.py): the rarest, "neighborhood after a zero-count insert", is met by seeds 17, 47 and 55
# (and by 2 and 45, whose multi-device contexts answer with SHK_FLAG_GROUP_GRAPH),
# "neighborhood on a saturated count" by 12, 19, 24, 49, 73 and 93, the poison step and the saturated count by 8 seeds
# each.  Of the third generator's positions the rarest are "retained reads on the second context of a two-context life"
# (seeds 84 and 88), "group-graph call after a zero-count insert" (2 and 45) and "retained reads across a poison step"
# (20, 70 and 84).  The routes need the engine: on an MI355X the rarest, `histo_rows` (a job whose one fresh page pass
# is finalized as it is, on a FLAG_TIMING seed), was met by no seed of the first 48 and by seeds 25, 75 and 94 before
# the third generator — a neighborhood call in front of such a finalize drops the fused histogram on purpose (seed
# 25's first job has one); with the third generator's operations between the others seed 25 still meets the route,
# 75 and 94 no longer do; `grow` by 11 seeds, `extend` by 22; `share_grew` by seeds 1 and 2, `store_moved` by 36 seeds.
# The 96 sequences (and the fixed ones below) take 77.8 s there with the third generator's operations, 55.4 s without
# them (the parent of the change that added them, same machine, same day; 59.3 s and 53.9 s were the two numbers of
# the graph observations), against 459 s for the rest of the GPU suite.
DEFAULT_SEEDS = 96
OVERRIDDEN = "SHK_SEQ_SEEDS" in os.environ or "SHK_SEQ_FIRST" in os.environ
N_SEEDS = int(os.environ.get("SHK_SEQ_SEEDS", str(DEFAULT_SEEDS)))
FIRST = int(os.environ.get("SHK_SEQ_FIRST", "0"))

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PANEL = [l.split("\t")[1:3] for l in open(os.path.join(G, "primer_panel_cnidaria.tsv")).read().splitlines()
         if l and not l.startswith("#")]
MAX_BASES = 2_000_000
SHK_ERR_INVALID_CHAR = -1   # include/shk.h: the code a poisoned context keeps
PRE_FINALIZE = ("n_reads_ingested", "n_bases_read", "n_bases_ingested")
POSITIONS = ("observation before the first finalize", "observation between two ingests",
             "ingest after finalize, then a second finalize", "reset followed by a job", "finalize twice",
             "poison step", "two-context life", "zero-count insert", "saturated count",
             "neighborhood between two ingests", "neighborhood before the first finalize",
             "neighborhood after a zero-count insert", "neighborhood on a saturated count", "pcr_extend after a reset",
             "neighborhood refused on a multi-device context",
             "retained call between two ingests", "retained call before the first finalize", "retained reads after a reset",
             "retained reads on the second context of a two-context life", "retained reads across a poison step",
             "retention with a packed ingest", "retention with a device ingest", "retention with a windowed ingest",
             "retention with ingest_batch", "group-graph neighborhood between two ingests", "group-graph pcr_extend",
             "group-graph call after a zero-count insert")
# store_moved: retained_info()["device_bytes"] rose between two looks at one store; share_grew: counters()["n_grows"]
# rose on a group-graph context between its creation or its last graph call and the end of a graph call
ROUTES = ("direct", "scatter", "pages", "histo", "histo_rows", "grow", "insert", "lookup", "export", "extend", "store_moved",
          "share_grew")
GRAPH_OPS = ("neighborhood", "pcr_extend")
GRAPH_SEED = 7_000_000   # the second generator: GRAPH_SEED + the sequence seed
GRAPH_RATE = 0.2
RETAIN_OPS = ("retain_switch", "retained_export", "filter_retained", "thread_retained", "thread_panel", "neighborhood_panel",
              "prune_panel", "dedup_panel")
RETAIN_SEED = 9_000_000  # the third generator: RETAIN_SEED + the sequence seed
RETAIN_RATE = 0.2
RETAIN_WEIGHTS = {True: (2.0, 2.5, 2.5, 1.0, 1.0, 1.2, 1.2),    # a context that retains: RETAIN_OPS[1:]
                  False: (0.3, 0.3, 0.3, 1.5, 1.5, 1.5, 1.5)}   # one that does not: the three refusals now and then
RETAIN_TEXTS = ("reads are not retained", "holds reads already", "not available on a multi-device context")
STORED = {"packed": "retention with a packed ingest", "device": "retention with a device ingest",
          "windowed": "retention with a windowed ingest", "ingest_batch": "retention with ingest_batch"}
THREAD_READS, THREAD_LEN, FILTER_WINDOW, HOST_CHECK = 32, 1500, 3000, 4000   # bounds that keep the model cheap
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
    """→ (contexts, hooks, operations): draw_graph_plan's, with the third generator's operations (RETAIN_OPS) after
    about every fifth one and a retention switch after some resets of a one-device context."""
    return _draw_third(seed)[:3]


def draw_properties(seed):
    """→ per context what lies beside it: dict(retain, capacity_bases, group_graph), from the third generator."""
    return _draw_third(seed)[3]


def _draw_third(seed):
    contexts, hooks, base = draw_graph_plan(seed)
    rng = np.random.default_rng(RETAIN_SEED + seed)
    props = []
    for ctx in contexts:
        coin, capacity = rng.random() < 0.5, int(rng.choice([0, 64, 1000]))
        plain = ctx["kind"] == "plain"
        props.append(dict(retain=bool(plain and coin), capacity_bases=capacity if plain else 0, group_graph=bool(not plain and coin)))
    ops, at, retaining = [], 0, props[0]["retain"]
    for op in base:
        ops.append(op)
        if op[0] == "second_context":
            at, retaining = 1, props[1]["retain"]
        ctx = contexts[at]
        if op[0] == "reset" and ctx["kind"] == "plain" and rng.random() < 0.4:   # off, or on again: the store goes to the cache
            retaining = bool(rng.random() < 0.6)
            ops.append(("retain_switch", dict(on=retaining, capacity_bases=int(rng.choice([0, 64, 1000])))))
        if rng.random() < RETAIN_RATE:
            w = np.array(RETAIN_WEIGHTS[retaining])
            if ctx["k"] < 2:   # a node is a (k-1)-mer
                w[[RETAIN_OPS.index(n) - 1 for n in ("thread_retained", "thread_panel", "prune_panel")]] = 0
            ops.append((RETAIN_OPS[1 + int(rng.choice(len(w), p=w / w.sum()))], dict(r=int(rng.integers(1, 1 << 30)))))
    return contexts, hooks, ops, props


def draw_graph_plan(seed):
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


COMPLEMENT = bytes.maketrans(b"ACGTN", b"TGCAN")


def rc_bytes(s):
    return s[::-1].translate(COMPLEMENT)


def encode(s):
    """ACGT bytes → the 2-bit number of kmer/encoding.rs, the first base highest."""
    x = 0
    for c in s:
        x = (x << 2) | b"ACGT".index(c)
    return x


def f64_bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


# ---- where in a context's life things happened ----------------------------------------------------------------

class Positions:
    def __init__(self, met):
        self.met = met
        self.fresh()

    def fresh(self, after_reset=False):
        self.n_final = 0          # successful finalizes since create / reset
        self.nonempty = False
        # i: ingest, o: observation, n: a neighborhood call, f: finalize — since create / reset; beside them r: a retained
        # call that answered, G: a neighbourhood answered by a group-graph context
        self.trail = ""
        self.after_reset = after_reset

    def ingest(self):
        self.nonempty = True
        last = self.trail.rfind("i")
        if last >= 0 and ("o" in self.trail[last + 1:] or "n" in self.trail[last + 1:]):
            self.met("observation between two ingests")
        if last >= 0 and "n" in self.trail[last + 1:]:
            self.met("neighborhood between two ingests")
        if last >= 0 and "r" in self.trail[last + 1:]:
            self.met("retained call between two ingests")
        if last >= 0 and "G" in self.trail[last + 1:]:
            self.met("group-graph neighborhood between two ingests")
        self.trail += "i"

    def mutate(self):
        self.nonempty = True

    def observe(self, neighborhood=False, retained=False, group_graph=False):
        if self.nonempty and self.n_final == 0:
            self.met("observation before the first finalize")
            if neighborhood:
                self.met("neighborhood before the first finalize")
            if retained:
                self.met("retained call before the first finalize")
        self.trail += ("n" if neighborhood else "o") + ("r" if retained else "") + ("G" if group_graph else "")

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
        self.props = draw_properties(seed)
        self.done = []
        self.met_here = set()
        self.routes = set()
        self.facts = []  # (operation, what its expected answer held): tests/test_lane_model_cpu.py asks that they are not vacuous
        self.pos = Positions(self.met_here.add)
        self.keep = []   # device buffers of asynchronous ingests
        self.eng = None

    def report(self, what=""):
        return "%s\nseed %d  hooks %s\ncontexts %s\nbeside them %s\noperations so far:\n  %s" % (
            what, self.seed, self.hooks, self.contexts, self.props, "\n  ".join("%s %s" % o for o in self.done))

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
            for text in RETAIN_TEXTS:   # the retained calls' refusals: the text of shk_retain_api.hip.h too
                assert text not in str(e) or text in got.msg, self.report("%s: message %r, expected %r in it" % (name, got.msg, text))
        else:
            raise AssertionError(self.report("%s did not fail; expected code %d" % (name, e.code)))

    def open(self, at):
        ctx, prop = self.contexts[at], self.props[at]
        self.ctx, self.ctx_at, self.multi = ctx, at, ctx["kind"] != "plain"
        self.group_graph = self.multi and prop["group_graph"]
        self.model = LaneModel(self.orc, ctx["k"], ctx["chunks"], ctx["histo_max"], multi_device=self.multi, group_graph=self.group_graph)
        self.pos.fresh()
        self.fresh_store()
        self.last_grows = 0
        self.met_here.add("kind " + ("multi-device" if self.multi else "plain"))
        if self.live:
            devs = {"plain": None, "multi2": [0, 0], "multi4": [0, 0, 0, 0]}[ctx["kind"]]
            flags = ctx["flags"] | (sa.FLAG_GROUP_GRAPH if self.group_graph else 0)
            self.eng = sa.KmerEngine(ctx["k"], ctx["chunks"], ctx["histo_max"], capacity_hint=ctx["hint"], flags=flags, device_ids=devs)
        if prop["retain"]:
            self.op_retain_switch(True, prop["capacity_bases"])

    def fresh_store(self):
        """The retained store is empty (create, reset, switched off): how its reads came, where its ingests ended."""
        self.stored, self.bounds, self.last_bytes, self.n_retained = set(), [], 0, 0

    def look_at_the_store(self):
        """After every operation: where an ingest began in the store, and whether the store's allocation rose."""
        n = len(self.model.retained)
        if n > self.n_retained > 0:
            self.bounds.append(self.n_retained)
        self.n_retained = n
        if self.live and self.model.retain:
            held = self.eng.retained_info()["device_bytes"]
            if held > self.last_bytes > 0:
                self.routes.add("store_moved")
            self.last_bytes = held

    def close(self):
        if self.live and self.eng is not None:
            if self.ctx["flags"] & sa.FLAG_TIMING:
                self.routes |= {name for name, (_, launches) in self.eng.timings().items() if launches}
            self.eng.close()
            self.eng = None
            self.keep = []

    def run(self):
        try:
            self.open(0)
            for name, p in self.ops:
                self.done.append((name, p))
                getattr(self, "op_" + name)(**p)
                self.look_at_the_store()
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
        if self.model.retain and len(offsets) > 1:   # (a window: the caller's offsets do not start at 0)
            self.stored.add("windowed" if route == "host" and window and int(offsets[0]) > 0 else route)

    def op_ingest_batch(self, r, chunk_id):
        bases, offsets = small_batch(r, 1500)
        self.model.ingest_batch(chunk_id, bases, offsets)
        self.call("ingest_batch", chunk_id, bases, offsets)
        self.pos.ingest()
        if self.model.retain and len(offsets) > 1:
            self.stored.add("ingest_batch")

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
        if self.model.retain:
            self.stored.add("ingest_batch")

    def op_reset(self):
        self.model.reset()
        self.call("reset")
        self.pos.fresh(after_reset=True)
        held = self.last_bytes   # (the store is emptied, its allocation stays)
        self.fresh_store()
        self.last_bytes = held

    def op_second_context(self):
        """The first context goes, the second is made of its blocks (the process-wide cache hands them on as they are)."""
        self.close()
        self.open(1)
        self.met_here.add("two-context life")

    def op_retain_switch(self, on, capacity_bases):
        """shk_retain_reads on a context that holds no reads: off hands the store's blocks to the cache, on starts a new one."""
        try:
            self.model.retain_reads(on)
        except ModelError as e:
            self.refused(e, "retain_reads", on, capacity_bases)
            return
        self.call("retain_reads", on, capacity_bases)
        if self.live:
            info = self.eng.retained_info()
            self.same((info["reads"], info["bases"]), (0, 0), "retained_info after the switch")
            assert on or info["device_bytes"] == 0, self.report("retain_reads(False) left %d bytes" % info["device_bytes"])
        if not on:
            self.fresh_store()

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
        if self.model.retain:   # the batch was appended before it poisoned: the store says so until the reset
            if self.live:
                for call in (lambda: self.eng.retained_reads(0, 0), lambda: self.eng.filter_reads_retained([[1]]),
                             lambda: self.eng.thread_reads_retained([], [])):
                    try:
                        call()
                    except sa.ShkError as e:
                        assert (e.code, e.msg) == (SHK_ERR_INVALID_CHAR, text), self.report("retained call on a poisoned context: %d %r" % (e.code, e.msg))
                    else:
                        raise AssertionError(self.report("a retained call answered on a poisoned context"))
            self.met_here.add("retained reads across a poison step")
        self.done.append(("reset", {}))
        self.op_reset()
        if self.model.retain and self.live:
            info = self.eng.retained_info()
            self.same((info["reads"], info["bases"]), (0, 0), "retained_info after the poisoned context's reset")
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
        self.graph_call_answered(counts)
        self.pos.observe(neighborhood=True, group_graph=self.group_graph)

    def graph_call_answered(self, counts):
        """A graph call has answered.  On a group-graph context: whether a share grew since the last one (the share
        directory is built anew from the shares' arrays), and whether the table holds a key of count 0."""
        if not self.group_graph:
            return
        if len(counts) and not counts.all():
            self.met_here.add("group-graph call after a zero-count insert")
        if self.live:
            grows = self.eng.counters()["n_grows"]
            if grows > self.last_grows:
                self.routes.add("share_grew")
            self.last_grows = grows

    def extend_args(self, rng):
        """→ (forward set, reverse set, parameters) of a shk_pcr_extend from the model's top-count k-mers in both
        orientations, the node budget small."""
        k = self.ctx["k"]
        keys, counts = self.model.export()
        # np.argsort(counts, kind="stable")[::-1][:8], sorting only what can be among the eight
        high = np.flatnonzero(counts >= np.partition(counts, len(counts) - 8)[len(counts) - 8]) if len(counts) > 8 else np.arange(len(counts))
        top = high[np.argsort(counts[high], kind="stable")[::-1][:8]]
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
        return sets[0], sets[1], a

    def op_pcr_extend(self, r):
        """shk_pcr_extend with extend_args' draw."""
        rng = np.random.default_rng(r)
        sets = [None, None]
        sets[0], sets[1], a = self.extend_args(rng)
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
        if self.group_graph:
            self.met_here.add("group-graph pcr_extend")
        self.graph_call_answered(self.model.export()[1])
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

    # ---- the third generator's operations: retained reads and the panel calls -------------------------
    def retained_call_answered(self):
        """A retained call has answered: where in the context's life, and how the reads it saw had come."""
        self.pos.observe(retained=True)
        if self.model.retained:
            if self.pos.after_reset:
                self.met_here.add("retained reads after a reset")
            if self.ctx_at == 1:
                self.met_here.add("retained reads on the second context of a two-context life")
            self.met_here.update(STORED[route] for route in self.stored if route in STORED)

    def canonical_kmer(self, window):
        return int(self.orc.kmers_from_ascii(bytes(window), self.ctx["k"])[0])

    def op_retained_export(self, r):
        """shk_retained_export over (0, all), (n_reads, 0), a range across the start of an ingest and one from anywhere."""
        rng = np.random.default_rng(r)
        try:
            info = self.model.retained_info()
            self.model.retained_export(0, 0)
        except ModelError as e:
            self.refused(e, "retained_reads", 0, 0)
            return
        n = info["reads"]
        ranges = [(0, n), (n, 0)]
        if self.bounds:
            first = max(self.bounds[int(rng.integers(0, len(self.bounds)))] - int(rng.integers(1, 40)), 0)
            ranges.append((first, min(int(rng.integers(2, 80)), n - first)))
        first = int(rng.integers(0, n + 1))
        ranges.append((first, int(rng.integers(0, min(n - first, 200) + 1))))
        self.done[-1] = ("retained_export", dict(r=r, ranges=ranges))
        if self.live:
            got = self.eng.retained_info()
            self.same((got["reads"], got["bases"]), (n, info["bases"]), "retained_info")
            for first, count in ranges:
                for what, got, want in zip(("bases", "offsets"), self.eng.retained_reads(first, count), self.model.retained_export(first, count)):
                    self.same(got, want, "retained reads %d + %d: %s" % (first, count, what))
        self.retained_call_answered()
        self.op_export()

    def draw_genes(self, rng, reads):
        """1-4 genes: the canonical k-mers of the first, the last and a middle window of a few of the reads (cut from
        the read or from its reverse complement) and two from nowhere; one gene is sometimes empty."""
        k = self.ctx["k"]
        genes = []
        n_genes = int(rng.integers(1, 5))
        for _ in range(n_genes):
            if n_genes > 1 and rng.random() < 0.2:
                genes.append(np.zeros(0, dtype=np.uint64))
                continue
            new = random_kmers(rng, k, 2)
            kmers = np.minimum(new, revcomp(new, k)).tolist()
            for _ in range(int(rng.integers(1, 3)) if reads else 0):
                read = reads[int(rng.integers(0, len(reads)))]
                for at in (0, len(read) - k, int(rng.integers(0, max(len(read) - k, 0) + 1))):
                    window = read[at:at + k] if at >= 0 else b""
                    if len(window) == k and b"N" not in window:
                        kmers.append(self.canonical_kmer(window if rng.random() < 0.5 else rc_bytes(window)))
            genes.append(np.array(kmers, dtype=np.uint64))
        return genes

    def op_filter_retained(self, r):
        """shk_filter_reads_panel_retained: per gene the ascending indices of the retained reads that match it — and, while
        the store is small, what shk_filter_reads_panel answers over the same reads as a host batch."""
        rng = np.random.default_rng(r)
        genes = self.draw_genes(rng, self.model.retained)
        self.done[-1] = ("filter_retained", dict(r=r, genes=[g.tolist() for g in genes]))
        try:
            want = self.model.filter_retained(genes)
        except ModelError as e:
            self.refused(e, "filter_reads_retained", genes)
            return
        self.facts.append(("filter_retained", dict(nonempty=any(want))))
        if self.live:
            got = self.eng.filter_reads_retained(genes)
            self.same(len(got), len(want), "filter_reads_retained: genes")
            for g, (a, b) in enumerate(zip(got, want)):
                self.same(a, np.array(b, dtype=np.uint64), "filter_reads_retained: gene %d" % g)
            if len(self.model.retained) <= HOST_CHECK:
                host = self.eng.filter_reads_panel(*self.model.retained_export(0, len(self.model.retained)), genes)
                for g, (a, b) in enumerate(zip(host, want)):
                    self.same(a, np.array(b, dtype=np.uint64), "filter_reads_panel over the retained reads: gene %d" % g)
        self.retained_call_answered()
        self.op_export()

    def draw_thread_case(self, rng, reads, n_total, lo):
        """Two graphs and their read lists over reads lo .. lo + len(reads) of a batch of n_total.  One graph is a chain
        over the (k-1)-mers of stretches of two or three of the reads, with one branch; the other is the model's
        pcr_extend graph when the context has one with edges.  A list is what the model's filter keeps for a few of the
        graph's edge k-mers, cut to THREAD_READS reads of at most THREAD_LEN bases, sometimes reversed or repeated.
        → (graphs as (sub_kmers, [(source, target)]), lists, read_index, mate)."""
        k = self.ctx["k"]
        graphs = []
        sub, edges, sources = [], [], []
        for _ in range(int(rng.integers(2, 4))):
            for _ in range(20 if reads else 0):   # a read with a stretch of k + 2 bases or more without an N
                at = int(rng.integers(0, len(reads)))
                parts = [p for p in reads[at][:THREAD_LEN].split(b"N") if len(p) >= k + 2]
                if parts:
                    part = parts[int(rng.integers(0, len(parts)))]
                    start = int(rng.integers(0, len(part) - (k + 2) + 1))
                    stretch = part[start:start + k + 2 + int(rng.integers(0, 60))]
                    first = len(sub)
                    sub += [encode(stretch[i:i + k - 1]) for i in range(len(stretch) - k + 2)]
                    edges += [(i, i + 1) for i in range(first, len(sub) - 1)]
                    sources.append(at)
                    break
        if sub:   # the branch: a second way out of the chain's second node, one base off the third
            sub.append(sub[2] ^ 1)
            edges.append((1, len(sub) - 1))
        else:     # (no read has such a stretch: two nodes and no edge)
            sub = [0, 1]
        graphs.append((sub, edges))
        try:
            fwd, rev, a = self.extend_args(rng)
            g = self.model.pcr_extend(fwd, rev, **a)[0]
            if g.edges:
                graphs.append((list(g.sub_kmer), [(s, t) for s, t, _ in g.edges]))
        except ModelError:   # (a multi-device context without the flag has no such graph)
            pass
        lists = []
        for sub, edges in graphs:
            some = [edges[int(i)] for i in rng.integers(0, len(edges), size=min(len(edges), 12))] if edges else []
            gene = [((sub[s] << 2) | (sub[t] & 3)) for s, t in some]
            gene = [min(x, int(revcomp(np.array([x], dtype=np.uint64), k)[0])) for x in gene]
            rows = self.model.filter_reads_panel(reads, [gene])[0] if gene else []
            ids = [i for i in rows if len(reads[i]) <= THREAD_LEN]
            if len(ids) > THREAD_READS:
                ids = sorted(set(sources) & set(ids)) + [ids[int(i)] for i in rng.integers(0, len(ids), size=THREAD_READS)]
            ids = [lo + i for i in ids[:THREAD_READS]]
            way = rng.random()
            lists.append(ids[::-1] if way < 0.25 else ids + ids if way < 0.5 else ids)
        if rng.random() < 0.4:   # the paired form: mates side by side, now and then a read without one
            read_index = np.arange(n_total, dtype=np.uint64) + np.uint64(int(rng.integers(0, 1000)) * 2)
            mate = (1 + np.arange(n_total) % 2).astype(np.uint8)
            mate[rng.random(n_total) < 0.1] = 0
        else:
            read_index = mate = None
        return graphs, lists, read_index, mate

    def thread_facts(self, name, want):
        self.facts.append((name, dict(read_edges=sum(sum(w[4]) for w in want), links=sum(len(w[2]) for w in want))))

    def same_annotations(self, got, want, what):
        self.same(len(got), len(want), "%s: genes" % what)
        for g, (a, w) in enumerate(zip(got, want)):
            for field, x, y in (("support_total", a.support_total, w[0]), ("support_unambiguous", a.support_unambiguous, w[1]),
                                ("links", a.links, np.array(w[2], dtype=np.uint32).reshape(-1, 2)), ("link_counts", a.link_counts, w[3]),
                                ("read_edges", a.read_edges, w[4]), ("n_paired_links", a.n_paired_links, w[5])):
                self.same(x, y, "%s: gene %d %s" % (what, g, field))

    @staticmethod
    def graph_arrays(graphs):
        return [(np.array(sub, dtype=np.uint64), np.array([e[0] for e in edges], dtype=np.uint32), np.array([e[1] for e in edges], dtype=np.uint32))
                for sub, edges in graphs]

    def op_thread_retained(self, r):
        """shk_thread_reads_panel_retained against tests/thread_ref.py: lists drawn from a window of the store."""
        rng = np.random.default_rng(r)
        try:
            self.model.retained_export(0, 0)
        except ModelError as e:
            self.refused(e, "thread_reads_retained", [], [])
            return
        n = len(self.model.retained)
        lo = int(rng.integers(0, max(n - FILTER_WINDOW, 0) + 1))
        graphs, lists, read_index, mate = self.draw_thread_case(rng, self.model.retained[lo:lo + FILTER_WINDOW], n, lo)
        self.done[-1] = ("thread_retained", dict(r=r, graphs=graphs, lists=lists, paired=mate is not None))
        want = self.model.thread_retained(graphs, lists, read_index, mate)
        self.thread_facts("thread_retained", want)
        if self.live:
            self.same_annotations(self.eng.thread_reads_retained(self.graph_arrays(graphs), lists, read_index, mate), want, "thread_reads_retained")
        self.retained_call_answered()
        self.op_export()

    def op_thread_panel(self, r):
        """shk_thread_reads_panel over a small batch, as host arrays and as device buffers, against tests/thread_ref.py."""
        rng = np.random.default_rng(r)
        bases, offsets = small_batch(r)
        raw = bases.tobytes()
        reads = [raw[int(a):int(b)] for a, b in zip(offsets[:-1], offsets[1:])]
        graphs, lists, read_index, mate = self.draw_thread_case(rng, reads, len(reads), 0)
        self.done[-1] = ("thread_panel", dict(r=r, graphs=graphs, lists=lists, paired=mate is not None))
        want = self.model.thread_reads_panel(reads, graphs, lists, read_index, mate)
        self.thread_facts("thread_panel", want)
        if self.live:
            arrays = self.graph_arrays(graphs)
            self.same_annotations(self.eng.thread_reads_panel(arrays, bases, offsets, lists, read_index, mate), want, "thread_reads_panel")
            if len(bases):
                import torch
                db, do = torch.from_numpy(bases.copy()).cuda(), torch.from_numpy(offsets.astype(np.int64)).cuda()
                torch.cuda.synchronize()
                self.same_annotations(self.eng.thread_reads_panel(arrays, db, do, lists, read_index, mate, device=True), want,
                                      "thread_reads_panel, device buffers")
        self.op_export()

    def op_neighborhood_panel(self, r):
        """shk_neighborhood_panel: 2-3 jobs of op_neighborhood's kind and bounds, one max_levels for all."""
        rng = np.random.default_rng(r)
        jobs, marks = [], []
        for _ in range(int(rng.integers(2, 4))):
            nodes, dirs, counts, m = self.graph_seeds(rng) if self.ctx["k"] >= 2 else ([0], [1], np.zeros(0, np.uint32), [])
            n_distinct = len({(n, b) for n, d in zip(nodes, dirs) for b in (1, 2) if d & b})
            jobs.append((nodes, dirs, int(rng.choice([0, 1, 2, int(counts[int(rng.integers(0, len(counts)))]) if len(counts) else 3, U32_MAX])),
                         int(rng.choice([0, 1, 64, 4096])), int(rng.choice([n_distinct, 64, 4096]))))
        max_levels = int(rng.integers(1, 7))
        self.done[-1] = ("neighborhood_panel", dict(r=r, jobs=jobs, max_levels=max_levels))
        try:
            want = self.model.neighborhood_panel(jobs, max_levels)
        except ModelError as e:   # a multi-device context without the flag (SHK_ERR_STATE), k = 1 (SHK_ERR_BAD_ARG)
            self.refused(e, "neighborhood_panel", jobs, max_levels)
            return
        if self.live:
            got = self.eng.neighborhood_panel(jobs, max_levels)
            self.same(len(got), len(want), "neighborhood_panel: jobs")
            for j, (a, b) in enumerate(zip(got, want)):
                for what, g, w in zip(("k-mers", "counts", "fringe nodes", "fringe dirs", "levels done"), a, b):
                    self.same(g, w, "neighborhood_panel: job %d %s" % (j, what))
        self.graph_call_answered(self.model.export()[1])
        self.pos.observe(group_graph=self.group_graph)
        self.op_export()

    def op_prune_panel(self, r):
        """shk_pcr_prune_panel against tests/prune_ref.py: the model's pcr_extend graph under the default parameters and
        under drawn ones, and a drawn graph that has something to remove — a chain from a start to an end node, tips of
        count 1 hanging off it and an island no walk reaches."""
        rng = np.random.default_rng(r)
        k = self.ctx["k"]
        graphs, fractions, stages = [], [], []
        try:
            fwd, rev, a = self.extend_args(rng)
            g = self.model.pcr_extend(fwd, rev, **a)[0]
            extended = (list(g.sub_kmer), g.flags(), [e[0] for e in g.edges], [e[1] for e in g.edges], [e[2] for e in g.edges])
            graphs += [extended, extended]
            fractions += [0.1, float(rng.choice([0.0, 0.5, 1.0, 3.0]))]
            stages += [3, int(rng.integers(1, 4))]
        except ModelError:   # (a multi-device context without the flag has no such graph)
            pass
        n = int(rng.integers(4, 30))
        flags = [1] + [0] * (n - 2) + [2]
        src, tgt, counts = list(range(n - 1)), list(range(1, n)), [int(c) for c in rng.integers(20, 60, size=n - 1)]
        for _ in range(int(rng.integers(1, 4))):   # a tip: one node, out of or into the chain
            at = int(rng.integers(1, n - 1))
            flags.append(0)
            src.append(at if rng.random() < 0.5 else len(flags) - 1)
            tgt.append(len(flags) - 1 if src[-1] == at else at)
            counts.append(1)
        flags += [0, 0]
        src.append(len(flags) - 2)
        tgt.append(len(flags) - 1)
        counts.append(int(rng.integers(1, 60)))
        graphs.append(([int(x) for x in random_kmers(rng, k - 1, len(flags))], flags, src, tgt, counts))
        fractions.append(0.1)
        stages.append(int(rng.choice([1, 2, 3, 3])))
        self.done[-1] = ("prune_panel", dict(r=r, graphs=graphs, fractions=fractions, stages=stages))
        want = self.model.prune_panel([g[1:] for g in graphs], fractions, stages)
        self.facts.append(("prune_panel", dict(removed=sum(len(w.node_keep) - sum(w.node_keep) for w in want))))
        if self.live:
            got = self.eng.pcr_prune_panel([(np.array(g[0], dtype=np.uint64), g[1], g[2], g[3], g[4]) for g in graphs], fractions, stages)
            self.same(len(got), len(want), "pcr_prune_panel: genes")
            for i, (a, w, g) in enumerate(zip(got, want, graphs)):
                for field, x, y in (("node_keep", a.node_keep, w.node_keep), ("node_index", a.node_index, w.node_index),
                                    ("node_flags", a.node_flags, w.node_flags), ("node_sub_kmers", a.node_sub_kmers, [g[0][v] for v in w.node_index]),
                                    ("edge_index", a.edge_index, w.edge_index), ("edge_src", a.edge_src, w.edge_src), ("edge_tgt", a.edge_tgt, w.edge_tgt),
                                    ("edge_counts", a.edge_counts, w.edge_counts), ("coverage_ratio", f64_bits(a.coverage_ratio), f64_bits(w.coverage_ratio)),
                                    ("median", f64_bits([a.median]), f64_bits([w.median])),
                                    ("tip_rounds, tips_removed, unreachable_removed", (a.tip_rounds, a.tips_removed, a.unreachable_removed),
                                     (w.tip_rounds, w.tips_removed, w.unreachable_removed))):
                    self.same(np.asarray(x).ravel(), np.asarray(y).ravel(), "pcr_prune_panel: gene %d %s" % (i, field))
        self.pos.observe()
        self.op_export()

    def op_dedup_panel(self, r):
        """shk_pcr_dedup_panel against tests/products_ref.py: per gene 3-8 records — a stretch of a retained (or a batch's)
        read, a copy of it, copies with a few substitutions and indels, a stretch from elsewhere."""
        rng = np.random.default_rng(r)
        reads = self.model.retained
        if not reads:
            bases, offsets = small_batch(r)
            raw = bases.tobytes()
            reads = [raw[int(a):int(b)] for a, b in zip(offsets[:-1], offsets[1:])]
        letters = np.frombuffer(b"ACGT", dtype=np.uint8)

        def stretch():
            n = int(rng.integers(30, 120))
            for _ in range(10 if reads else 0):
                parts = [p for p in reads[int(rng.integers(0, len(reads)))][:THREAD_LEN].split(b"N") if len(p) >= n]
                if parts:
                    at = int(rng.integers(0, len(parts[0]) - n + 1))
                    return parts[0][at:at + n].decode()
            return letters[rng.integers(0, 4, size=n)].tobytes().decode()

        def edited(s, n_edits):
            s = list(s)
            for _ in range(n_edits):
                at, how = int(rng.integers(0, len(s))), int(rng.integers(0, 3))
                if how == 0:
                    s[at] = "ACGT"[("ACGT".index(s[at]) + 1 + int(rng.integers(0, 3))) % 4]
                elif how == 1:
                    s.insert(at, "ACGT"[int(rng.integers(0, 4))])
                elif len(s) > 1:
                    del s[at]
            return "".join(s)

        records, scores, thresholds = [], [], []
        for _ in range(int(rng.integers(1, 3))):
            base = stretch()
            recs = [base, base, stretch()]
            while len(recs) < int(rng.integers(3, 9)):
                recs.append(edited(base, int(rng.choice([1, 1, 2, 3, 12]))))
            recs = [recs[int(i)] for i in rng.permutation(len(recs))]
            records.append(recs)
            scores.append([float(x) for x in rng.integers(0, 3, size=len(recs))])
            thresholds.append(int(rng.choice([0, 1, 10])))
        self.done[-1] = ("dedup_panel", dict(r=r, records=records, scores=scores, thresholds=thresholds))
        want = self.model.dedup_panel(records, scores, thresholds)
        self.facts.append(("dedup_panel", dict(within=any(any(w[1]) for w in want), outside=any(not all(w[1]) for w in want))))
        if self.live:
            got = self.eng.pcr_dedup_panel(records, scores, thresholds, want_pairs=True)
            self.same(len(got), len(want), "pcr_dedup_panel: genes")
            for g, (a, w) in enumerate(zip(got, want)):
                for field, x, y in (("order", a.order, w[0]), ("pair bits", a.pair_bits, w[1]), ("kept", a.kept, w[2]),
                                    ("generated, retained", (a.generated, a.retained), w[3:])):
                    self.same(np.asarray(x).ravel(), np.asarray(y).ravel(), "pcr_dedup_panel: gene %d %s" % (g, field))
        self.pos.observe()
        self.op_export()


def _brief(x):
    if isinstance(x, tuple):
        return "(" + ", ".join(_brief(y) for y in x) + ")"
    a = np.asarray(x)
    return "%s%s %s%s" % (a.dtype, list(a.shape), a.ravel()[:8].tolist(), "…" if a.size > 8 else "")


def dry_run(orc, seed):
    """The draw and the model alone → what the seed covers (positions and kinds; the routes need the engine)."""
    return dry_sequence(orc, seed).met_here


def dry_sequence(orc, seed):
    """The same → the Sequence itself: met_here, and `facts` — what the third generator's expected answers held."""
    s = Sequence(orc, seed, engine=False)
    s.run()
    return s


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
