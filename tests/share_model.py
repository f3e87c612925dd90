"""A world of W owner shares, call by call — the expected answer of tests/test_gpu_share_sequences.py.  CPU only, oracle
only, built on tests/lane_model.py's parts: a share is a LaneModel that is handed k-mers instead of reads.

Share o holds exactly the canonical k-mers whose owner — shk_key_owner(k, W, k-mer), restated here as `owner_of` and
held against the library by tests/test_share_model_cpu.py — is o; their chunk lanes follow the GLOBAL read index (read i
→ lane (i / 1000) % chunks, io.rs:340-361), whoever scattered or ingested the read.  What a round moves is computed when
it is scattered (`ShareWorld.scatter` → a Parcel: per owner and lane the k-mers and how often) and lands when it is
delivered (`deliver`): a reset, an observation or nothing at all may lie in between, and a parcel that is never
delivered leaves no trace but the scattering share's read and base counters (include/shk.h: they count every read
HANDED to the context).

Beside the shares there is `whole`: the one-context LaneModel of the same job — every delivered batch ingested as
reads, every insert applied once — which the union of the shares must equal at every observation (`check_union`).  A
reset of ONE share has no counterpart there: `whole_valid` is false from then until the next reset of all of them.

The feasibility of the owner-layout round is restated from shk_engine.hip (part_geom, xl_feasible, xl64_feasible,
xchg_rec_bytes at the geometry shk_create leaves) in `xchg_geometry`; the GPU sweep holds it against
shk_xchg_feasible on every context it makes."""
from __future__ import annotations

import math

import numpy as np

from lane_model import LaneModel, ModelError, SHK_ERR_STATE

MIX_M32, MIX_M64, MIX_NARROW_BITS = 0xC2B2AE35, 0x9E3779B97F4A7C15, 42   # sharkmer_amd/csrc/shk_mix.h
FLAG_FORCE_DIRECT = 2                                                     # include/shk.h
PAGE_LOG, MAX_LOG_PAGES, MAX_PARTS, TILE_T, RB_LOG = 13, 20, 4096, 16384, 10   # shk_device.hip.h

# the refusals' texts (shk_engine.hip, shk_table_api.hip.h); "%s": the call's name
NOT_A_SHARE = "not an owner share (shk_config.n_owners = 0: say 1 for a share that is the whole key space)"
TAKE_THE_WIDE_ROUND = "take the wide round or merge the tables at finalize instead"
IS_A_SHARE = "%s needs the whole table on one device: this context is an owner share (n_owners > 1)"
SCATTER_BEGUN = "an exchange scatter is begun and not ended (shk_xchg_scatter_end)"
NO_SCATTER_BEGUN = "no exchange scatter is begun (shk_xchg_scatter_begin)"
REFUSAL_TEXTS = (NOT_A_SHARE, TAKE_THE_WIDE_ROUND, IS_A_SHARE, SCATTER_BEGUN, NO_SCATTER_BEGUN)
KMER_TOTALS = ("n_kmers_ingested", "n_unique_kmers", "n_hashed_kmers")


def owner_of(k: int, W: int, keys) -> np.ndarray:
    """shk_key_owner: the top log2(W) bits of (key · M) mod 2^2k."""
    keys = np.asarray(keys, dtype=np.uint64)
    lw, bits = W.bit_length() - 1, 2 * k
    if lw == 0:
        return np.zeros(len(keys), dtype=np.int64)
    m = np.uint64(MIX_M32 if bits <= MIX_NARROW_BITS else MIX_M64)
    with np.errstate(over="ignore"):
        mixed = (keys * m) & np.uint64((1 << bits) - 1)
    return (mixed >> np.uint64(bits - lw)).astype(np.int64)


def xchg_geometry(k: int, chunks: int, W: int, hint: int, flags: int, hooks: dict) -> dict:
    """What shk_create leaves an owner share with, as far as the exchange looks at it → dict(log_p1, record_bytes (0: only
    the wide round), region_cap(layout_bases))."""
    env = lambda name, dflt: int(hooks.get(name, dflt))
    lw, lanes, lvl1 = W.bit_length() - 1, max(chunks, 1), env("SHK_LEVEL1_LOG", 10)
    want = hint * 2 if hint else 1 << 20
    if 2 * k > 32 + lw and 2 * k - 32 <= lvl1:
        want = max(want, (1 << PAGE_LOG) << (2 * k - 32 - lw))
    if lvl1 > lw:
        want = max(want, (1 << PAGE_LOG) << (lvl1 - lw))
    lp = 0
    while ((1 << PAGE_LOG) << lp) < want and lp + lw < MAX_LOG_PAGES:
        lp += 1
    lpg = lp + lw
    log_p1 = max(min(lvl1, lpg), lw)
    log_sub, P1 = lpg - log_p1, 1 << log_p1
    rbits, r1_bits = max(2 * k - lpg, 0), max(2 * k - log_p1, 0)
    rec32 = 11 <= rbits <= 32 and r1_bits <= 32
    lds32 = 16 * 1024 * 8 + P1 * 12 + 32 <= 160 * 1024 - 2048
    xl = rec32 and lds32 and (1 << log_sub) <= MAX_PARTS and lanes <= 128 and lpg <= MAX_LOG_PAGES
    lds64 = (16 * 1024 + P1) * 8 + P1 * 12 + (1024 + 2) * 8 + 32 <= 160 * 1024 - 2048
    xl64 = (not rec32 and log_p1 >= 3 and P1 <= 1024 and k >= 18 and lds64 and log_sub <= 10 and lanes <= 32 and lpg <= MAX_LOG_PAGES
            and env("SHK_XL64", 1) != 0)
    deferred = lpg <= 20 and lanes <= 128 and not (flags & FLAG_FORCE_DIRECT) and (xl or xl64)   # count_path(c, 0) == PATH_DEFER
    record_bytes = 4 if xl and deferred else 8 if xl64 else 0

    def region_cap(layout_bases: int) -> int:   # xchg_plan
        B = -(-layout_bases // TILE_T) * TILE_T
        lane_ub = min(B, B // lanes * 11 // 10 + 262144) if lanes > 1 else B
        mean = lane_ub / P1
        cap = int(mean * 1.05 + 8.0 * math.sqrt(mean)) + 1024
        return -(-cap // (1 << RB_LOG)) * (1 << RB_LOG)
    return dict(log_p1=log_p1, record_bytes=record_bytes, region_cap=region_cap)


class ShareModel(LaneModel):
    """One owner share: LaneModel's lanes, observations and checks over the k-mers it owns."""

    def __init__(self, orc, k, chunks, histo_max, W, owner):
        self.W, self.owner = W, owner
        super().__init__(orc, k, chunks, histo_max)

    def is_empty(self) -> bool:
        """shk_engine.hip, finalize_scan: a share without reads does not fail (the caller looks at the sum over the shares)."""
        return False

    def handed(self, bases, offsets):
        """The read and base counters of a batch handed to this context, whatever becomes of its k-mers."""
        lo, hi = int(offsets[0]), int(offsets[-1])
        self.n_reads += len(offsets) - 1
        self.n_bases_read += hi - lo
        self.n_bases_ingested += int((np.asarray(bases[lo:hi]) != ord("N")).sum())

    def add(self, lane: int, keys, counts):
        """Occurrences of owned k-mers: `counts[i]` saturating adds of one (counting.rs:82-85) are one add of counts[i]."""
        self._obs = None
        table = self.lanes[lane]
        for key, c in zip(np.asarray(keys).tolist(), np.asarray(counts).tolist()):
            table.insert(key, c)

    def graph_table(self, what: str):
        if self.W > 1:
            raise ModelError(IS_A_SHARE % what, SHK_ERR_STATE)
        return super().graph_table(what)


class Parcel:
    """One rank's scattered batch: per owner [(lane, k-mers, occurrences)], and the batch itself for `whole`."""

    def __init__(self, rank, per_owner, bases, offsets, first):
        self.rank, self.per_owner, self.bases, self.offsets, self.first = rank, per_owner, bases, offsets, first

    def occurrences(self, owner: int) -> int:
        return sum(int(c.sum()) for _, _, c in self.per_owner[owner])


class ShareWorld:
    def __init__(self, orc, k: int, chunks: int, histo_max: int, W: int):
        self.orc, self.k, self.chunks, self.histo_max, self.W = orc, k, chunks, histo_max, W
        self.n_lanes = max(chunks, 1)
        self.shares = [ShareModel(orc, k, chunks, histo_max, W, o) for o in range(W)]
        self.whole = LaneModel(orc, k, chunks, histo_max)
        self.whole_valid = True

    def owner_of(self, keys) -> np.ndarray:
        return owner_of(self.k, self.W, keys)

    def split(self, bases, offsets, first: int):
        """→ per owner [(lane, k-mers, occurrences)] of reads whose global indices start at `first`."""
        off = np.asarray(offsets, dtype=np.int64)
        lo, hi = int(off[0]), int(off[-1])
        kmers, read = self.orc.canonical_kmers_numpy(np.asarray(bases[lo:hi], dtype=np.uint8), off - lo, self.k, return_read_id=True)
        lane = ((first + read) // 1000) % self.n_lanes
        own = self.owner_of(kmers)
        out = []
        for o in range(self.W):
            parts = []
            for l in np.unique(lane[own == o]).tolist():
                keys, counts = np.unique(kmers[(own == o) & (lane == l)], return_counts=True)
                parts.append((int(l), keys, counts))
            out.append(parts)
        return out

    def scatter(self, rank: int, bases, offsets, first: int) -> Parcel:
        """Any of the three round forms on share `rank`: set_read_index(first), then the batch.  An invalid byte: the
        reference's error (encoding.rs:353-356), nothing counted."""
        bad = LaneModel.first_bad_byte(bases, [int(x) for x in offsets])
        if bad is not None:
            raise ModelError(LaneModel.bad_byte_message(bad))
        s = self.shares[rank]
        s.handed(bases, offsets)
        s.read_index = first + len(offsets) - 1
        return Parcel(rank, self.split(bases, offsets, first), bases, offsets, first)

    def deliver(self, parcel: Parcel):
        """Every owner absorbs its segment of the parcel."""
        for o in range(self.W):
            for lane, keys, counts in parcel.per_owner[o]:
                self.shares[o].add(lane, keys, counts)
        if len(parcel.offsets) > 1:
            self.whole.set_read_index(parcel.first)
            self.whole.ingest_reads(parcel.bases, parcel.offsets)

    def drop_ingest(self, bases, offsets, first: int):
        """Drop-mode ingest: every share is handed the batch at the same global index and keeps what it owns."""
        per_owner = self.split(bases, offsets, first)
        for o, s in enumerate(self.shares):
            s.handed(bases, offsets)
            s.read_index = first + len(offsets) - 1
            for lane, keys, counts in per_owner[o]:
                s.add(lane, keys, counts)
        self.whole.set_read_index(first)
        self.whole.ingest_reads(bases, offsets)

    def insert(self, lane: int, keys, counts, ranks=None):
        """shk_insert_counts / shk_insert_device on the shares `ranks` (None: all): foreign k-mers are dropped."""
        keys, counts = np.asarray(keys, dtype=np.uint64), np.asarray(counts, dtype=np.uint32)
        own = self.owner_of(keys)
        for o in range(self.W) if ranks is None else ranks:
            mine = own == o
            if mine.any():
                self.shares[o].insert(lane, keys[mine], counts[mine])
                self.whole.insert(lane, keys[mine], counts[mine])

    def reset(self, rank=None):
        if rank is None:
            for s in self.shares:
                s.reset()
            self.whole.reset()
            self.whole_valid = True
        else:
            self.shares[rank].reset()
            self.whole_valid = self.whole_valid and self.W == 1
            if self.W == 1:
                self.whole.reset()

    def union(self):
        """→ (Σ histogram columns, the shares' exports merged and sorted, Σ k-mer totals, any share saturated)."""
        cols = sum(s.observe().columns.astype(object) for s in self.shares)
        keys = np.concatenate([s.export()[0] for s in self.shares])
        counts = np.concatenate([s.export()[1] for s in self.shares])
        order = np.argsort(keys, kind="stable")
        tot = {f: sum(s.totals()[f] for s in self.shares) for f in KMER_TOTALS}
        return cols, keys[order], counts[order], tot, int(any(s.totals()["any_saturated"] for s in self.shares))

    def check_union(self) -> bool:
        """The shares together are the one-context model of the same job: histogram columns, table, totals.  Share by
        share, every key is its owner's.  → whether `whole` was there to compare with."""
        for o, s in enumerate(self.shares):
            assert (self.owner_of(s.export()[0]) == o).all(), "share %d holds a k-mer it does not own" % o
        if not self.whole_valid:
            return False
        cols, keys, counts, tot, sat = self.union()
        w = self.whole.observe()
        assert np.array_equal(cols, w.columns.astype(object)), "Σ shares' histogram columns differ from the one-context model's"
        assert np.array_equal(keys, w.keys) and np.array_equal(counts, w.counts), "the union of the shares' tables differs from the one-context model's"
        wt = self.whole.totals()
        assert tot == {f: wt[f] for f in KMER_TOTALS} and sat == wt["any_saturated"], (tot, sat, wt)
        return True
