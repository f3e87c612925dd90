// shk_device.hip.h — gfx950 device code of libshk (hand-written HIP, wave64).
//
// Data layout in HBM:
//   bases      u8 [n_bases]             concatenated ASCII reads (as handed over)
//   startbits  u32[n_bases/32+2]        bit p set ⇔ position p is the first base of a read
//   tiles      TileDesc[n_tiles]        ≤TILE_T-base spans, never crossing a 1000-read block
//   keys       u64[n_pages*PAGE_SLOTS]  canonical k-mer or EMPTY; page = top hash bits,
//                                       linear probing confined to the page
//   vals       u32[n_lanes][capacity]   per-chunk-lane counts, lane-major
//
// Reference semantics reproduced (file:line under /root/reference):
//   extraction   src/kmer/encoding.rs:332-371 (kmers_from_ascii), :374-376
//   counting     src/kmer/counting.rs:82-85 (entry().or_insert(0); saturating_add)
//   histogram    src/kmer/counting.rs:171-202 + src/kmer/histogram.rs:51-85,125-134
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>
#include <stddef.h>
#include <stdint.h>

#include "shk_inflate_core.h"
#include "shk_fastq_text_core.h"
#include "shk_retain_core.h"
#include "shk_mix.h"

namespace shk {

constexpr uint64_t EMPTY = 0xFFFFFFFFFFFFFFFFull;  // never a k-mer: k<32 ⇒ key < 2^62
constexpr int PAGE_LOG = 13;
constexpr uint32_t PAGE_SLOTS = 1u << PAGE_LOG;     // 8192 slots: 64 KiB keys + 32 KiB counts in LDS
constexpr int WG = 256;                             // 4 waves
constexpr int TILE_T = 16384;                       // k-mer end positions per tile
constexpr int HALO = 32;                            // ≥ k-1 bases before the tile (k ≤ 31)
constexpr int TILE_LDS = TILE_T + HALO;               // code bytes of one staged tile
constexpr int TILE_GROUPS = TILE_LDS / 16;            // 16-base groups
constexpr int STAGE_BYTES = TILE_LDS + 4 * TILE_GROUPS;  // + one (N|start) mask word per group

struct TileDesc {
  uint64_t begin;  // first k-mer END position owned by the tile
  uint64_t end;    // one past the last
  uint32_t lane;   // chunk lane of the enclosing 1000-read block
  uint32_t pad;
};

struct DevStats {
  unsigned long long bad;          // min over (position<<8 | byte) of invalid bytes; ~0 = none
  unsigned long long bad_pad;      // (bad, bad_pad) = the control block's first 16-B word: reset fills it with ~0
  unsigned long long n_distinct;   // keys inserted so far (all launches)
  unsigned long long spill_count;  // entries in the spill list (this launch)
  unsigned long long n_tiles;      // written by k_build_tiles
  unsigned long long scratch[3];
};
static_assert(sizeof(DevStats) == 64 && offsetof(DevStats, bad) == 0, "control block layout");

struct TableRef {
  uint64_t *keys;
  uint32_t *vals;
  uint64_t cap;      // n_pages * PAGE_SLOTS
  uint32_t log_pages;
  uint32_t n_lanes;
  uint32_t key_bits;  // 2k
  // OWNER SHARE (key-space-partitioned ingest, SURVEY.md §8e "alternative when local tables do not
  // fit"): the table is the slice of owner `owner_id` — the pages whose top `owner_bits` bits of the
  // GLOBAL page index (top owner_bits + log_pages bits of the mixed key) equal owner_id — of a virtual
  // table of 2^(owner_bits + log_pages) pages.  owner_bits = 0: the whole key space (owner_id = 0).
  uint32_t owner_bits;
  uint32_t owner_id;
  uint32_t pad_;
};

struct BatchRef {
  const uint8_t *bases;
  const uint32_t *startbits;
  uint64_t n_bases;
  const TileDesc *tiles;  // nullptr ⇒ one block: tile t = [t*TILE_T, …) ∩ [0,n_bases), lane = lane0
  const DevStats *stats;  // n_tiles lives here when tiles != nullptr
  uint64_t n_tiles_single;
  uint64_t tile_first;  // this launch covers tiles [tile_first, tile_first + tile_count)
  uint64_t tile_count;
  uint32_t lane0;
  int k;
};

struct SpillRef {
  uint64_t *keys;
  uint32_t *lanes;
  uint32_t *counts;
  uint64_t cap;
  unsigned long long *count;  // the list's fill counter; nullptr = DevStats::spill_count (k_scatter32 only looks at this)
};

// ---- hashing.  Results never depend on it — only speed does, and on gfx950
// 32-bit integer multiplies issue at quarter rate while 24-bit ones (v_mad_u32_u24) are full
// rate.  So: multilinear hash of the key's three 24-bit chunks (full rate) + one xorshift-
// multiply finaliser.  Page = top log_pages bits, in-page home slot = the next 12.
// tools/hash_eval.py: page occupancy and slot collisions match a Poisson process on random,
// AT-rich, tandem-repeat and sequential keys (without the finaliser sequential keys collide).
constexpr uint32_t MAX_LOG_PAGES = 20;  // page bits + the 11 home-bucket bits ≤ 32 hash bits; 2^33 slots ≈ 103 GB
// mix_key / unmix_key, the bijective key mix everything below reads its geometry from: shk_mix.h (shared with the host side).
// the 32 hash bits the table geometry is read from: the top of the mixed key
__device__ __forceinline__ uint32_t hash64(uint64_t key, uint32_t bits) {
  return (uint32_t)((mix_key(key, bits) << (64 - bits)) >> 32);
}
// a full-avalanche hash for small open-addressing sets that index by LOW bits (k_filter_reads' primer set)
__host__ __device__ __forceinline__ uint32_t set_hash(uint64_t key) {
  key ^= key >> 31;
  return (uint32_t)((key * MIX_M64) >> 32);
}
__device__ __forceinline__ uint64_t page_of(uint32_t h, uint32_t log_pages) {
  return log_pages ? (uint64_t)(h >> (32 - log_pages)) : 0ull;
}
// Home slots are bucket-aligned (multiples of 4): a key is almost always found inside the 32-B
// bucket its probe sequence starts in, which k_pages reads with two 16-B LDS loads.
__device__ __forceinline__ uint32_t slot_of(uint32_t h, uint32_t log_pages) {
  return ((h >> (32 - (PAGE_LOG - 2) - log_pages)) & (PAGE_SLOTS / 4 - 1)) << 2;  // the 11 bits below the page bits
}
static_assert(MAX_LOG_PAGES + PAGE_LOG - 2 <= 32, "page + home-bucket bits come out of 32 hash bits");
// Where a key lives in a table that may be an owner share: page (as a slot base in the LOCAL arrays),
// home slot, and whether this table owns the key at all.
struct Home {
  uint64_t base;
  uint32_t slot;
  bool owned;
};
__device__ __forceinline__ Home home_of(const TableRef &tb, uint64_t key) {
  const uint32_t h = hash64(key, tb.key_bits);
  const uint32_t lpg = tb.log_pages + tb.owner_bits;  // page bits of the virtual global table
  const uint64_t gp = page_of(h, lpg);
  Home r;
  r.owned = (uint32_t)(gp >> tb.log_pages) == tb.owner_id;
  r.base = (gp & ((1ull << tb.log_pages) - 1ull)) << PAGE_LOG;
  r.slot = slot_of(h, lpg);
  return r;
}

__device__ __forceinline__ uint32_t sat_add_u32(uint32_t a, uint32_t b) {
  uint32_t s = a + b;
  return s < a ? 0xFFFFFFFFu : s;
}

// ---- tile geometry -------------------------------------------------------------------
__device__ __forceinline__ bool tile_get(const BatchRef &b, uint64_t t, uint64_t &t0, uint64_t &t1,
                                         uint32_t &lane) {
  if (t >= b.tile_count) return false;
  t += b.tile_first;
  if (b.tiles) {
    if (t >= b.stats->n_tiles) return false;
    TileDesc d = b.tiles[t];
    t0 = d.begin;
    t1 = d.end;
    lane = d.lane;
  } else {
    if (t >= b.n_tiles_single) return false;
    t0 = t * (uint64_t)TILE_T;
    t1 = t0 + TILE_T < b.n_bases ? t0 + TILE_T : b.n_bases;
    lane = b.lane0;
  }
  return true;
}

// Advance t (stride gridDim.x) to this workgroup's next tile, optionally only tiles of one
// chunk lane.  Uniform across the workgroup.
__device__ __forceinline__ bool next_tile(const BatchRef &b, uint64_t &t, bool use_filter,
                                          uint32_t lane_filter, uint64_t &t0, uint64_t &t1,
                                          uint32_t &lane) {
  while (tile_get(b, t, t0, t1, lane)) {
    if (!use_filter || lane == lane_filter) return true;
    t += gridDim.x;
  }
  return false;
}

// ASCII → 2-bit base for 4 bytes at once: A,C,G,T → 0..3 via ((c>>1)^(c>>2))&3 ('N' → 0);
// *nbytes gets 0x80 in every byte that is 'N' — for VALID input: among A,C,G,T,N only N has
// bit 3 set.  (Input with any other byte is rejected as a whole, encoding.rs:353-356: nothing
// derived from it is ever used.)
__device__ __forceinline__ uint32_t codes4(uint32_t w, uint32_t *nbytes) {
  *nbytes = (w << 4) & 0x80808080u;
  return ((w >> 1) ^ (w >> 2)) & 0x03030303u;
}
// the four byte-MSBs of z gathered into bits 0-3, byte order kept
__device__ __forceinline__ uint32_t msb_gather4(uint32_t z) { return (z * 0x00204081u) >> 28; }
// Bytes of w that are none of A,C,G,T,N (non-zero result ⇔ some byte is invalid,
// encoding.rs:341-356), given w's codes c: a byte is valid exactly when it equals the letter
// that its own (bit 3, 2-bit code) stands for, and that letter comes out of an 8-entry byte table
// in one v_perm_b32 — selectors 0-3 → A C G T, 4 → N (bit 3 set, code 0), 5-7 → 0x00, which no
// byte with bit 3 set equals.
__device__ __forceinline__ uint32_t invalid_bytes4(uint32_t w, uint32_t c) {
  const uint32_t sel = c | ((w >> 1) & 0x04040404u);
  return w ^ __builtin_amdgcn_perm(0x0000004Eu /* . . . N */, 0x54474341u /* T G C A */, sel);
}

// Is byte c one of A,C,G,T,N?  (A=0x41 C=0x43 G=0x47 N=0x4E T=0x54 → bits 1,3,7,14,20 of
// the 0x40..0x5F word.)  encoding.rs:341-356.
__device__ __forceinline__ bool byte_is_acgtn(uint32_t c) {
  return (c >> 5) == 2 && ((0x0010408Au >> (c & 31)) & 1u);
}
// 2-bit packed copies of a staged tile (16 bases per u32, first base on top): PACK_WORDS words
// each — the forward stream, and the mirrored complement stream in which base j of the tile is
// base TILE_LDS-1-j, so that the reverse complement of a window is a window again.
constexpr int PACK_WORDS = TILE_GROUPS + 2;  // + 2 pad words (a window read touches 3 words)
static_assert(TILE_T <= (1 << 14) && TILE_LDS % 16 == 0, "sorted entries: 14-bit position + strand bit");
__device__ __forceinline__ uint32_t pack4(uint32_t c) {  // 4 code bytes (0..3 each) → 8 bits, first base on top
  return (c * 0x40100401u) >> 24;                        // the four 2-bit fields land in bits 31..24, no carries
}
__device__ __forceinline__ uint32_t pack16(uint4 c4) {
  return (pack4(c4.x) << 24) | (pack4(c4.y) << 16) | (pack4(c4.z) << 8) | pack4(c4.w);
}
// reverse the order of the sixteen 2-bit fields of x
__device__ __forceinline__ uint32_t rev2(uint32_t x) {
  x = ((x >> 2) & 0x33333333u) | ((x & 0x33333333u) << 2);
  x = ((x >> 4) & 0x0F0F0F0Fu) | ((x & 0x0F0F0F0Fu) << 4);
  return __builtin_bswap32(x);
}

// Stage positions [t0-HALO, t0+TILE_T) of the batch into LDS as one code byte per base:
// bits 0-1 = base, bit 2 = "a valid k-mer ENDS here", i.e. the k bases up to and including
// this one lie in one read and none is N (encoding.rs:346-352,363: n_valid ≥ k).  The bit is
// computed bit-parallel for 16 positions at a time from per-group masks of N positions and
// read-start positions (smeared over k resp. k-1 positions), so the walks below carry no
// per-base validity state at all.
// VALIDATE: additionally check every byte of [t0,t1) against ACGTN (encoding.rs:353-356;
// the first offender in input order is reported through stats->bad) and return this
// thread's count of non-N bytes in [t0,t1) (count_valid_bases, encoding.rs:374-376).
// Contains one __syncthreads(); the caller adds another before reading the codes.
// Bytewise staging of a 16-base group that touches the start or the end of the batch (a few
// groups per launch).  Kept out of line: inlined into the unrolled staging loop it costs the
// callers > 100 VGPRs.  Returns x = the 16 base codes, 2 bits each (base i at bits 2i),
// y = the group's N / outside-the-batch mask, z = its non-N count (VALIDATE only).
__device__ __noinline__ uint4 stage_edge_group(const uint8_t *bases, uint64_t n_bases, int64_t p,
                                               uint64_t t0, uint64_t t1, bool validate,
                                               DevStats *stats) {
  uint32_t codes = 0, nmask = 0, n_non_n = 0;
  for (int r = 0; r < 16; ++r) {
    int64_t pp = p + r;
    uint32_t c = 0, isn = 1;  // outside the batch: behaves like N
    if (pp >= 0 && (uint64_t)pp < n_bases) {
      uint32_t a = bases[pp];
      isn = a == 'N';
      c = isn ? 0u : (((a >> 1) ^ (a >> 2)) & 3u);
      if (validate && (uint64_t)pp >= t0 && (uint64_t)pp < t1) {
        if (!byte_is_acgtn(a)) atomicMin(&stats->bad, ((unsigned long long)pp << 8) | a);
        n_non_n += (a != 'N');
      }
    }
    codes |= c << (2 * r);
    nmask |= isn << r;
  }
  return make_uint4(codes, nmask, n_non_n, 0u);
}

// Raw bytes + read-start words of one thread's share of a tile, loaded ahead of time so that
// the HBM latency of tile i+1 hides behind the processing of tile i.
template <int NT, int TT = TILE_T>
struct StageRegs {
  static constexpr int GROUPS = (TT + HALO) / 16;  // 16-base groups of one staged tile of TT end positions
  static constexpr int R = (GROUPS + NT - 1) / NT;
  uint32_t raw[R][4];
  uint32_t sb0[R], sb1[R];
};
template <int NT, int TT = TILE_T>
__device__ __forceinline__ void stage_prefetch(const BatchRef &b, uint64_t t0, StageRegs<NT, TT> &pre) {
  constexpr int TILE_GROUPS = StageRegs<NT, TT>::GROUPS;
  const int64_t p0 = (int64_t)t0 - HALO;
#pragma unroll
  for (int r = 0; r < StageRegs<NT, TT>::R; ++r) {
    const int m = threadIdx.x + r * NT;
    const int64_t p = p0 + (int64_t)m * 16;
    if (m < TILE_GROUPS && p >= 0 && (uint64_t)p + 16 <= b.n_bases) {
      __builtin_memcpy(pre.raw[r], b.bases + p, 16);  // unaligned 16-B global load (one dwordx4)
      pre.sb0[r] = b.startbits[(uint64_t)p >> 5];
      pre.sb1[r] = b.startbits[((uint64_t)p >> 5) + 1];
    }
  }
}

// NOBYTES (k_scatter32): no code byte per base at all — the first pass writes the 2-bit packed stream
// straight from its registers, the second one 16-bit word of "k-mer ends here" bits per group
// (okbits); `lds` then only holds the group masks.  The walk reads one word + one half-word per thread.
template <bool VALIDATE, int NT = WG, bool PACK = false, int TT = TILE_T, bool NOBYTES = false>
__device__ __forceinline__ uint32_t stage_tile(const BatchRef &b, uint64_t t0, uint64_t t1,
                                               uint8_t *lds, DevStats *stats,
                                               const StageRegs<NT, TT> &pre, uint32_t *packed = nullptr,
                                               uint32_t *rcpacked = nullptr, uint16_t *okbits = nullptr) {
  constexpr int TILE_GROUPS = StageRegs<NT, TT>::GROUPS;  // (shadow the file-scope constants: this
  constexpr int TILE_LDS = TT + HALO;                      // function stages tiles of TT positions)
  uint32_t *gmask = reinterpret_cast<uint32_t *>(NOBYTES ? lds : lds + TILE_LDS);  // nmask16 | smask16<<16
  const int64_t p0 = (int64_t)t0 - HALO;
  uint32_t n_non_n = 0;
#pragma unroll
  for (int r = 0; r < StageRegs<NT, TT>::R; ++r) {
    const int m = threadIdx.x + r * NT;
    if (m >= TILE_GROUPS) continue;  // (no break: keeps r a compile-time index into `pre`)
    int64_t p = p0 + (int64_t)m * 16;
    uint32_t w[4];
    uint32_t nmask = 0;
    const bool fast = p >= 0 && (uint64_t)p + 16 <= b.n_bases;  // same test as stage_prefetch
    if (fast) {
      w[0] = pre.raw[r][0];
      w[1] = pre.raw[r][1];
      w[2] = pre.raw[r][2];
      w[3] = pre.raw[r][3];
      if (VALIDATE && (uint64_t)p >= t0 && (uint64_t)p < t1) {
        if ((uint64_t)p + 16 <= t1) {
          uint32_t bad = 0, nn = 0;
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            uint32_t z;
            const uint32_t c = codes4(w[q], &z);  // (the conversion below recomputes it: CSE)
            bad |= invalid_bytes4(w[q], c);
            nn += __builtin_popcount(z);
          }
          n_non_n += 16 - nn;
          if (bad) {
            for (int r = 0; r < 16; ++r) {
              uint32_t c = (w[r >> 2] >> (8 * (r & 3))) & 0xFF;
              if (!byte_is_acgtn(c)) {
                atomicMin(&stats->bad, ((unsigned long long)(p + r) << 8) | c);
                break;
              }
            }
          }
        } else {
          for (int r = 0; r < 16 && (uint64_t)p + r < t1; ++r) {
            uint32_t c = (w[r >> 2] >> (8 * (r & 3))) & 0xFF;
            if (!byte_is_acgtn(c)) atomicMin(&stats->bad, ((unsigned long long)(p + r) << 8) | c);
            n_non_n += (c != 'N');
          }
        }
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        uint32_t z;
        w[q] = codes4(w[q], &z);
        nmask |= msb_gather4(z) << (4 * q);
      }
    } else {
      uint4 e = stage_edge_group(b.bases, b.n_bases, p, t0, t1, VALIDATE, stats);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        uint32_t c8 = (e.x >> (8 * q)) & 0xFFu;  // four 2-bit codes
        w[q] = (c8 & 3u) | (((c8 >> 2) & 3u) << 8) | (((c8 >> 4) & 3u) << 16) | (((c8 >> 6) & 3u) << 24);
      }
      nmask = e.y;
      n_non_n += e.z;
    }
    // read-start flags for these 16 positions: bits [p, p+16) of startbits
    uint32_t f = 0;
    if (fast) {
      uint64_t two = (uint64_t)pre.sb0[r] | ((uint64_t)pre.sb1[r] << 32);
      f = (uint32_t)(two >> ((uint32_t)p & 31)) & 0xFFFFu;
    } else if (p >= 0 && (uint64_t)p < b.n_bases) {
      uint64_t wi = (uint64_t)p >> 5;
      uint32_t sh = (uint32_t)p & 31;
      uint64_t two = (uint64_t)b.startbits[wi] | ((uint64_t)b.startbits[wi + 1] << 32);
      f = (uint32_t)(two >> sh) & 0xFFFFu;
    } else if (p < 0 && p + 16 > 0) {  // straddles position 0
      uint32_t lo = b.startbits[0];
      f = (lo << (uint32_t)(-p)) & 0xFFFFu;
    }
    if (NOBYTES) packed[m] = pack16(make_uint4(w[0], w[1], w[2], w[3]));
    else *reinterpret_cast<uint4 *>(lds + m * 16) = make_uint4(w[0], w[1], w[2], w[3]);
    gmask[m] = nmask | (f << 16);
    __builtin_amdgcn_sched_barrier(0);  // one group at a time: interleaving the unrolled
  }                                     // iterations costs > 100 VGPRs
  __syncthreads();
  // "k-mer ends here" bits: position j is bad if an N lies in [j-k+1, j] or a read starts in
  // [j-k+2, j].  48 mask bits (this group and the two before it) are smeared upwards.  Positions
  // at or beyond t1 (a tile that ends at a 1000-read block boundary) never get the bit, so the
  // walks need no end-of-tile test.  PACK: the 2-bit packed streams are written on the way.
  const int k = b.k;
  const int n_lds = (int)(t1 - t0) + HALO;  // LDS positions below this may end a k-mer
  if (NOBYTES) {
    if (threadIdx.x < 2) {  // the stream's pad words; halo groups never end a k-mer
      packed[TILE_GROUPS + threadIdx.x] = 0;
      okbits[threadIdx.x] = 0;
    }
  } else if (PACK) {
    for (int m = threadIdx.x; m < 2 + 2; m += NT) {  // halo groups 0,1 and the streams' pad words
      if (m < 2) {
        const uint32_t v = pack16(*reinterpret_cast<const uint4 *>(lds + m * 16));
        packed[m] = v;
        if (rcpacked) rcpacked[TILE_GROUPS - 1 - m] = rev2(~v);
      } else {
        packed[TILE_GROUPS + m - 2] = 0;
        if (rcpacked) rcpacked[TILE_GROUPS + m - 2] = 0;
      }
    }
  }
  for (int m = 2 + threadIdx.x; m < TILE_GROUPS; m += NT) {
    const uint32_t g0 = gmask[m - 2], g1 = gmask[m - 1], g2 = gmask[m];
    uint64_t N = (uint64_t)(g0 & 0xFFFFu) | ((uint64_t)(g1 & 0xFFFFu) << 16) |
                 ((uint64_t)(g2 & 0xFFFFu) << 32);
    uint64_t S = (uint64_t)(g0 >> 16) | ((uint64_t)(g1 >> 16) << 16) | ((uint64_t)(g2 >> 16) << 32);
    int s = 1;
    while (2 * s <= k) {
      N |= N << s;
      s *= 2;
    }
    if (k > s) N |= N << (k - s);
    if (k >= 2) {
      s = 1;
      while (2 * s <= k - 1) {
        S |= S << s;
        s *= 2;
      }
      if (k - 1 > s) S |= S << (k - 1 - s);
    } else {
      S = 0;
    }
    uint32_t ok = ~(uint32_t)((N | S) >> 32) & 0xFFFFu;  // m ≥ 2: ≥ 32 ≥ k-1 bases of history
    const int lim = n_lds - m * 16;                       // positions of this group below t1
    if (lim < 16) ok = lim > 0 ? ok & ((1u << lim) - 1u) : 0u;
    if (NOBYTES) {
      okbits[m] = (uint16_t)ok;
    } else if (PACK || ok) {
      uint4 c4 = *reinterpret_cast<const uint4 *>(lds + m * 16);
      if (PACK) {
        const uint32_t v = pack16(c4);
        packed[m] = v;
        if (rcpacked) rcpacked[TILE_GROUPS - 1 - m] = rev2(~v);
      }
      if (ok) {
        uint32_t cw[4] = {c4.x, c4.y, c4.z, c4.w};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          uint32_t fq = (ok >> (4 * q)) & 0xF;
          cw[q] |= ((fq & 1) << 2) | ((fq & 2) << 9) | ((fq & 4) << 16) | ((fq & 8) << 23);
        }
        *reinterpret_cast<uint4 *>(lds + m * 16) = make_uint4(cw[0], cw[1], cw[2], cw[3]);
      }
    }
  }
  return n_non_n;
}

// ---- k_scatter32's staging: one 16-base group per thread, kept in REGISTERS -------------------------------
// Thread t owns group t + 2 of the staged tile — exactly the sixteen end positions it walks — so the
// group's packed bases and its "a k-mer ends here" bits never leave its registers; only what its
// NEIGHBOURS need (the packed word for the walk's warm-up window, the N / read-start masks for the
// validity smear) goes through LDS, as one (packed, masks) pair per group, behind ONE barrier.
// Threads 0 and 1 stage the two halo groups as well.  (stage_tile's generic form — code bytes or packed
// streams in LDS, a second pass for the validity bits behind a second barrier — serves the other kernels.)
template <int NT, int TT>
struct StageRegs32 {
  uint32_t raw[2][4];
  uint32_t sb0[2], sb1[2];
};
// group index of (thread, slot): slot 0 = the thread's own group, slot 1 = a halo group (threads 0, 1)
template <int NT>
__device__ __forceinline__ int stage32_group(int slot) { return slot == 0 ? (int)threadIdx.x + 2 : (int)threadIdx.x; }
template <int NT, int TT>
__device__ __forceinline__ void stage32_prefetch(const BatchRef &b, uint64_t t0, StageRegs32<NT, TT> &pre) {
  const int64_t p0 = (int64_t)t0 - HALO;
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    if (r == 1 && threadIdx.x >= 2) break;
    const int m = stage32_group<NT>(r);
    const int64_t p = p0 + (int64_t)m * 16;
    if (p >= 0 && (uint64_t)p + 16 <= b.n_bases) {
      __builtin_memcpy(pre.raw[r], b.bases + p, 16);  // unaligned 16-B global load (one dwordx4)
      pre.sb0[r] = b.startbits[(uint64_t)p >> 5];
      pre.sb1[r] = b.startbits[((uint64_t)p >> 5) + 1];
    }
  }
}
// One group: validate + count non-N bases (positions in [t0, t1) only), 2-bit pack, N / read-start masks.
// Returns the packed word (first base on top); *gm = nmask16 | startmask16 << 16; *nn += non-N bases.
__device__ __forceinline__ uint32_t stage32_group_regs(const BatchRef &b, uint64_t t0, uint64_t t1, int m, const uint32_t (&raw)[4],
                                                       uint32_t sb0, uint32_t sb1, DevStats *stats, uint32_t *gm, uint32_t *nn) {
  const int64_t p = (int64_t)t0 - HALO + (int64_t)m * 16;
  uint32_t w[4];
  uint32_t nmask = 0;
  const bool fast = p >= 0 && (uint64_t)p + 16 <= b.n_bases;  // same test as stage32_prefetch
  if (fast) {
    w[0] = raw[0], w[1] = raw[1], w[2] = raw[2], w[3] = raw[3];
    if ((uint64_t)p >= t0 && (uint64_t)p < t1) {
      if ((uint64_t)p + 16 <= t1) {
        uint32_t bad = 0, n_n = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          uint32_t z;
          const uint32_t c = codes4(w[q], &z);  // (the conversion below recomputes it: CSE)
          bad |= invalid_bytes4(w[q], c);
          n_n += __builtin_popcount(z);
        }
        *nn += 16 - n_n;
        if (bad) {
          for (int r = 0; r < 16; ++r) {
            const uint32_t c = (w[r >> 2] >> (8 * (r & 3))) & 0xFF;
            if (!byte_is_acgtn(c)) {
              atomicMin(&stats->bad, ((unsigned long long)(p + r) << 8) | c);
              break;
            }
          }
        }
      } else {
        for (int r = 0; r < 16 && (uint64_t)p + r < t1; ++r) {
          const uint32_t c = (w[r >> 2] >> (8 * (r & 3))) & 0xFF;
          if (!byte_is_acgtn(c)) atomicMin(&stats->bad, ((unsigned long long)(p + r) << 8) | c);
          *nn += (c != 'N');
        }
      }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      uint32_t z;
      w[q] = codes4(w[q], &z);
      nmask |= msb_gather4(z) << (4 * q);
    }
  } else {
    const uint4 e = stage_edge_group(b.bases, b.n_bases, p, t0, t1, true, stats);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const uint32_t c8 = (e.x >> (8 * q)) & 0xFFu;  // four 2-bit codes
      w[q] = (c8 & 3u) | (((c8 >> 2) & 3u) << 8) | (((c8 >> 4) & 3u) << 16) | (((c8 >> 6) & 3u) << 24);
    }
    nmask = e.y;
    *nn += e.z;
  }
  uint32_t f = 0;  // read-start flags for these 16 positions: bits [p, p+16) of startbits
  if (fast) {
    const uint64_t two = (uint64_t)sb0 | ((uint64_t)sb1 << 32);
    f = (uint32_t)(two >> ((uint32_t)p & 31)) & 0xFFFFu;
  } else if (p >= 0 && (uint64_t)p < b.n_bases) {
    const uint64_t wi = (uint64_t)p >> 5;
    const uint64_t two = (uint64_t)b.startbits[wi] | ((uint64_t)b.startbits[wi + 1] << 32);
    f = (uint32_t)(two >> ((uint32_t)p & 31)) & 0xFFFFu;
  } else if (p < 0 && p + 16 > 0) {  // straddles position 0
    f = (b.startbits[0] << (uint32_t)(-p)) & 0xFFFFu;
  }
  *gm = nmask | (f << 16);
  return pack16(make_uint4(w[0], w[1], w[2], w[3]));
}
// "a k-mer ends here" bits of a group from its own masks g2 and those of the two groups before it
// (position j is bad if an N lies in [j-k+1, j] or a read starts in [j-k+2, j]); positions at or beyond
// the tile's end never get the bit.
__device__ __forceinline__ uint32_t stage32_okbits(uint32_t g0, uint32_t g1, uint32_t g2, int k, int lim) {
  uint64_t N = (uint64_t)(g0 & 0xFFFFu) | ((uint64_t)(g1 & 0xFFFFu) << 16) | ((uint64_t)(g2 & 0xFFFFu) << 32);
  uint64_t S = (uint64_t)(g0 >> 16) | ((uint64_t)(g1 >> 16) << 16) | ((uint64_t)(g2 >> 16) << 32);
  // an N at p spoils the end positions [p, p+k-1], a read start at p the end positions [p, p+k-2]: ONE
  // smear of N | S over k-1 positions, plus the N's themselves k-1 further on
  uint64_t T = k >= 2 ? N | S : N;
  if (k >= 2) {
    int s = 1;
    while (2 * s <= k - 1) {
      T |= T << s;
      s *= 2;
    }
    if (k - 1 > s) T |= T << (k - 1 - s);
    T |= N << (k - 1);
  }
  uint32_t ok = ~(uint32_t)(T >> 32) & 0xFFFFu;  // ≥ 32 ≥ k-1 bases of history
  if (lim < 16) ok = lim > 0 ? ok & ((1u << lim) - 1u) : 0u;
  return ok;
}

// workgroup sum of a per-thread u32, result valid in thread 0 (red: WG/64 words of LDS)
template <int NT = WG>
__device__ __forceinline__ uint32_t wg_sum(uint32_t v, uint32_t *red) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  uint32_t s = 0;
  if (threadIdx.x == 0)
    for (int w = 0; w < NT / 64; ++w) s += red[w];
  return s;
}

// Rolling frames of encoding.rs:359-367, kept as 32-bit halves so that every step is a
// handful of full-rate 32-bit ops: the forward frame right-aligned and masked to 2k bits, the
// reverse-complement frame LEFT-aligned in 64 bits (its new base always enters at bit 62).
struct Roll {
  uint32_t f_lo, f_hi, r_lo, r_hi;
};
__device__ __forceinline__ void roll_step(Roll &x, uint32_t base, uint32_t mask_lo, uint32_t mask_hi) {
  x.f_hi = __builtin_amdgcn_alignbit(x.f_hi, x.f_lo, 30) & mask_hi;
  x.f_lo = ((x.f_lo << 2) | base) & mask_lo;
  x.r_lo = __builtin_amdgcn_alignbit(x.r_hi, x.r_lo, 2);
  x.r_hi = (x.r_hi >> 2) | ((base ^ 3u) << 30);
}
__device__ __forceinline__ uint64_t roll_canonical(const Roll &x, int k) {
  uint64_t fwd = ((uint64_t)x.f_hi << 32) | x.f_lo;
  uint64_t rev = (((uint64_t)x.r_hi << 32) | x.r_lo) >> (64 - 2 * k);
  return fwd < rev ? fwd : rev;
}

// Walk this thread's SPAN end positions of the staged tile and hand every canonical k-mer to
// emit(kmer).  The walk starts k-1 bases early (rounded down to a ds_read_b64 boundary) to
// warm the frames up; bit 2 of the code byte says where a k-mer may be emitted.
template <int NT = WG, class Emit>
__device__ __forceinline__ void walk_tile(const uint8_t *lds, uint64_t t0, uint64_t t1, int k,
                                          Emit &&emit) {
  constexpr int SPAN = TILE_T / NT;
  const uint64_t mask = (1ull << (2 * k)) - 1;
  const uint32_t mask_lo = (uint32_t)mask, mask_hi = (uint32_t)(mask >> 32);
  const int e0 = threadIdx.x * SPAN;  // first end position (tile-relative)
  const int n_end = (int)(t1 - t0);   // valid end positions in this tile
  if (e0 >= n_end) return;
  const int jemit = HALO + e0;
  const int jend = HALO + (e0 + SPAN < n_end ? e0 + SPAN : n_end);
  Roll x{0, 0, 0, 0};
  for (int j = (jemit - (k - 1)) & ~7; j < jemit; j += 8) {  // warm-up: no emission
    uint64_t w = *reinterpret_cast<const uint64_t *>(lds + j);
#pragma unroll
    for (int r = 0; r < 8; ++r) roll_step(x, (uint32_t)(w >> (8 * r)) & 3u, mask_lo, mask_hi);
  }
  for (int j = jemit; j < jend; j += 8) {
    uint64_t w = *reinterpret_cast<const uint64_t *>(lds + j);
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      uint32_t c = (uint32_t)(w >> (8 * r)) & 0xFF;
      roll_step(x, c & 3u, mask_lo, mask_hi);
      if ((c & 4u) && j + r < jend) emit(roll_canonical(x, k));
    }
  }
}

// ---- open-addressing probe inside one page ----------------------------------------------
// Keys only ever go EMPTY → key, so a stale read can only show EMPTY where a key already
// sits; the device-scope CAS is the arbiter.  Returns the slot index or -1 (page full).
__device__ __forceinline__ int64_t find_or_insert(uint64_t *keys, uint64_t base, uint32_t s0,
                                                  uint64_t key, bool &inserted) {
  uint32_t s = s0;
  for (uint32_t i = 0; i < PAGE_SLOTS; ++i) {
    uint64_t cur = __hip_atomic_load(&keys[base + s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur == key) return (int64_t)(base + s);
    if (cur == EMPTY) {
      uint64_t prev = atomicCAS((unsigned long long *)&keys[base + s], (unsigned long long)EMPTY,
                                (unsigned long long)key);
      if (prev == EMPTY) {
        inserted = true;
        return (int64_t)(base + s);
      }
      if (prev == key) return (int64_t)(base + s);
    }
    s = (s + 1) & (PAGE_SLOTS - 1);
  }
  return -1;
}

__device__ __forceinline__ int64_t find_slot(const uint64_t *keys, uint64_t base, uint32_t s0,
                                             uint64_t key) {
  uint32_t s = s0;
  for (uint32_t i = 0; i < PAGE_SLOTS; ++i) {
    uint64_t cur = keys[base + s];
    if (cur == key) return (int64_t)(base + s);
    if (cur == EMPTY) return -1;
    s = (s + 1) & (PAGE_SLOTS - 1);
  }
  return -1;
}

// Saturating add of an arbitrary delta (counting.rs:82-92 semantics) without a CAS loop (a CAS
// loop livelocks for seconds when millions of records hit one k-mer, e.g. poly-A input): a
// returning add, and if that add wrapped the slot (old > MAX - delta) a repair with
// atomicMax(MAX).  Every wrapping add is followed by its own repair and an add that lands after
// a repair wraps again and repairs again, so the last operation on a saturated slot leaves MAX.
__device__ __forceinline__ void sat_add_atomic(uint32_t *p, uint32_t delta) {
  if (!delta) return;
  uint32_t old = atomicAdd(p, delta);
  if (old > 0xFFFFFFFFu - delta) atomicMax(p, 0xFFFFFFFFu);
}

// ==========================================================================================
// K_FILL: up to four buffers set to a 64-bit pattern in ONE launch (table reset: keys = EMPTY,
// counts = 0, control block = initial state).  Every segment is 16-B aligned and a multiple of
// 16 B long; the segments are walked as one concatenated range of 16-B words.
// ==========================================================================================
struct FillSegs {
  void *ptr[4];
  uint64_t n16[4];  // length in 16-B words
  uint64_t val[4];  // 64-bit pattern
};
__global__ void __launch_bounds__(WG) k_fill(FillSegs f) {
  const uint64_t total = f.n16[0] + f.n16[1] + f.n16[2] + f.n16[3];
  for (uint64_t i = (uint64_t)blockIdx.x * WG + threadIdx.x; i < total; i += (uint64_t)gridDim.x * WG) {
    uint64_t j = i;
    int sgm = 0;
#pragma unroll
    for (int q = 0; q < 3; ++q)
      if (sgm == q && j >= f.n16[q]) {
        j -= f.n16[q];
        sgm = q + 1;
      }
    ulonglong2 v;
    v.x = v.y = f.val[sgm];
    reinterpret_cast<ulonglong2 *>(f.ptr[sgm])[j] = v;
  }
}

// ==========================================================================================
// K_PACK / K_UNPACK: the 2-bit packed input format.  A batch's concatenated bases as ONE sequence in the
// layout of the reference's Read::from_str (src/kmer/encoding.rs:60-95): 4 bases per byte, first base in
// the two most significant bits (A 00, C 01, G 10, T 11), the tail left-aligned in its byte — plus what
// from_str has no room for and kmers_from_ascii needs (encoding.rs:346-352): an N mask, bit p % 32 of word
// p / 32 set where base p is N (its 2-bit code is then 00).  0.28 B/base instead of 1: what a host sends
// over PCIe when it packs (shk_pack_reads) before it hands a batch over (shk_ingest_packed).
// An N mask that is nearly all zeros crosses the link as the list of its non-zero words (ingest_host): the staged
// mask is cleared on the device and the listed words are written into it.
__global__ void __launch_bounds__(WG) k_nmask_sparse(uint32_t *__restrict__ nm, const uint2 *__restrict__ list, uint32_t n) {
  const uint32_t i = blockIdx.x * WG + threadIdx.x;
  if (i < n) nm[list[i].x] = list[i].y;
}

// k_unpack restores the ASCII batch in HBM for the counting kernels; k_pack is the device-side packer
// (validation as in encoding.rs:353-356: the first offender in input order through stats->bad).
// ==========================================================================================
__global__ void __launch_bounds__(WG) k_pack(const uint8_t *__restrict__ bases, uint64_t n_bases,
                                             uint8_t *__restrict__ packed, uint32_t *__restrict__ nmask,
                                             DevStats *__restrict__ stats) {
  const uint64_t g = (uint64_t)blockIdx.x * WG + threadIdx.x;  // one 32-base group = 8 packed bytes + 1 mask word
  const uint64_t p0 = g * 32;
  if (p0 >= n_bases) return;
  const uint32_t n = n_bases - p0 < 32 ? (uint32_t)(n_bases - p0) : 32u;
  uint32_t nm = 0;
  uint64_t bits = 0;  // 32 bases, first base on top
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t c = bases[p0 + i];
    if (!byte_is_acgtn(c)) atomicMin(&stats->bad, ((unsigned long long)(p0 + i) << 8) | c);
    const uint32_t isn = c == 'N';
    nm |= isn << i;
    bits |= (uint64_t)(isn ? 0u : (((c >> 1) ^ (c >> 2)) & 3u)) << (62 - 2 * i);
  }
  nmask[g] = nm;
  for (uint32_t j = 0; j < (n + 3) / 4; ++j) packed[g * 8 + j] = (uint8_t)(bits >> (56 - 8 * j));
}

// (a slice of a batch starts at a read boundary, not at a byte or word boundary of the streams: pk_base0, nm_base0)
__global__ void __launch_bounds__(WG) k_unpack(const uint8_t *__restrict__ packed, uint32_t pk_base0,
                                               const uint32_t *__restrict__ nmask, uint32_t nm_base0,
                                               uint64_t n_bases, uint8_t *__restrict__ out) {
  const uint64_t q = ((uint64_t)blockIdx.x * WG + threadIdx.x) * 16;  // 16 bases → one 16-byte store
  if (q >= n_bases) return;
  // output position 0 is base pk_base0 (0-3) of packed[0] and bit nm_base0 (0-31) of nmask[0]
  const uint64_t sp = pk_base0 + q;
  const uint64_t by = sp >> 2;
  const uint32_t r = (uint32_t)sp & 3u;
  // 16 bases = 32 bits from bit 2r of byte `by` on: five bytes, first base on top
  uint64_t five = 0;
#pragma unroll
  for (int j = 0; j < 5; ++j) five = (five << 8) | packed[by + j];  // (the staging buffers are padded: no read past the allocation)
  const uint32_t w = (uint32_t)(five >> (8 - 2 * r));
  const uint64_t sn = nm_base0 + q;
  const uint64_t nw = sn >> 5;
  const uint32_t nsh = (uint32_t)sn & 31u;
  const uint64_t two = (uint64_t)nmask[nw] | ((uint64_t)nmask[nw + 1] << 32);
  const uint32_t nm = (uint32_t)(two >> nsh) & 0xFFFFu;
  uint32_t o[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const uint32_t c8 = (w >> (24 - 8 * j)) & 0xFFu, n4 = (nm >> (4 * j)) & 0xFu;
    // selector byte = 2-bit code | N bit << 2: 0-3 → A C G T, 4-7 → N
    const uint32_t sel = ((c8 >> 6) & 3u) | (((c8 >> 4) & 3u) << 8) | (((c8 >> 2) & 3u) << 16) | ((c8 & 3u) << 24) |
                         ((n4 & 1u) << 2) | ((n4 & 2u) << 9) | ((n4 & 4u) << 16) | ((n4 & 8u) << 23);
    o[j] = __builtin_amdgcn_perm(0x4E4E4E4Eu /* N N N N */, 0x54474341u /* T G C A */, sel);
  }
  if (q + 16 <= n_bases) {
    *reinterpret_cast<uint4 *>(out + q) = make_uint4(o[0], o[1], o[2], o[3]);
  } else {
    for (uint32_t i = 0; q + i < n_bases; ++i) out[q + i] = (uint8_t)(o[i >> 2] >> (8 * (i & 3)));
  }
}

// ==========================================================================================
// K_MARK: read-start bitmap.  One thread per read, NO atomics and no zeroed bitmap to start from:
// the reads are in offset order, so the first read of every 32-position word (the "leader")
// gathers the start bits of all reads that begin in that word, stores the word, and zero-fills
// the words up to the next leader's — together the leaders write every word of the bitmap
// exactly once.  (A memset + one atomicOr per read cost 27 µs per million reads; this costs 8.)
// ==========================================================================================
// It also clears the small per-launch state of the counting pass that follows it on the stream
// (partition cursors, spill counter), which saves two fill launches per batch.
__global__ void __launch_bounds__(WG) k_mark_starts(const uint64_t *__restrict__ offsets,
                                                    uint64_t n_seqs, uint64_t n_bases,
                                                    uint32_t *__restrict__ startbits, uint64_t sb_words,
                                                    unsigned int *__restrict__ zero_u32, uint32_t n_zero,
                                                    unsigned long long *__restrict__ zero_u64, uint64_t off_bias,
                                                    uint4 *__restrict__ zero_a16 = nullptr, uint32_t n_a16 = 0,
                                                    uint4 *__restrict__ zero_b16 = nullptr, uint32_t n_b16 = 0) {
  // off_bias: what the offsets are ahead of the batch's first byte by (a slice of a host batch is handed on with
  // the caller's own offsets: no re-based copy is made on the host)
  const uint64_t i = (uint64_t)blockIdx.x * WG + threadIdx.x;
  for (uint64_t j = i; j < n_zero; j += (uint64_t)gridDim.x * WG) zero_u32[j] = 0;
  if (i == 0 && zero_u64) *zero_u64 = 0;
  // (the histogram and totals a finalize has read back: cleared here, on the way, instead of by a launch of their own)
  for (uint64_t j = i; j < n_a16; j += (uint64_t)gridDim.x * WG) zero_a16[j] = make_uint4(0u, 0u, 0u, 0u);
  for (uint64_t j = i; j < n_b16; j += (uint64_t)gridDim.x * WG) zero_b16[j] = make_uint4(0u, 0u, 0u, 0u);
  if (i >= n_seqs) return;
  const uint64_t o = offsets[i] - off_bias;
  const uint64_t w = o >> 5;
  if (i > 0 && ((offsets[i - 1] - off_bias) >> 5) == w) return;  // not the first read of its word
  uint32_t bits = 0;
  uint64_t j = i, oj = o;
  while (j < n_seqs && (oj >> 5) == w) {  // usually one iteration: reads are longer than a word
    const uint64_t ej = offsets[j + 1] - off_bias;
    if (ej > oj && oj < n_bases) bits |= 1u << (oj & 31);  // empty reads start nothing
    oj = ej;
    ++j;
  }
  uint64_t w_next = j < n_seqs ? oj >> 5 : sb_words;
  if (w_next > sb_words) w_next = sb_words;
  if (i == 0)
    for (uint64_t x = 0; x < w && x < sb_words; ++x) startbits[x] = 0;  // (offsets[0] is 0 in practice)
  if (w < sb_words) startbits[w] = bits;
  for (uint64_t x = w + 1; x < w_next; ++x) startbits[x] = 0;
}

// ==========================================================================================
// K_MARK (part 2): tile list for multi-chunk batches.  Blocks are the runs of reads between
// global read indices that are multiples of 1000 (io.rs:340-343, 355-361); every tile lies
// inside one block so it has one chunk lane.  Single workgroup; exclusive scan over blocks.
// ==========================================================================================
constexpr int TB_WG = 1024;
__global__ void __launch_bounds__(TB_WG) k_build_tiles(const uint64_t *__restrict__ offsets,
                                                       uint64_t n_seqs, uint64_t g0,
                                                       uint32_t n_chunks, uint64_t n_blocks,
                                                       TileDesc *__restrict__ tiles,
                                                       DevStats *__restrict__ stats, uint64_t off_bias) {
  __shared__ uint64_t sc[TB_WG];
  __shared__ uint64_t running;
  if (threadIdx.x == 0) running = 0;
  __syncthreads();
  const uint64_t first = (g0 % 1000 == 0) ? 1000 : 1000 - g0 % 1000;
  for (uint64_t jb = 0; jb < n_blocks; jb += TB_WG) {
    uint64_t j = jb + threadIdx.x;
    uint64_t nt = 0, b0 = 0, b1 = 0;
    uint32_t lane = 0;
    if (j < n_blocks) {
      uint64_t r0 = j == 0 ? 0 : first + (j - 1) * 1000;
      uint64_t r1 = first + j * 1000;
      if (r1 > n_seqs) r1 = n_seqs;
      b0 = offsets[r0] - off_bias;
      b1 = offsets[r1] - off_bias;
      nt = (b1 - b0 + TILE_T - 1) / TILE_T;
      lane = (uint32_t)(((g0 + r0) / 1000) % n_chunks);
    }
    sc[threadIdx.x] = nt;
    __syncthreads();
    for (int d = 1; d < TB_WG; d <<= 1) {  // inclusive Hillis–Steele scan
      uint64_t v = threadIdx.x >= (unsigned)d ? sc[threadIdx.x - d] : 0;
      __syncthreads();
      sc[threadIdx.x] += v;
      __syncthreads();
    }
    uint64_t excl = running + sc[threadIdx.x] - nt;
    for (uint64_t t = 0; t < nt; ++t) {
      TileDesc d;
      d.begin = b0 + t * TILE_T;
      d.end = d.begin + TILE_T < b1 ? d.begin + TILE_T : b1;
      d.lane = lane;
      d.pad = 0;
      tiles[excl + t] = d;
    }
    __syncthreads();
    if (threadIdx.x == TB_WG - 1) running += sc[TB_WG - 1];
    __syncthreads();
  }
  if (threadIdx.x == 0) stats->n_tiles = running;
}

// ==========================================================================================
// K_SCAN: validate bytes (encoding.rs:353-356) and count non-N bases per chunk lane
// (encoding.rs:374-376 via chunk.rs:28).  Runs before any counting kernel, so an invalid
// byte aborts the batch with the table untouched.
// ==========================================================================================
__global__ void __launch_bounds__(WG) k_scan(BatchRef b, DevStats *__restrict__ stats,
                                             unsigned long long *__restrict__ lane_bases) {
  __shared__ uint32_t red[WG / 64];
  for (uint64_t t = blockIdx.x;; t += gridDim.x) {
    uint64_t t0, t1;
    uint32_t lane;
    if (!tile_get(b, t, t0, t1, lane)) break;
    uint32_t n_valid = 0;
    for (uint64_t p = t0 + (uint64_t)threadIdx.x * 16; p < t1; p += (uint64_t)WG * 16) {
      uint8_t buf[16];
      int n = (int)(t1 - p < 16 ? t1 - p : 16);
      if (n == 16) {
        __builtin_memcpy(buf, b.bases + p, 16);
      } else {
        for (int r = 0; r < n; ++r) buf[r] = b.bases[p + r];
      }
      for (int r = 0; r < n; ++r) {
        uint32_t c = buf[r];
        if (!byte_is_acgtn(c)) {
          atomicMin(&stats->bad, ((unsigned long long)(p + r) << 8) | c);
        }
        n_valid += (c != 'N');
      }
    }
    // wave reduce, then one atomic per workgroup
    for (int off = 32; off > 0; off >>= 1) n_valid += __shfl_down(n_valid, off, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = n_valid;
    __syncthreads();
    if (threadIdx.x == 0) {
      uint32_t s = 0;
      for (int w = 0; w < WG / 64; ++w) s += red[w];
      if (s) atomicAdd(&lane_bases[lane], (unsigned long long)s);
    }
    __syncthreads();
  }
}

// ==========================================================================================
// K_DIRECT: extract + insert with global device-scope atomics.  General path: any table
// size, any batch size; also the re-insert path for spilled k-mers.
// counting.rs:82-85: entry(kmer).or_insert(0); *c = c.saturating_add(1).
// Saturation stays exact with a returning add: an add that observes old == u32::MAX has
// wrapped the slot and repairs it with atomicMax(MAX); every wrap is followed by its own
// repair, so the last operation on a saturated slot always leaves MAX.
// ==========================================================================================
__device__ __forceinline__ void count_one(const TableRef &tb, uint64_t key, uint32_t lane,
                                          DevStats *stats, const SpillRef &sp,
                                          uint32_t &n_new) {
  const Home hm = home_of(tb, key);
  if (!hm.owned) return;  // another owner's k-mer (owner share: foreign records are dropped)
  bool inserted = false;
  int64_t s = find_or_insert(tb.keys, hm.base, hm.slot, key, inserted);
  if (s < 0) {
    unsigned long long i = atomicAdd(&stats->spill_count, 1ull);
    if (i < sp.cap) {
      sp.keys[i] = key;
      sp.lanes[i] = lane;
      sp.counts[i] = 1u;
    }
    return;
  }
  n_new += inserted;
  uint32_t *v = tb.vals + (uint64_t)lane * tb.cap + (uint64_t)s;
  uint32_t old = atomicAdd(v, 1u);
  if (old == 0xFFFFFFFFu) atomicMax(v, 0xFFFFFFFFu);
}

__global__ void __launch_bounds__(WG) k_direct(BatchRef b, TableRef tb, DevStats *__restrict__ stats,
                                               SpillRef sp) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[STAGE_BYTES];
  uint32_t n_new = 0;
  if (stats->bad != ~0ull) return;  // k_scan found an invalid byte: leave the table untouched
  uint64_t t = blockIdx.x, t0, t1;
  uint32_t lane;
  bool have = next_tile(b, t, false, 0, t0, t1, lane);
  StageRegs<WG> pre;
  if (have) stage_prefetch<WG>(b, t0, pre);
  while (have) {
    __syncthreads();
    stage_tile<false, WG>(b, t0, t1, lds, stats, pre);
    uint64_t tn = t + gridDim.x, n0, n1;
    uint32_t nl;
    const bool hn = next_tile(b, tn, false, 0, n0, n1, nl);
    if (hn) stage_prefetch<WG>(b, n0, pre);
    __syncthreads();
    walk_tile(lds, t0, t1, b.k, [&](uint64_t kmer) { count_one(tb, kmer, lane, stats, sp, n_new); });
    t = tn;
    t0 = n0;
    t1 = n1;
    lane = nl;
    have = hn;
  }
  for (int off = 32; off > 0; off >>= 1) n_new += __shfl_down(n_new, off, 64);
  if ((threadIdx.x & 63) == 0 && n_new) atomicAdd(&stats->n_distinct, (unsigned long long)n_new);
}

// ---- the WIDE exchange: k-mers too long for the owner layout's 4-byte records (k > 21 at a fan-out of 1024) ----------
// The batch's canonical k-mers (kmers_from_ascii, encoding.rs:332-371) as whole 64-bit values, grouped by OWNER — the
// top owner_bits of the mixed key, what home_of reads — with their chunk lanes beside them.  Two launches of this
// kernel: PLACE = false counts every owner's k-mers (owner_count[o] += …), the host turns the counts into segment
// bases, PLACE = true writes them (owner_count[o] then is owner o's running cursor, starting at its segment's base).
// Per tile: the k-mers are counted by owner in LDS, one device-scope add per (tile, owner) reserves a run, and a second
// walk of the same tile (walk_tile is deterministic) puts every k-mer at run base + its rank.
__device__ __forceinline__ uint32_t owner_of(uint64_t key, uint32_t key_bits, uint32_t owner_bits) {
  return owner_bits ? hash64(key, key_bits) >> (32 - owner_bits) : 0u;
}
template <bool PLACE>
__global__ void __launch_bounds__(WG) k_xw_scatter(BatchRef b, uint32_t key_bits, uint32_t owner_bits, DevStats *__restrict__ stats,
                                                   unsigned long long *__restrict__ owner_count, uint64_t *__restrict__ out_kmers,
                                                   uint32_t *__restrict__ out_lanes) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[STAGE_BYTES];
  __shared__ uint32_t cnt[64];
  __shared__ unsigned long long run_base[64];
  if (stats->bad != ~0ull) return;  // k_scan found an invalid byte: nothing is handed on
  const uint32_t W = 1u << owner_bits;
  uint64_t t = blockIdx.x, t0, t1;
  uint32_t lane;
  bool have = next_tile(b, t, false, 0, t0, t1, lane);
  StageRegs<WG> pre;
  if (have) stage_prefetch<WG>(b, t0, pre);
  while (have) {
    __syncthreads();
    stage_tile<false, WG>(b, t0, t1, lds, stats, pre);
    if (threadIdx.x < 64) cnt[threadIdx.x] = 0;
    uint64_t tn = t + gridDim.x, n0, n1;
    uint32_t nl;
    const bool hn = next_tile(b, tn, false, 0, n0, n1, nl);
    if (hn) stage_prefetch<WG>(b, n0, pre);
    __syncthreads();
    walk_tile(lds, t0, t1, b.k, [&](uint64_t kmer) { atomicAdd(&cnt[owner_of(kmer, key_bits, owner_bits)], 1u); });
    __syncthreads();
    if (threadIdx.x < W) {
      const uint32_t c1 = cnt[threadIdx.x];
      const unsigned long long at = c1 ? atomicAdd(&owner_count[threadIdx.x], (unsigned long long)c1) : 0ull;
      if (PLACE) {
        run_base[threadIdx.x] = at;
        cnt[threadIdx.x] = 0;
      }
    }
    if (PLACE) {
      __syncthreads();
      walk_tile(lds, t0, t1, b.k, [&](uint64_t kmer) {
        const uint32_t o = owner_of(kmer, key_bits, owner_bits);
        const unsigned long long at = run_base[o] + atomicAdd(&cnt[o], 1u);
        out_kmers[at] = kmer;
        out_lanes[at] = lane;
      });
    }
    t = tn;
    t0 = n0;
    t1 = n1;
    lane = nl;
    have = hn;
  }
}

// ==========================================================================================
// K_INSERT: (kmer, lane, count) records — KmerCounts::insert (counting.rs:152-154) and the
// re-insert of spilled k-mers after a grow.  lanes == nullptr ⇒ all records use lane0;
// counts == nullptr ⇒ count 1.
// ==========================================================================================
__global__ void __launch_bounds__(WG) k_insert(const uint64_t *__restrict__ kmers,
                                               const uint32_t *__restrict__ lanes,
                                               const uint32_t *__restrict__ counts, uint64_t n,
                                               uint32_t lane0, TableRef tb,
                                               DevStats *__restrict__ stats, SpillRef sp) {
  uint32_t n_new = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * WG + threadIdx.x; i < n; i += (uint64_t)gridDim.x * WG) {
    uint64_t key = kmers[i];
    uint32_t lane = lanes ? lanes[i] : lane0;
    uint32_t cnt = counts ? counts[i] : 1u;
    const Home hm = home_of(tb, key);
    if (!hm.owned) continue;
    bool inserted = false;
    int64_t s = find_or_insert(tb.keys, hm.base, hm.slot, key, inserted);
    if (s < 0) {
      unsigned long long j = atomicAdd(&stats->spill_count, 1ull);
      if (j < sp.cap) {
        sp.keys[j] = key;
        sp.lanes[j] = lane;
        sp.counts[j] = cnt;
      }
      continue;
    }
    n_new += inserted;
    sat_add_atomic(tb.vals + (uint64_t)lane * tb.cap + (uint64_t)s, cnt);
  }
  for (int off = 32; off > 0; off >>= 1) n_new += __shfl_down(n_new, off, 64);
  if ((threadIdx.x & 63) == 0 && n_new) atomicAdd(&stats->n_distinct, (unsigned long long)n_new);
}

// ==========================================================================================
// K_GROW: rehash every occupied slot of the old table into a table with more pages.  A
// page's entries land in its 2^d child pages, each of which has room for all of them.
// ==========================================================================================
__global__ void __launch_bounds__(WG) k_grow(TableRef oldt, TableRef newt) {
  for (uint64_t i = (uint64_t)blockIdx.x * WG + threadIdx.x; i < oldt.cap;
       i += (uint64_t)gridDim.x * WG) {
    uint64_t key = oldt.keys[i];
    if (key == EMPTY) continue;
    const Home hm = home_of(newt, key);
    bool inserted = false;
    int64_t s = find_or_insert(newt.keys, hm.base, hm.slot, key, inserted);
    // s >= 0 by construction (child pages cannot overflow)
    for (uint32_t l = 0; l < oldt.n_lanes; ++l)
      newt.vals[(uint64_t)l * newt.cap + (uint64_t)s] = oldt.vals[(uint64_t)l * oldt.cap + i];
  }
}

// ==========================================================================================
// K_HISTO: one pass over pages [page0,page1) → every histogram column + totals.
// Column j of the reference is the histogram of the table after merging chunks 0..j with
// saturating adds (counting.rs:171-202; histogram.rs:51-85) — sequential saturating adds of
// non-negative lane counts equal the clamped prefix sum, so column j is the histogram of
// min(Σ_{c≤j} lane_c, u32::MAX); counts > histo_max fold into bin histo_max+1
// (histogram.rs:125-134); zero prefix sums (k-mer not seen yet) are not counted.
// Low bins are privatised in LDS (u32), the rest go straight to global u64 atomics.  The grid is
// ≤ 256 workgroups of 1024 threads: enough loads in flight to stream the table, and few enough
// workgroups that the final flush (every workgroup adds its non-zero bins to the same few cache
// lines of `hist`) stays short — measured: 1024 × 256-thread workgroups spend 25 µs in that flush.
// ==========================================================================================
struct HistoTotals {
  unsigned long long n_unique;       // occupied slots
  unsigned long long n_hashed;       // Σ merged (clamped) counts
  unsigned long long n_lane_sum;     // Σ over lanes of Σ counts  (= n_kmers_ingested)
  unsigned long long any_saturated;
};

constexpr int HISTO_WG = 1024;  // few, large workgroups: the flush of a workgroup's bins is what contends
// KEYS = false: occupancy is read off the counts — a slot holds a key exactly when its counts are not
// all zero, unless a key was inserted with count 0 (shk_insert_counts can; the host then asks for
// KEYS = true) — so the scan reads 4 B per slot and lane instead of 8 + 4.
template <bool KEYS>
__global__ void __launch_bounds__(HISTO_WG) k_histo(TableRef tb, uint64_t slot0, uint64_t slot1,
                                              uint64_t histo_max, uint32_t n_cols,
                                              uint32_t lds_bins,
                                              unsigned long long *__restrict__ hist,
                                              HistoTotals *__restrict__ tot) {
  extern __shared__ uint32_t lh[];  // n_cols * lds_bins
  __shared__ unsigned long long wtot[HISTO_WG / 64][4];
  const uint32_t n_l = n_cols * lds_bins;
  for (uint32_t i = threadIdx.x; i < n_l; i += HISTO_WG) lh[i] = 0;
  __syncthreads();
  const uint64_t hlen = histo_max + 2;
  unsigned long long n_unique = 0, n_hashed = 0, n_lane = 0, sat = 0;
  // four consecutive slots per thread per step: keys as 2×16 B, each lane's counts as 16 B,
  // all loads issued before any is consumed (slot0/slot1 are multiples of PAGE_SLOTS)
  const uint64_t stride = (uint64_t)gridDim.x * HISTO_WG * 4;
  uint64_t s = slot0 + ((uint64_t)blockIdx.x * HISTO_WG + threadIdx.x) * 4;
  if (!KEYS && tb.n_lanes == 1 && n_cols <= 1) {
    // One chunk lane, counts only: a step is a single 16-B load, far too little in flight for a scan
    // — four steps' loads are issued together.
    auto one = [&](const uint4 &v4) {
      const uint32_t v[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (v[q] == 0) continue;
        n_lane += v[q];
        n_unique++;
        n_hashed += v[q];
        sat |= (v[q] == 0xFFFFFFFFu);
        if (n_cols) {
          const uint64_t bin = v[q] <= histo_max ? v[q] : histo_max + 1;
          if (bin < lds_bins)
            atomicAdd(&lh[(uint32_t)bin], 1u);
          else
            atomicAdd(&hist[bin], 1ull);
        }
      }
    };
    for (; s + 3 * stride < slot1; s += 4 * stride) {
      const uint4 a0 = *reinterpret_cast<const uint4 *>(tb.vals + s);
      const uint4 a1 = *reinterpret_cast<const uint4 *>(tb.vals + s + stride);
      const uint4 a2 = *reinterpret_cast<const uint4 *>(tb.vals + s + 2 * stride);
      const uint4 a3 = *reinterpret_cast<const uint4 *>(tb.vals + s + 3 * stride);
      one(a0);
      one(a1);
      one(a2);
      one(a3);
    }
  }
  for (; s < slot1; s += stride) {
    uint32_t cum[4] = {0, 0, 0, 0};
    bool occ[4] = {true, true, true, true};
    if (KEYS) {
      const ulonglong2 ka = *reinterpret_cast<const ulonglong2 *>(tb.keys + s);
      const ulonglong2 kb = *reinterpret_cast<const ulonglong2 *>(tb.keys + s + 2);
      occ[0] = ka.x != EMPTY, occ[1] = ka.y != EMPTY, occ[2] = kb.x != EMPTY, occ[3] = kb.y != EMPTY;
      if (!(occ[0] | occ[1] | occ[2] | occ[3])) continue;
    }
    for (uint32_t l0 = 0; l0 < tb.n_lanes; l0 += 4) {  // four lanes' counts in flight together
      uint4 vv[4];
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (l0 + j < tb.n_lanes) vv[j] = *reinterpret_cast<const uint4 *>(tb.vals + (uint64_t)(l0 + j) * tb.cap + s);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint32_t l = l0 + j;
        if (l >= tb.n_lanes) break;
        const uint32_t v[4] = {vv[j].x, vv[j].y, vv[j].z, vv[j].w};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          if (!occ[q]) continue;
          n_lane += v[q];
          cum[q] = sat_add_u32(cum[q], v[q]);
          if (l < n_cols && cum[q] > 0) {
            uint64_t bin = cum[q] <= histo_max ? cum[q] : histo_max + 1;
            if (bin < lds_bins)
              atomicAdd(&lh[l * lds_bins + (uint32_t)bin], 1u);
            else
              atomicAdd(&hist[(uint64_t)l * hlen + bin], 1ull);
          }
        }
      }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (KEYS ? !occ[q] : cum[q] == 0) continue;
      n_unique++;
      n_hashed += cum[q];
      sat |= (cum[q] == 0xFFFFFFFFu);
    }
  }
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < n_l; i += HISTO_WG) {
    uint32_t v = lh[i];
    if (v) {
      uint32_t l = i / lds_bins, bin = i % lds_bins;
      if ((uint64_t)bin < hlen) atomicAdd(&hist[(uint64_t)l * hlen + bin], (unsigned long long)v);
    }
  }
  // totals: wave reduce, then one workgroup reduce, then ONE set of atomics per workgroup —
  // same-line atomics retire one after the other (≈2 ns each on MI355X), so their number, not
  // their payload, is what costs
  for (int off = 32; off > 0; off >>= 1) {
    n_unique += __shfl_down(n_unique, off, 64);
    n_hashed += __shfl_down(n_hashed, off, 64);
    n_lane += __shfl_down(n_lane, off, 64);
    sat |= __shfl_down(sat, off, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    unsigned long long *w = wtot[threadIdx.x >> 6];
    w[0] = n_unique;
    w[1] = n_hashed;
    w[2] = n_lane;
    w[3] = sat;
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    unsigned long long v = 0;
    for (int w = 0; w < HISTO_WG / 64; ++w) v = threadIdx.x == 3 ? (v | wtot[w][3]) : v + wtot[w][threadIdx.x];
    if (v) {
      if (threadIdx.x == 0) atomicAdd(&tot->n_unique, v);
      if (threadIdx.x == 1) atomicAdd(&tot->n_hashed, v);
      if (threadIdx.x == 2) atomicAdd(&tot->n_lane_sum, v);
      if (threadIdx.x == 3) atomicOr(&tot->any_saturated, 1ull);
    }
  }
}

// The control block (launch outcome, totals, lane sums, histogram) straight into the caller's pinned, device-visible
// copy of it: the first `head8` words whatever they hold, the histogram words only where they are not zero (the host
// cleared its copy before the launch; nearly all of them are, and stores over the link are slow).  Takes the place of
// a copy queued behind k_histo — the barrier between a kernel and a blit costs 12-14 µs, a fortieth of a 1 M-read job.
__global__ void __launch_bounds__(WG) k_ctl_out(const unsigned long long *__restrict__ src, unsigned long long *__restrict__ dst,
                                                uint32_t n8, uint32_t head8) {
  const uint32_t i = blockIdx.x * WG + threadIdx.x;
  if (i >= n8) return;
  const unsigned long long v = src[i];
  if (i < head8 || v) dst[i] = v;
}

// ==========================================================================================
// K_LOOKUP / K_EXPORT: merged-table read API (counting.rs:205-241).
// ==========================================================================================
__device__ __forceinline__ uint64_t revcomp(uint64_t kmer, int k) {
  // complement = bitwise NOT of each 2-bit code; reverse 2-bit groups of the 64-bit word
  uint64_t x = ~kmer;
  x = ((x >> 2) & 0x3333333333333333ull) | ((x & 0x3333333333333333ull) << 2);
  x = ((x >> 4) & 0x0F0F0F0F0F0F0F0Full) | ((x & 0x0F0F0F0F0F0F0F0Full) << 4);
  x = __builtin_bswap64(x);
  return x >> (64 - 2 * k);
}

// BOUNDED: the count at a depth — the saturating sum of lanes 0..lanes−1 only (1 ≤ lanes ≤ tb.n_lanes:
// the host's check), 0 for a key that only later chunks hold.  A template parameter, so the merged probe is the code it was.
template <bool BOUNDED>
__device__ __forceinline__ uint32_t merged_count_upto(const TableRef &tb, uint64_t key, uint32_t lanes) {
  const Home hm = home_of(tb, key);
  if (!hm.owned) return 0u;
  int64_t s = find_slot(tb.keys, hm.base, hm.slot, key);
  if (s < 0) return 0;
  uint32_t cum = 0;
  const uint32_t n = BOUNDED ? lanes : tb.n_lanes;
  for (uint32_t l = 0; l < n; ++l) cum = sat_add_u32(cum, tb.vals[(uint64_t)l * tb.cap + s]);
  return cum;
}
__device__ __forceinline__ uint32_t merged_count(const TableRef &tb, uint64_t key) { return merged_count_upto<false>(tb, key, 0u); }
__device__ __forceinline__ uint32_t merged_count(const TableRef &tb, uint64_t key, uint32_t lanes) {
  return merged_count_upto<true>(tb, key, lanes);
}

// merged_count over the shares of a multi-device context (SHK_FLAG_GROUP_GRAPH): dir[d] is share d's table, 2^owner_bits
// of them (owner_bits >= 1), all of one key length.  Exactly one share owns a key — the top owner_bits of its hash, the
// bits home_of tests — so the probe is merged_count on that share's arrays: plain loads, nothing is written during the call.
__device__ __forceinline__ uint32_t merged_count_sharded(const TableRef *dir, uint32_t owner_bits, uint64_t key) {
  const uint32_t owner = hash64(key, dir[0].key_bits) >> (32 - owner_bits);
  const TableRef tb = dir[owner];  // (the descriptor once: 48 bytes)
  return merged_count(tb, key);    // (.owned holds by construction)
}
// (its depth form, for the day a multi-device context takes a depth: every share has the context's lanes)
__device__ __forceinline__ uint32_t merged_count_sharded(const TableRef *dir, uint32_t owner_bits, uint64_t key, uint32_t lanes) {
  const uint32_t owner = hash64(key, dir[0].key_bits) >> (32 - owner_bits);
  const TableRef tb = dir[owner];
  return merged_count(tb, key, lanes);
}

__global__ void __launch_bounds__(WG) k_lookup(TableRef tb, const uint64_t *__restrict__ kmers,
                                               uint32_t *__restrict__ out, uint64_t n, int canonical,
                                               int k) {
  uint64_t i = (uint64_t)blockIdx.x * WG + threadIdx.x;
  if (i >= n) return;
  uint64_t key = kmers[i];
  if (canonical) {
    uint64_t rc = revcomp(key, k);
    key = key < rc ? key : rc;
  }
  out[i] = merged_count(tb, key);
}
// k_lookup at a depth: the counts of chunks 0..lanes−1.
__global__ void __launch_bounds__(WG) k_lookup_depth(TableRef tb, const uint64_t *__restrict__ kmers,
                                                     uint32_t *__restrict__ out, uint64_t n, int canonical,
                                                     int k, uint32_t lanes) {
  uint64_t i = (uint64_t)blockIdx.x * WG + threadIdx.x;
  if (i >= n) return;
  uint64_t key = kmers[i];
  if (canonical) {
    uint64_t rc = revcomp(key, k);
    key = key < rc ? key : rc;
  }
  out[i] = merged_count(tb, key, lanes);
}

__global__ void __launch_bounds__(WG) k_export(TableRef tb, uint64_t slot0, uint64_t slot1,
                                               uint64_t *__restrict__ kmers,
                                               uint32_t *__restrict__ counts, uint64_t cap,
                                               unsigned long long *__restrict__ n_out) {
  for (uint64_t s = slot0 + (uint64_t)blockIdx.x * WG + threadIdx.x; s < slot1;
       s += (uint64_t)gridDim.x * WG) {
    uint64_t key = tb.keys[s];
    if (key == EMPTY) continue;
    uint32_t cum = 0;
    for (uint32_t l = 0; l < tb.n_lanes; ++l) cum = sat_add_u32(cum, tb.vals[(uint64_t)l * tb.cap + s]);
    unsigned long long i = atomicAdd(n_out, 1ull);
    if (i < cap) {
      kmers[i] = key;
      counts[i] = cum;
    }
  }
}

// ==========================================================================================
// K_EXTEND: the bulk neighbourhoods of many seed sets side by side (shk_neighborhood_panel; shk_neighborhood is its
// one-job case and runs the same kernels), the table side of sPCR's graph extension
// (extend_graph, src/pcr/graph.rs:377-525): breadth-first over (node, dir) entries — a node is a (k−1)-mer, dir 0
// extends it forward ((node << 2) | b), dir 1 backward ((b << 2(k−1)) | node) — where an entry's four candidate
// k-mers are looked up in the merged table and the accepted ones (merged count ≥ min_count) lead to the next level.
//
// Two sets in device memory, both open addressing over 64-bit words probed with atomicCAS only (so that every access
// is served by L2 and no wave reads a stale line): `vis`, the entries (node << 1 | dir) of every level so far, and
// `kset`, the accepted canonical k-mers.  Whoever wins an insert appends: to the k-mer list, or to the next level.
// Fills past a list's capacity are counted but not written; the level then did not fit and the host drops it (the
// k-mer list is cut back to its fill at the level's start, the entry list of the level itself is untouched).
// ==========================================================================================
constexpr int NB_WG = 1024;            // k_nb_narrow_panel: one workgroup per job
constexpr uint32_t NB_NARROW = 1024;   // … carries a level of up to this many entries
constexpr uint32_t NB_RUN = 0, NB_COMPLETE = 1, NB_LIMIT = 2, NB_OVERFLOW = 3, NB_WIDE = 4;

struct NbCtl {                 // host ↔ device state of one job
  unsigned long long k_n;      // accepted k-mers appended so far
  unsigned long long next_n;   // entries of the level under construction (counted past fringe_cap)
  unsigned long long cur_n;    // entries of the current (unexpanded) level
  uint32_t levels_done;
  uint32_t cur_sel;            // which of the two entry lists holds the current level
  uint32_t status;             // NB_*
  uint32_t set_full;           // a set ran out of slots: only in a level that does not fit the capacities the sets are sized for
};

struct NbRef {
  uint64_t *vis, *kset;        // EMPTY-filled
  uint64_t vis_mask, kset_mask;
  uint64_t *list[2];           // entry lists, fringe_cap each
  uint64_t *kmers;             // cap
  uint32_t *counts;            // cap
  uint64_t cap, fringe_cap;
  uint32_t min_count, max_levels;
  int k;
  uint32_t lanes;              // the job's depth (the *_depths kernels read it; 0 otherwise): in what was tail padding
};
static_assert(sizeof(NbRef) == 96, "NbRef is a kernel argument and an uploaded array: lanes must not grow it");

// 1: inserted, 0: was there, −1: no free slot
__device__ __forceinline__ int nb_set_insert(uint64_t *set, uint64_t mask, uint64_t key) {
  uint64_t s = ((key ^ (key >> 29)) * MIX_M64 >> 20) & mask;
  for (uint64_t i = 0; i <= mask; ++i) {
    const uint64_t prev = atomicCAS((unsigned long long *)&set[s], (unsigned long long)EMPTY, (unsigned long long)key);
    if (prev == EMPTY) return 1;
    if (prev == key) return 0;
    s = (s + 1) & mask;
  }
  return -1;
}

// What the table-probing kernels below take as "the table": a context's own TableRef, or the share directory of a
// multi-device context — a template parameter of the kernels, so that the one-table instantiation is the code it was.
struct NbShards {
  const TableRef *dir;  // TableRef[2^owner_bits]: device memory (k_nb_wide), or the workgroup's LDS copy (k_nb_narrow_panel)
  uint32_t owner_bits;
};
constexpr uint32_t NB_MAX_SHARES = 64;  // shares of a multi-device context at most (group_create)
template <bool SHARDED>
using NbTable = std::conditional_t<SHARDED, NbShards, TableRef>;
__device__ __forceinline__ uint32_t nb_count(const TableRef &tb, uint64_t key) { return merged_count(tb, key); }
__device__ __forceinline__ uint32_t nb_count(const NbShards &sh, uint64_t key) { return merged_count_sharded(sh.dir, sh.owner_bits, key); }
__device__ __forceinline__ uint32_t nb_count(const TableRef &tb, uint64_t key, uint32_t lanes) { return merged_count(tb, key, lanes); }
__device__ __forceinline__ uint32_t nb_count(const NbShards &sh, uint64_t key, uint32_t lanes) { return merged_count_sharded(sh.dir, sh.owner_bits, key, lanes); }

// One (entry, base) pair of the current level.  k_n / next_n: the two fill counters (LDS in k_nb_narrow_panel, the control
// block in k_nb_wide); lds_next: where k_nb_narrow_panel keeps the first NB_NARROW entries of the next level.
// DEPTH: the probe stops at the job's nb.lanes, so jobs of different depths share a launch.
template <bool DEPTH = false, class Table>
__device__ __forceinline__ void nb_expand(const Table &tb, const NbRef &nb, uint64_t entry, uint32_t b,
                                          uint64_t *next_list, unsigned long long *k_n, unsigned long long *next_n,
                                          uint32_t *set_full, uint64_t *lds_next) {
  const uint64_t node = entry >> 1, dir = entry & 1ull;
  const int sh = 2 * (nb.k - 1);
  const uint64_t x = dir ? ((uint64_t)b << sh) | node : (node << 2) | b;
  const uint64_t rc = revcomp(x, nb.k);
  const uint64_t cn = x < rc ? x : rc;
  uint32_t cnt;
  if constexpr (DEPTH) cnt = nb_count(tb, cn, nb.lanes);
  else cnt = nb_count(tb, cn);
  if (cnt < nb.min_count) return;
  const int ins = nb_set_insert(nb.kset, nb.kset_mask, cn);
  if (ins < 0) {
    atomicOr(set_full, 1u);
    return;
  }
  if (ins) {
    const unsigned long long at = atomicAdd(k_n, 1ull);
    if (at >= nb.cap) return;  // the level does not fit: nothing of it will be kept
    nb.kmers[at] = cn;
    nb.counts[at] = cnt;
  }
  const uint64_t succ = (dir ? x >> 2 : x & ((1ull << sh) - 1ull)) << 1 | dir;
  const int v = nb_set_insert(nb.vis, nb.vis_mask, succ);
  if (v < 0) atomicOr(set_full, 1u);
  if (v <= 0) return;
  const unsigned long long at = atomicAdd(next_n, 1ull);
  if (at < nb.fringe_cap) next_list[at] = succ;
  if (lds_next && at < NB_NARROW) lds_next[at] = succ;
}

// WIDE: one level per launch, one thread per (entry, base); the host reads the two fills back and decides.  SHARDED: a
// thread makes one probe, so it reads its share's descriptor from the directory in device memory, once.
template <bool SHARDED>
__global__ void __launch_bounds__(WG) k_nb_wide(NbTable<SHARDED> tb, NbRef nb, NbCtl *ctl, uint32_t cur_sel, uint64_t cur_n) {
  const uint64_t t = (uint64_t)blockIdx.x * WG + threadIdx.x;
  if (t >= cur_n * 4) return;
  nb_expand(tb, nb, nb.list[cur_sel][t >> 2], (uint32_t)(t & 3), nb.list[cur_sel ^ 1], &ctl->k_n, &ctl->next_n,
            &ctl->set_full, nullptr);
}
// k_nb_wide with the probe bounded by nb.lanes (one table; a multi-device context takes no depth).
__global__ void __launch_bounds__(WG) k_nb_wide_depth(TableRef tb, NbRef nb, NbCtl *ctl, uint32_t cur_sel, uint64_t cur_n) {
  const uint64_t t = (uint64_t)blockIdx.x * WG + threadIdx.x;
  if (t >= cur_n * 4) return;
  nb_expand<true>(tb, nb, nb.list[cur_sel][t >> 2], (uint32_t)(t & 3), nb.list[cur_sel ^ 1], &ctl->k_n, &ctl->next_n,
                  &ctl->set_full, nullptr);
}

// NARROW: one workgroup takes a level of at most NB_NARROW entries through as many levels as it stays that thin —
// the two entry lists and the fill counters in LDS, a workgroup barrier between levels, no host round trip.  It
// stops with ctl->status = why: the neighbourhood is complete, max_levels reached, the next level did not fit the
// caller's capacities (ctl then describes the level before it), or it is too wide for one workgroup (k_nb_wide's).
// (The level loop itself; k_nb_narrow_panel runs it for its job.)
template <bool DEPTH = false, class Table>
__device__ __forceinline__ void nb_narrow_levels(const Table &tb, const NbRef &nb, NbCtl *ctl) {
  __shared__ uint64_t s_list[2][NB_NARROW];
  __shared__ unsigned long long s_kn, s_kstart, s_nextn, s_curfull;  // s_curfull: the current level's size, s_curn capped
  __shared__ uint32_t s_full, s_status, s_curn, s_sel, s_levels;
  const uint32_t tid = threadIdx.x;
  if (tid == 0) {
    s_kn = s_kstart = ctl->k_n;
    s_curfull = ctl->cur_n;
    s_nextn = 0;
    s_full = 0;
    s_status = NB_RUN;
    s_curn = (uint32_t)ctl->cur_n;  // ≤ NB_NARROW: the host's launch condition
    s_sel = ctl->cur_sel;
    s_levels = ctl->levels_done;
  }
  __syncthreads();
  const uint32_t sel0 = s_sel;
  const uint64_t *list0 = sel0 ? nb.list[1] : nb.list[0];  // (a select, not an index: nb stays in registers)
  for (uint32_t i = tid; i < s_curn; i += NB_WG) s_list[sel0][i] = list0[i];
  __syncthreads();
  while (true) {
    const uint32_t sel = s_sel, cur_n = s_curn;
    for (uint32_t t = tid; t < cur_n * 4; t += NB_WG)
      nb_expand<DEPTH>(tb, nb, s_list[sel][t >> 2], t & 3, sel ? nb.list[0] : nb.list[1], &s_kn, &s_nextn, &s_full, s_list[sel ^ 1]);
    __syncthreads();
    if (tid == 0) {
      if (s_full || s_kn > nb.cap || s_nextn > nb.fringe_cap) {
        s_kn = s_kstart;  // the level is dropped: the k-mer list back to its start, the entry list as it was
        s_status = NB_OVERFLOW;
      } else {
        s_levels += 1;
        s_sel = sel ^ 1;
        s_kstart = s_kn;
        s_curfull = s_nextn;
        s_curn = (uint32_t)(s_nextn < NB_NARROW ? s_nextn : NB_NARROW);
        if (s_nextn == 0)
          s_status = NB_COMPLETE;
        else if (nb.max_levels && s_levels >= nb.max_levels)
          s_status = NB_LIMIT;
        else if (s_nextn > NB_NARROW)
          s_status = NB_WIDE;
        s_nextn = 0;
      }
    }
    __syncthreads();
    if (s_status != NB_RUN) break;
  }
  if (tid == 0) {
    ctl->k_n = s_kn;
    ctl->next_n = 0;
    ctl->cur_n = s_curfull;
    ctl->levels_done = s_levels;
    ctl->cur_sel = s_sel;
    ctl->status = s_status;
    ctl->set_full = s_full;
  }
}

// The jobs: many independent ones side by side, each with its own NbRef (two sets, two entry lists, k-mer list) and
// NbCtl in device arrays.  Nothing is shared between jobs and no workgroup waits for another:
// jobs beyond what the card holds at once queue behind the others.
//
// Level 0 of every job in one launch: seed i (the jobs' sorted seed lists back to back) belongs to job seed_job[i],
// whose seeds start at seed_start[job]; it goes into that job's first entry list and visited set.
__global__ void __launch_bounds__(WG) k_nb_seed_panel(const NbRef *__restrict__ refs, NbCtl *ctls,
                                                      const uint64_t *__restrict__ seeds,
                                                      const uint32_t *__restrict__ seed_job,
                                                      const uint64_t *__restrict__ seed_start, uint64_t n) {
  const uint64_t i = (uint64_t)blockIdx.x * WG + threadIdx.x;
  if (i >= n) return;
  const uint32_t j = seed_job[i];
  const uint64_t e = seeds[i];
  refs[j].list[0][i - seed_start[j]] = e;  // (< the job's distinct seeds ≤ its fringe_cap: the host's check)
  if (nb_set_insert(refs[j].vis, refs[j].vis_mask, e) < 0) atomicOr(&ctls[j].set_full, 1u);
}

// One workgroup per job, blockIdx.x the job: the narrow level loop on the job's own NbRef / NbCtl.  A job that is
// not there to be run — no seeds (NB_COMPLETE from the host) or a level 0 too wide for a workgroup (NB_WIDE) — is left
// as it is; the host takes the wide ones on afterwards, one at a time (k_nb_wide per level, and this kernel with a grid
// of 1 on the job's own pair when a level fits a workgroup again).
// SHARDED: which share a probe goes to differs from lane to lane, so the directory is staged into LDS once per workgroup
// (at most 64 × 48 B = 3 KiB beside the 16 KiB of entry lists) and choosing the owner is one LDS read, not a chain of
// dependent global loads per probe.
template <bool SHARDED>
__global__ void __launch_bounds__(NB_WG) k_nb_narrow_panel(NbTable<SHARDED> tb, const NbRef *__restrict__ refs, NbCtl *ctls) {
  NbCtl *ctl = &ctls[blockIdx.x];
  if (ctl->status != NB_RUN || ctl->cur_n == 0 || ctl->cur_n > NB_NARROW) return;  // (the same for every thread: ctl is written at the end only)
  const NbRef nb = refs[blockIdx.x];  // (a private copy: scalar loads once, not after every atomic of the level loop)
  if constexpr (SHARDED) {
    static_assert(sizeof(TableRef) % 8 == 0, "the directory is copied in 8-byte words");
    __shared__ TableRef s_dir[NB_MAX_SHARES];
    constexpr uint32_t W = sizeof(TableRef) / 8;
    const uint32_t n8 = (1u << (tb.owner_bits < 6 ? tb.owner_bits : 6)) * W;  // (≤ NB_MAX_SHARES entries whatever the argument says)
    for (uint32_t i = threadIdx.x; i < n8; i += NB_WG)
      reinterpret_cast<uint64_t *>(s_dir)[i] = reinterpret_cast<const uint64_t *>(tb.dir)[i];
    __syncthreads();
    nb_narrow_levels(NbShards{s_dir, tb.owner_bits}, nb, ctl);
  } else {
    nb_narrow_levels(tb, nb, ctl);
  }
}
// k_nb_narrow_panel with every job's probe bounded by its own refs[job].lanes (one table).
__global__ void __launch_bounds__(NB_WG) k_nb_narrow_panel_depth(TableRef tb, const NbRef *__restrict__ refs, NbCtl *ctls) {
  NbCtl *ctl = &ctls[blockIdx.x];
  if (ctl->status != NB_RUN || ctl->cur_n == 0 || ctl->cur_n > NB_NARROW) return;
  const NbRef nb = refs[blockIdx.x];
  nb_narrow_levels<true>(tb, nb, ctl);
}

// What a job hands back, packed: its k_n k-mers and counts from pack_k, its n_f fringe entries (the unexpanded level,
// list[sel]) from pack_f — so that the host fetches three arrays for the whole panel whatever the capacities were.
struct NbPack {
  unsigned long long k_n, n_f, pack_k, pack_f;
  uint32_t sel, pad;
};
__global__ void __launch_bounds__(WG) k_nb_pack_panel(const NbRef *__restrict__ refs, const NbPack *__restrict__ pk,
                                                      uint64_t *__restrict__ out_k, uint32_t *__restrict__ out_c,
                                                      uint64_t *__restrict__ out_f) {
  const NbPack p = pk[blockIdx.x];
  const NbRef &nb = refs[blockIdx.x];
  const uint64_t *kmers = nb.kmers;
  const uint32_t *counts = nb.counts;
  for (unsigned long long i = threadIdx.x; i < p.k_n; i += WG) {
    out_k[p.pack_k + i] = kmers[i];
    out_c[p.pack_k + i] = counts[i];
  }
  const uint64_t *src = (p.sel & 1u) ? nb.list[1] : nb.list[0];
  for (unsigned long long i = threadIdx.x; i < p.n_f; i += WG) out_f[p.pack_f + i] = src[i];
}

// ==========================================================================================
// K_OLIGO: the primer seed scan of sPCR, find_oligos_in_kmers (src/pcr/primers.rs:163-226): one
// bandwidth-bound pass over the merged table.  A k-mer with count ≥ min_count is reported as
// is when its first oligo_len bases equal one of the oligos, or reverse-complemented when its
// LAST oligo_len bases equal the reverse complement of one (primers.rs:212-223).  The two
// sorted oligo sets sit in LDS; membership = binary search.
// ==========================================================================================
__device__ __forceinline__ bool in_sorted(const uint64_t *a, uint32_t n, uint64_t x) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    uint32_t mid = (lo + hi) >> 1;
    if (a[mid] < x) lo = mid + 1;
    else hi = mid;
  }
  return lo < n && a[lo] == x;
}

__global__ void __launch_bounds__(WG) k_find_oligos(TableRef tb, uint64_t slot0, uint64_t slot1, int k,
                                                    int oligo_len, uint32_t min_count,
                                                    const uint64_t *__restrict__ fwd_set /* shifted, sorted */,
                                                    const uint64_t *__restrict__ rc_set /* sorted */,
                                                    uint32_t n_oligos, uint64_t *__restrict__ out_kmers,
                                                    uint32_t *__restrict__ out_counts, uint64_t cap,
                                                    unsigned long long *__restrict__ n_out) {
  extern __shared__ uint64_t sets[];  // fwd then rc
  for (uint32_t i = threadIdx.x; i < n_oligos; i += WG) {
    sets[i] = fwd_set[i];
    sets[n_oligos + i] = rc_set[i];
  }
  __syncthreads();
  const uint64_t mask = ((1ull << (2 * oligo_len)) - 1) << (2 * (k - oligo_len));
  const uint64_t rc_mask = (1ull << (2 * oligo_len)) - 1;
  for (uint64_t s = slot0 + (uint64_t)blockIdx.x * WG + threadIdx.x; s < slot1;
       s += (uint64_t)gridDim.x * WG) {
    const uint64_t key = tb.keys[s];
    if (key == EMPTY) continue;
    uint32_t cum = 0;
    for (uint32_t l = 0; l < tb.n_lanes; ++l) cum = sat_add_u32(cum, tb.vals[(uint64_t)l * tb.cap + s]);
    if (cum < min_count) continue;
    uint64_t hit = EMPTY;
    if (in_sorted(sets, n_oligos, key & mask)) hit = key;
    else if (in_sorted(sets + n_oligos, n_oligos, key & rc_mask)) hit = revcomp(key, k);
    if (hit != EMPTY) {
      unsigned long long i = atomicAdd(n_out, 1ull);
      if (i < cap) {
        out_kmers[i] = hit;
        out_counts[i] = cum;
      }
    }
  }
}

// ==========================================================================================
// K_PRIMER: sPCR's primer seed discovery, get_primer_kmers (src/pcr/primers.rs:234-480), for a panel of
// primer directions and all their mismatch levels in one pass over the merged table.  Level m of a primer
// P (length L) holds the strings with m positions i whose base is not in allowed(P[i]) (shk_primer.cpp),
// so per k-mer: four "base equals b" planes (one bit per 2-bit field), ANDed with the primer's allow
// masks (zero outside the first L fields) → f = L − popcount.  The same on revcomp(key) gives r.  A
// k-mer yields key at level f (f ≤ M) and revcomp(key) at level r (r ≤ M, r ≠ f: primers.rs:212-223).
// Records go out through one atomic per wave; per-(primer, level) hit counts are kept in LDS and are
// complete even when the record buffer overflows (the host then reruns with the levels cut).
// ==========================================================================================
struct PrimerDev {  // 48 B
  uint64_t allow[4];
  uint32_t L, M;    // M: the highest level kept (the primer's M, or its cut level on a rerun)
  uint32_t min_count, pad_;
};
struct PrimerRec {  // 16 B
  uint64_t kmer;
  uint32_t count;
  uint32_t tag;     // primer << 8 | level
};

__device__ __forceinline__ void base_planes(uint64_t x, uint64_t eq[4]) {
  constexpr uint64_t LO = 0x5555555555555555ull;
#pragma unroll
  for (uint32_t b = 0; b < 4; ++b) {
    const uint64_t y = x ^ (LO * b);  // field == b ⇔ both bits of the field zero
    eq[b] = ~(y | (y >> 1)) & LO;
  }
}

__global__ void __launch_bounds__(WG) k_primer_scan(TableRef tb, uint64_t slot0, uint64_t slot1, int k,
                                                    const PrimerDev *__restrict__ prim, uint32_t n_prim,
                                                    uint32_t p_base, uint32_t stride /* levels per primer in LDS */,
                                                    PrimerRec *__restrict__ out, uint64_t cap,
                                                    unsigned long long *__restrict__ n_out,
                                                    unsigned long long *__restrict__ hits /* [p][SHK_PRIMER_LEVELS] */) {
  extern __shared__ uint64_t lds[];
  PrimerDev *sp = (PrimerDev *)lds;
  uint32_t *cnt = (uint32_t *)(sp + n_prim);
  for (uint32_t i = threadIdx.x; i < n_prim * 6; i += WG) lds[i] = ((const uint64_t *)prim)[i];
  for (uint32_t i = threadIdx.x; i < n_prim * stride; i += WG) cnt[i] = 0;
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t below = (1ull << lane) - 1ull;
  // the loop bound is per workgroup, so every wave runs every trip (ballots see whole waves)
  for (uint64_t s0 = slot0 + (uint64_t)blockIdx.x * WG; s0 < slot1; s0 += (uint64_t)gridDim.x * WG) {
    const uint64_t s = s0 + threadIdx.x;
    const uint64_t key = s < slot1 ? tb.keys[s] : EMPTY;
    uint32_t cum = 0;
    if (key != EMPTY)
      for (uint32_t l = 0; l < tb.n_lanes; ++l) cum = sat_add_u32(cum, tb.vals[(uint64_t)l * tb.cap + s]);
    if (!__any(key != EMPTY)) continue;
    const uint64_t rk = revcomp(key, k);
    uint64_t ef[4], er[4];
    base_planes(key, ef);
    base_planes(rk, er);
    for (uint32_t p = 0; p < n_prim; ++p) {
      const PrimerDev &P = sp[p];
      const bool ok = key != EMPTY && cum >= P.min_count;
      const uint32_t f = P.L - (uint32_t)__popcll((ef[0] & P.allow[0]) | (ef[1] & P.allow[1]) |
                                                  (ef[2] & P.allow[2]) | (ef[3] & P.allow[3]));
      const uint32_t r = P.L - (uint32_t)__popcll((er[0] & P.allow[0]) | (er[1] & P.allow[1]) |
                                                  (er[2] & P.allow[2]) | (er[3] & P.allow[3]));
      const bool hf = ok && f <= P.M;
      const bool hr = ok && r <= P.M && r != f;
      const uint64_t bf = __ballot(hf), br = __ballot(hr);
      if (!(bf | br)) continue;
      const uint32_t nf = (uint32_t)__popcll(bf);
      unsigned long long at = 0;
      if (lane == 0) at = atomicAdd(n_out, (unsigned long long)(nf + __popcll(br)));
      at = __shfl(at, 0);
      const uint32_t tag = (p_base + p) << 8;
      if (hf) {
        const unsigned long long i = at + __popcll(bf & below);
        if (i < cap) out[i] = PrimerRec{key, cum, tag | f};
        atomicAdd(&cnt[p * stride + f], 1u);
      }
      if (hr) {
        const unsigned long long i = at + nf + __popcll(br & below);
        if (i < cap) out[i] = PrimerRec{rk, cum, tag | r};
        atomicAdd(&cnt[p * stride + r], 1u);
      }
    }
  }
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < n_prim * stride; i += WG)
    if (cnt[i]) atomicAdd(&hits[(uint64_t)(p_base + i / stride) * SHK_PRIMER_LEVELS + i % stride], (unsigned long long)cnt[i]);
}

// K_PRIMER at several depths in one pass (shk_primer_kmers_depths).  Per slot the running saturating lane
// sum is snapshot at the listed depths (ascending, at most SHK_PCR_MAX_DEPTHS: the loops over them are unrolled, so the
// snapshots stay in registers); f and r are computed once per (key, primer) whatever the number of depths.  A hit at
// depth j is snap[j] ≥ min_count (the host passes max(min_count, 1): a key whose prefix sum is 0 is not in that table)
// at a level ≤ cut[j], the primer's M or its cut level at that depth on a rerun.  Hits are monotone in j, so a
// (key, primer) that misses at the last depth is dropped before any per-depth work.  Records and hit counters are those
// of k_primer_scan for the virtual primer j · n_all + p.
struct PrimerDepths {  // a kernel argument: uniform, in scalar registers
  uint32_t n;
  uint32_t d[SHK_PCR_MAX_DEPTHS];
};
struct PrimerDevD {    // 64 B
  PrimerDev p;         // (p.M: the highest cut of any depth)
  uint8_t cut[SHK_PCR_MAX_DEPTHS];
};

__global__ void __launch_bounds__(WG) k_primer_scan_depths(TableRef tb, uint64_t slot0, uint64_t slot1, int k,
                                                           const PrimerDevD *__restrict__ prim, uint32_t n_prim,
                                                           uint32_t p_base, uint32_t n_all /* primers of the call */,
                                                           uint32_t stride, PrimerDepths dep,
                                                           PrimerRec *__restrict__ out, uint64_t cap,
                                                           unsigned long long *__restrict__ n_out,
                                                           unsigned long long *__restrict__ hits /* [depth][p][SHK_PRIMER_LEVELS] */) {
  extern __shared__ uint64_t lds[];
  PrimerDevD *sp = (PrimerDevD *)lds;
  uint32_t *cnt = (uint32_t *)(sp + n_prim);  // [p][depth][stride]
  const uint32_t n_cnt = n_prim * dep.n * stride;
  for (uint32_t i = threadIdx.x; i < n_prim * 8; i += WG) lds[i] = ((const uint64_t *)prim)[i];
  for (uint32_t i = threadIdx.x; i < n_cnt; i += WG) cnt[i] = 0;
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t below = (1ull << lane) - 1ull;
  for (uint64_t s0 = slot0 + (uint64_t)blockIdx.x * WG; s0 < slot1; s0 += (uint64_t)gridDim.x * WG) {
    const uint64_t s = s0 + threadIdx.x;
    const uint64_t key = s < slot1 ? tb.keys[s] : EMPTY;
    uint32_t snap[SHK_PCR_MAX_DEPTHS];
    {
      uint32_t cum = 0, l = 0;
#pragma unroll
      for (uint32_t j = 0; j < SHK_PCR_MAX_DEPTHS; ++j) {
        if (j < dep.n && key != EMPTY)
          for (; l < dep.d[j]; ++l) cum = sat_add_u32(cum, tb.vals[(uint64_t)l * tb.cap + s]);
        snap[j] = cum;  // (beyond dep.n: the last depth's, never read)
      }
    }
    const uint32_t deepest = snap[SHK_PCR_MAX_DEPTHS - 1];
    if (!__any(deepest != 0)) continue;
    const uint64_t rk = revcomp(key, k);
    uint64_t ef[4], er[4];
    base_planes(key, ef);
    base_planes(rk, er);
    for (uint32_t p = 0; p < n_prim; ++p) {
      const PrimerDev &P = sp[p].p;
      const bool ok = key != EMPTY && deepest >= P.min_count;
      const uint32_t f = P.L - (uint32_t)__popcll((ef[0] & P.allow[0]) | (ef[1] & P.allow[1]) |
                                                  (ef[2] & P.allow[2]) | (ef[3] & P.allow[3]));
      const uint32_t r = P.L - (uint32_t)__popcll((er[0] & P.allow[0]) | (er[1] & P.allow[1]) |
                                                  (er[2] & P.allow[2]) | (er[3] & P.allow[3]));
      const bool cf = ok && f <= P.M;
      const bool cr = ok && r <= P.M && r != f;
      if (!__any(cf || cr)) continue;
#pragma unroll
      for (uint32_t j = 0; j < SHK_PCR_MAX_DEPTHS; ++j) {
        if (j < dep.n) {  // (uniform)
          const uint32_t cut = sp[p].cut[j];
          const bool here = snap[j] >= P.min_count;
          const bool hf = cf && here && f <= cut;
          const bool hr = cr && here && r <= cut;
          const uint64_t bf = __ballot(hf), br = __ballot(hr);
          if (bf | br) {
            const uint32_t nf = (uint32_t)__popcll(bf);
            unsigned long long at = 0;
            if (lane == 0) at = atomicAdd(n_out, (unsigned long long)(nf + __popcll(br)));
            at = __shfl(at, 0);
            const uint32_t tag = (j * n_all + p_base + p) << 8;
            uint32_t *c = cnt + (p * dep.n + j) * stride;
            if (hf) {
              const unsigned long long i = at + __popcll(bf & below);
              if (i < cap) out[i] = PrimerRec{key, snap[j], tag | f};
              atomicAdd(&c[f], 1u);
            }
            if (hr) {
              const unsigned long long i = at + nf + __popcll(br & below);
              if (i < cap) out[i] = PrimerRec{rk, snap[j], tag | r};
              atomicAdd(&c[r], 1u);
            }
          }
        }
      }
    }
  }
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < n_cnt; i += WG)
    if (cnt[i]) {
      const uint32_t p = i / (dep.n * stride), j = i / stride % dep.n, m = i % stride;
      atomicAdd(&hits[((uint64_t)j * n_all + p_base + p) * SHK_PRIMER_LEVELS + m], (unsigned long long)cnt[i]);
    }
}

// ==========================================================================================
// What the read walkers below share (K_FILTER, K_KMERS, K_THREAD, K_FILTER_PANEL): the probe of a lookup set, the key runs
// behind it, and a read's bytes as canonical k-mers — rolling, one thread per read; as bit planes, one wave per read.
// ==========================================================================================
constexpr uint32_t SET_NONE = 0xFFFFFFFFu;         // set_find: the key is not in the set
// The slot of `key` in an open-addressing set of mask + 1 slots (EMPTY where free; from set_hash(key) on, linear; the
// host keeps the load ≤ 1/2, so a probe ends), or SET_NONE.  keys may lie in LDS or in global memory.
__device__ __forceinline__ uint32_t set_find(const uint64_t *keys, uint32_t mask, uint64_t key) {
  for (uint32_t s = set_hash(key) & mask;; s = (s + 1) & mask) {
    const uint64_t cur = keys[s];
    if (cur == key) return s;
    if (cur == EMPTY) return SET_NONE;
  }
}

// KEYRUNS: a lookup set whose every key owns a run of items — the edges that spell a k-mer (K_THREAD), the genes that
// hold a primer k-mer (K_FILTER_PANEL).  The host builds it (key_runs_build, shk_reads_api.hip.h).
struct KeyRuns {
  const uint64_t *keys;   // [mask + 1] canonical k-mer or EMPTY: the set set_find probes
  const uint32_t *start;  // [mask + 1] the key's first item in items
  const uint32_t *items;  // [n_items] ascending by (key, item): a key's items lie side by side
  const uint32_t *last;   // [(n_items + 31) / 32] bit i: items[i] is the last of its key's run (run_ends)
  uint32_t mask, n_items;
};
__device__ __forceinline__ bool run_ends(const uint32_t *last, uint32_t i) { return (last[i >> 5] >> (i & 31u)) & 1u; }
// Its bytes and its layout in LDS: keys, start, items, last from an 8-byte-aligned base, so the uint64_t array stays
// 8-byte aligned; a uint4 array goes in FRONT of it at a 16-byte-aligned base (K_THREAD's meta: the keys stay aligned).
__host__ __device__ inline size_t key_runs_bytes(uint32_t cap, uint32_t n_items) {
  return (size_t)cap * 12 + (size_t)n_items * 4 + (size_t)((n_items + 31) / 32) * 4;
}
// every thread of the workgroup (nt threads) calls it; the caller's __syncthreads() completes the copy
__device__ __forceinline__ KeyRuns key_runs_to_lds(const KeyRuns &g, uint8_t *base, uint32_t nt) {
  const uint32_t cap = g.mask + 1, n = g.n_items;
  uint64_t *lk = (uint64_t *)base;
  uint32_t *ls = (uint32_t *)(lk + cap), *li = ls + cap, *ll = li + n;
  for (uint32_t i = threadIdx.x; i < cap; i += nt) lk[i] = g.keys[i], ls[i] = g.start[i];
  for (uint32_t i = threadIdx.x; i < n; i += nt) li[i] = g.items[i];
  for (uint32_t i = threadIdx.x; i < (n + 31) / 32; i += nt) ll[i] = g.last[i];
  return KeyRuns{lk, ls, li, ll, g.mask, n};
}

// kmers_from_ascii (src/kmer/encoding.rs:332-371) one byte at a time: the one-thread-per-read form of K_FILTER and K_KMERS.
struct RollingKmer {
  uint64_t mask, fwd = 0, rev = 0;
  int k, n_valid = 0;
  __device__ __forceinline__ explicit RollingKmer(int k_) : mask((1ull << (2 * k_)) - 1), k(k_) {}
  // → 1: *key = the canonical k-mer that ends at c; 0: none (an N restarts, encoding.rs:346-352); −1: c is outside ACGTN (:353-356)
  __device__ __forceinline__ int step(uint32_t c, uint64_t *key) {
    if (c == 'N') return n_valid = 0;
    if (!byte_is_acgtn(c)) return -1;
    const uint64_t b2 = ((c >> 1) ^ (c >> 2)) & 3u;
    fwd = ((fwd << 2) | b2) & mask;
    rev = (rev >> 2) | ((3 - b2) << (2 * (k - 1)));
    if (++n_valid < k) return 0;
    *key = fwd < rev ? fwd : rev;
    return 1;
  }
};

// One wave step's bytes rb[p] (p = the step's first byte + lane; beyond len: 'A') as wave-wide bit planes: code bit 0,
// code bit 1, N, and whether any of them is outside ACGTN.  Ballots: the planes live in scalar registers.
struct ReadPlanes {
  uint64_t p0, p1, n;
  bool bad;
};
__device__ __forceinline__ ReadPlanes read_planes(const uint8_t *__restrict__ rb, uint32_t p, uint32_t len) {
  const uint32_t c = p < len ? rb[p] : (uint32_t)'A';
  const uint32_t b2 = ((c >> 1) ^ (c >> 2)) & 3u;
  return ReadPlanes{__ballot(b2 & 1u), __ballot(b2 >> 1), __ballot(c == 'N'), __ballot(!byte_is_acgtn(c)) != 0};
}
// Where the wave-per-read walks (K_THREAD, K_FILTER_PANEL) take a read's planes from.  A batch source opens read r as
// a read source and gives its length; planes(s, lane, len) are the 64 positions from s on, lane l's at s + l.
//   AsciiReads / AsciiRead     the batch as ASCII plus offsets in HBM: a byte load per lane and four ballots per step.
//   PlaneReads / PlaneRead     the retained store (K_RETAIN below): the planes lie there as bits, so a step
//                              is six wave-uniform 8-byte loads and three funnel shifts (retain_plane).  The addresses are
//                              formed through readfirstlane: the loads are the scalar unit's.  No read of the store has an
//                              invalid byte (the ingest that found one poisoned the context): bad is constant false.
struct AsciiRead {
  const uint8_t *rb;
  __device__ __forceinline__ ReadPlanes planes(uint32_t s, uint32_t lane, uint32_t len) const { return read_planes(rb, s + lane, len); }
};
struct AsciiReads {
  const uint8_t *bases;
  const uint64_t *offsets;
  __device__ __forceinline__ AsciiRead open(uint64_t r, uint32_t *len) const {
    const uint64_t b0 = offsets[r];
    *len = (uint32_t)(offsets[r + 1] - b0);
    return AsciiRead{bases + b0};
  }
};
__device__ __forceinline__ uint64_t uniform64(uint64_t x) {
  return ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(x >> 32)) << 32) |
         (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)x);
}
struct PlaneRead {
  const uint64_t *p0, *p1, *nn;
  uint64_t b0;  // the read's first bit (wave-uniform)
  __device__ __forceinline__ ReadPlanes planes(uint32_t s, uint32_t, uint32_t len) const {
    const uint32_t su = (uint32_t)__builtin_amdgcn_readfirstlane((int)s), lu = (uint32_t)__builtin_amdgcn_readfirstlane((int)len);
    return ReadPlanes{retain_plane(p0, b0, su, lu), retain_plane(p1, b0, su, lu), retain_plane(nn, b0, su, lu), false};
  }
};
struct PlaneReads {
  const uint64_t *p0, *p1, *nn;
  const uint64_t *offsets;  // [n_reads + 1] first bit of every read, the store's end last
  __device__ __forceinline__ PlaneRead open(uint64_t r, uint32_t *len) const {
    const uint64_t ru = uniform64(r), b0 = offsets[ru];
    *len = (uint32_t)(offsets[ru + 1] - b0);
    return PlaneRead{p0, p1, nn, b0};
  }
};

// bit i of x → bit 2i
__device__ __forceinline__ uint64_t spread2(uint32_t x) {
  uint64_t v = x;
  v = (v | (v << 16)) & 0x0000FFFF0000FFFFull;
  v = (v | (v << 8)) & 0x00FF00FF00FF00FFull;
  v = (v | (v << 4)) & 0x0F0F0F0F0F0F0F0Full;
  v = (v | (v << 2)) & 0x3333333333333333ull;
  v = (v | (v << 1)) & 0x5555555555555555ull;
  return v;
}
// bits l … l+31 of the 128-bit value hi:lo (l < 64)
__device__ __forceinline__ uint32_t window32(uint64_t lo, uint64_t hi, uint32_t l) {
  return (uint32_t)((lo >> l) | ((hi << 1) << (63 - l)));
}
// Lane `lane`'s window of the step at s0: bits lane … lane+k−1 of two steps' planes (lo: the bytes from s0 on, hi: the
// next 64), km = 2^k − 1, k ≤ 31.  → whether it is a list element (one of the read's n_win windows, without an N) and if
// so *key = its canonical k-mer: the code planes bit-reversed and interleaved, or their complements, not reversed.
__device__ __forceinline__ bool window_key(const ReadPlanes &lo, const ReadPlanes &hi, uint32_t lane, int k, uint32_t km, uint32_t s0,
                                           uint32_t n_win, uint64_t *key) {
  if (s0 + lane >= n_win || (window32(lo.n, hi.n, lane) & km) != 0) return false;
  const uint32_t w0 = window32(lo.p0, hi.p0, lane) & km, w1 = window32(lo.p1, hi.p1, lane) & km;
  const uint64_t fwd = spread2(__brev(w0) >> (32 - k)) | (spread2(__brev(w1) >> (32 - k)) << 1);
  const uint64_t rev = spread2(~w0 & km) | (spread2(~w1 & km) << 1);
  *key = fwd < rev ? fwd : rev;
  return true;
}

// ==========================================================================================
// K_FILTER: PrimerReadFilter::matches (src/pcr/read_filter.rs:43-49) for a batch of reads: a read
// matches when kmers_from_ascii accepts it (no byte outside ACGTN — otherwise the reference
// returns false for the whole read) and at least one of its canonical k-mers is in the set.
// One thread per read (reads are a few hundred bases; this is the step before sPCR's read
// threading, not the counting hot path); the set is a small open-addressing table of mixed keys.
// ==========================================================================================
__global__ void __launch_bounds__(WG) k_filter_reads(const uint8_t *__restrict__ bases,
                                                     const uint64_t *__restrict__ offsets, uint64_t n_seqs,
                                                     int k, const uint64_t *__restrict__ set_keys,
                                                     uint32_t set_mask, uint8_t *__restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * WG + threadIdx.x;
  if (i >= n_seqs) return;
  RollingKmer roll(k);
  uint64_t key = 0;
  bool hit = false, ok = true;
  for (uint64_t p = offsets[i], e = offsets[i + 1]; p < e; ++p) {
    const int got = roll.step(bases[p], &key);
    if (got < 0) {  // → Err → matches() is false
      ok = false;
      break;
    }
    if (got && !hit) hit = set_find(set_keys, set_mask, key) != SET_NONE;
  }
  out[i] = ok && hit;
}

// ==========================================================================================
// K_KMERS: kmers_from_ascii (src/kmer/encoding.rs:332-371) for a batch of reads, k-mers returned in
// read order (what thread_reads consumes, pcr/threading.rs:97-101).  Same one-thread-per-read
// rolling form as K_FILTER; read i writes at koff[i] (host prefix of max(0, len − k + 1)).
// ==========================================================================================
__global__ void __launch_bounds__(WG) k_kmers_from_reads(const uint8_t *__restrict__ bases,
                                                         const uint64_t *__restrict__ offsets,
                                                         const uint64_t *__restrict__ koff, uint64_t n_seqs,
                                                         int k, uint64_t *__restrict__ out,
                                                         uint32_t *__restrict__ n_out,
                                                         uint8_t *__restrict__ bad_byte) {
  const uint64_t i = (uint64_t)blockIdx.x * WG + threadIdx.x;
  if (i >= n_seqs) return;
  RollingKmer roll(k);
  uint64_t key = 0;
  uint32_t n = 0, bad = 0;
  uint64_t *dst = out + koff[i];
  for (uint64_t p = offsets[i], e = offsets[i + 1]; p < e; ++p) {
    const uint32_t c = bases[p];
    const int got = roll.step(c, &key);
    if (got < 0) {  // → Err for the whole read
      bad = c;
      break;
    }
    if (got) dst[n++] = key;
  }
  n_out[i] = bad ? 0u : n;
  bad_byte[i] = (uint8_t)bad;
}

// ==========================================================================================
// K_THREAD: thread_reads (src/pcr/threading.rs:87-192) for a batch of reads against a graph given as a lookup set
// the host built (shk_thread_reads; the kernel is k_thread_panel below).  One WAVE per read, THREAD_TILE = 64 window start positions per
// step, one per lane:
//   bases      64 new bytes per step as bit planes (read_planes), each lane's window and key from them (window_key).  A
//              window with an N is no list element (encoding.rs:346-352): its lane sits out, and "the previous element"
//              of a lane is the nearest lower lane that has one — or the carry from the step before.
//   probe      position-parallel (set_find) → first candidate (build_edge_lookup, threading.rs:203-220).  An element
//              with ONE candidate has its edge there and then.
//   resolve    the only sequential step (resolve_candidates, threading.rs:233-256): elements with more candidates,
//              in list order (a ballot and a loop over its bits, wave-uniform), each after its predecessor is final.
//   runs       from the neighbour lanes (find_contiguous_runs, threading.rs:261-315): an element CONTINUES the run
//              when its predecessor hit and tgt(prev) == src(this); a continuing pair over a branch node is a BRANCH
//              PAIR (record_branch_links, threading.rs:341-364).  "some branch pair between the run's start and
//              here" (pre) is a few mask operations on two ballots.
// What crosses a step: the last element's (hit, target, link base, pre).  What a read's counters need and a step
// cannot know — whether the read is valid at all (an invalid byte anywhere cancels it, threading.rs:98-101) and
// whether the run goes on to meet a branch pair LATER (is_run_unambiguous, threading.rs:321-337) — is why the first
// sweep only writes (edge, flags | link slot) per position to the wave's scratch, and a second sweep, last step
// first, carrying "a branch pair between here and the run's end" (suf) the other way, does every atomic: support_total
// per element, support_unambiguous when neither pre nor suf, the link's slot per branch pair.
// A graph's set lies in LDS (copied by a workgroup once; it then walks many reads) with the two support counters
// LDS-private, flushed when the workgroup lets go of the graph — or it stays in global memory: the same code over the
// global arrays.
// ==========================================================================================
constexpr int THREAD_WG = 1024;                    // 16 waves: one workgroup per CU when the set fills its LDS
constexpr uint32_t THREAD_TILE = 64;               // list elements per wave step (engine.py mirrors it as THREAD_TILE)
constexpr uint32_t TH_NONE = 0xFFFFFFFFu;          // no edge / no link base (edge indices and slots stay below)
static_assert(THREAD_TILE == 64, "one window per lane of a wave");
constexpr int THREAD_LDS_EDGES = 2048;             // graphs up to this many edges keep their set in LDS (SHK_THREAD_LDS_EDGES) …
constexpr size_t THREAD_LDS_MAX = 128u << 10;      // … if it fits this much of a CU's 160 KiB (2048 edges: at most 104.3 KiB)

// bytes of LDS of a graph whose set k_thread_panel keeps there, in its order: meta, the key runs, the two private counters
__host__ __device__ inline size_t thread_lds_bytes(uint32_t cap, uint32_t n_edges) {
  return (size_t)n_edges * 16 + key_runs_bytes(cap, n_edges) + (size_t)n_edges * 8;
}

// A graph in front of the walk of one read: its set and meta, in LDS or in global memory, and its counters — the
// two supports where the kernel keeps them (LDS-private or global), the link slots always global.
struct ThreadView {
  KeyRuns runs;       // canonical edge k-mer → its candidates: the edges, ascending by (key, edge)
  const uint4 *meta;  // [runs.n_items] {src, tgt, link slot base of the pairs (e, ·) or TH_NONE, rank of e among its source's out-edges}
  uint32_t *total, *unamb, *links;
};

// The walk of ONE read by one wave — both sweeps, from its first bytes to its last atomic (see K_THREAD above): rd, len
// the read as its source opened it (AsciiRead or PlaneRead), scr the wave's scratch (one entry per window of the read) →
// the edges the read was mapped to (read_edges).  thread_panel_body calls it with the view of the gene it holds.
template <class Read>
__device__ __forceinline__ uint32_t thread_walk(const ThreadView &t, const Read &rd, uint32_t len, int k, uint2 *__restrict__ scr, uint32_t lane) {
  const uint32_t km = (1u << k) - 1u;         // k ≤ 31
  const uint64_t below = (1ull << lane) - 1;  // the lanes under mine
  const uint64_t upto = below | (1ull << lane);
  const uint32_t n_win = len >= (uint32_t)k ? len - (uint32_t)k + 1u : 0u;  // (a shorter read has no k-mer, valid or not)
  uint32_t n_hit = 0;
  bool bad = false;
  // ---- sweep 1, first step first: edges, run flags, link slots → scratch
  uint32_t c_hit = 0, c_tgt = 0, c_lbase = TH_NONE, c_pre = 0;  // the last list element so far
  ReadPlanes lo{0, 0, 0, false};
  if (n_win) lo = rd.planes(0, lane, len);
  bad = lo.bad;
  for (uint32_t s0 = 0; s0 < n_win && !bad; s0 += THREAD_TILE) {
    const ReadPlanes hi = rd.planes(s0 + THREAD_TILE, lane, len);  // the step's new bytes: the upper half of its windows' span
    if (hi.bad) {  // encoding.rs:353-356 → Err → the read is skipped whole
      bad = true;
      break;
    }
    uint64_t key = 0;
    const bool v = window_key(lo, hi, lane, k, km, s0, n_win, &key);  // a list element
    uint32_t edge = TH_NONE, src = 0, tgt = 0, lbase = TH_NONE, orank = 0, cstart = 0;
    int hit = 0;
    bool multi = false;
    if (v) {
      const uint32_t s = set_find(t.runs.keys, t.runs.mask, key);
      if (s != SET_NONE) {
        hit = 1, cstart = t.runs.start[s];
        multi = !run_ends(t.runs.last, cstart);
        if (!multi) {
          edge = t.runs.items[cstart];
          const uint4 m = t.meta[edge];
          src = m.x, tgt = m.y, lbase = m.z, orank = m.w;
        }
      }
    }
    const uint64_t vm = __ballot(v);
    for (uint64_t mm = __ballot(multi); mm; mm &= mm - 1) {  // in list order; everything here is wave-uniform
      const int m = __ffsll((unsigned long long)mm) - 1;
      const uint64_t under = vm & ((1ull << m) - 1);
      const int pl = under ? 63 - __clzll((long long)under) : 0;
      const int sh = __shfl(hit, pl);
      const uint32_t st = __shfl(tgt, pl);
      const bool ph = under ? sh != 0 : c_hit != 0;
      const uint32_t pt = under ? st : c_tgt;
      const uint32_t first = __shfl(cstart, m);
      uint32_t pick = t.runs.items[first];  // no previous edge, or none adjacent: candidate 0 (threading.rs:255)
      if (ph)
        for (uint32_t i = first;; ++i) {
          const uint32_t e = t.runs.items[i];
          if (t.meta[e].x == pt) {
            pick = e;
            break;
          }
          if (run_ends(t.runs.last, i)) break;
        }
      const uint4 pm = t.meta[pick];
      if ((int)lane == m) edge = pick, src = pm.x, tgt = pm.y, lbase = pm.z, orank = pm.w;
    }
    // my predecessor in the list
    const uint64_t under = vm & below;
    const int pl = under ? 63 - __clzll((long long)under) : 0;
    const int sh = __shfl(hit, pl);
    const uint32_t st = __shfl(tgt, pl), sl = __shfl(lbase, pl);
    const bool ph = under ? sh != 0 : c_hit != 0;
    const uint32_t pt = under ? st : c_tgt, plb = under ? sl : c_lbase;
    const bool cont = hit && ph && pt == src;
    const bool bp = cont && plb != TH_NONE;
    const uint64_t sm = __ballot(v && !cont), bm = __ballot(bp);
    const uint64_t s_le = sm & upto;
    const bool pre = s_le ? (bm & upto & ~((1ull << (63 - __clzll((long long)s_le))) - 1)) != 0 : ((bm & upto) != 0 || c_pre != 0);
    scr[s0 + lane] = make_uint2(edge, bp ? plb + orank : 0x80000000u | (v ? 4u : 0u) | (pre ? 2u : 0u) | (cont ? 1u : 0u));
    n_hit += (uint32_t)__popcll(__ballot(hit));
    if (vm) {
      const int top = 63 - __clzll((long long)vm);
      c_hit = (uint32_t)__shfl(hit, top), c_tgt = __shfl(tgt, top), c_lbase = __shfl(lbase, top);
      c_pre = (uint32_t)__shfl((int)pre, top);
    }
    lo = hi;
  }
  if (bad) n_hit = 0;
  if (!n_hit) return 0;
  // ---- sweep 2, last step first: the atomics
  __threadfence_block();  // the wave reads what its other lanes wrote
  uint32_t c_suf = 0;     // a branch pair between the next step's start and the end of the run that enters it
  for (uint32_t s0 = (n_win - 1) & ~(THREAD_TILE - 1);; s0 -= THREAD_TILE) {
    const uint2 q = scr[s0 + lane];
    const bool bp = !(q.y >> 31), v = bp || (q.y & 4u), cont = bp || (q.y & 1u), pre = bp || (q.y & 2u);
    const uint64_t sm = __ballot(v && !cont), bm = __ballot(bp);
    const uint64_t s_gt = sm & ~upto;
    const bool suf = s_gt ? (bm & ~upto & ((1ull << (__ffsll((unsigned long long)s_gt) - 1)) - 1)) != 0 : ((bm & ~upto) != 0 || c_suf != 0);
    if (q.x != TH_NONE) {
      atomicAdd(&t.total[q.x], 1u);
      if (!pre && !suf) atomicAdd(&t.unamb[q.x], 1u);
    }
    if (bp) atomicAdd(&t.links[q.y], 1u);
    c_suf = sm ? (bm & ((1ull << (__ffsll((unsigned long long)sm) - 1)) - 1)) != 0 : (bm != 0 || c_suf != 0);
    if (s0 == 0) break;
  }
  return n_hit;
}

// k_thread_panel: the walk for a whole sPCR panel in one launch (shk_thread_reads_panel; shk_thread_reads
// is the panel of one gene that lists every read).  The host
// concatenates every gene's set into one upload and describes each gene in a ThreadGene; the genes' read lists, cut
// into slices, are the JOBS, in (gene, slice) order.  Workgroups are persistent: each walks a contiguous range of jobs
// and so holds one gene at a time — its set in LDS with LDS-private supports, or pointers to the global arrays.  At a job
// of another gene: a barrier (no wave is still walking), the held gene's private supports flushed (one global atomic
// per touched edge), a barrier (nobody still reads what the load overwrites), the new gene loaded, a barrier.  Inside a
// job wave w takes the slice's reads w, w + 16, …: list position → list_reads → offsets → bytes (list_reads == nullptr:
// list position i is read i); read_edges is written at the list position.  No workgroup reads what another wrote: counters meet in global atomics and the host reads
// them after the launch.
struct ThreadGene {              // 64 bytes
  uint64_t keys, start, items, last, meta;  // byte offsets of the gene's arrays within the upload (16-byte aligned each)
  uint32_t mask, n_edges;        // of its set: slots − 1; items = edges
  uint32_t cnt_base, link_base;  // its first edge in total / unamb, its first slot in links
  uint32_t lds, pad;             // whether its set goes to LDS
};
static_assert(sizeof(ThreadGene) == 64, "a gene's descriptor is 64 bytes");
struct ThreadJob {               // 16 bytes
  uint64_t first;                // list position of the slice's first read (within list_reads as uploaded)
  uint32_t gene, n;              // n reads
};
static_assert(sizeof(ThreadJob) == 16, "a job is 16 bytes");
constexpr int THREAD_PANEL_JOB = THREAD_WG / 64;   // reads per job (SHK_THREAD_PANEL_JOB): one per wave of the workgroup — the finest cut that
                                                   // leaves no wave without a read, so the workgroups' shares differ by at most 16 reads; a job
                                                   // costs 16 bytes and one scalar load, a gene change depends on the ranges, not on the cut
static_assert(SHK_THREAD_MAX_GENES == SHK_FILTER_MAX_GENES, "the lists come from shk_filter_reads_panel");

__device__ __forceinline__ ThreadView thread_view_global(const ThreadGene &g, const uint8_t *__restrict__ up, uint32_t *total, uint32_t *unamb,
                                                         uint32_t *links) {
  return ThreadView{KeyRuns{(const uint64_t *)(up + g.keys), (const uint32_t *)(up + g.start), (const uint32_t *)(up + g.items),
                            (const uint32_t *)(up + g.last), g.mask, g.n_edges},
                    (const uint4 *)(up + g.meta), total + g.cnt_base, unamb + g.cnt_base, links + g.link_base};
}

// (the body of k_thread_panel and k_thread_panel_retained: th_lds is the kernel's dynamic LDS — the held gene's meta, key
// runs and two private supports, thread_lds_bytes)
template <class Reads>
__device__ __forceinline__ void thread_panel_body(uint8_t *th_lds, const Reads &rs, const uint64_t *__restrict__ list_reads,
                                                  const ThreadGene *__restrict__ genes, const ThreadJob *__restrict__ jobs, uint32_t n_jobs,
                                                  const uint8_t *__restrict__ upload, int k, uint2 *__restrict__ scratch, uint32_t scr_stride,
                                                  uint32_t *__restrict__ total, uint32_t *__restrict__ unamb, uint32_t *__restrict__ links,
                                                  uint32_t *__restrict__ read_edges) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wib = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  uint2 *scr = scratch + ((uint64_t)blockIdx.x * (THREAD_WG / 64) + wib) * scr_stride;
  // this workgroup's jobs: a contiguous range, so that it changes gene as rarely as possible
  const uint32_t j0 = (uint32_t)((uint64_t)n_jobs * blockIdx.x / gridDim.x), j1 = (uint32_t)((uint64_t)n_jobs * (blockIdx.x + 1) / gridDim.x);
  uint32_t held = TH_NONE;  // the gene this workgroup holds
  ThreadGene g{};
  // the held gene's two private supports, flushed: every thread its own indices
  auto flush = [&]() {
    const uint32_t E = g.n_edges;
    const uint32_t *lt = (const uint32_t *)(th_lds + (size_t)E * 16 + key_runs_bytes(g.mask + 1, E)), *lu = lt + E;
    for (uint32_t i = threadIdx.x; i < E; i += THREAD_WG) {
      if (lt[i]) atomicAdd(&total[g.cnt_base + i], lt[i]);
      if (lu[i]) atomicAdd(&unamb[g.cnt_base + i], lu[i]);
    }
  };
  for (uint32_t j = j0; j < j1; ++j) {
    const ThreadJob job = jobs[j];
    if (job.gene != held) {  // (the same for every thread of the workgroup: the barriers are met by all)
      __syncthreads();
      if (held != TH_NONE && g.lds) flush();
      __syncthreads();
      held = job.gene;
      g = genes[held];
      if (g.lds) {
        const uint32_t E = g.n_edges;
        const ThreadView gv = thread_view_global(g, upload, total, unamb, links);
        uint4 *lm = (uint4 *)th_lds;
        uint32_t *lt = (uint32_t *)(th_lds + (size_t)E * 16 + key_runs_bytes(g.mask + 1, E)), *lu = lt + E;
        key_runs_to_lds(gv.runs, th_lds + (size_t)E * 16, THREAD_WG);
        for (uint32_t i = threadIdx.x; i < E; i += THREAD_WG) lm[i] = gv.meta[i], lt[i] = 0, lu[i] = 0;
      }
      __syncthreads();
    }
    uint32_t *re = read_edges + job.first;
    if (g.lds) {
      const uint32_t E = g.n_edges, cap = g.mask + 1;
      uint8_t *kb = th_lds + (size_t)E * 16;  // key_runs_to_lds' layout
      uint32_t *ls = (uint32_t *)(kb + (size_t)cap * 8), *lt = (uint32_t *)(kb + key_runs_bytes(cap, E));
      const ThreadView view{KeyRuns{(const uint64_t *)kb, ls, ls + cap, ls + cap + E, g.mask, E}, (const uint4 *)th_lds, lt, lt + E,
                            links + g.link_base};
      for (uint32_t i = wib; i < job.n; i += THREAD_WG / 64) {
        const uint64_t r = list_reads ? list_reads[job.first + i] : job.first + i;
        uint32_t len;
        const auto rd = rs.open(r, &len);
        const uint32_t n_hit = thread_walk(view, rd, len, k, scr, lane);
        if (lane == 0) re[i] = n_hit;
      }
    } else {
      const ThreadView view = thread_view_global(g, upload, total, unamb, links);
      for (uint32_t i = wib; i < job.n; i += THREAD_WG / 64) {
        const uint64_t r = list_reads ? list_reads[job.first + i] : job.first + i;
        uint32_t len;
        const auto rd = rs.open(r, &len);
        const uint32_t n_hit = thread_walk(view, rd, len, k, scr, lane);
        if (lane == 0) re[i] = n_hit;
      }
    }
  }
  if (held != TH_NONE && g.lds) {
    __syncthreads();
    flush();
  }
}

__global__ void __launch_bounds__(THREAD_WG) k_thread_panel(const uint8_t *__restrict__ bases, const uint64_t *__restrict__ offsets,
                                                            const uint64_t *__restrict__ list_reads, const ThreadGene *__restrict__ genes,
                                                            const ThreadJob *__restrict__ jobs, uint32_t n_jobs,
                                                            const uint8_t *__restrict__ upload, int k, uint2 *__restrict__ scratch,
                                                            uint32_t scr_stride, uint32_t *__restrict__ total, uint32_t *__restrict__ unamb,
                                                            uint32_t *__restrict__ links, uint32_t *__restrict__ read_edges) {
  extern __shared__ __align__(16) uint8_t th_lds[];
  thread_panel_body(th_lds, AsciiReads{bases, offsets}, list_reads, genes, jobs, n_jobs, upload, k, scratch, scr_stride, total, unamb, links,
                    read_edges);
}
// … over the retained store (shk_thread_reads_panel_retained): list_reads are retained read indices
__global__ void __launch_bounds__(THREAD_WG) k_thread_panel_retained(PlaneReads rs, const uint64_t *__restrict__ list_reads,
                                                                     const ThreadGene *__restrict__ genes, const ThreadJob *__restrict__ jobs,
                                                                     uint32_t n_jobs, const uint8_t *__restrict__ upload, int k,
                                                                     uint2 *__restrict__ scratch, uint32_t scr_stride,
                                                                     uint32_t *__restrict__ total, uint32_t *__restrict__ unamb,
                                                                     uint32_t *__restrict__ links, uint32_t *__restrict__ read_edges) {
  extern __shared__ __align__(16) uint8_t th_lds[];
  thread_panel_body(th_lds, rs, list_reads, genes, jobs, n_jobs, upload, k, scratch, scr_stride, total, unamb, links, read_edges);
}

// ==========================================================================================
// K_FILTER_PANEL: PrimerReadFilter::matches (src/pcr/read_filter.rs:43-49) of every read of a batch against every
// gene of a panel in one walk (shk_filter_reads_panel).  The lookup set the host built maps a canonical
// k-mer to the genes that hold it.  One WAVE per read, THREAD_TILE window start positions per step as in K_THREAD:
//   bases      as K_THREAD: read_planes and window_key, so every byte is loaded once.
//   probe      position-parallel (set_find); a read of a run mostly belongs to no amplicon, so the common step is load,
//              four ballots and one probe that ends on an EMPTY slot.
//   hit        the lane ORs its key's genes into the wave's bitmap of n_genes bits in LDS.
//   emit       only behind the read's last byte — a later invalid byte cancels the read (kmers_from_ascii fails as
//              a whole, encoding.rs:353-356): the lanes walk the bitmap's words, append one (gene, read) record per
//              set bit to a global list (a ballot and one atomic per round, as k_primer_scan) and clear the words;
//              an invalid read only clears.  Records past `cap` are counted, not written: the host reruns with room.
// A record is gene << FILTER_READ_BITS | read, so that sorting the list as numbers gives (gene, read).
// LDS = true: keys and gene runs are copied into LDS by every workgroup once; false: the global arrays, which L2 serves.
// ==========================================================================================
constexpr int FILTER_WG = 1024;                    // 16 waves, as K_THREAD
constexpr uint32_t FILTER_MAX_GENES = 4096;        // a wave's bitmap: 512 bytes at the limit, 8 KiB per workgroup
static_assert(FILTER_MAX_GENES == SHK_FILTER_MAX_GENES, "the header states the limit");
constexpr int FILTER_LDS_KEYS = 4096;              // panels up to this many distinct keys keep their set in LDS (SHK_FILTER_LDS_KEYS) …
constexpr size_t FILTER_LDS_MAX = 128u << 10;      // … if set and bitmaps fit this much of a CU's 160 KiB
constexpr int FILTER_READ_BITS = 52;               // of a record; the gene above (12 bits)
static_assert((FILTER_MAX_GENES - 1) >> (64 - FILTER_READ_BITS) == 0, "a gene fits a record's top bits");

struct PanelSet {
  KeyRuns runs;  // canonical primer k-mer → the genes that hold it: gene ids by (key, gene), each pair once
  uint32_t n_genes;
};
// bytes of dynamic LDS: the 16 bitmaps first (both variants), then the set (k_filter_panel<true>)
__host__ __device__ inline size_t filter_bitmap_bytes(uint32_t n_genes) { return (size_t)(FILTER_WG / 64) * ((n_genes + 31) / 32) * 4; }
__host__ __device__ inline size_t filter_set_bytes(uint32_t cap, uint32_t n_pairs) { return key_runs_bytes(cap, n_pairs); }

// (the body of k_filter_panel and k_filter_panel_retained: fp_lds is the kernel's dynamic LDS)
template <bool LDS, class Reads>
__device__ __forceinline__ void filter_panel_body(uint8_t *fp_lds, const Reads &rs, uint64_t n_seqs, int k, const PanelSet &gs,
                                                  unsigned long long *__restrict__ out, uint64_t cap, unsigned long long *__restrict__ n_out) {
  const uint32_t n_words = (gs.n_genes + 31) / 32;
  uint32_t *bm_all = (uint32_t *)fp_lds;  // (16 · n_words words: a multiple of 64 bytes, so the keys behind stay aligned)
  for (uint32_t i = threadIdx.x; i < (FILTER_WG / 64) * n_words; i += FILTER_WG) bm_all[i] = 0;
  KeyRuns ks = gs.runs;
  if (LDS) ks = key_runs_to_lds(gs.runs, fp_lds + filter_bitmap_bytes(gs.n_genes), FILTER_WG);
  __syncthreads();

  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wib = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t wave = (uint64_t)blockIdx.x * (FILTER_WG / 64) + wib;
  const uint64_t n_waves = (uint64_t)gridDim.x * (FILTER_WG / 64);
  uint32_t *bm = bm_all + wib * n_words;      // this wave's bitmap: all zero between two reads
  const uint32_t km = (1u << k) - 1u;         // k ≤ 31
  const uint64_t below = (1ull << lane) - 1;  // the lanes under mine

  for (uint64_t r = wave; r < n_seqs; r += n_waves) {
    uint32_t len;
    const auto rd = rs.open(r, &len);
    if (len < (uint32_t)k) continue;  // no k-mer, valid or not: matches nothing
    const uint32_t n_win = len - (uint32_t)k + 1u;
    ReadPlanes lo = rd.planes(0, lane, len);
    bool bad = lo.bad, any = false;
    for (uint32_t s0 = 0; s0 < n_win && !bad; s0 += THREAD_TILE) {
      const ReadPlanes hi = rd.planes(s0 + THREAD_TILE, lane, len);  // the step's new bytes: the upper half of its windows' span
      if (hi.bad) {  // encoding.rs:353-356 → Err → matches() is false for every gene
        bad = true;
        break;
      }
      bool hit = false;
      uint64_t key = 0;
      if (window_key(lo, hi, lane, k, km, s0, n_win, &key)) {  // a window without an N: a k-mer
        const uint32_t s = set_find(ks.keys, ks.mask, key);
        if (s != SET_NONE) {
          hit = true;
          for (uint32_t i = ks.start[s];; ++i) {
            const uint32_t g = ks.items[i];
            atomicOr(&bm[g >> 5], 1u << (g & 31u));
            if (run_ends(ks.last, i)) break;
          }
        }
      }
      any |= __ballot(hit) != 0;
      lo = hi;
    }
    if (!any) continue;
    __threadfence_block();  // the wave reads what its other lanes set
    for (uint32_t w0 = 0; w0 < n_words; w0 += 64) {
      const uint32_t wi = w0 + lane;
      uint32_t word = wi < n_words ? bm[wi] : 0u;
      if (word) bm[wi] = 0;
      if (bad) word = 0;  // an invalid read clears and emits nothing
      for (uint64_t m = __ballot(word != 0); m; m = __ballot(word != 0)) {  // a round: every lane's lowest gene
        unsigned long long at = 0;
        if (lane == 0) at = atomicAdd(n_out, (unsigned long long)__popcll(m));
        at = __shfl(at, 0);
        if (word) {
          const uint32_t g = wi * 32u + (uint32_t)__ffs((int)word) - 1u;
          const unsigned long long i = at + (unsigned long long)__popcll(m & below);
          if (i < cap) out[i] = ((unsigned long long)g << FILTER_READ_BITS) | r;
          word &= word - 1u;
        }
      }
    }
    __threadfence_block();  // the cleared words, before the next read's hits
  }
}

template <bool LDS>
__global__ void __launch_bounds__(FILTER_WG) k_filter_panel(const uint8_t *__restrict__ bases, const uint64_t *__restrict__ offsets,
                                                            uint64_t n_seqs, int k, PanelSet gs, unsigned long long *__restrict__ out,
                                                            uint64_t cap, unsigned long long *__restrict__ n_out) {
  extern __shared__ __align__(16) uint8_t fp_lds[];
  filter_panel_body<LDS>(fp_lds, AsciiReads{bases, offsets}, n_seqs, k, gs, out, cap, n_out);
}
// … over the retained store (shk_filter_reads_panel_retained): read r is retained read r
template <bool LDS>
__global__ void __launch_bounds__(FILTER_WG) k_filter_panel_retained(PlaneReads rs, uint64_t n_seqs, int k, PanelSet gs,
                                                                     unsigned long long *__restrict__ out, uint64_t cap,
                                                                     unsigned long long *__restrict__ n_out) {
  extern __shared__ __align__(16) uint8_t fp_lds[];
  filter_panel_body<LDS>(fp_lds, rs, n_seqs, k, gs, out, cap, n_out);
}

// ==========================================================================================
// K_RETAIN: a batch of ASCII reads appended to the retained store (shk_retain_reads; layout and
// invariant in shk_retain_core.h).  The batch's first base goes to absolute bit S, wherever in a word that is.  One
// WAVE per RETAIN_WAVE_WORDS destination words (of the words the batch touches, from S / 64), its byte loads issued
// together: for word w lane l looks at source byte 64·w + l − S if that lies inside the batch, three ballots make the
// word's planes, lane 0 stores them.  The store's end word is
// shared with the batch before when S % 64 != 0: its bits from S % 64 on are zero (the invariant), the wave that owns
// it is its only writer and ORs; every other word is written whole, with zeros behind the batch's end, which keeps the
// invariant.  The read offsets follow rebased: entry i + 1 of st_offsets (the store's, from its last read's end on) =
// offsets[i + 1] − off_bias + S, held to the batch.
// ==========================================================================================
constexpr uint32_t RETAIN_WAVE_WORDS = 4;
__global__ void __launch_bounds__(WG) k_retain(const uint8_t *__restrict__ bases, uint64_t n_bases, const uint64_t *__restrict__ offsets,
                                               uint64_t n_seqs, uint64_t off_bias, uint64_t S, uint64_t n_words, uint64_t *__restrict__ p0,
                                               uint64_t *__restrict__ p1, uint64_t *__restrict__ nn, uint64_t *__restrict__ st_offsets) {
  const uint64_t t = (uint64_t)blockIdx.x * WG + threadIdx.x;
  if (t < n_seqs) {  // (offsets[0] − off_bias is the batch's first byte: the entry of the store's end stays as it is)
    const uint64_t o = offsets[t + 1] - off_bias;
    st_offsets[t + 1] = S + (o < n_bases ? o : n_bases);
  }
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t i0 = (t >> 6) * RETAIN_WAVE_WORDS;  // the wave's first word among the batch's (the same for its 64 lanes)
  if (i0 >= n_words) return;
  uint32_t c[RETAIN_WAVE_WORDS];
#pragma unroll
  for (uint32_t j = 0; j < RETAIN_WAVE_WORDS; ++j) {
    const uint64_t p = ((S >> 6) + i0 + j) * 64 + lane;  // absolute bit
    const bool in = i0 + j < n_words && p >= S && p - S < n_bases;
    c[j] = in ? bases[p - S] : (uint32_t)'A';
  }
#pragma unroll
  for (uint32_t j = 0; j < RETAIN_WAVE_WORDS; ++j) {
    const uint64_t i = i0 + j, w = (S >> 6) + i;
    if (i >= n_words) break;  // (wave-uniform)
    const bool isn = c[j] == 'N';
    const uint32_t b2 = isn ? 0u : retain_code(c[j]);
    const uint64_t w0 = __ballot(b2 & 1u), w1 = __ballot(b2 >> 1), wn = __ballot(isn);
    if (lane == 0) {
      if (i == 0 && (S & 63u)) {
        p0[w] |= w0, p1[w] |= w1, nn[w] |= wn;
      } else {
        p0[w] = w0, p1[w] = w1, nn[w] = wn;
      }
    }
  }
}

// K_RETAINED_EXPORT: the inverse — bases [B0, B0 + n) of the store back to ASCII, N where nn is set: 16 bases per
// thread and one 16-byte store, as k_unpack (out is padded to a multiple of 16 bytes).
__global__ void __launch_bounds__(WG) k_retained_export(const uint64_t *__restrict__ p0, const uint64_t *__restrict__ p1,
                                                        const uint64_t *__restrict__ nn, uint64_t B0, uint64_t n, uint8_t *__restrict__ out) {
  const uint64_t q = ((uint64_t)blockIdx.x * WG + threadIdx.x) * 16;
  if (q >= n) return;
  const uint64_t A = B0 + q, w = A >> 6;
  const uint32_t sh = (uint32_t)(A & 63u);
  const uint32_t a0 = (uint32_t)retain_window(p0[w], p0[w + 1], sh) & 0xFFFFu, a1 = (uint32_t)retain_window(p1[w], p1[w + 1], sh) & 0xFFFFu,
                 an = (uint32_t)retain_window(nn[w], nn[w + 1], sh) & 0xFFFFu;
  uint32_t o[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    o[j] = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) o[j] |= (uint32_t)retain_ascii(a0, a1, an, 4 * j + b) << (8 * b);
  }
  *reinterpret_cast<uint4 *>(out + q) = make_uint4(o[0], o[1], o[2], o[3]);
}

// K_GATHER_READS: reads ids[j] of a batch copied back to back into a batch of their own (shk_gather_reads_device):
// one wave per read, its lanes on consecutive bytes.  out_offsets is the host's prefix sum of the lengths.
__global__ void __launch_bounds__(WG) k_gather_reads(const uint8_t *__restrict__ bases, const uint64_t *__restrict__ offsets,
                                                     const uint64_t *__restrict__ ids, uint64_t n_ids,
                                                     const uint64_t *__restrict__ out_offsets, uint8_t *__restrict__ out) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t wave = (uint64_t)blockIdx.x * (WG / 64) + (threadIdx.x >> 6), n_waves = (uint64_t)gridDim.x * (WG / 64);
  for (uint64_t j = wave; j < n_ids; j += n_waves) {
    const uint64_t id = ids[j], b0 = offsets[id], len = offsets[id + 1] - b0;
    const uint8_t *src = bases + b0;
    uint8_t *dst = out + out_offsets[j];
    for (uint64_t p = lane; p < len; p += 64) dst[p] = src[p];
  }
}

// ==========================================================================================
// K_OWNER_COUNTS / K_COMPACT_OWNERS: the sender side of the multi-GPU merge.  Owner o of W owns the
// slots [o·spo, (o+1)·spo) (a contiguous page range).  Instead of shipping its range as it lies
// in the table — EMPTY slots included, ≥ half of it — a rank ships only the occupied (key, counts)
// entries: first the per-owner entry counts, then the entries, owner after owner.  The grid is
// W × blocks_per_owner; a block owns a fixed slice of one owner's range, counts it, reserves its
// share of the owner's segment with ONE atomic, and writes its entries in slot order.
// ==========================================================================================
__global__ void __launch_bounds__(WG) k_owner_counts(TableRef tb, uint64_t spo, uint32_t OWNER_BLOCKS,
                                                     unsigned long long *__restrict__ counts) {
  __shared__ uint32_t red[WG / 64];
  const uint32_t o = blockIdx.x / OWNER_BLOCKS, j = blockIdx.x % OWNER_BLOCKS;
  const uint64_t per = (spo + OWNER_BLOCKS - 1) / OWNER_BLOCKS;
  const uint64_t s0 = (uint64_t)o * spo + (uint64_t)j * per;
  const uint64_t s1 = s0 + per < (uint64_t)(o + 1) * spo ? s0 + per : (uint64_t)(o + 1) * spo;
  uint32_t n = 0;
  for (uint64_t s = s0 + threadIdx.x; s < s1; s += WG) n += tb.keys[s] != EMPTY;
  const uint32_t tot = wg_sum<WG>(n, red);
  if (threadIdx.x == 0 && tot) atomicAdd(&counts[o], (unsigned long long)tot);
}

__global__ void __launch_bounds__(WG) k_compact_owners(TableRef tb, uint64_t spo,
                                                       const unsigned long long *__restrict__ seg_offset,
                                                       unsigned long long *__restrict__ seg_cursor,
                                                       uint64_t *__restrict__ out_keys,
                                                       uint32_t *__restrict__ out_vals, uint64_t lane_stride,
                                                       uint32_t skip_owner, uint32_t OWNER_BLOCKS,
                                                       const unsigned long long *__restrict__ packed,
                                                       unsigned long long hdr_bytes, unsigned long long *__restrict__ max_count) {
  __shared__ uint32_t red[WG / 64];
  __shared__ uint32_t wbase[WG / 64];
  __shared__ unsigned long long blk_base;
  const uint32_t o = blockIdx.x / OWNER_BLOCKS, j = blockIdx.x % OWNER_BLOCKS;
  if (o == skip_owner) return;  // (a rank does not ship its own range to itself)
  const uint64_t per = (spo + OWNER_BLOCKS - 1) / OWNER_BLOCKS;
  const uint64_t s0 = (uint64_t)o * spo + (uint64_t)j * per;
  const uint64_t s1 = s0 + per < (uint64_t)(o + 1) * spo ? s0 + per : (uint64_t)(o + 1) * spo;
  uint32_t n = 0;
  for (uint64_t s = s0 + threadIdx.x; s < s1; s += WG) n += tb.keys[s] != EMPTY;
  const uint32_t tot = wg_sum<WG>(n, red);  // valid in thread 0
  if (threadIdx.x == 0) {
    const unsigned long long at0 = tot ? atomicAdd(&seg_cursor[o], (unsigned long long)tot) : 0ull;
    blk_base = seg_offset[o] + at0;
    if (max_count && tot) atomicMax(max_count, at0 + tot);  // (fixed-capacity pieces: the sender learns how many entries an owner really had)
  }
  __syncthreads();
  unsigned long long at = blk_base;
  const uint32_t wave = threadIdx.x >> 6, lane_id = threadIdx.x & 63;
  for (uint64_t sb = s0; sb < s1; sb += WG) {  // second pass: the slice is L2-resident by now
    const uint64_t s = sb + threadIdx.x;
    const uint64_t key = s < s1 ? tb.keys[s] : EMPTY;
    const unsigned long long mm = __ballot(key != EMPTY);
    if (lane_id == 0) wbase[wave] = (uint32_t)__popcll(mm);
    __syncthreads();
    uint32_t off = 0, chunk = 0;
    for (uint32_t w = 0; w < WG / 64; ++w) {
      if (w < wave) off += wbase[w];
      chunk += wbase[w];
    }
    if (key != EMPTY) {
      const unsigned long long i = at + off + __popcll(mm & ((1ull << lane_id) - 1ull));
      if (packed) {
        // PACKED: owner o's entries are one self-contained piece — [keys 8·c][lane 0 counts 4·c]…[lane L-1] at
        // byte offset seg_offset[o]·(8 + 4L), c = packed[o] — so keys and every lane's counts cross the
        // links in ONE collective; i counts from seg_offset[o]
        // (fixed-capacity pieces: hdr_bytes in front of every piece, entries beyond the capacity are not written
        // — max_count tells the receivers, who then leave ALL pieces alone: shk_compact_owners_fixed)
        const unsigned long long so = seg_offset[o], c_o = packed[o], j = i - so;
        if (j < c_o) {
          char *const seg = reinterpret_cast<char *>(out_keys) + so * (8ull + 4ull * tb.n_lanes) + (o + 1ull) * hdr_bytes;
          __builtin_memcpy(seg + j * 8ull, &key, 8);  // (4-byte aligned when L and the offset are odd)
          for (uint32_t l = 0; l < tb.n_lanes; ++l)
            *reinterpret_cast<uint32_t *>(seg + c_o * 8ull + ((unsigned long long)l * c_o + j) * 4ull) = tb.vals[(uint64_t)l * tb.cap + s];
        }
      } else {
        out_keys[i] = key;
        for (uint32_t l = 0; l < tb.n_lanes; ++l) out_vals[(uint64_t)l * lane_stride + i] = tb.vals[(uint64_t)l * tb.cap + s];
      }
    }
    at += chunk;
    __syncthreads();
  }
}

// ==========================================================================================
// K_MERGE: KmerCounts::extend across devices (counting.rs:157-166): fold a peer's page range
// (same geometry) into this table, lane by lane, saturating.
// ==========================================================================================
__global__ void __launch_bounds__(WG) k_merge(TableRef tb, uint64_t n_slots, uint64_t lane_stride,
                                              const uint64_t *__restrict__ pkeys,
                                              const uint32_t *__restrict__ pvals_,
                                              DevStats *__restrict__ stats, SpillRef sp,
                                              uint64_t piece_cap, uint32_t skip_piece) {
  if (piece_cap) {
    // Every piece's header holds how many entries its sender's fullest owner range had.  Every rank gets one
    // piece from every sender (its own included), so every rank sees the same maximum here: beyond the capacity
    // NOBODY merges anything (the tables stay as they were; the host repeats the exchange with exact counts).
    const uint64_t n_pieces = n_slots / piece_cap;
    unsigned long long most = 0;
    for (uint64_t p = 0; p < n_pieces; ++p) {
      unsigned long long h;
      __builtin_memcpy(&h, reinterpret_cast<const uint32_t *>(pkeys) + p * (2ull + piece_cap * (2ull + tb.n_lanes)), 8);
      most = h > most ? h : most;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicMax(&stats->scratch[2], most);
    if (most > piece_cap) return;
  }
  uint32_t n_new = 0;
  for (uint64_t i0 = (uint64_t)blockIdx.x * WG + threadIdx.x; i0 < n_slots;
       i0 += (uint64_t)gridDim.x * WG) {
    uint64_t i = i0, key;
    const uint32_t *pvals = pvals_;
    if (piece_cap) {
      // several self-contained pieces of piece_cap entries each ([header][k-mers][lane 0]…[lane L-1]) in one launch
      const uint64_t piece = i0 / piece_cap;
      if (piece == skip_piece) continue;
      i = i0 - piece * piece_cap;
      const uint32_t *pb = reinterpret_cast<const uint32_t *>(pkeys) + piece * (2ull + piece_cap * (2ull + tb.n_lanes)) + 2;
      __builtin_memcpy(&key, pb + 2 * i, 8);
      pvals = pb + 2 * piece_cap;
    } else {
      key = pkeys[i];
    }
    if (key == EMPTY) continue;
    const Home hm = home_of(tb, key);
    if (!hm.owned) continue;
    bool inserted = false;
    int64_t s = find_or_insert(tb.keys, hm.base, hm.slot, key, inserted);
    if (s < 0) {
      // page full: one spill record per non-zero lane
      for (uint32_t l = 0; l < tb.n_lanes; ++l) {
        uint32_t v = pvals[(uint64_t)l * lane_stride + i];
        if (!v) continue;
        unsigned long long j = atomicAdd(&stats->spill_count, 1ull);
        if (j < sp.cap) {
          sp.keys[j] = key;
          sp.lanes[j] = l;
          sp.counts[j] = v;
        }
      }
      continue;
    }
    n_new += inserted;
    for (uint32_t l = 0; l < tb.n_lanes; ++l) {
      uint32_t v = pvals[(uint64_t)l * lane_stride + i];
      if (v) sat_add_atomic(tb.vals + (uint64_t)l * tb.cap + (uint64_t)s, v);
    }
  }
  for (int off = 32; off > 0; off >>= 1) n_new += __shfl_down(n_new, off, 64);
  if ((threadIdx.x & 63) == 0 && n_new) atomicAdd(&stats->n_distinct, (unsigned long long)n_new);
}

// shk_finalize_begin: the words a reduction over the ranks sums besides the totals and the histogram.
__global__ void k_fin_extras(unsigned long long *__restrict__ extra, unsigned long long n_reads,
                             unsigned long long n_bases_read, unsigned long long user_word,
                             const DevStats *__restrict__ stats, uint32_t was_unsettled,
                             const unsigned long long *__restrict__ lane_bases, unsigned long long *__restrict__ lane_sum,
                             uint32_t n_lanes) {
  // the live per-lane base counters go into the summed block afresh on every finalize (they are never reduced in place)
  for (uint32_t l = threadIdx.x; l < n_lanes; l += blockDim.x) lane_sum[l] = lane_bases[l];
  if (threadIdx.x == 0) {
    extra[0] = n_reads;
    extra[1] = n_bases_read;
    extra[2] = (was_unsettled && (stats->spill_count || stats->bad != ~0ull)) ? 1ull : 0ull;
    extra[3] = user_word;
  }
}

__global__ void k_piece_headers(uint32_t *__restrict__ buf, uint32_t n_pieces, unsigned long long piece_ints,
                                const DevStats *__restrict__ stats) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p < n_pieces) {
    // (scratch[1]: entries of the fullest owner range.  A launch before the compaction that spilled records or
    // met an invalid byte left a table that is not what the pieces should say: nobody may merge them.)
    const unsigned long long m = (stats->spill_count || stats->bad != ~0ull) ? ~0ull : stats->scratch[1];
    __builtin_memcpy(buf + p * piece_ints, &m, 8);
  }
}

// ==========================================================================================
// K_SYNTH: synthetic reads: implicit uniform genome, fixed-length reads,
// random strand, optional substitutions and N.  Must match sharkmer_amd/synth.py bit for bit.
// ==========================================================================================
__host__ __device__ __forceinline__ uint64_t splitmix64(uint64_t x) {
  uint64_t z = x + 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

struct SynthSpec {
  uint64_t seed_genome, seed_reads, genome_len;
  uint32_t read_len, sub_per_64k, n_per_64k, pad;
};

__global__ void __launch_bounds__(WG) k_synth(SynthSpec sp, uint64_t first_read, uint64_t n_reads,
                                              uint8_t *__restrict__ bases,
                                              uint64_t *__restrict__ offsets) {
  // one thread per 8 bases: 8-byte stores, coalesced
  const uint64_t L = sp.read_len;
  const uint64_t total = n_reads * L;
  uint64_t g = ((uint64_t)blockIdx.x * WG + threadIdx.x) * 8;
  if (g <= n_reads && g + 8 > 0) {
    for (int r = 0; r < 8; ++r)
      if (g + r <= n_reads) offsets[g + r] = (g + r) * L;
  }
  if (g >= total) return;
  uint8_t out[8];
  const char LUT[4] = {'A', 'C', 'G', 'T'};
  for (int r = 0; r < 8; ++r) {
    uint64_t p = g + r;
    if (p >= total) { out[r] = 0; continue; }
    uint64_t i = first_read + p / L, j = p % L;
    uint64_t h1 = splitmix64(sp.seed_reads + 2 * i);
    uint64_t h2 = splitmix64(sp.seed_reads + 2 * i + 1);
    uint64_t start = h1 % (sp.genome_len - L + 1);
    bool rc = (h2 >> 63) != 0;
    uint64_t gp = rc ? start + (L - 1 - j) : start + j;
    uint32_t b = (uint32_t)(splitmix64(sp.seed_genome + gp) & 3);
    if (rc) b = 3 - b;
    uint8_t ch = (uint8_t)LUT[b];
    if (sp.sub_per_64k | sp.n_per_64k) {
      uint64_t e = splitmix64((sp.seed_reads ^ 0xE44044ull) + i * L + j);
      uint32_t u = (uint32_t)(e & 0xFFFF);
      if (u < sp.n_per_64k) {
        ch = 'N';
      } else if (u < sp.n_per_64k + sp.sub_per_64k) {
        uint32_t d = 1 + (uint32_t)((e >> 16) % 3);
        ch = (uint8_t)LUT[(b + d) & 3];
      }
    }
    out[r] = ch;
  }
  if (g + 8 <= total) {
    __builtin_memcpy(bases + g, out, 8);
  } else {
    for (int r = 0; r < 8 && g + r < total; ++r) bases[g + r] = out[r];
  }
}

// ==========================================================================================
// K_PRUNE: the pruning stage of sPCR between extension and threading:
// remove_low_coverage_tips (src/pcr/pruning.rs:19-149) and reachability_pruning (:170-214) for
// every gene of a panel, one workgroup per gene, blockIdx.x the gene.  Nothing is shared
// between genes and no workgroup waits for another; inside a gene the phases are separated by
// workgroup barriers only, and every loop is bounded by the gene's size.
//
// A gene is its two CSR sides as the host's counting sort made them: in_first / out_first
// (n + 1 entries), in_nbr[j] the SOURCE of the j-th edge into a node, out_nbr[j] the TARGET of
// the j-th edge out of it (parallel edges and self-loops listed severally), and one bit per
// list position, "this edge's count, as f64, is >= min_tip_count" (the only thing the tip rule
// asks of a count).  No answer depends on the order inside a node's list.
//
// Working state, 4 words per node:
//   mark     0 = alive, r = removed by tip round r.  "Alive at the start of round r" is
//            mark ∈ {0, r}: the decide phase may set r while others still read it.
//   indeg / outdeg   live edge counts (neighbors_directed(..).count()); after the tip stage the
//            same words are the two BFS queues (a node enters a queue once: n entries each)
//   fr       bits 0-1 the node's flags (1 is_start, 2 is_end), bit 2 reached forward from a
//            start, bit 3 reached backward from an end
// LDS form: CSR and state live in the workgroup's LDS (copied in first); global form: the CSR
// is read where the host put it and the state lives in the context's scratch.  Both forms are
// prune_gene over a PruneView, inlined once with LDS pointers and once with global ones.
// ==========================================================================================
constexpr int PRUNE_WG = 1024;                     // one workgroup per gene
constexpr size_t PRUNE_LDS_MAX = 79u << 10;        // two genes per CU: 2 × (79 KiB + the counters below) within 160 KiB
constexpr int PRUNE_LDS_NODES = 2560;              // default of SHK_PRUNE_LDS_NODES: 24 B per node + 8.25 B per edge ≤ PRUNE_LDS_MAX at n = e

struct PruneGene {
  uint64_t in_first, out_first, in_nbr, out_nbr, in_heavy, out_heavy, flags;  // byte offsets into the uploaded block
  uint64_t work;   // global form: first of the gene's 4 · n state words
  uint64_t keep;   // the gene's first byte of node_keep
  uint32_t n, e;
  uint32_t lds, stages;
};
struct PruneCounters { uint32_t tip_rounds, tips_removed, unreachable_removed, pad; };

__host__ __device__ inline size_t prune_lds_bytes(uint64_t n, uint64_t e) {
  return (size_t)(4 * (2 * (n + 1) + 2 * e + 2 * ((e + 31) / 32) + 4 * n));
}

struct PruneView {
  const uint32_t *in_first, *out_first, *in_nbr, *out_nbr, *in_heavy, *out_heavy;
  uint32_t *mark, *indeg, *outdeg, *fr;
};

__device__ __forceinline__ bool prune_alive(const uint32_t *mark, uint32_t v, uint32_t r) {
  const uint32_t m = mark[v];
  return m == 0 || m == r;
}

// One side of the tip rule for dead end v at the start of round r: the walk of tip_length_backward (first/nbr/heavy the
// INCOMING side, deg_same = indeg, deg_other = outdeg, stop = is_start) or of tip_length_forward (the mirror image)
// stays below k nodes, and no live edge on that side of v is heavy.
__device__ __forceinline__ bool prune_tip_side(const uint32_t *first, const uint32_t *nbr, const uint32_t *heavy, const uint32_t *mark,
                                               const uint32_t *deg_same, const uint32_t *deg_other, const uint32_t *fr, uint32_t stop,
                                               uint32_t v, uint32_t r, uint32_t k) {
  for (uint32_t j = first[v], j1 = first[v + 1]; j < j1; ++j)
    if (((heavy[j >> 5] >> (j & 31)) & 1u) && prune_alive(mark, nbr[j], r)) return false;
  uint32_t cur = v;
  for (uint32_t len = 1;; ++len) {  // (at most k turns)
    if (len >= k) return false;
    if (deg_same[cur] != 1) return true;
    uint32_t next = ~0u;
    for (uint32_t j = first[cur], j1 = first[cur + 1]; j < j1; ++j)
      if (prune_alive(mark, nbr[j], r)) {
        next = nbr[j];
        break;
      }
    if (next == ~0u || deg_other[next] > 1 || (fr[next] & stop)) return true;
    cur = next;
  }
}

__device__ __forceinline__ void prune_gene(const PruneView &g, uint32_t n, uint32_t stages, uint32_t k, uint8_t *__restrict__ keep,
                                           PruneCounters *__restrict__ out) {
  __shared__ uint32_t s_cnt[2], s_fn[3], s_bn[3], s_kept, s_live;
  const uint32_t tid = threadIdx.x;
  if (tid == 0) {
    s_cnt[0] = s_cnt[1] = 0;
    s_fn[0] = s_fn[1] = s_fn[2] = s_bn[0] = s_bn[1] = s_bn[2] = 0;
    s_kept = s_live = 0;
  }
  for (uint32_t v = tid; v < n; v += PRUNE_WG) {
    g.mark[v] = 0;
    g.indeg[v] = g.in_first[v + 1] - g.in_first[v];
    g.outdeg[v] = g.out_first[v + 1] - g.out_first[v];
  }
  __syncthreads();
  uint32_t rounds = 0, removed = 0;
  if (stages & 1u) {
    // a round that goes on removes a node: at most n of them, and one more that finds nothing
    for (uint64_t r64 = 1; r64 <= (uint64_t)n + 1; ++r64) {
      const uint32_t r = (uint32_t)r64;
      // decide, on the graph as the round found it
      for (uint32_t v = tid; v < n; v += PRUNE_WG) {
        if (g.mark[v] != 0 || (g.fr[v] & 3u)) continue;
        const uint32_t od = g.outdeg[v], id = g.indeg[v];
        if (od && id) continue;
        bool rm = true;
        if (od == 0) rm = prune_tip_side(g.in_first, g.in_nbr, g.in_heavy, g.mark, g.indeg, g.outdeg, g.fr, 1u, v, r, k);
        if (rm && id == 0) rm = prune_tip_side(g.out_first, g.out_nbr, g.out_heavy, g.mark, g.outdeg, g.indeg, g.fr, 2u, v, r, k);
        if (rm) {
          g.mark[v] = r;
          atomicAdd(&s_cnt[r & 1u], 1u);
        }
      }
      __syncthreads();
      const uint32_t n_rm = s_cnt[r & 1u];
      if (n_rm == 0) break;  // (the same for every thread)
      rounds += 1;
      removed += n_rm;
      if (tid == 0) s_cnt[(r + 1) & 1u] = 0;  // (last read behind the previous round's decide barrier)
      // apply: the marked nodes leave with their edges
      for (uint32_t v = tid; v < n; v += PRUNE_WG) {
        if (g.mark[v] != r) continue;
        for (uint32_t j = g.out_first[v], j1 = g.out_first[v + 1]; j < j1; ++j)
          if (prune_alive(g.mark, g.out_nbr[j], r)) atomicSub(&g.indeg[g.out_nbr[j]], 1u);
        for (uint32_t j = g.in_first[v], j1 = g.in_first[v + 1]; j < j1; ++j)
          if (prune_alive(g.mark, g.in_nbr[j], r)) atomicSub(&g.outdeg[g.in_nbr[j]], 1u);
      }
      __syncthreads();
    }
  }
  if (stages & 2u) {
    // both searches in one level loop; level L counts its new entries in s_fn / s_bn[L % 3] and clears the pair of
    // level L + 1, which was last read behind the barrier of level L − 2
    uint32_t *fq = g.indeg, *bq = g.outdeg;
    __syncthreads();  // (a round that broke off: everyone is past its reads of the degrees)
    for (uint32_t v = tid; v < n; v += PRUNE_WG) {
      if (g.mark[v] != 0) continue;
      const uint32_t f = g.fr[v];
      if (f & 1u) {
        g.fr[v] = f | (f & 2u ? 12u : 4u);
        fq[atomicAdd(&s_fn[0], 1u)] = v;
      }
      if (f & 2u) {
        if (!(f & 1u)) g.fr[v] = f | 8u;
        bq[atomicAdd(&s_bn[0], 1u)] = v;
      }
    }
    __syncthreads();
    uint32_t fh = 0, ft = s_fn[0], bh = 0, bt = s_bn[0];
    // a level that goes on enters a node into a queue: at most 2n of them
    for (uint64_t lvl = 1; lvl <= 2 * (uint64_t)n + 1; ++lvl) {
      const uint64_t nf = ft - fh, nb = bt - bh;
      if (nf + nb == 0) break;  // (the same for every thread)
      const uint32_t c = (uint32_t)(lvl % 3), cz = (uint32_t)((lvl + 1) % 3);
      if (tid == 0) s_fn[cz] = s_bn[cz] = 0;
      for (uint64_t i = tid; i < nf + nb; i += PRUNE_WG) {
        if (i < nf) {
          const uint32_t v = fq[fh + (uint32_t)i];
          for (uint32_t j = g.out_first[v], j1 = g.out_first[v + 1]; j < j1; ++j) {
            const uint32_t u = g.out_nbr[j];
            if (g.mark[u] == 0 && !(atomicOr(&g.fr[u], 4u) & 4u)) fq[ft + atomicAdd(&s_fn[c], 1u)] = u;
          }
        } else {
          const uint32_t v = bq[bh + (uint32_t)(i - nf)];
          for (uint32_t j = g.in_first[v], j1 = g.in_first[v + 1]; j < j1; ++j) {
            const uint32_t u = g.in_nbr[j];
            if (g.mark[u] == 0 && !(atomicOr(&g.fr[u], 8u) & 8u)) bq[bt + atomicAdd(&s_bn[c], 1u)] = u;
          }
        }
      }
      __syncthreads();
      fh = ft, ft += s_fn[c];
      bh = bt, bt += s_bn[c];
    }
  }
  uint32_t kept = 0, live = 0;
  for (uint32_t v = tid; v < n; v += PRUNE_WG) {
    const bool alive = g.mark[v] == 0;
    const bool kp = alive && (!(stages & 2u) || (g.fr[v] & 12u) == 12u);
    keep[v] = kp ? 1 : 0;
    kept += kp, live += alive;
  }
  if (kept) atomicAdd(&s_kept, kept);
  if (live) atomicAdd(&s_live, live);
  __syncthreads();
  if (tid == 0) *out = PruneCounters{rounds, removed, s_live - s_kept, 0};
}

__global__ void __launch_bounds__(PRUNE_WG) k_prune_panel(const PruneGene *__restrict__ genes, const uint8_t *__restrict__ up,
                                                          uint32_t *__restrict__ work, uint8_t *__restrict__ keep,
                                                          PruneCounters *__restrict__ counters, uint32_t k) {
  extern __shared__ uint32_t s_prune[];
  const PruneGene d = genes[blockIdx.x];
  const uint32_t n = d.n, e = d.e, tid = threadIdx.x;
  PruneCounters *out = counters + blockIdx.x;
  if (n == 0) {  // (the same for every thread)
    if (tid == 0) *out = PruneCounters{0, 0, 0, 0};
    return;
  }
  const uint32_t *in_first = (const uint32_t *)(up + d.in_first), *out_first = (const uint32_t *)(up + d.out_first);
  const uint32_t *in_nbr = (const uint32_t *)(up + d.in_nbr), *out_nbr = (const uint32_t *)(up + d.out_nbr);
  const uint32_t *in_heavy = (const uint32_t *)(up + d.in_heavy), *out_heavy = (const uint32_t *)(up + d.out_heavy);
  const uint8_t *flags = up + d.flags;
  const uint32_t hw = (e + 31) / 32;
  if (d.lds) {
    // prune_lds_bytes' layout: in_first, out_first, in_nbr, out_nbr, in_heavy, out_heavy, mark, indeg, outdeg, fr
    uint32_t *l_in_first = s_prune, *l_out_first = l_in_first + (n + 1), *l_in_nbr = l_out_first + (n + 1), *l_out_nbr = l_in_nbr + e;
    uint32_t *l_in_heavy = l_out_nbr + e, *l_out_heavy = l_in_heavy + hw, *l_mark = l_out_heavy + hw, *l_indeg = l_mark + n;
    uint32_t *l_outdeg = l_indeg + n, *l_fr = l_outdeg + n;
    for (uint32_t i = tid; i <= n; i += PRUNE_WG) l_in_first[i] = in_first[i], l_out_first[i] = out_first[i];
    for (uint32_t i = tid; i < e; i += PRUNE_WG) l_in_nbr[i] = in_nbr[i], l_out_nbr[i] = out_nbr[i];
    for (uint32_t i = tid; i < hw; i += PRUNE_WG) l_in_heavy[i] = in_heavy[i], l_out_heavy[i] = out_heavy[i];
    for (uint32_t i = tid; i < n; i += PRUNE_WG) l_fr[i] = flags[i] & 3u;
    __syncthreads();
    prune_gene(PruneView{l_in_first, l_out_first, l_in_nbr, l_out_nbr, l_in_heavy, l_out_heavy, l_mark, l_indeg, l_outdeg, l_fr}, n, d.stages, k,
               keep + d.keep, out);
  } else {
    uint32_t *w = work + d.work;
    for (uint32_t i = tid; i < n; i += PRUNE_WG) w[3 * (uint64_t)n + i] = flags[i] & 3u;
    prune_gene(PruneView{in_first, out_first, in_nbr, out_nbr, in_heavy, out_heavy, w, w + n, w + 2 * (uint64_t)n, w + 3 * (uint64_t)n}, n, d.stages,
               k, keep + d.keep, out);
  }
}

}  // namespace shk

// ##########################################################################################
// Paged path: the table is a sequence of PAGE_SLOTS-slot pages, each an independent
// open-addressing table that fits in LDS (64 KiB keys + 32 KiB counts).  One counting pass =
//   K_SCATTER  k_part_scatter_sorted  validate + extract k-mers tile by tile, counting-sort each
//                                     tile by page in LDS, append every page's run to that page's
//                                     region of part_buf (reserved with one returning atomic per
//                                     (tile, page)) as aligned 16-B record pairs
//   K_PAGES    k_pages                one workgroup per page: page → LDS, stream the page's
//                                     region through LDS atomics, page → HBM
// HBM traffic per k-mer occurrence: 8 B written + 8 B read, all of it streaming; the table
// is read and written once per pass.  counting.rs:82-85 semantics, exact incl. saturation.
// ##########################################################################################
namespace shk {

constexpr int MAX_PARTS = 4096;   // partitions one LDS sort fans out to; more pages ⇒ two levels
constexpr int PG_WG = 512;        // k_pages workgroup: 8 waves; two workgroups (80 KiB LDS each) per CU
constexpr uint32_t PAGE_FILL_CAP = PAGE_SLOTS - PAGE_SLOTS / 8;  // new keys spill beyond this

// ------------------------------------------------------------------------------------------
// k_part_scatter_sorted: the same job as k_part_scatter, but every tile is counting-sorted by
// partition in LDS first, so that a partition's k-mers leave the CU as runs of consecutive
// 8-B records (coalesced 64..512-B requests) instead of one 8-B request per k-mer.
// Measured on MI355X (tools/wbench.hip): 8-B scattered stores 0.6 TB/s, 64-B chunks 3.2 TB/s,
// ≥128-B chunks 4.9 TB/s.
//   walk    : rolling extraction; per k-mer a returning LDS add gives its rank inside its
//             partition; (partition, rank) stays in a register
//   scan    : exclusive scan of the tile's partition counts
//   place   : sorted[tstart[p] + rank] = end position (u16), aliasing the dead code bytes
//   write   : entry i → k-mer re-read from the 2-bit packed copy of the tile → its place in
//             the partition's output run
// ------------------------------------------------------------------------------------------
#ifndef SORTED_WAVES_PER_SIMD
#define SORTED_WAVES_PER_SIMD 4
#endif
// LDS bytes of the sorted-entry region: TILE_T entries + one possible pad per page (u16), and it
// doubles as the staging area (code bytes + group masks) before the sort
__host__ __device__ inline uint32_t sort_region_bytes(uint32_t P) {
  uint32_t a = 2u * ((uint32_t)TILE_T + P), b = (uint32_t)STAGE_BYTES;
  return ((a > b ? a : b) + 15u) & ~15u;
}

// Inclusive prefix sum over the 64 lanes of a wave with DPP row shifts / broadcasts (VALU only;
// the __shfl_up formulation costs six ds_bpermute round trips).
__device__ __forceinline__ uint32_t wave_scan_incl(uint32_t v) {
  // within each row of 16 lanes: shifts by 1, 2, 4, 8 (bound_ctrl: lanes shifted in read 0)
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xF, 0xF, true);  // row_shr:1
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xF, 0xF, true);  // row_shr:2
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xF, 0xF, true);  // row_shr:4
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xF, 0xF, true);  // row_shr:8
  // across rows: lane 15 of a row into the next row (rows 1 and 3), then lane 31 into rows 2 and 3
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xA, 0xF, false);  // row_bcast:15
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xC, 0xF, false);  // row_bcast:31
  return v;
}

// the k-base window that starts at base index q of an MSB-first packed stream
__device__ __forceinline__ uint64_t window_at(const uint32_t *stream, int q, int k) {
  const int s = 2 * q;
  const int wi = s >> 5;
  const uint32_t off = (uint32_t)s & 31u;
  // 64 stream bits from bit s on, as two funnel shifts (v_alignbit_b32 shifts by its count mod 32,
  // hence the selects for off = 0); the third word is a pad word at worst, never out of bounds
  const uint32_t w0 = stream[wi], w1 = stream[wi + 1], w2 = stream[wi + 2];
  const uint32_t hi = off ? __builtin_amdgcn_alignbit(w0, w1, 32u - off) : w0;
  const uint32_t lo = off ? __builtin_amdgcn_alignbit(w1, w2, 32u - off) : w1;
  return (((uint64_t)hi << 32) | lo) >> (64 - 2 * k);
}
// Canonical k-mer whose LAST base sits at LDS position j (halo included).  The walk has already
// decided the strand: rc = 1 ⇔ the reverse complement is the smaller one, and that is a plain
// window of the mirrored complement stream (base j of the tile is its base TILE_LDS-1-j).
__device__ __forceinline__ uint64_t kmer_at(const uint32_t *packed, const uint32_t *rcpacked, int j,
                                            uint32_t rc, int k) {
  return window_at(rc ? rcpacked : packed, rc ? TILE_LDS - 1 - j : j - k + 1, k);  // one window read, no branch
}

// Layout of the 4-byte-record buffers: BLOCK-INTERLEAVED.  Record j of region r (a page, or a
// super-page at level 1) lives at
//     ((j >> RB_LOG) · n_regions + r) << RB_LOG  |  (j & (2^RB_LOG - 1))
// i.e. the regions' 4-KiB blocks alternate.  All regions fill at nearly the same rate (the hash
// spreads k-mers evenly), so the write fronts of all ≤ 4096 regions stay within a few MiB of one
// another instead of one per region-sized stride, and the scatter's stores — every store
// instruction touches a dozen regions — keep hitting the same few address translations.
constexpr uint32_t RB_LOG = 10;  // records per block: 4 KiB
__device__ __forceinline__ uint32_t rec_slot(uint32_t region, uint32_t n_regions, uint32_t j) {
  return (((j >> RB_LOG) * n_regions + region) << RB_LOG) | (j & ((1u << RB_LOG) - 1u));
}
__device__ __forceinline__ uint64_t rec_slot64(uint64_t region, uint64_t n_regions, uint32_t j) {
  return ((((uint64_t)(j >> RB_LOG)) * n_regions + region) << RB_LOG) | (j & ((1u << RB_LOG) - 1u));
}

// REC32: the 4-byte-record variant (one level, 2k - log_parts ≤ 32): a record is the low
// 2k - log_parts bits of the MIXED key (the page is implied by the region, mix_key is a bijection),
// runs are packed without padding, one 4-B store per record.
template <int NT, bool REC32>
__global__ void __launch_bounds__(NT, SORTED_WAVES_PER_SIMD) k_part_scatter_sorted(
    BatchRef b, uint32_t log_parts, uint32_t lane_filter, unsigned int *__restrict__ cursor,
    uint32_t cap_p, void *__restrict__ part_buf_, DevStats *__restrict__ stats,
    unsigned long long *__restrict__ lane_bases, SpillRef sp, unsigned long long *__restrict__ dbg) {
  extern __shared__ __attribute__((aligned(16))) uint32_t sh[];
  __shared__ uint32_t wsum[NT / 64];
  __shared__ uint32_t red[NT / 64];
  constexpr int SPAN = TILE_T / NT;
  const uint32_t P = 1u << log_parts;
  const uint32_t sort_bytes = sort_region_bytes(P);
  uint8_t *codes = reinterpret_cast<uint8_t *>(sh);                 // STAGE_BYTES ≤ sort_bytes
  uint16_t *sorted = reinterpret_cast<uint16_t *>(sh);              // TILE_T + P entries; aliases codes
  uint32_t *packed = sh + sort_bytes / 4;                           // PACK_WORDS
  uint32_t *rcpacked = packed + PACK_WORDS;                         // PACK_WORDS: mirrored complement
  uint32_t *cnt = rcpacked + PACK_WORDS;                            // P
  uint32_t *tstart = cnt + P;                                       // P
  uint32_t *gbase = tstart + P;                                     // P: this tile's reservation per page
#ifdef SHK_PHASE_TIMING
  unsigned long long ph[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  unsigned long long tprev = 0;
#define STAMP(i)                                        \
  do {                                                  \
    unsigned long long tn = __builtin_readcyclecounter(); \
    ph[i] += tn - tprev;                                \
    tprev = tn;                                         \
  } while (0)
#else
#define STAMP(i)
#endif
  // This kernel is also the validation pass (encoding.rs:353-356) and the non-N base count
  // (chunk.rs:28): both ride on the staging loads.  An invalid byte found by ANY workgroup
  // keeps k_pages from running (it tests stats->bad), so the table stays untouched.
  uint32_t n_non_n = 0;
  const int k = b.k;
  const uint64_t mask = (1ull << (2 * k)) - 1;
  const uint32_t mask_lo = (uint32_t)mask, mask_hi = (uint32_t)(mask >> 32);
  const uint32_t per = P / NT ? P / NT : 1;  // partitions per thread in the scan (P ≥ WG or P < WG)
  uint64_t *part_buf = reinterpret_cast<uint64_t *>(part_buf_);
  uint32_t *part_buf32 = reinterpret_cast<uint32_t *>(part_buf_);
  const uint32_t pad1 = REC32 ? 0u : 1u;  // runs are padded to even length unless REC32

  uint64_t t = blockIdx.x, t0, t1;
  uint32_t lane;
  bool have = next_tile(b, t, true, lane_filter, t0, t1, lane);
  StageRegs<NT> pre;
  if (have) stage_prefetch<NT>(b, t0, pre);
  while (have) {
    __syncthreads();  // previous tile's write phase is done with sorted/cnt/tstart
#ifdef SHK_PHASE_TIMING
    tprev = __builtin_readcyclecounter();
#endif
    for (uint32_t i = threadIdx.x; i < P; i += NT) cnt[i] = 0;
    n_non_n += stage_tile<true, NT, true>(b, t0, t1, codes, stats, pre, packed, rcpacked);
    uint64_t tn = t + gridDim.x, n0, n1;
    uint32_t nl;
    const bool hn = next_tile(b, tn, true, lane_filter, n0, n1, nl);
    if (hn) stage_prefetch<NT>(b, n0, pre);  // in flight during the rest of this tile
    __syncthreads();
    STAMP(0);
    STAMP(1);
    // ---- walk: (partition, rank) per end position, kept in registers -------------------
    uint32_t pr[SPAN];
    {
      const int e0 = threadIdx.x * SPAN;
      const int n_end = (int)(t1 - t0);
      const int jemit = HALO + e0;
      const int jend = HALO + (e0 + SPAN < n_end ? e0 + SPAN : n_end);
      Roll x{0, 0, 0, 0};
      if (e0 < n_end) {
        // the frames as they stand just before the first end position: the k bases up to
        // jemit-1, read as one window of either packed stream (N / foreign bases pack as A; the
        // "k-mer ends here" bits keep windows that contain them from being emitted)
        const uint64_t f0 = window_at(packed, jemit - k, k);
        const uint64_t r0 = window_at(rcpacked, TILE_LDS - jemit, k) << (64 - 2 * k);
        x.f_lo = (uint32_t)f0;
        x.f_hi = (uint32_t)(f0 >> 32);
        x.r_lo = (uint32_t)r0;
        x.r_hi = (uint32_t)(r0 >> 32);
      }
#pragma unroll
      for (int q = 0; q < SPAN / 8; ++q) {
        uint64_t w = 0;
        if (jemit + q * 8 < jend) w = *reinterpret_cast<const uint64_t *>(codes + jemit + q * 8);
#pragma unroll
        for (int r = 0; r < 8; ++r) {
          uint32_t c = (uint32_t)(w >> (8 * r)) & 0xFF;
          roll_step(x, c & 3u, mask_lo, mask_hi);
          uint32_t v = 0xFFFFFFFFu;
          if (c & 4u) {  // (never set at or beyond the tile's end: stage_tile)
            const uint64_t fwd = ((uint64_t)x.f_hi << 32) | x.f_lo;
            const uint64_t rev = (((uint64_t)x.r_hi << 32) | x.r_lo) >> (64 - 2 * k);
            const bool rc = rev < fwd;
            const uint32_t pc = (uint32_t)page_of(hash64(rc ? rev : fwd, 2 * k), log_parts);
            v = (pc << 16) | (rc ? 0x8000u : 0u) | atomicAdd(&cnt[pc], 1u);  // rank < 2^14
          }
          pr[q * 8 + r] = v;
        }
      }
    }
    __syncthreads();
    STAMP(2);
    // ---- exclusive scan of the even-padded counts → tstart (every run starts on a pair) ------
    {
      uint32_t lo = threadIdx.x * per, s = 0;
      if (lo < P)
        for (uint32_t i = 0; i < per; ++i) s += (cnt[lo + i] + pad1) & ~pad1;
      const uint32_t inc = wave_scan_incl(s);
      if ((threadIdx.x & 63) == 63) wsum[threadIdx.x >> 6] = inc;
      __syncthreads();
      const uint32_t wv = threadIdx.x >> 6, ln = threadIdx.x & 63;
      const uint32_t part = (ln < wv && ln < (uint32_t)(NT / 64)) ? wsum[ln] : 0u;
      const uint32_t woff = (uint32_t)__builtin_amdgcn_readlane((int)wave_scan_incl(part), 63);
      uint32_t run = woff + inc - s;
      if (lo < P)
        for (uint32_t i = 0; i < per; ++i) {
          tstart[lo + i] = run;
          run += (cnt[lo + i] + pad1) & ~pad1;
        }
    }
    // reserve this tile's (even-padded) run in every page's output region: one returning
    // device-scope add per non-empty (tile, page); consecutive lanes hit consecutive cursors.
    // The results are first needed by the write phase, a barrier and the place phase later, so
    // they are parked in registers and only stored to LDS (where the wait for them sits) then.
    uint32_t gres[MAX_PARTS / NT];  // stay in registers until the place phase is over
#pragma unroll
    for (int r = 0; r < MAX_PARTS / NT; ++r) {
      const uint32_t i = threadIdx.x + r * NT;
      gres[r] = 0;
      if (i < P) {
        const uint32_t c2 = (cnt[i] + pad1) & ~pad1;
        if (c2) gres[r] = atomicAdd(&cursor[i], c2);
      }
    }
    __syncthreads();  // codes are dead from here: `sorted` may overwrite them
    STAMP(3);
    // ---- place (the odd runs' padding slot gets the sentinel 0xFFFF) ---------------------------
#pragma unroll
    for (int i = 0; i < SPAN; ++i) {
      uint32_t v = pr[i];
      if (v != 0xFFFFFFFFu)  // entry = end position | strand << 14
        sorted[tstart[v >> 16] + (v & 0x7FFFu)] = (uint16_t)((threadIdx.x * SPAN + i) | ((v & 0x8000u) >> 1));
    }
    if (!REC32)
      for (uint32_t i = threadIdx.x; i < P; i += NT)
        if (cnt[i] & 1u) sorted[tstart[i] + cnt[i]] = 0xFFFFu;
#pragma unroll
    for (int r = 0; r < MAX_PARTS / NT; ++r)  // the reservations have had the place phase to come back
      if (threadIdx.x + r * NT < P)  // gbase - tstart: what the write phase adds to an entry's index
        gbase[threadIdx.x + r * NT] = gres[r] - tstart[threadIdx.x + r * NT];
    __syncthreads();
    STAMP(4);
    // ---- write: one PAIR of records per lane per store (16 B, aligned: runs start on even
    // record indices in LDS and in HBM); pairs never straddle partitions ----------------------
    if (REC32) {
      const uint32_t n_rec = tstart[P - 1] + cnt[P - 1];
      const uint32_t rbits = 2u * (uint32_t)k - log_parts;  // ≤ 32
      // two consecutive entries per lane: they nearly always belong to the same page, and then
      // leave as one 8-B store (4-B aligned is enough for global memory)
      const uint32_t *sorted2r = reinterpret_cast<const uint32_t *>(sorted);
      const uint32_t rmask = (uint32_t)(0xFFFFFFFFull >> (32 - rbits));
      auto spill_km = [&](uint64_t km) {  // the page's region is full (skewed input)
        const unsigned long long j = atomicAdd(&stats->spill_count, 1ull);
        if (j < sp.cap) {
          sp.keys[j] = km;
          sp.lanes[j] = lane;
          sp.counts[j] = 1u;
        }
      };
      for (uint32_t i = threadIdx.x; 2 * i < n_rec; i += NT) {
        const uint32_t ee = sorted2r[i];
        const uint32_t ea = ee & 0xFFFFu, eb = ee >> 16;
        const bool two = 2 * i + 1 < n_rec;
        const uint64_t km0 = kmer_at(packed, rcpacked, HALO + (int)(ea & 0x3FFFu), ea >> 14, k);
        const uint64_t km1 = two ? kmer_at(packed, rcpacked, HALO + (int)(eb & 0x3FFFu), (eb >> 14) & 1u, k) : km0;
        const uint64_t y0 = mix_key(km0, 2 * k), y1 = mix_key(km1, 2 * k);
        const uint32_t pc0 = (uint32_t)(y0 >> rbits), pc1 = (uint32_t)(y1 >> rbits);  // = page_of(hash64(km))
        const uint32_t r0 = (uint32_t)y0 & rmask, r1 = (uint32_t)y1 & rmask;
        const uint32_t at0 = gbase[pc0] + 2 * i;  // record index inside the page's region
        // (a launch covers ≤ 2^28 k-mers: byte offsets into part_buf fit 32 bits)
        char *const base = reinterpret_cast<char *>(part_buf32);
        if (two && pc1 == pc0 && at0 + 2 <= cap_p && (at0 & ((1u << RB_LOG) - 1u)) != (1u << RB_LOG) - 1u) {
          uint2 rec2 = make_uint2(r0, r1);  // (both records in one block)
          __builtin_memcpy(base + rec_slot(pc0, P, at0) * 4u, &rec2, 8);
        } else {
          if (at0 < cap_p) *reinterpret_cast<uint32_t *>(base + rec_slot(pc0, P, at0) * 4u) = r0;
          else spill_km(km0);
          if (two) {
            const uint32_t at1 = gbase[pc1] + 2 * i + 1;
            if (at1 < cap_p) *reinterpret_cast<uint32_t *>(base + rec_slot(pc1, P, at1) * 4u) = r1;
            else spill_km(km1);
          }
        }
      }
    }
    const uint32_t n_pairs = REC32 ? 0u : (tstart[P - 1] + ((cnt[P - 1] + 1u) & ~1u)) >> 1;
    const uint32_t *sorted2 = reinterpret_cast<const uint32_t *>(sorted);
    for (uint32_t i = threadIdx.x; i < n_pairs; i += NT) {
      const uint32_t ee = sorted2[i];
      const uint32_t e0 = ee & 0xFFFFu, e1 = ee >> 16;
      const uint64_t km0 = kmer_at(packed, rcpacked, HALO + (int)(e0 & 0x3FFFu), e0 >> 14, k);
      const uint64_t km1 =
          e1 == 0xFFFFu ? EMPTY : kmer_at(packed, rcpacked, HALO + (int)(e1 & 0x3FFFu), e1 >> 14, k);
      const uint32_t pc = (uint32_t)page_of(hash64(km0, 2 * k), log_parts);
      const uint32_t at = gbase[pc] + 2 * i;  // record index inside page pc's region
      if (at + 2 <= cap_p) {
        ulonglong2 rec;
        rec.x = km0;
        rec.y = km1;
        const uint32_t byte_off = (pc * cap_p + at) * 8u;  // < 2^32: ≤ 2^28 k-mers per launch
        *reinterpret_cast<ulonglong2 *>(reinterpret_cast<char *>(part_buf) + byte_off) = rec;
      } else {  // the page's region is full (skewed input): these records take the spill path
        const unsigned long long j = atomicAdd(&stats->spill_count, km1 == EMPTY ? 1ull : 2ull);
        if (j < sp.cap) {
          sp.keys[j] = km0;
          sp.lanes[j] = lane;
          sp.counts[j] = 1u;
        }
        if (km1 != EMPTY && j + 1 < sp.cap) {
          sp.keys[j + 1] = km1;
          sp.lanes[j + 1] = lane;
          sp.counts[j + 1] = 1u;
        }
      }
    }
    __syncthreads();
    STAMP(5);
    t = tn;
    t0 = n0;
    t1 = n1;
    lane = nl;
    have = hn;
  }
  __syncthreads();
  {
    uint32_t tot = wg_sum<NT>(n_non_n, red);
    if (threadIdx.x == 0 && tot) atomicAdd(&lane_bases[lane_filter], (unsigned long long)tot);
  }
#ifdef SHK_PHASE_TIMING
  if (dbg && threadIdx.x == 0)
    for (int i = 0; i < 8; ++i) dbg[(uint64_t)blockIdx.x * 8 + i] = ph[i];
#endif
}

// ------------------------------------------------------------------------------------------
// k_scatter32: the 4-byte-record scatter with the records kept in LDS.  Same job and same output
// as k_part_scatter_sorted<.., true>, but a (macro) tile is processed as TILE_T/TT sub-tiles of
// TT end positions, small enough that the RECORD of every k-mer (32 bits) stays in LDS from the
// walk to the write-out:
//   walk   : rolling extraction → mix_key → page (top bits) and record (low bits); the record goes
//            to recs[], (page, rank) stays in a register
//   scan, reserve : as before
//   place  : sorted[tstart[page] + rank] = page << 14 | index into recs    (32-bit entries)
//   write  : entry → record from recs[], page from the entry: no k-mer is rebuilt, nothing is
//            hashed a second time; two entries per lane, one 8-B store when they share a page
// LDS: 4·TT (entries; aliases the staged code bytes) + 4·TT (records) + one packed stream
// (walk warm-up) + 12·P.
// ------------------------------------------------------------------------------------------
// place phase of k_scatter32.  The __restrict__ parameters are the point: `sorted` and `tstart`
// are carved out of the same LDS block, and without the promise that they do not overlap every
// tstart read has to wait behind the previous entry's write (one LDS round trip per entry).
template <int NT, int SPAN>
__device__ __forceinline__ void place_entries(uint32_t *__restrict__ sorted, const uint32_t *__restrict__ tstart,
                                              const uint32_t (&pr)[SPAN], uint32_t P) {
  const char *const ts_b = reinterpret_cast<const char *>(tstart);
#pragma unroll
  for (int i = 0; i < SPAN; ++i) {
    const uint32_t v = pr[i];  // partition · 2^18 | rank; partitions ≥ P are the walk's spare counters (no record)
    // (v >> 16 = partition · 4: tstart's byte offset; the entry keeps the partition field and gets the record's byte offset)
    if (v < (P << 18))
      sorted[*reinterpret_cast<const uint32_t *>(ts_b + (v >> 16)) + (v & 0x3FFFFu)] = (v & 0xFFFC0000u) | ((i * NT + threadIdx.x) << 2);
  }
}

// LOGP: the fan-out as a compile-time constant (0 = log_parts_ at run time).  1024 partitions — one per
// thread — is what every table from 8 M slots up gets (one level up to 4096 pages aside), so the
// scan, reserve and place phases are specialised for it.
// ALL: ALL-LANES mode (lane_filter = ~0) as a compile-time constant: with one lane and LOGP the number
// of regions is an immediate and rec_slot a shift and an or.
// OWN (with ALL): the OWNER layout of key-space-partitioned ingest.  The fan-out 2^log_parts covers the
// virtual global table: the top log_w bits of a partition index are the record's OWNER, the rest its
// super-page inside the owner's share.  Regions and cursors are ordered [owner][lane][super-page], every
// owner's regions block-interleave among themselves only, so that what one owner gets — its seg_recs
// records' worth of regions and their cursor words — is ONE contiguous piece of each array (what crosses
// the link in a multi-GPU run).  keep = an owner id: records of every other owner are dropped in the walk
// and there is a single segment (seg_recs = 0); keep = ~0: all owners' records are kept.
// Cursor SEGMENTS (without OWN; own.segs = S): a partition's region is S segments, each with its own cursor word and
// its own capacity cap_p — segment s of partition p of lane l is region (l·S + s)·P + p of lanes·S·P block-interleaved
// regions, its cursor word at the same index.  A workgroup reserves in segment blockIdx.x % S for its whole life, so
// the cursor lines the workgroups meet on are S × 64 instead of 64; k_pages32 reads a lane's S segments in turn.
constexpr uint32_t SC32_MAX_LANES = 128;  // chunk lanes one all-lanes pass of k_scatter32 takes (its per-lane base counts: 1 KiB of static LDS)
struct OwnerCfg {
  uint32_t log_w;     // owner bits (≤ log_parts)
  uint32_t keep;      // owner id to keep, or ~0 = all
  uint32_t seg_recs;  // records per owner segment (0: one segment only)
  uint32_t segs;      // without OWN: cursor segments per region (a power of two; 0 = 1), see k_scatter32
};
template <int NT, int TT, bool WIDE, int LOGP = 0, bool ALL = false, bool OWN = false>
__global__ void __launch_bounds__(NT, 4) k_scatter32(
    BatchRef b, uint32_t log_parts_, uint32_t lane_filter, unsigned int *__restrict__ cursor,
    uint32_t cap_p, uint32_t *__restrict__ part_buf32, DevStats *__restrict__ stats,
    unsigned long long *__restrict__ lane_bases, SpillRef sp, unsigned long long *__restrict__ dbg,
    uint32_t n_region_lanes, OwnerCfg own) {
  static_assert(!OWN || (ALL && !WIDE), "the owner layout is an all-lanes, per-launch layout");
  extern __shared__ __attribute__((aligned(16))) uint32_t sh[];
  __shared__ uint32_t wsum[NT / 64];
  __shared__ uint32_t red[NT / 64];
  __shared__ unsigned long long lane_nn[SC32_MAX_LANES];  // ALL-LANES mode: non-N bases per chunk lane
  // lane_filter = ~0: ALL-LANES mode — one pass over the tiles of every chunk lane; region and cursor
  // index = lane · P + page (n_region_lanes · P regions, block-interleaved together)
  constexpr bool all_lanes = ALL;  // (the host picks the variant from lane_filter == ~0)
  if (all_lanes && threadIdx.x < SC32_MAX_LANES) lane_nn[threadIdx.x] = 0;
  static_assert(TILE_T % TT == 0 && TT % (8 * NT) == 0 && 4 * TT >= TT + HALO + 4 * ((TT + HALO) / 16), "tile shape");
  constexpr int SPAN = TT / NT;
  constexpr int GROUPS = (TT + HALO) / 16;
  const uint32_t log_parts = LOGP ? (uint32_t)LOGP : log_parts_;
  const uint32_t P = 1u << log_parts;
  uint2 *pg = reinterpret_cast<uint2 *>(sh);         // the stage's (packed word, N | read-start masks) per group, for the neighbours; dead once the walk starts
  static_assert(SPAN == 16 && GROUPS == NT + 2 && 2 * GROUPS <= TT, "a thread walks exactly the group it staged; the staged pairs fit the entries they alias");
  uint32_t *sorted = sh;                             // TT + P entries (every partition's run starts at an EVEN entry: up to P holes); aliases pg
  uint32_t *recs = sh + TT + P;                      // TT records: thread t's i-th end position at i·NT + t
  uint32_t *cnt = recs + TT;                         // P
  uint32_t *tstart = cnt + P;                        // P
  uint32_t *gbase = cnt;                             // P: ((this tile's reservation) - tstart) · 4 — takes cnt's place once the runs are placed
  __shared__ uint32_t n_ent_sh;                      // entries of this tile, holes included
  // (cnt[P..P+7] = tstart[0..7] double as the spare counters of the walk: tstart is written after it)
#ifdef SHK_PHASE_TIMING
  unsigned long long ph[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  unsigned long long tprev = 0;
#endif
  uint32_t n_non_n = 0;
  const int k = b.k;
  const uint64_t mask = (1ull << (2 * k)) - 1;
  const uint32_t mask_lo = (uint32_t)mask, mask_hi = (uint32_t)(mask >> 32);
  const uint32_t per = P / NT ? P / NT : 1;
  const uint32_t rbits = 2u * (uint32_t)k - log_parts;  // ≤ 32: bits of a record
  const uint32_t rmask = (uint32_t)(0xFFFFFFFFull >> (32 - rbits));
  const uint32_t segs = OWN || own.segs == 0u ? 1u : own.segs;
  const uint32_t seg = blockIdx.x & (segs - 1u);
  const uint32_t n_regions = (all_lanes ? n_region_lanes : 1u) * segs * P;
  // owner layout
  const uint32_t log_p1w = OWN ? log_parts - own.log_w : 0u;  // super-page bits inside an owner's share
  const uint32_t p1w_mask = (1u << log_p1w) - 1u;
  const uint32_t n_grp = n_region_lanes << log_p1w;           // regions of one owner segment
  const uint32_t keep_mask = own.keep == 0xFFFFFFFFu ? 0u : 0xFFFFFFFFu;
  // cursor word / region-in-segment of partition i for this tile's lane; owner segment of partition i
  auto own_grp = [&](uint32_t i, uint32_t ln) -> uint32_t { return (ln << log_p1w) | (i & p1w_mask); };
  auto own_seg = [&](uint32_t i) -> uint32_t { return own.seg_recs ? i >> log_p1w : 0u; };

  // iteration over sub-tiles: (macro tile t = [t0,t1) of chunk lane `lane`, sub-tile index sub)
  uint64_t t = blockIdx.x, t0, t1;
  uint32_t lane;
  bool have = next_tile(b, t, !all_lanes, lane_filter, t0, t1, lane);
  uint32_t sub = 0;
  StageRegs32<NT, TT> pre;
  if (have) stage32_prefetch<NT, TT>(b, t0, pre);
  // ALL-LANES mode walks a tile LIST (k_build_tiles): a tile's descriptor is two dependent loads away (how many tiles
  // there are, then the descriptor), and the prefetch of its bases a third — asked for when the tile before it is
  // staged, that chain stood in the stage phase of every tile (10 lanes: 169 k cycles per workgroup against 63 k with
  // one lane).  So the descriptor of the tile AFTER the next one is asked for a whole tile ahead.
  // (… and through the VECTOR memory path: a scalar load shares its counter with the LDS operations, so the first LDS
  // wait after it would wait for it as well)
  const uint64_t n_tiles_all = all_lanes && b.tiles ? (uint64_t)b.stats->n_tiles : 0;
  auto desc_ahead = [&](uint64_t tt, uint64_t &d0, uint64_t &d1, uint32_t &dl) -> bool {
    if (!b.tiles) return tile_get(b, tt, d0, d1, dl);
    if (tt >= b.tile_count || tt + b.tile_first >= n_tiles_all) return false;
    const TileDesc *p = b.tiles + tt + b.tile_first;
    asm volatile("" : "+v"(p));  // (the address in vector registers: a global_load, counted by vmcnt)
    const TileDesc d = *p;
    d0 = d.begin;
    d1 = d.end;
    dl = d.lane;
    return true;
  };
  uint64_t at = t + gridDim.x, a0 = 0, a1 = 0;
  uint32_t al = 0;
  bool a_have = false;
  if (all_lanes && have) a_have = desc_ahead(at, a0, a1, al);
  while (have) {
    const uint64_t s0 = t0 + (uint64_t)sub * TT;
    const uint64_t s1 = s0 + TT < t1 ? s0 + TT : t1;
    __syncthreads();  // previous sub-tile's write phase is done with sorted/recs/cnt/tstart/gbase
#ifdef SHK_PHASE_TIMING
    tprev = __builtin_readcyclecounter();
#endif
    for (uint32_t i = threadIdx.x; i < P; i += NT) cnt[i] = 0;
    // ---- stage: this thread's group (and, threads 0 and 1, a halo group) → registers + one LDS pair ----
    uint32_t my_pw, my_gm;
    {
      uint32_t nn = 0;
      my_pw = stage32_group_regs(b, s0, s1, (int)threadIdx.x + 2, pre.raw[0], pre.sb0[0], pre.sb1[0], stats, &my_gm, &nn);
      pg[threadIdx.x + 2] = make_uint2(my_pw, my_gm);
      if (threadIdx.x < 2) {
        uint32_t gm1;
        const uint32_t pw1 = stage32_group_regs(b, s0, s1, (int)threadIdx.x, pre.raw[1], pre.sb0[1], pre.sb1[1], stats, &gm1, &nn);
        pg[threadIdx.x] = make_uint2(pw1, gm1);
      }
      if (all_lanes) {  // this tile's lane: wave sum, one LDS add per wave
        uint32_t v = nn;
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        if ((threadIdx.x & 63) == 0 && v) atomicAdd(&lane_nn[lane], (unsigned long long)v);
      } else {
        n_non_n += nn;
      }
    }
    // the next sub-tile: of this macro tile, or the first one of this workgroup's next macro tile
    uint64_t nt = t, n0 = t0, n1 = t1;
    uint32_t nl = lane, nsub = sub + 1;
    bool hn = true;
    if (t0 + (uint64_t)nsub * TT >= t1) {
      nsub = 0;
      if (all_lanes) {  // the descriptor asked for a tile ago; the one after it is asked for now
        nt = at, hn = a_have, n0 = a0, n1 = a1, nl = al;
        at = nt + gridDim.x;
        if (hn) a_have = desc_ahead(at, a0, a1, al);
      } else {
        nt = t + gridDim.x;
        hn = next_tile(b, nt, !all_lanes, lane_filter, n0, n1, nl);
      }
    }
    if (hn) stage32_prefetch<NT, TT>(b, n0 + (uint64_t)nsub * TT, pre);  // in flight during the rest of this one
    __syncthreads();
    STAMP(0);
    // ---- walk ---------------------------------------------------------------------------------
    uint32_t pr[SPAN];
    {
      const int e0 = threadIdx.x * SPAN;
      const int n_end = (int)(s1 - s0);
      const int jemit = HALO + e0;
      const int jend = HALO + (e0 + SPAN < n_end ? e0 + SPAN : n_end);
      Roll x{0, 0, 0, 0};
      // the two groups before mine: their packed words are the walk's warm-up window, their masks the
      // history of my validity bits
      const uint2 gA = pg[threadIdx.x], gB = pg[threadIdx.x + 1];
      const uint32_t my_ok = stage32_okbits(gA.y, gB.y, my_gm, k, n_end + HALO - ((int)threadIdx.x + 2) * 16);
      {
        // frames just before the first end position: the k bases up to jemit-1 are the low 2k bits of the
        // 32 bases of the two groups before mine
        const uint64_t f0 = (((uint64_t)gA.x << 32) | gB.x) & mask;
        const uint64_t r0 = revcomp(f0, k) << (64 - 2 * k);
        x.f_lo = (uint32_t)f0;
        x.f_hi = (uint32_t)(f0 >> 32);
        x.r_lo = (uint32_t)r0;
        x.r_hi = (uint32_t)(r0 >> 32);
      }
      // Copies of the loop: with 32-bit records — k = 21 on 1024 pages — page and record are simply
      // the two words of the mixed key; and for the usual k (KC = 17, 19, 21; KC = 0: any k at run
      // time) the masks, shifts and the fold of mix_key are compile-time constants (scatter
      // 0.461 → 0.450 → 0.431 ms at k = 21).
      auto walk = [&](auto rb32_t, auto k_t) {
      constexpr bool RB32 = decltype(rb32_t)::value;
      constexpr int KC = decltype(k_t)::value;
      constexpr uint64_t MKC = KC ? (1ull << (2 * KC)) - 1 : 0;
      const int kk = KC ? KC : k;
      const uint32_t mlo = KC ? (uint32_t)MKC : mask_lo, mhi = KC ? (uint32_t)(MKC >> 32) : mask_hi;
      // this thread's sixteen end positions are exactly group 2 + threadIdx.x of the staged tile: their
      // bases are one word of the packed stream (first base on top), their "a k-mer ends here" bits one
      // half-word (never set at or beyond the tile's end)
      const uint32_t pw = my_pw;
      const uint32_t okw = my_ok;
      const uint32_t spare_pc = P + (threadIdx.x & 7u);
      (void)jend;
      (void)jemit;
      const uint32_t rbits_c = RB32 ? 32u : rbits;
      // the window copies (KC ≥ 17): the 48 bases in sight and their reverse complement, as packed words
      const uint32_t w0 = gA.x, w1 = gB.x, w2 = pw;
      const uint32_t rw0 = rev2(~w2), rw1 = rev2(~w1), rw2 = rev2(~w0);
      (void)w0, (void)w1, (void)w2, (void)rw0, (void)rw1, (void)rw2;
      (void)rbits_c;
#pragma unroll
      for (int q = 0; q < SPAN / 8; ++q) {
        // Straight-line on purpose: every lane mixes and issues its LDS add (end positions without
        // a k-mer — bit 2 clear; never set at or beyond the tile's end — count into a spare
        // counter behind cnt[P-1]), and the eight returned ranks are only looked at after the
        // eighth add has been issued.  With a branch per k-mer the wave sits out a full LDS round
        // trip for every single rank.
        uint32_t pcs[8], rks[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) {
          const uint32_t c = ((pw >> (30 - 2 * (q * 8 + r))) & 3u) | (((okw >> (q * 8 + r)) & 1u) << 2);
          uint64_t y;
          uint32_t page;
#ifdef SHK_EXP_GENERIC_WALK
          if (false) {
#else
          if (KC >= 17) {
#endif
            // Hand-shaped for instruction COUNT (every integer VALU op of this loop — 64-bit shifts, compares
            // and v_mad_u64_u32 included — issues at the same 4 cycles per wave on gfx950, tools/ibench2.hip,
            // and the kernel is 70 % VALU-busy).  No rolling state at all: the 48 bases this thread can see
            // — the two groups before its own and its own, three packed words, first base on top — hold
            // every k-mer it emits as a WINDOW, and so do the three words of their reverse complement
            // (rw0..rw2, built once per tile).  A frame LEFT-aligned in 64 bits is two funnel shifts by
            // compile-time counts; the bits below the k-mer are neighbouring bases, cleared once, after the
            // select: min(fwd, rev) is one 64-bit compare on the frames as they are (k odd: a k-mer is never
            // its own reverse complement, so those bits cannot decide it; k even: a tie is a palindrome and
            // both arms are the same k-mer).  The product by the 32-bit multiplier is one v_mul_lo_u32 + one
            // v_mad_u64_u32: mod 2^64 on a left-aligned key IS mod 2^2k on the key.
            constexpr int KK = KC ? KC : 1;
            constexpr uint32_t LS = 64u - 2u * KK;                 // left shift of a frame (22 at k = 21)
            constexpr int j = 0;
            (void)j;
            const int e = q * 8 + r;                               // this step's end position in my group (compile-time: unrolled)
            const int of = 2 * (32 + e - KK + 1);                  // bit offset of the forward window in w0:w1:w2
            const int orv = 2 * (15 - e);                          // … of the reverse-complement window in rw0:rw1:rw2
            uint32_t f_hi, f_lo, r_hi, r_lo;
            if (of < 32) {
              f_hi = of ? __builtin_amdgcn_alignbit(w0, w1, (32 - of) & 31) : w0;
              f_lo = of ? __builtin_amdgcn_alignbit(w1, w2, (32 - of) & 31) : w1;
            } else {
              f_hi = of > 32 ? __builtin_amdgcn_alignbit(w1, w2, (64 - of) & 31) : w1;
              f_lo = of > 32 ? w2 << ((of - 32) & 31) : w2;
            }
            r_hi = orv ? __builtin_amdgcn_alignbit(rw0, rw1, (32 - orv) & 31) : rw0;
            r_lo = orv ? __builtin_amdgcn_alignbit(rw1, rw2, (32 - orv) & 31) : rw1;
            // min(fwd, rev) on the 32-bit halves: the borrow of rev - fwd (two carry-chained subtracts) selects —
            // a 64-bit compare wants its operands in register PAIRS, which costs two or three v_mov per k-mer
            uint32_t c_hi, c_lo, scratch;
            asm("v_sub_co_u32 %2, vcc, %5, %3\n\t"
                "v_subb_co_u32 %2, vcc, %6, %4, vcc\n\t"
                "v_cndmask_b32 %0, %3, %5, vcc\n\t"
                "v_cndmask_b32 %1, %4, %6, vcc"
                : "=&v"(c_lo), "=&v"(c_hi), "=&v"(scratch)
                : "v"(f_lo), "v"(f_hi), "v"(r_lo), "v"(r_hi)
                : "vcc");
            const uint64_t cL = (((uint64_t)c_hi << 32) | c_lo) & ~((1ull << LS) - 1ull);
            const uint64_t yL = (uint64_t)(uint32_t)cL * (uint32_t)MIX_M32 + ((uint64_t)((uint32_t)(cL >> 32) * (uint32_t)MIX_M32) << 32);
            y = yL >> LS;                                          // (the record below takes its low 32 bits)
            page = (uint32_t)(yL >> ((LS + rbits_c) & 63));
          } else {
            roll_step(x, c & 3u, mlo, mhi);
            const uint64_t fwd = ((uint64_t)x.f_hi << 32) | x.f_lo;
            const uint64_t rev = (((uint64_t)x.r_hi << 32) | x.r_lo) >> (64 - 2 * kk);
            y = mix_key(rev < fwd ? rev : fwd, 2 * kk);
            page = RB32 ? (uint32_t)(y >> 32) : (uint32_t)(y >> rbits);
          }
          // emit mask as arithmetic (all ones / zero) and a bit-select instead of ?: — the compiler turns a
          // select whose one arm is expensive into an exec-mask branch around that arm, per k-mer
          uint32_t em;
          asm("v_bfe_i32 %0, %1, %2, 1" : "=v"(em) : "v"(okw), "n"(q * 8 + r));  // all ones where a k-mer ends here
          if (OWN) em &= 0u - (uint32_t)((((page >> log_p1w) ^ own.keep) & keep_mask) == 0u);  // a foreign owner's record: dropped
          asm("v_bfi_b32 %0, %1, %2, %3" : "=v"(pcs[r]) : "v"(em), "v"(page), "v"(spare_pc));  // (em & page) | (~em & spare)
          recs[(q * 8 + r) * NT + threadIdx.x] = RB32 ? (uint32_t)y : (uint32_t)y & rmask;  // transposed: no bank conflicts
          rks[r] = atomicAdd(&cnt[pcs[r]], 1u);  // rank < 2^14
        }
#pragma unroll
        for (int r = 0; r < 8; ++r) pr[q * 8 + r] = (pcs[r] << 18) | rks[r];  // partition · 2^18 | rank (a spare counter, ≥ P: no record — place_entries looks)
      }
      };
      auto walk_k = [&](auto rb32_t) {
        switch (k) {
          case 21: walk(rb32_t, std::integral_constant<int, 21>{}); break;
          case 19: walk(rb32_t, std::integral_constant<int, 19>{}); break;
          case 17: walk(rb32_t, std::integral_constant<int, 17>{}); break;
          default: walk(rb32_t, std::integral_constant<int, 0>{}); break;
        }
      };
      if (rbits == 32) walk_k(std::true_type{});
      else walk_k(std::false_type{});
    }
    __syncthreads();
    STAMP(2);
    // ---- exclusive scan of the counts → tstart ---------------------------------------------------
    {
      // (a run takes an even number of entries: the write phase works on aligned pairs, and a pair never
      // straddles two partitions; an odd run's last pair ends in a hole)
      uint32_t lo = threadIdx.x * per, sacc = 0;
      if (lo < P)
        for (uint32_t i = 0; i < per; ++i) sacc += (cnt[lo + i] + 1u) & ~1u;
      const uint32_t inc = wave_scan_incl(sacc);
      if ((threadIdx.x & 63) == 63) wsum[threadIdx.x >> 6] = inc;
      __syncthreads();
      // offset of this wave = sum of the totals of the waves before it: one masked read per lane
      // and a wave reduction instead of a serial loop over up to NT/64 LDS reads
      const uint32_t wv = threadIdx.x >> 6, ln = threadIdx.x & 63;
      const uint32_t part = (ln < wv && ln < (uint32_t)(NT / 64)) ? wsum[ln] : 0u;
      const uint32_t woff = (uint32_t)__builtin_amdgcn_readlane((int)wave_scan_incl(part), 63);
      uint32_t run = woff + inc - sacc;
      if (lo < P)
        for (uint32_t i = 0; i < per; ++i) {
          tstart[lo + i] = run;
          run += (cnt[lo + i] + 1u) & ~1u;
        }
    }
    const uint32_t rbase = ((all_lanes ? lane * segs : 0u) + seg) * P;  // first region of this tile's lane, in this workgroup's segment
    // reserve this sub-tile's run in every page's region: one returning device-scope add per
    // non-empty (sub-tile, page); the results are parked in registers over the place phase
    uint32_t gres[MAX_PARTS / NT > 0 ? MAX_PARTS / NT : 1];
#pragma unroll
    for (int r = 0; r < (int)(sizeof(gres) / 4); ++r) {
      const uint32_t i = threadIdx.x + r * NT;
      gres[r] = 0;
      if (i < P) {
        const uint32_t c1 = cnt[i];
        if (c1) gres[r] = atomicAdd(&cursor[OWN ? own_seg(i) * n_grp + own_grp(i, lane) : rbase + i], c1);
      }
    }
    __syncthreads();  // codes are dead from here: `sorted` may overwrite them; tstart is complete
    STAMP(3);
    // ---- place ------------------------------------------------------------------------------------
    place_entries<NT, SPAN>(sorted, tstart, pr, P);
#pragma unroll
    for (int r = 0; r < (int)(sizeof(gres) / 4); ++r) {
      const uint32_t i = threadIdx.x + r * NT;
      if (i < P) {
        const uint32_t ts = tstart[i], c1 = cnt[i];
        gbase[i] = (gres[r] - ts) << 2;              // (overwrites cnt[i]: nobody else looks at it any more)
        if (c1 & 1u) sorted[ts + c1] = 0xFFFFFFFFu;  // the hole behind an odd run
        if (i == P - 1) n_ent_sh = ts + ((c1 + 1u) & ~1u);
      }
    }
    __syncthreads();
    STAMP(4);
    // ---- write: one aligned PAIR of entries per lane and step, both of one partition -------------------
    {
      const uint32_t n_ent = n_ent_sh;  // entries, holes included (even)
      const uint2 *sorted2 = reinterpret_cast<const uint2 *>(sorted);
      char *const base = reinterpret_cast<char *>(part_buf32);
      const char *const recs_b = reinterpret_cast<const char *>(recs);
      const char *const gbase_b = reinterpret_cast<const char *>(gbase);
      auto spill_rec = [&](uint32_t pc, uint32_t rec) {  // the page's region is full (skewed input)
        const uint64_t km = unmix_key(((uint64_t)pc << rbits) | rec, 2 * k);
        const unsigned long long j = atomicAdd(OWN && sp.count ? sp.count : &stats->spill_count, 1ull);
        if (j < sp.cap) {
          sp.keys[j] = km;
          sp.lanes[j] = lane;
          sp.counts[j] = 1u;
        }
      };
      // record index `at` inside partition pc's region → where it lives (block-interleaved regions; WIDE:
      // the buffer accumulates the records of many launches and needs 64-bit offsets)
      auto slot_ptr = [&](uint32_t pc, uint32_t at) -> uint32_t * {
        if (OWN)  // segment of pc's owner, then the block-interleave among that owner's regions
          return reinterpret_cast<uint32_t *>(base + (own_seg(pc) * own.seg_recs + rec_slot(own_grp(pc, lane), n_grp, at)) * 4u);
        if (WIDE) return part_buf32 + rec_slot64(rbase + pc, n_regions, at);
        return reinterpret_cast<uint32_t *>(base + rec_slot(rbase + pc, n_regions, at) * 4u);
      };
      const uint32_t cap4 = cap_p << 2;
      // LOGP, one lane: the region count goes into the multiplier and the segment into the base — whole as long as it
      // fits __umul24's 24 bits (S ≤ 4 at LOGP = 10), in blocks beyond (wave-uniform: one of two copies of the loop)
      const uint32_t nreg_m1 = n_regions - 1u;
      constexpr bool FOLDED = !OWN && !WIDE && !ALL && LOGP != 0;  // (the variant that folds; every other one has ONE copy of the loop)
      const bool f24 = !FOLDED || nreg_m1 < (1u << (24 - (RB_LOG + 2)));
      const uint32_t fac = f24 ? nreg_m1 << (RB_LOG + 2) : nreg_m1;
      char *const base_seg = base + ((size_t)(seg * P) << (RB_LOG + 2));
      auto write_out = [&](auto f24_t) {
#pragma unroll 2
      for (uint32_t i = threadIdx.x; 2 * i < n_ent; i += NT) {
        const uint2 ee = sorted2[i];
        const uint32_t pcb = ee.x >> 16;  // partition · 4 (a byte offset into gbase)
        const uint32_t r0 = *reinterpret_cast<const uint32_t *>(recs_b + (ee.x & 0xFFFCu));
        const uint32_t r1 = *reinterpret_cast<const uint32_t *>(recs_b + (ee.y & 0xFFFCu));  // (a hole reads some record: unused)
        const uint32_t at4 = *reinterpret_cast<const uint32_t *>(gbase_b + pcb) + 8u * i;  // record index inside the region, · 4
        const bool hole = ee.y == 0xFFFFFFFFu;
        const bool edge = (at4 & (((1u << RB_LOG) - 1u) << 2)) == (((1u << RB_LOG) - 1u) << 2);  // last record of a block
        if (!hole && !edge && at4 + 8u <= cap4) {
          const uint2 rec2 = make_uint2(r0, r1);  // (both records in one block: one 8-byte store)
          if (!OWN && !WIDE && !ALL && LOGP) {
            // 2^LOGP regions of one lane: byte offset = at·4 + (at >> 10)·(regions - 1)·4096 + region·4096
            const uint32_t m = __umul24(at4 >> (RB_LOG + 2), fac);
            const uint32_t off = (decltype(f24_t)::value ? m : m << (RB_LOG + 2)) + at4 + (pcb << RB_LOG);
            __builtin_memcpy(base_seg + off, &rec2, 8);
          } else if (!OWN && !WIDE && ALL) {
            // the same with the regions of all lanes block-interleaved together (their number is a wave-uniform
            // run-time value; a lane's buffer stays below 4 GiB or the launch is a WIDE one)
            const uint32_t off = (at4 >> (RB_LOG + 2)) * ((n_regions - 1u) << (RB_LOG + 2)) + at4 + ((rbase << (RB_LOG + 2)) + (pcb << RB_LOG));
            __builtin_memcpy(base + off, &rec2, 8);
          } else {
            __builtin_memcpy(slot_ptr(pcb >> 2, at4 >> 2), &rec2, 8);
          }
        } else {
          const uint32_t pc = pcb >> 2, at0 = at4 >> 2;
          if (at0 < cap_p) *slot_ptr(pc, at0) = r0;
          else spill_rec(pc, r0);
          if (!hole) {
            if (at0 + 1 < cap_p) *slot_ptr(pc, at0 + 1) = r1;
            else spill_rec(pc, r1);
          }
        }
      }
      };
      if constexpr (FOLDED) {
        if (f24) write_out(std::true_type{});
        else write_out(std::false_type{});
      } else {
        write_out(std::true_type{});
      }
    }
    STAMP(5);
    t = nt;
    t0 = n0;
    t1 = n1;
    lane = nl;
    sub = nsub;
    have = hn;
  }
  __syncthreads();
  if (all_lanes) {
    if (threadIdx.x < SC32_MAX_LANES && threadIdx.x < n_region_lanes && lane_nn[threadIdx.x])
      atomicAdd(&lane_bases[threadIdx.x], lane_nn[threadIdx.x]);
  } else {
    uint32_t tot = wg_sum<NT>(n_non_n, red);
    if (threadIdx.x == 0 && tot) atomicAdd(&lane_bases[lane_filter], (unsigned long long)tot);
  }
#ifdef SHK_PHASE_TIMING
  if (dbg && threadIdx.x == 0)
    for (int i = 0; i < 8; ++i) dbg[(uint64_t)blockIdx.x * 8 + i] = ph[i];
#endif
}

// ------------------------------------------------------------------------------------------
// k_scatter64: the 8-byte-record scatter (k-mers whose mixed-key remainder does not fit 32 bits: every
// table at k ≥ 22) with k_scatter32's machine — a persistent 1024-thread workgroup per CU, 16 Ki-position
// tiles, the thread's group staged in registers, the window walk — and the RECORDS (canonical k-mers, what
// k_part_rescatter and k_pages read) carried in registers from the walk to the place phase:
//   walk   : windows of the 48 bases in sight → canonical k-mer (two registers per end position, sixteen
//            positions per thread) + partition off the top of the mixed key + rank (returning LDS add)
//   scan, reserve : as k_scatter32 (runs are even: the write-out moves aligned PAIRS)
//   place  : sorted[tstart[partition] + rank] = k-mer — the 8-byte record itself, not an index
//   write  : one 16-byte LDS read and one 16-byte store per lane and step; the partition of a pair is
//            re-read off its first k-mer (one 64-bit multiply per PAIR)
// k_part_scatter_sorted<.., false>, which it replaces for ≤ 1024 partitions and k ≥ 18, kept 16-bit
// position entries and rebuilt every k-mer from the packed tile in its write phase (three LDS reads, funnel
// shifts and the multiply per RECORD: 37 % of that kernel on BASELINE configs[2]).
// LDS: 8·(TT + P) (the sorted records) + 12·P + 8·(NT + 2) (the staged pairs, a buffer of their own: the next
// tile is staged while this one's records wait to be written); same output, same cursors, same padding (EMPTY
// behind an odd run) as the kernel it replaces.
// ------------------------------------------------------------------------------------------
// IL: the output regions BLOCK-INTERLEAVED in blocks of RS_TILE records (record j of region r at
// ((j / RS_TILE) · P + r) · RS_TILE + j mod RS_TILE) — the level-1 buffer k_part_rescatter reads tile by tile: the P
// write fronts stay within P · 32 KiB of one another instead of one per region-sized stride (a dozen address
// translations per store instruction otherwise).  !IL: region r at r · cap_p (page regions k_pages reads).
constexpr int S64_IL_LOG = 12;  // = log2(RS_TILE), asserted below
// OWN (layout 2): the OWNER layout of the exchange between owner shares, as k_scatter32's — the fan-out covers the
// virtual table (the top own.log_w bits of a partition are the record's owner), regions and cursors are ordered
// [owner][lane][super-page], every owner's own.seg_recs records' worth of regions one contiguous piece (what crosses the
// link), linear inside; records of all owners are kept, a full region spills to the list sp.count counts.
constexpr int S64_LINEAR = 0, S64_INTERLEAVED = 1, S64_OWNER = 2;
template <int NT, int TT, int LAYOUT>
__global__ void __launch_bounds__(NT, 4) k_scatter64(
    BatchRef b, uint32_t log_parts, uint32_t lane_filter, unsigned int *__restrict__ cursor,
    uint32_t cap_p, uint64_t *__restrict__ part_buf, DevStats *__restrict__ stats,
    unsigned long long *__restrict__ lane_bases, SpillRef sp, unsigned long long *__restrict__ dbg,
    OwnerCfg own = OwnerCfg{}, uint32_t n_region_lanes = 1) {
  constexpr bool IL = LAYOUT == S64_INTERLEAVED, OWN = LAYOUT == S64_OWNER;
  const uint32_t log_p1w = OWN ? log_parts - own.log_w : 0u;  // super-page bits inside an owner's share
  const uint32_t p1w_mask = (1u << log_p1w) - 1u;
  const uint32_t n_grp = n_region_lanes << log_p1w;           // regions of one owner segment
  // region of partition i for a tile of chunk lane ln, among ALL regions of the launch ([owner][lane][super-page]);
  // own.keep = an owner id: only that owner's records are kept (dropped in the walk) and there is ONE segment
  // (own.seg_recs = 0) — a share's own ingest; own.keep = ~0: every owner's records, a segment each (the exchange)
  const uint32_t keep_mask = own.keep == 0xFFFFFFFFu ? 0u : 0xFFFFFFFFu;
  auto own_region = [&](uint32_t i, uint32_t ln) -> uint32_t {
    return (own.seg_recs ? i >> log_p1w : 0u) * n_grp + ((ln << log_p1w) | (i & p1w_mask));
  };
  extern __shared__ __attribute__((aligned(16))) uint32_t sh[];
  __shared__ uint32_t wsum[NT / 64];
  __shared__ uint32_t red[NT / 64];
  __shared__ uint32_t n_ent_sh;
  static_assert(TILE_T % TT == 0 && TT % (8 * NT) == 0, "tile shape");
  constexpr int SPAN = TT / NT;
  constexpr int GROUPS = (TT + HALO) / 16;
  static_assert(SPAN == 16 && GROUPS == NT + 2, "a thread walks exactly the group it staged");
  const uint32_t P = 1u << log_parts;                  // ≤ NT
  uint2 *sorted = reinterpret_cast<uint2 *>(sh);       // TT + P records (every run starts at an EVEN index)
  uint32_t *cnt = sh + 2 * (TT + P);                   // P
  uint32_t *tstart = cnt + P;                          // P  (tstart[0..7] double as the walk's spare counters: rewritten by every scan)
  uint32_t *gbase = tstart + P;                        // P: (this tile's reservation) − tstart, in records
  uint2 *pg = reinterpret_cast<uint2 *>(gbase + P);    // GROUPS staged (packed word, masks) pairs — of the NEXT tile while this one is written out
#ifdef SHK_PHASE_TIMING
  unsigned long long ph[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  unsigned long long tprev = 0;
#endif
  uint32_t n_non_n = 0;
  const int k = b.k;                                   // 18 ≤ k ≤ 31 (the host's choice)
  const uint32_t LS = 64u - 2u * (uint32_t)k;          // left shift of a frame: 2 … 28
  const uint32_t of0 = 2u * (33u - (uint32_t)k);       // bit offset of the first end position's window in w0:w1:w2 (4 … 30)
  const uint32_t lo_keep = 0xFFFFFFFFu << LS;          // the k-mer's bits of a left-aligned frame's low word
  const uint64_t M = 2u * (uint32_t)k <= MIX_NARROW_BITS ? MIX_M32 : MIX_M64;
  const uint32_t M_lo = (uint32_t)M, M_hi = (uint32_t)(M >> 32);
  const uint32_t psh = 32u - log_parts;                // log_parts ≥ 1

  // The tiles of this workgroup, one after another; a tile's sub-tiles of TT end positions.  Three in flight: the one
  // being walked (c_*), the one staged next (n_*: its bytes are in `pre`), the one after it (asked for when n is staged).
  uint64_t c_t = blockIdx.x, c_t0 = 0, c_t1 = 0, n_t = 0, n_t0 = 0, n_t1 = 0;
  uint32_t c_lane = 0, c_sub = 0, n_lane = 0, n_sub = 0;
  bool c_have = next_tile(b, c_t, true, lane_filter, c_t0, c_t1, c_lane), n_have = false;
#define SHK_S64_BOUNDS(t0_, t1_, sub_, s0_, s1_) \
  const uint64_t s0_ = (t0_) + (uint64_t)(sub_) * TT; \
  const uint64_t s1_ = s0_ + TT < (t1_) ? s0_ + TT : (t1_)
  // (XX_*) ← the sub-tile after (YY_*)
#define SHK_S64_ADVANCE(XX, YY)                                                        \
  do {                                                                               \
    XX##_t = YY##_t, XX##_t0 = YY##_t0, XX##_t1 = YY##_t1, XX##_lane = YY##_lane;            \
    XX##_sub = YY##_sub + 1;                                                           \
    XX##_have = true;                                                                 \
    if (YY##_t0 + (uint64_t)XX##_sub * TT >= YY##_t1) {                                 \
      XX##_sub = 0;                                                                   \
      XX##_t = YY##_t + gridDim.x;                                                     \
      XX##_have = next_tile(b, XX##_t, true, lane_filter, XX##_t0, XX##_t1, XX##_lane);   \
    }                                                                                \
  } while (0)
  StageRegs32<NT, TT> pre;
  uint32_t my_pw = 0, my_gm = 0;  // this thread's group of the tile about to be walked: packed bases, N | read-start masks
  // stage: the prefetched bytes of a sub-tile → this thread's registers + one LDS pair for the neighbours
  auto stage = [&](uint64_t s0, uint64_t s1) {
    uint32_t nn = 0;
    my_pw = stage32_group_regs(b, s0, s1, (int)threadIdx.x + 2, pre.raw[0], pre.sb0[0], pre.sb1[0], stats, &my_gm, &nn);
    pg[threadIdx.x + 2] = make_uint2(my_pw, my_gm);
    if (threadIdx.x < 2) {
      uint32_t gm1;
      const uint32_t pw1 = stage32_group_regs(b, s0, s1, (int)threadIdx.x, pre.raw[1], pre.sb0[1], pre.sb1[1], stats, &gm1, &nn);
      pg[threadIdx.x] = make_uint2(pw1, gm1);
    }
    n_non_n += nn;
  };

  if (threadIdx.x < P) cnt[threadIdx.x] = 0;
  if (c_have) {
    SHK_S64_BOUNDS(c_t0, c_t1, c_sub, s0, s1);
    stage32_prefetch<NT, TT>(b, s0, pre);
    stage(s0, s1);
    SHK_S64_ADVANCE(n, c);
    if (n_have) {
      SHK_S64_BOUNDS(n_t0, n_t1, n_sub, ns0, ns1);
      (void)ns1;
      stage32_prefetch<NT, TT>(b, ns0, pre);
    }
  }
  // Order of a tile's phases: walk, scan + reserve, place, THE NEXT TILE'S STAGE, write.  The stores of the write
  // phase are the last thing a tile issues: they drain under the next tile's walk, and nothing that waits on the
  // vector-memory counter (the prefetched bytes are consumed before them, the reservations' returns a walk later)
  // stands behind them.
  while (c_have) {
    SHK_S64_BOUNDS(c_t0, c_t1, c_sub, s0, s1);
    const uint32_t lane = c_lane;
    __syncthreads();  // the staged pairs and the cleared counts are there; the previous write phase is done with sorted / gbase
#ifdef SHK_PHASE_TIMING
    tprev = __builtin_readcyclecounter();
#endif
    // ---- walk ---------------------------------------------------------------------------------
    uint32_t pr[SPAN], km_lo[SPAN], km_hi[SPAN];
    {
      const int n_end = (int)(s1 - s0);
      const uint2 gA = pg[threadIdx.x], gB = pg[threadIdx.x + 1];
      const uint32_t okw = stage32_okbits(gA.y, gB.y, my_gm, k, n_end + HALO - ((int)threadIdx.x + 2) * 16);
      const uint32_t spare_pc = P + (threadIdx.x & 7u);
      // the 48 bases in sight (the two groups before mine and mine, first base on top), shifted up so that
      // the window of end position e starts 2e bits in — a compile-time funnel shift for ANY k — and the
      // three words of their reverse complement, where that window starts 2·(15 − e) bits in
      const uint32_t w0 = gA.x, w1 = gB.x, w2 = my_pw;
      const uint32_t v0 = __builtin_amdgcn_alignbit(w0, w1, 32u - of0), v1 = __builtin_amdgcn_alignbit(w1, w2, 32u - of0), v2 = w2 << of0;
      const uint32_t rw0 = rev2(~w2), rw1 = rev2(~w1), rw2 = rev2(~w0);
#pragma unroll
      for (int q = 0; q < SPAN / 8; ++q) {
        uint32_t pcs[8], rks[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) {
          const int e = q * 8 + r;
          const int orv = 2 * (15 - e);
          const uint32_t f_hi = e ? __builtin_amdgcn_alignbit(v0, v1, (32 - 2 * e) & 31) : v0;
          const uint32_t f_lo = e ? __builtin_amdgcn_alignbit(v1, v2, (32 - 2 * e) & 31) : v1;
          const uint32_t r_hi = orv ? __builtin_amdgcn_alignbit(rw0, rw1, (32 - orv) & 31) : rw0;
          const uint32_t r_lo = orv ? __builtin_amdgcn_alignbit(rw1, rw2, (32 - orv) & 31) : rw1;
          // min(fwd, rev) on the frames as they are (see k_scatter32): the borrow of rev − fwd selects
          uint32_t c_hi, c_lo, scratch;
          asm("v_sub_co_u32 %2, vcc, %5, %3\n\t"
              "v_subb_co_u32 %2, vcc, %6, %4, vcc\n\t"
              "v_cndmask_b32 %0, %3, %5, vcc\n\t"
              "v_cndmask_b32 %1, %4, %6, vcc"
              : "=&v"(c_lo), "=&v"(c_hi), "=&v"(scratch)
              : "v"(f_lo), "v"(f_hi), "v"(r_lo), "v"(r_hi)
              : "vcc");
          km_lo[e] = __builtin_amdgcn_alignbit(c_hi, c_lo, LS);  // the k-mer, right-aligned (LS < 32)
          km_hi[e] = c_hi >> LS;
          // top word of (left-aligned key · M) mod 2^64 = the top of the mixed key
          const uint32_t cl = c_lo & lo_keep;
          const uint32_t yhi = __umulhi(cl, M_lo) + cl * M_hi + c_hi * M_lo;
          const uint32_t page = yhi >> psh;
          uint32_t em;
          asm("v_bfe_i32 %0, %1, %2, 1" : "=v"(em) : "v"(okw), "n"(q * 8 + r));  // all ones where a k-mer ends here
          if (OWN) em &= 0u - (uint32_t)((((page >> log_p1w) ^ own.keep) & keep_mask) == 0u);  // a foreign owner's record: dropped
          asm("v_bfi_b32 %0, %1, %2, %3" : "=v"(pcs[r]) : "v"(em), "v"(page), "v"(spare_pc));
          rks[r] = atomicAdd(&cnt[pcs[r]], 1u);  // rank < 2^14
        }
#pragma unroll
        for (int r = 0; r < 8; ++r) pr[q * 8 + r] = (pcs[r] << 18) | rks[r];
      }
    }
    __syncthreads();
    STAMP(2);
    // ---- exclusive scan of the even-padded counts → tstart ---------------------------------------
    uint32_t gres = 0, my_c1 = 0;
    {
      const bool mine = threadIdx.x < P;
      my_c1 = mine ? cnt[threadIdx.x] : 0u;
      const uint32_t sacc = (my_c1 + 1u) & ~1u;
      // reserve this sub-tile's (even-padded) run in the partition's region: the return is looked at in the place phase
      if (my_c1) gres = atomicAdd(&cursor[OWN ? own_region(threadIdx.x, lane) : threadIdx.x], sacc);
      const uint32_t inc = wave_scan_incl(sacc);
      if ((threadIdx.x & 63) == 63) wsum[threadIdx.x >> 6] = inc;
      __syncthreads();
      const uint32_t wv = threadIdx.x >> 6, ln = threadIdx.x & 63;
      const uint32_t part = (ln < wv && ln < (uint32_t)(NT / 64)) ? wsum[ln] : 0u;
      const uint32_t woff = (uint32_t)__builtin_amdgcn_readlane((int)wave_scan_incl(part), 63);
      if (mine) tstart[threadIdx.x] = woff + inc - sacc;
    }
    __syncthreads();  // tstart is complete; nobody looks at the counts any more
    STAMP(3);
    // ---- place: the records themselves ---------------------------------------------------------
    {
      const char *const ts_b = reinterpret_cast<const char *>(tstart);
      uint2 *__restrict__ const dst = sorted;
#pragma unroll
      for (int i = 0; i < SPAN; ++i) {
        const uint32_t v = pr[i];  // partition · 2^18 | rank; partitions ≥ P are the spare counters (no record)
        if (v < (P << 18)) dst[*reinterpret_cast<const uint32_t *>(ts_b + (v >> 16)) + (v & 0x3FFFFu)] = make_uint2(km_lo[i], km_hi[i]);
      }
      if (threadIdx.x < P) {
        const uint32_t ts = tstart[threadIdx.x];
        gbase[threadIdx.x] = gres - ts;
        if (my_c1 & 1u) dst[ts + my_c1] = make_uint2(0xFFFFFFFFu, 0xFFFFFFFFu);  // EMPTY behind an odd run
        if (threadIdx.x == P - 1) n_ent_sh = ts + ((my_c1 + 1u) & ~1u);
        cnt[threadIdx.x] = 0;  // for the next tile's walk
      }
    }
    STAMP(4);
    // ---- the next tile's stage (its bytes were asked for a tile ago), and the one after it asked for ----
    uint64_t a_t = 0, a_t0 = 0, a_t1 = 0;
    uint32_t a_lane = 0, a_sub = 0;
    bool a_have = false;
#ifdef SHK_PHASE_TIMING
    asm volatile("s_waitcnt vmcnt(0)");  // (phase build only: what the stage would wait for, booked apart)
    STAMP(6);
#endif
    if (n_have) {
      SHK_S64_BOUNDS(n_t0, n_t1, n_sub, ns0, ns1);
      stage(ns0, ns1);
      SHK_S64_ADVANCE(a, n);
    }
    STAMP(1);
    __syncthreads();  // the sorted records are complete
    STAMP(0);
    // ---- write: one aligned PAIR of records per lane and step, both of one partition; four steps' LDS reads
    // (the pair, then its partition's base) are in flight together — one step at a time the loop is a chain of two
    // LDS round trips per store ------------------------------------------------------------------------------
    {
      const uint32_t n_pairs = n_ent_sh >> 1;  // (records, padding included: even)
      const ulonglong2 *sorted2 = reinterpret_cast<const ulonglong2 *>(sorted);
      char *const base = reinterpret_cast<char *>(part_buf);
#ifndef SHK_S64_WB
#define SHK_S64_WB 1
#endif
      constexpr int WB = SHK_S64_WB;
      for (uint32_t i0 = threadIdx.x; i0 < n_pairs; i0 += WB * NT) {
        ulonglong2 rec[WB];
        uint32_t pc[WB], at[WB];
#pragma unroll
        for (int j = 0; j < WB; ++j) {
          const uint32_t i = i0 + j * NT;
          rec[j] = sorted2[i < n_pairs ? i : n_pairs - 1u];
        }
#pragma unroll
        for (int j = 0; j < WB; ++j) pc[j] = (uint32_t)(((rec[j].x * M) << LS) >> 32) >> psh;
#pragma unroll
        for (int j = 0; j < WB; ++j) at[j] = gbase[pc[j]] + 2 * (i0 + j * NT);  // record index inside partition pc's region
#pragma unroll
        for (int j = 0; j < WB; ++j) {
          if (i0 + j * NT >= n_pairs) continue;
          if (at[j] + 2 <= cap_p) {
            const uint32_t rec_off = IL ? ((((at[j] >> S64_IL_LOG) << log_parts) + pc[j]) << S64_IL_LOG) | (at[j] & ((1u << S64_IL_LOG) - 1u))
                                        : (OWN ? own_region(pc[j], lane) : pc[j]) * cap_p + at[j];
            const uint32_t byte_off = rec_off * 8u;  // < 2^32 (the host sizes a launch's regions so)
            *reinterpret_cast<ulonglong2 *>(base + byte_off) = rec[j];
          } else {  // the region is full (skewed input): these records take the spill path
            const unsigned long long jj = atomicAdd(OWN && sp.count ? sp.count : &stats->spill_count, rec[j].y == EMPTY ? 1ull : 2ull);
            if (jj < sp.cap) {
              sp.keys[jj] = rec[j].x;
              sp.lanes[jj] = lane;
              sp.counts[jj] = 1u;
            }
            if (rec[j].y != EMPTY && jj + 1 < sp.cap) {
              sp.keys[jj + 1] = rec[j].y;
              sp.lanes[jj + 1] = lane;
              sp.counts[jj + 1] = 1u;
            }
          }
        }
      }
    }
    // the bytes of the tile after the next one: asked for BEHIND this tile's stores (in front of them the loads' misses
    // hold up the stores of every wave of the CU in the L1's queue: write phase 2.4× as long), consumed a tile later
    if (a_have) {
      SHK_S64_BOUNDS(a_t0, a_t1, a_sub, as0, as1);
      (void)as1;
      stage32_prefetch<NT, TT>(b, as0, pre);
    }
    STAMP(5);
    c_t = n_t, c_t0 = n_t0, c_t1 = n_t1, c_lane = n_lane, c_sub = n_sub, c_have = n_have;
    n_t = a_t, n_t0 = a_t0, n_t1 = a_t1, n_lane = a_lane, n_sub = a_sub, n_have = a_have;
  }
#undef SHK_S64_BOUNDS
#undef SHK_S64_ADVANCE
  __syncthreads();
  {
    uint32_t tot = wg_sum<NT>(n_non_n, red);
    if (threadIdx.x == 0 && tot) atomicAdd(&lane_bases[lane_filter], (unsigned long long)tot);
  }
#ifdef SHK_PHASE_TIMING
  if (dbg && threadIdx.x == 0)
    for (int i = 0; i < 8; ++i) dbg[(uint64_t)blockIdx.x * 8 + i] = ph[i];
#endif
}

// ------------------------------------------------------------------------------------------
// k_part_rescatter: second level of the partition for tables with more pages than one LDS sort
// can fan out to (> MAX_PARTS).  Level 1 (k_part_scatter_sorted with log_parts < log_pages) has
// grouped the records by SUPER-PAGE (2^log_sub consecutive pages); this kernel takes one
// 16 Ki-record tile of one super-page's region, counting-sorts it by page inside the super-page
// in LDS, reserves each page's share of the final page regions with one returning atomic per
// (tile, page) and writes the records there as aligned pairs — the same machine as level 1 with
// "re-read the record from the LDS copy of the tile" in place of "re-read the k-mer from the
// packed bases" (the fan-out is small here, so 4 Ki-record tiles already give long runs).
// Costs one more 8-B read + 8-B write per k-mer occurrence.
// ------------------------------------------------------------------------------------------
#ifndef SHK_RS_NT
#define SHK_RS_NT 512  // (8 records per thread; with 256 threads the 8-byte re-scatter of config 3 took 58 ms instead of 50)
#endif
constexpr int RS_NT = SHK_RS_NT;
constexpr int RS_TILE = 4096;              // records per tile: they stay in LDS (32 KiB) for the write-out
constexpr int RS_SPAN = RS_TILE / RS_NT;   // records per thread
// LIST mode of k_part_rescatter (below): a flat list of n k-mers (+ lanes) as the source; sub_shift / owner bits: which
// bits of a k-mer's page this pass sorts by (0 / none for the ordinary second level)
struct RescatterList {
  const uint32_t *lanes;  // chunk lane per k-mer, or nullptr: all of them are `lane`'s
  uint64_t n;             // 0: not a list
  uint32_t sub_shift, owner_bits, owner_id, pad;
};
__global__ void __launch_bounds__(RS_NT) k_part_rescatter(
    const uint64_t *__restrict__ src_buf, const unsigned int *__restrict__ src_cursor, uint32_t src_cap,
    uint32_t tiles_per_region, uint32_t log_pages, uint32_t log_sub, uint32_t key_bits,
    unsigned int *__restrict__ dst_cursor,
    uint32_t dst_cap, uint64_t *__restrict__ dst_buf, uint32_t lane, DevStats *__restrict__ stats,
    SpillRef sp, uint32_t src_interleaved, RescatterList ls = RescatterList{}) {
  extern __shared__ __attribute__((aligned(16))) uint32_t sh[];
  __shared__ uint32_t wsum[RS_NT / 64];
  static_assert(RS_TILE == 1 << S64_IL_LOG, "k_scatter64's interleave block is this kernel's tile");
  if (stats->bad != ~0ull) return;
  const uint32_t S = 1u << log_sub;  // pages per super-page
  // (the tiles of one source region go to ONE XCD: see k_part_rescatter32)
  uint32_t bid = blockIdx.x;
  if ((gridDim.x & 7u) == 0) bid = (blockIdx.x & 7u) * (gridDim.x >> 3) + (blockIdx.x >> 3);
  // LIST mode (ls.n > 0): the source is a flat list of k-mers (+ their chunk lanes) instead of a region — the first
  // level of the partition for k-mers that arrive as k-mers (shk_insert_device: the wide exchange round's receiver).
  // One "region" 0, tile = workgroup; k-mers of other lanes and — on an owner share — of other owners are skipped.
  const bool list = ls.n != 0;
  const uint32_t region = list ? 0u : bid / tiles_per_region, tile = list ? bid : bid % tiles_per_region;
  const uint64_t filled = list ? ls.n : (uint64_t)(src_cursor[region] < src_cap ? src_cursor[region] : src_cap);
  const uint64_t r0 = (uint64_t)tile * RS_TILE;
  if (r0 >= filled) return;
  const uint32_t n = filled - r0 < (uint64_t)RS_TILE ? (uint32_t)(filled - r0) : (uint32_t)RS_TILE;  // (even, except a list's last tile)
  const uint32_t lp_mask = log_pages >= 32 ? 0xFFFFFFFFu : (1u << log_pages) - 1u;
  // the page of a k-mer inside this table (an owner share: the low log_pages bits of its page in the virtual table;
  // *own = the top bits name this share) and from it the partition this pass sorts by
  auto sub_of = [&](uint64_t km, bool *own) -> uint32_t {
    const uint32_t gp = (uint32_t)page_of(hash64(km, key_bits), log_pages + ls.owner_bits);
    if (own) *own = ls.owner_bits == 0 || (gp >> log_pages) == ls.owner_id;
    return ((gp & lp_mask) >> ls.sub_shift) & (S - 1u);
  };
  // (src_interleaved: k_scatter64<.., true>'s layout — tile t of region r is block t · n_regions + r)
  const uint64_t *src = list ? src_buf + r0
                        : src_interleaved ? src_buf + (((uint64_t)tile * (gridDim.x / tiles_per_region) + region) << S64_IL_LOG)
                                          : src_buf + (uint64_t)region * src_cap + r0;
  uint64_t *recs = reinterpret_cast<uint64_t *>(sh);                       // RS_TILE records
  uint16_t *sorted = reinterpret_cast<uint16_t *>(sh + 2 * RS_TILE);       // RS_TILE + S entries
  uint32_t *cnt = sh + 2 * RS_TILE + (((uint32_t)RS_TILE + S) * 2 + 15) / 16 * 4;  // S
  uint32_t *tstart = cnt + S;                                              // S
  uint32_t *gbase = tstart + S;                                            // S
  for (uint32_t i = threadIdx.x; i < S; i += RS_NT) cnt[i] = 0;
  __syncthreads();
  // ---- rank: (page-in-super-page, rank) per record, in registers -------------------------------
  uint32_t pr[RS_SPAN];
#pragma unroll
  for (int q = 0; q < RS_SPAN / 2; ++q) {
    const uint32_t i = (uint32_t)(q * RS_NT + threadIdx.x) * 2;  // record pair, coalesced 16-B loads
    uint32_t va = 0xFFFFFFFFu, vb = 0xFFFFFFFFu;
    if (i < n) {
      ulonglong2 rec;
      if (list) {  // single k-mers, the lane's and the share's own only
        rec.x = !ls.lanes || ls.lanes[r0 + i] == lane ? src[i] : EMPTY;
        rec.y = i + 1 < n && (!ls.lanes || ls.lanes[r0 + i + 1] == lane) ? src[i + 1] : EMPTY;
      } else {
        rec = *reinterpret_cast<const ulonglong2 *>(src + i);
      }
      uint32_t sa = 0, sb = 0;
      if (rec.x != EMPTY) {
        bool own;
        sa = sub_of(rec.x, &own);
        if (!own) rec.x = EMPTY;
      }
      if (rec.y != EMPTY) {
        bool own;
        sb = sub_of(rec.y, &own);
        if (!own) rec.y = EMPTY;
      }
      *reinterpret_cast<ulonglong2 *>(recs + i) = rec;
      if (rec.x != EMPTY) va = (sa << 16) | atomicAdd(&cnt[sa], 1u);
      if (rec.y != EMPTY) vb = (sb << 16) | atomicAdd(&cnt[sb], 1u);
    }
    pr[2 * q] = va;
    pr[2 * q + 1] = vb;
  }
  __syncthreads();
  // ---- exclusive scan of the even-padded counts; reservation in the final page regions ---------
  {
    const uint32_t per = S / RS_NT ? S / RS_NT : 1;
    uint32_t lo = threadIdx.x * per, sacc = 0;
    if (lo < S)
      for (uint32_t i = 0; i < per; ++i) sacc += (cnt[lo + i] + 1u) & ~1u;
    const uint32_t inc = wave_scan_incl(sacc);
    if ((threadIdx.x & 63) == 63) wsum[threadIdx.x >> 6] = inc;
    __syncthreads();
    const uint32_t wv = threadIdx.x >> 6, ln = threadIdx.x & 63;
    const uint32_t part = (ln < wv && ln < (uint32_t)(RS_NT / 64)) ? wsum[ln] : 0u;
    const uint32_t woff = (uint32_t)__builtin_amdgcn_readlane((int)wave_scan_incl(part), 63);
    uint32_t run = woff + inc - sacc;
    if (lo < S)
      for (uint32_t i = 0; i < per; ++i) {
        tstart[lo + i] = run;
        run += (cnt[lo + i] + 1u) & ~1u;
      }
  }
  for (uint32_t i = threadIdx.x; i < S; i += RS_NT) {
    const uint32_t c2 = (cnt[i] + 1u) & ~1u;
    gbase[i] = c2 ? atomicAdd(&dst_cursor[((uint64_t)region << log_sub) + i], c2) : 0u;
  }
  __syncthreads();
  // ---- place: entry = record index inside the tile (0xFFFF = pad) ------------------------------------
#pragma unroll
  for (int q = 0; q < RS_SPAN / 2; ++q) {
    const uint32_t i = (uint32_t)(q * RS_NT + threadIdx.x) * 2;
    const uint32_t va = pr[2 * q], vb = pr[2 * q + 1];
    if (va != 0xFFFFFFFFu) sorted[tstart[va >> 16] + (va & 0xFFFFu)] = (uint16_t)i;
    if (vb != 0xFFFFFFFFu) sorted[tstart[vb >> 16] + (vb & 0xFFFFu)] = (uint16_t)(i + 1);
  }
  for (uint32_t i = threadIdx.x; i < S; i += RS_NT)
    if (cnt[i] & 1u) sorted[tstart[i] + cnt[i]] = 0xFFFFu;
  __syncthreads();
  // ---- write: pairs of records, re-read from the LDS copy of the tile ---------------------------
  const uint32_t n_pairs = (tstart[S - 1] + ((cnt[S - 1] + 1u) & ~1u)) >> 1;
  const uint32_t *sorted2 = reinterpret_cast<const uint32_t *>(sorted);
  for (uint32_t i = threadIdx.x; i < n_pairs; i += RS_NT) {
    const uint32_t ee = sorted2[i];
    const uint32_t ea = ee & 0xFFFFu, eb = ee >> 16;
    const uint64_t km0 = recs[ea];
    const uint64_t km1 = eb == 0xFFFFu ? EMPTY : recs[eb];
    const uint32_t sub = sub_of(km0, nullptr);
    const uint32_t at = gbase[sub] + (2 * i - tstart[sub]);
    const uint64_t page = ((uint64_t)region << log_sub) + sub;
    if (at + 2 <= dst_cap) {
      ulonglong2 rec;
      rec.x = km0;
      rec.y = km1;
      *reinterpret_cast<ulonglong2 *>(dst_buf + page * dst_cap + at) = rec;
    } else {
      const unsigned long long j = atomicAdd(&stats->spill_count, km1 == EMPTY ? 1ull : 2ull);
      if (j < sp.cap) {
        sp.keys[j] = km0;
        sp.lanes[j] = lane;
        sp.counts[j] = 1u;
      }
      if (km1 != EMPTY && j + 1 < sp.cap) {
        sp.keys[j + 1] = km1;
        sp.lanes[j + 1] = lane;
        sp.counts[j + 1] = 1u;
      }
    }
  }
}

// k_part_rescatter32: the same second level for 4-byte records.  A level-1 record is the low
// R1 = 2k - log_p1 bits of the mixed key (its super-page is the region it sits in); the page inside
// the super-page is its top log_sub bits, and what goes on to k_pages32 is the rest.  Runs are packed
// (no padding), two entries per lane leave as one 8-B store when they share a page.
#ifndef SHK_RS32_TILE
#define SHK_RS32_TILE 8192
#endif
#ifndef SHK_RS32_NT
#define SHK_RS32_NT 512  // (16 records per thread; 256 threads × 32 records: re-scatter 0.64 → 0.43 ms on a 30 Mb genome)
#endif
constexpr int RS32_TILE = SHK_RS32_TILE;       // records per tile (4 B each in LDS)
constexpr int RS32_NT = SHK_RS32_NT;
constexpr int RS32_SPAN = RS32_TILE / RS32_NT;   // 32 records per thread
static_assert(RS32_TILE <= 65536 && RS32_SPAN % 4 == 0, "16-bit entries; four records per load");
__global__ void __launch_bounds__(RS32_NT) k_part_rescatter32(
    const uint32_t *__restrict__ src_buf, const unsigned int *__restrict__ src_cursor, uint32_t src_cap,
    uint32_t tiles_per_region, uint32_t log_sub, uint32_t r1_bits, uint32_t key_bits,
    unsigned int *__restrict__ dst_cursor, uint32_t dst_cap, uint32_t *__restrict__ dst_buf, uint32_t lane_,
    DevStats *__restrict__ stats, SpillRef sp, uint64_t dst_region_base_, uint64_t n_dst_total,
    uint32_t log_src_lane, uint32_t region_hi, uint64_t dst_lane_stride) {
  extern __shared__ __attribute__((aligned(16))) uint32_t sh[];
  __shared__ uint32_t wsum[RS32_NT / 64];
  if (stats->bad != ~0ull) return;
  const uint32_t S = 1u << log_sub;  // pages per super-page
  // Source regions: one per super-page, or — the owner layout of k_scatter32 — [lane][super-page] with
  // 2^log_src_lane super-pages per lane (log_src_lane = 31: a single lane, lane_).  `region` below is the
  // super-page inside this table's share; region_hi carries the owner bits above it for a key rebuild.
  // Workgroups are dealt to the 8 XCDs round robin; every XCD has its own L2.  All tiles of a source region
  // append to the same 2^log_sub destination regions — runs that lie next to each other in HBM, and cursors
  // that are bumped once per tile — so the tiles of one region are given to ONE XCD (logical block = the XCD's
  // share of the grid, taken in order): its L2 merges the neighbouring partial-line writes and keeps the cursors.
  uint32_t bid = blockIdx.x;
  if ((gridDim.x & 7u) == 0) bid = (blockIdx.x & 7u) * (gridDim.x >> 3) + (blockIdx.x >> 3);
  const uint32_t src_region = bid / tiles_per_region, tile = bid % tiles_per_region;
  const uint32_t lane = lane_ + (src_region >> log_src_lane);
  const uint32_t region = src_region & ((1u << log_src_lane) - 1u);
  const uint64_t dst_region_base = dst_region_base_ + (uint64_t)(src_region >> log_src_lane) * dst_lane_stride;
  const uint32_t filled = src_cursor[src_region] < src_cap ? src_cursor[src_region] : src_cap;
  const uint32_t r0 = tile * RS32_TILE;
  if (r0 >= filled) return;
  const uint32_t n = filled - r0 < (uint32_t)RS32_TILE ? filled - r0 : (uint32_t)RS32_TILE;
  const uint32_t n_src_regions = gridDim.x / tiles_per_region;  // level-1 regions of the source buffer
  uint32_t *recs = sh;                                                      // RS32_TILE records
  uint16_t *sorted = reinterpret_cast<uint16_t *>(sh + RS32_TILE);          // RS32_TILE entries
  uint32_t *cnt = sh + RS32_TILE + RS32_TILE / 2;                           // S
  uint32_t *tstart = cnt + S;                                               // S
  uint32_t *gbase = tstart + S;                                             // S
  for (uint32_t i = threadIdx.x; i < S; i += RS32_NT) cnt[i] = 0;
  __syncthreads();
  // ---- rank: (page-in-super-page, rank) per record, in registers; four records per 16-B load ----
  const uint32_t rbits2 = r1_bits - log_sub;  // record bits that go on to the page workgroup
  uint32_t pr[RS32_SPAN];
  uint4 pre[RS32_SPAN / 4];  // this thread's full quads, all loads issued before the first is used
#pragma unroll
  for (int q = 0; q < RS32_SPAN / 4; ++q) {
    const uint32_t i = (uint32_t)(q * RS32_NT + threadIdx.x) * 4;
    if (i + 4 <= n) pre[q] = *reinterpret_cast<const uint4 *>(src_buf + rec_slot64(src_region, n_src_regions, r0 + i));
  }
#pragma unroll
  for (int q = 0; q < RS32_SPAN / 4; ++q) {
    const uint32_t i = (uint32_t)(q * RS32_NT + threadIdx.x) * 4;
    uint32_t rr[4] = {0, 0, 0, 0};
    if (i + 4 <= n) {  // (four records at a multiple of four never straddle a block)
      const uint4 v = pre[q];
      rr[0] = v.x, rr[1] = v.y, rr[2] = v.z, rr[3] = v.w;
      *reinterpret_cast<uint4 *>(recs + i) = v;
    } else {
      for (int r = 0; r < 4; ++r)
        if (i + r < n) recs[i + r] = rr[r] = src_buf[rec_slot64(src_region, n_src_regions, r0 + i + r)];
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      uint32_t v = 0xFFFFFFFFu;
      if (i + r < n) {
        const uint32_t sub = log_sub ? rr[r] >> rbits2 : 0u;
        v = (sub << 16) | atomicAdd(&cnt[sub], 1u);
      }
      pr[4 * q + r] = v;
    }
  }
  __syncthreads();
  // ---- exclusive scan of the counts; reservation in the final page regions ---------------------
  {
    const uint32_t per = S / RS32_NT ? S / RS32_NT : 1;
    uint32_t lo = threadIdx.x * per, sacc = 0;
    if (lo < S)
      for (uint32_t i = 0; i < per; ++i) sacc += cnt[lo + i];
    const uint32_t inc = wave_scan_incl(sacc);
    if ((threadIdx.x & 63) == 63) wsum[threadIdx.x >> 6] = inc;
    __syncthreads();
    const uint32_t wv = threadIdx.x >> 6, ln = threadIdx.x & 63;
    const uint32_t part = (ln < wv && ln < (uint32_t)(RS32_NT / 64)) ? wsum[ln] : 0u;
    const uint32_t woff = (uint32_t)__builtin_amdgcn_readlane((int)wave_scan_incl(part), 63);
    uint32_t run = woff + inc - sacc;
    if (lo < S)
      for (uint32_t i = 0; i < per; ++i) {
        tstart[lo + i] = run;
        run += cnt[lo + i];
      }
  }
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < S; i += RS32_NT) {
    const uint32_t c1 = cnt[i];
    gbase[i] = (c1 ? atomicAdd(&dst_cursor[dst_region_base + ((uint64_t)region << log_sub) + i], c1) : 0u) - tstart[i];
  }
  // ---- place: entry = record index inside the tile -----------------------------------------------
#pragma unroll
  for (int q = 0; q < RS32_SPAN / 4; ++q) {
    const uint32_t i = (uint32_t)(q * RS32_NT + threadIdx.x) * 4;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const uint32_t v = pr[4 * q + r];
      if (v != 0xFFFFFFFFu) sorted[tstart[v >> 16] + (v & 0xFFFFu)] = (uint16_t)(i + r);
    }
  }
  __syncthreads();
  // ---- write: two entries per lane, re-read from the LDS copy of the tile ------------------------
  const uint32_t *sorted2 = reinterpret_cast<const uint32_t *>(sorted);
  const uint32_t rmask2 = rbits2 >= 32 ? 0xFFFFFFFFu : ((1u << rbits2) - 1u);
  auto spill_rec = [&](uint32_t rec) {  // the page's region is full: the whole key takes the spill path
    const uint64_t key = unmix_key(((uint64_t)(region_hi | region) << r1_bits) | rec, key_bits);
    const unsigned long long j = atomicAdd(&stats->spill_count, 1ull);
    if (j < sp.cap) {
      sp.keys[j] = key;
      sp.lanes[j] = lane;
      sp.counts[j] = 1u;
    }
  };
  for (uint32_t i = threadIdx.x; 2 * i < n; i += RS32_NT) {
    const uint32_t ee = sorted2[i];
    const bool two = 2 * i + 1 < n;
    const uint32_t ra = recs[ee & 0xFFFFu], rb = two ? recs[ee >> 16] : 0u;
    const uint32_t sa = log_sub ? ra >> rbits2 : 0u, sb = two ? (log_sub ? rb >> rbits2 : 0u) : sa;
    const uint32_t at0 = gbase[sa] + 2 * i;
    // destination regions: (this lane's first region) + page; n_dst regions interleave together
    const uint64_t pa = dst_region_base + ((uint64_t)region << log_sub) + sa, pb = dst_region_base + ((uint64_t)region << log_sub) + sb;
    const uint64_t n_dst = n_dst_total;
    if (two && sb == sa && at0 + 2 <= dst_cap && (at0 & ((1u << RB_LOG) - 1u)) != (1u << RB_LOG) - 1u) {
      const uint2 rec2 = make_uint2(ra & rmask2, rb & rmask2);
      __builtin_memcpy(dst_buf + rec_slot64(pa, n_dst, at0), &rec2, 8);
    } else {
      if (at0 < dst_cap) dst_buf[rec_slot64(pa, n_dst, at0)] = ra & rmask2;
      else spill_rec(ra);
      if (two) {
        const uint32_t at1 = gbase[sb] + 2 * i + 1;
        if (at1 < dst_cap) dst_buf[rec_slot64(pb, n_dst, at1)] = rb & rmask2;
        else spill_rec(rb);
      }
    }
  }
}

// In LDS a page is 8192 keys (64 KiB) + 8192 sixteen-bit DELTAS of this pass (16 KiB, two per
// word) = 80 KiB, so two page workgroups share a CU.  The deltas are folded into the page's
// 32-bit counts in HBM when the workgroup leaves (saturating, counting.rs:82-85) — and earlier
// for any slot whose delta reaches 2^15, which a sweep checks every SWEEP_EVERY steps: between two
// sweeps a slot gains at most SWEEP_EVERY·4·PG_WG = 24576 on top of < 2^15, so a delta never wraps.
__device__ __forceinline__ void delta_add(uint32_t *dl, uint32_t slot) {
  atomicAdd(&dl[slot >> 1], 1u << (16 * (slot & 1)));
}

// Workgroup reduction through a few words of scratch LDS (sum), result to every thread.
__device__ __forceinline__ uint32_t pg_wg_sum(uint32_t v, uint32_t *scratch) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
  __syncthreads();
  uint32_t s = 0;
  for (int w = 0; w < PG_WG / 64; ++w) s += scratch[w];
  __syncthreads();
  return s;
}

// LDS budget: 64 KiB keys + 16 KiB deltas = exactly half a CU's 160 KiB, so there is no room
// for even one shared counter: occupancy and new-key counts are reduced through the (then
// idle) delta words, and every wave keeps its own miss queue (a slice of the page's miss_buf
// region) with the fill level in a wave-uniform register — ballot/popcount, no atomics.
constexpr uint32_t MISS_SLACK = 4096;  // extra records per page region of miss_buf (8 slices)
#ifndef SHK_PG_DRAIN_EVERY
#define SHK_PG_DRAIN_EVERY 4
#endif
constexpr uint32_t PG_DRAIN_EVERY = SHK_PG_DRAIN_EVERY; // k_pages: steps (of 4 records per thread) between miss-queue drains
// A wave's queue is emptied at every drain, so it never holds more than the records the wave saw
// since the last one: a page's slice of miss_buf is capped at that, however large its region is.
constexpr uint32_t MISS_WAVE_MAX = PG_DRAIN_EVERY * 4 * 64;
constexpr uint32_t MISS_PAGE_MAX = (PG_WG / 64) * MISS_WAVE_MAX;
// FK / FV: the table holds nothing yet and its memory has not been cleared (the first page pass after a reset, over
// every page and lane: k_pages32's FRESH, for 8-byte records) — FK: the page's keys are not read (they start EMPTY)
// and are written out whole at the end; FV: this lane's counts of the page are zeroed here, first, instead of by a
// fill of the whole table that the pass would then read back.  Lane 0's launch of the pass is <true, true>, the other
// lanes' <false, true>.
template <bool FK, bool FV>
__global__ void __launch_bounds__(PG_WG) k_pages(TableRef tb, uint32_t lane_lo, uint32_t lane_hi, uint32_t lane_stride,
                                                 const unsigned int *__restrict__ cursor, uint32_t cap_p,
                                                 const uint64_t *__restrict__ part_buf,
                                                 uint64_t *__restrict__ miss_buf,
                                                 DevStats *__restrict__ stats, SpillRef sp, uint32_t page0 = 0) {
  // Chunk lanes [lane_lo, lane_hi) one after the other on the same LDS copy of the page's keys (as k_pages32): lane l's
  // records are region l · lane_stride + page of part_buf, its fill level cursor[l · lane_stride + page] (lane_stride
  // = 0: the arrays are one lane's).  The keys are read once and written once however many lanes there are — a launch
  // per lane read and wrote them per lane (ten lanes at k = 31: 215 GB through the page passes of 12.5 M reads, 49 ms).
  __shared__ __attribute__((aligned(16))) uint64_t keys[PAGE_SLOTS];
  __shared__ __attribute__((aligned(16))) uint32_t dl[PAGE_SLOTS / 2];
  if (stats->bad != ~0ull) return;
  const uint32_t page = blockIdx.x + page0;  // (page0: a launch over a range of pages — grouped flush, see flush_acc)
  uint64_t *gk = tb.keys + ((uint64_t)page << PAGE_LOG);
  if (!FK && !FV) {
    uint32_t any = 0;
    for (uint32_t l = lane_lo; l < lane_hi; ++l) any |= cursor[(uint64_t)l * lane_stride + page];
    if (any == 0) return;  // nothing for this page in any lane: leave it untouched in HBM
  }
  // page keys → LDS (16-B vectors), counting occupied slots on the way
  uint32_t my_occ = 0;
  for (uint32_t i = threadIdx.x; i < PAGE_SLOTS / 2; i += PG_WG) {
    ulonglong2 v;
    if (FK) v.x = v.y = EMPTY;
    else v = reinterpret_cast<const ulonglong2 *>(gk)[i];
    reinterpret_cast<ulonglong2 *>(keys)[i] = v;
    my_occ += (v.x != EMPTY) + (v.y != EMPTY);
  }
  const uint32_t occ0 = pg_wg_sum(my_occ, dl);
  // every wave may add its share of what is left below the fill cap; beyond it new keys spill
  const uint32_t room = occ0 < PAGE_FILL_CAP ? (PAGE_FILL_CAP - occ0) / (PG_WG / 64) : 0u;
  uint32_t n_new = 0;   // per thread, over all lanes
  uint32_t lane = lane_lo;
  for (; lane < lane_hi; ++lane) {
  const uint32_t filled0 = cursor[(uint64_t)lane * lane_stride + page];
  const uint32_t filled = filled0 < cap_p ? filled0 : cap_p;  // beyond cap_p: spilled
  uint32_t *gv = tb.vals + (uint64_t)lane * tb.cap + ((uint64_t)page << PAGE_LOG);
  if (FV) {
    for (uint32_t j = threadIdx.x; j < PAGE_SLOTS / 4; j += PG_WG) reinterpret_cast<uint4 *>(gv)[j] = make_uint4(0u, 0u, 0u, 0u);
  }
  if (filled == 0) continue;  // (uniform) nothing of this lane for the page
  for (uint32_t i = threadIdx.x; i < PAGE_SLOTS / 2; i += PG_WG) dl[i] = 0;
  __syncthreads();
  const uint64_t n = filled;
  const uint64_t *src = part_buf + ((uint64_t)lane * lane_stride + page) * cap_p;
  const uint32_t wave = threadIdx.x >> 6, lane_id = threadIdx.x & 63;
  const uint32_t slice_n = (uint32_t)(n / (PG_WG / 64)) + MISS_SLACK / (PG_WG / 64);
  const uint32_t slice = slice_n < MISS_WAVE_MAX ? slice_n : MISS_WAVE_MAX;
  const uint32_t mq_stride = cap_p + MISS_SLACK < MISS_PAGE_MAX ? cap_p + MISS_SLACK : MISS_PAGE_MAX;
  uint64_t *mq = miss_buf + (uint64_t)page * mq_stride + (uint64_t)wave * slice;
  uint32_t n_miss = 0;  // wave-uniform
  // The fill cap is soft: whether this wave may still insert new keys is decided once per
  // drain from its running total, so a wave can overshoot its share by one drain's misses; a
  // page that fills up completely still ends in the spill path (bounded probe).
  bool may_insert = room > 0;
  auto update_may_insert = [&]() {
    uint32_t w = n_new;
    for (int off = 32; off > 0; off >>= 1) w += __shfl_xor(w, off, 64);
    may_insert = w < room;
  };
  // general probe of one record into the LDS page: find the key or insert it, add one.  Bucket by bucket (two
  // 16-B LDS reads bring a bucket's four keys; the first of them, in probe order, that is this key or EMPTY ends
  // the search) instead of one LDS round trip per slot — see k_pages32.
  auto spill = [&](uint64_t key) {
    unsigned long long i = atomicAdd(&stats->spill_count, 1ull);
    if (i < sp.cap) {
      sp.keys[i] = key;
      sp.lanes[i] = lane;
      sp.counts[i] = 1u;
    }
  };
  auto insert = [&](uint64_t key) {
    if (key == EMPTY) return;  // padding record of an odd (tile, page) run
    const uint32_t b0 = slot_of(hash64(key, tb.key_bits), tb.log_pages + tb.owner_bits) >> 2;
    for (uint32_t nb = 0; nb < PAGE_SLOTS / 4;) {
      const uint32_t s0 = ((b0 + nb) & (PAGE_SLOTS / 4 - 1)) << 2;
      const ulonglong2 ka = *reinterpret_cast<const ulonglong2 *>(&keys[s0]);
      const ulonglong2 kb = *reinterpret_cast<const ulonglong2 *>(&keys[s0 + 2]);
      const uint32_t e0 = (ka.x == key) | (ka.x == EMPTY), e1 = (ka.y == key) | (ka.y == EMPTY),
                     e2 = (kb.x == key) | (kb.x == EMPTY), e3 = (kb.y == key) | (kb.y == EMPTY);
      if (!(e0 | e1 | e2 | e3)) {
        ++nb;
        continue;
      }
      const uint32_t q = e0 ? 0u : e1 ? 1u : e2 ? 2u : 3u;
      const uint64_t cur = e0 ? ka.x : e1 ? ka.y : e2 ? kb.x : kb.y;
      if (cur == key) {
        delta_add(dl, s0 + q);
        return;
      }
      if (!may_insert) break;  // this wave's share of the page is used up → spill
      const uint64_t prev = atomicCAS((unsigned long long *)&keys[s0 + q], (unsigned long long)EMPTY,
                                      (unsigned long long)key);
      if (prev == EMPTY) {
        n_new++;
        delta_add(dl, s0 + q);
        return;
      }
      // somebody else took the slot: look at the bucket again (it may be this very key)
    }
    spill(key);
  };
  // Four records per thread per step.  The global loads of the NEXT step, then the four 32-B
  // home buckets (two ds_read_b128 each), are in flight together; a record whose key sits in
  // its home bucket (≈99 % at load ≤ 1/2) costs one non-returning LDS add.  The others (first
  // occurrences, displaced keys) are only QUEUED here and handled densely by the general probe
  // afterwards: a divergent in-line slow path would be executed by nearly every wave for one or
  // two lanes each.  Regions are sequences of aligned record PAIRS (padding = EMPTY): one 16-B
  // load per lane fetches two records; two such loads per step.
  const ulonglong2 *src2 = reinterpret_cast<const ulonglong2 *>(src);
  const uint32_t n_quads = (uint32_t)(n / (4 * PG_WG));  // steps of four records per thread
  constexpr uint32_t DRAIN_EVERY = PG_DRAIN_EVERY;        // steps between miss-queue drains
  // 16-bit deltas: a sweep moves every delta ≥ 2^15 to the 32-bit counts in HBM, so a slot starts an
  // interval below 2^15 and gains at most SWEEP_EVERY·4·PG_WG in it (+ the tail of < 4·PG_WG records)
  constexpr uint32_t SWEEP_EVERY = 12;
  static_assert(0x7FFF + SWEEP_EVERY * 4 * PG_WG + 4 * PG_WG <= 0xFFFF, "a 16-bit delta must not wrap between sweeps");
  ulonglong2 nxt[2];
  if (n_quads) {
    nxt[0] = src2[threadIdx.x];
    nxt[1] = src2[threadIdx.x + PG_WG];
  }
  for (uint32_t quad = 0; quad < n_quads; ++quad) {
    uint64_t kk[4] = {nxt[0].x, nxt[0].y, nxt[1].x, nxt[1].y};
    uint32_t ss[4];
    ulonglong2 ba[4], bb[4];
    if (quad + 1 < n_quads) {  // next step's loads are in flight while this one is processed
      const uint64_t ib = (uint64_t)(quad + 1) * 2 * PG_WG + threadIdx.x;
      nxt[0] = src2[ib];
      nxt[1] = src2[ib + PG_WG];
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) ss[q] = slot_of(hash64(kk[q], tb.key_bits), tb.log_pages + tb.owner_bits);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      ba[q] = *reinterpret_cast<const ulonglong2 *>(&keys[ss[q]]);
      bb[q] = *reinterpret_cast<const ulonglong2 *>(&keys[ss[q] + 2]);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const uint64_t kq = kk[q];
      // straight-line (a ?: chain comes out as nested exec-mask branches): at most one of the four
      // keys can match, so the matching index is a sum of the compare bits; a record that missed —
      // or a padding record — adds 0 to the bucket's first delta instead of skipping the add
      const uint32_t e0 = ba[q].x == kq, e1 = ba[q].y == kq, e2 = bb[q].x == kq, e3 = bb[q].y == kq;
      const uint32_t idx = e1 + 2u * e2 + 3u * e3;
      const uint32_t found = e0 | e1 | e2 | e3;       // (EMPTY = padding "finds" a free slot)
      const uint32_t slot = ss[q] + idx;
      atomicAdd(&dl[slot >> 1], (found & (uint32_t)(kq != EMPTY)) << (16u * (slot & 1u)));
      const bool missed = !found;
      const unsigned long long mm = __ballot(missed);
      if (missed) mq[n_miss + __builtin_amdgcn_mbcnt_hi((uint32_t)(mm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mm, 0u))] = kq;
      n_miss += (uint32_t)__popcll(mm);
    }
    // drain after each of the first DRAIN_EVERY steps (an empty page misses on every first
    // occurrence, and on its repeats until it is inserted), then every DRAIN_EVERY steps
    // (no barrier: the queue is the wave's own, and a key another wave is inserting right now is at
    // worst missed once more and found by the general probe)
    if (quad < DRAIN_EVERY || (quad % DRAIN_EVERY) == DRAIN_EVERY - 1 || quad + 1 == n_quads) {
      for (uint32_t j = lane_id; j < n_miss; j += 64) insert(mq[j]);  // this wave's own queue
      n_miss = 0;
      update_may_insert();
    }
    if ((quad % SWEEP_EVERY) == SWEEP_EVERY - 1) {
      __syncthreads();
      // deltas >= 2^15 go to the 32-bit counts in HBM now (a slot gains < 2^15 between checks)
      for (uint32_t j = threadIdx.x; j < PAGE_SLOTS / 2; j += PG_WG) {
        const uint32_t w = dl[j];
        if (w & 0x80008000u) {
          if (w & 0x8000u) gv[2 * j] = sat_add_u32(gv[2 * j], w & 0xFFFFu);
          if (w & 0x80000000u) gv[2 * j + 1] = sat_add_u32(gv[2 * j + 1], w >> 16);
          dl[j] = (w & 0x8000u ? 0u : (w & 0xFFFFu)) | (w & 0x80000000u ? 0u : (w & 0xFFFF0000u));
        }
      }
      __syncthreads();
    }
  }
  // tail (< 4*PG_WG records): straight through the general probe
  for (uint64_t i = (uint64_t)n_quads * 4 * PG_WG + threadIdx.x; i < n; i += PG_WG) insert(src[i]);
  __syncthreads();
  // LDS → page: counts += deltas (saturating), four slots per lane; then the keys if any is new
  for (uint32_t j = threadIdx.x; j < PAGE_SLOTS / 4; j += PG_WG) {
    const uint2 d = reinterpret_cast<const uint2 *>(dl)[j];
    if (d.x | d.y) {
      uint4 v = reinterpret_cast<const uint4 *>(gv)[j];
      v.x = sat_add_u32(v.x, d.x & 0xFFFFu);
      v.y = sat_add_u32(v.y, d.x >> 16);
      v.z = sat_add_u32(v.z, d.y & 0xFFFFu);
      v.w = sat_add_u32(v.w, d.y >> 16);
      reinterpret_cast<uint4 *>(gv)[j] = v;
    }
  }
  __syncthreads();  // (the next lane clears the deltas)
  }  // lanes
  const uint32_t nnew = pg_wg_sum(n_new, dl);
  if (nnew || FK) {
    for (uint32_t j = threadIdx.x; j < PAGE_SLOTS / 2; j += PG_WG)
      reinterpret_cast<ulonglong2 *>(gk)[j] = reinterpret_cast<const ulonglong2 *>(keys)[j];
    if (threadIdx.x == 0 && nnew) atomicAdd(&stats->n_distinct, (unsigned long long)nnew);
  }
}

// ------------------------------------------------------------------------------------------
// k_pages32: the page workgroup for 4-byte records (k_part_scatter_sorted<.., true>).  A record
// is rec = mix_key(key) mod 2^R, R = 2k - log_pages ≤ 32: home bucket = its top 11 bits,
// fingerprint fp = the R-11 bits below.  The page sits in LDS as 32-bit TAGS instead of keys:
//     tag(slot) = fp(key) << 4 | d ,  d = (bucket(slot) - home bucket(key)) mod 2048, d ≤ 14
// which — mix_key being a bijection and the page known — identifies the key.  A record hits when
// one of the four tags of its home bucket (ONE ds_read_b128) equals fp << 4; no hash is computed
// here at all.  Everything else (first occurrences, displaced keys) goes through a per-wave miss
// queue IN LDS (the tags leave room for it) and the general probe, which compares (fp, d) slot
// by slot, inserts with a CAS on the tag and then writes the rebuilt key (unmix_key) to the
// page in HBM.  What a tag cannot express — a key ≥ 15 buckets from home (d = 15, only ever created
// by the direct path) met on a probe, or a probe that would have to insert that far out —
// sends the record to the spill list, i.e. through the exact global-memory path.
// Counts: 16-bit deltas as in k_pages.  Keys are written when inserted, so the page's keys are
// never written back wholesale.
// ------------------------------------------------------------------------------------------
// A workgroup barrier that orders LDS traffic only: global stores still in flight are not waited for.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

constexpr uint32_t TAG_EMPTY = 0xFFFFFFFFu;
// A tag's low TAG_DB bits: how many buckets past its home bucket the key sits (0 … TAG_FAR - 1; TAG_FAR = all ones:
// farther than a tag can say — only ever created by the direct path — or, with all other bits set too, EMPTY).
// Four bits since round 2 (the fingerprint has at most 21): with three, ONE k-mer of a 3 M-k-mer input that came to
// lie 7 buckets from home sent its ≈1000 records through the spill path in every job.
constexpr uint32_t TAG_DB = 4, TAG_FAR = (1u << TAG_DB) - 1u;
constexpr uint32_t MQ32 = 512;              // miss-queue entries per wave (LDS)
constexpr uint32_t P32_RPS = 4;             // records per thread per step (one 16-B load)
constexpr uint32_t P32_EARLY = 4;           // steps after which the miss queue is drained regardless of its fill
static_assert(PAGE_SLOTS * 4 + PAGE_SLOTS * 4 + (PG_WG / 64) * MQ32 * 4 <= 81920, "two page workgroups per CU");
static_assert(MQ32 >= 2 * 64 * P32_RPS, "the queue must take a whole step of misses on top of the drain threshold");
// Chunk lanes [lane_lo, lane_hi) are processed one after the other on the same LDS copy of the
// page (tags stay, the per-pass counts are written back and cleared in between); lane l's records
// are region l·lane_stride + page of the n_regions block-interleaved regions (lane_stride = 0: the
// buffer holds one lane, region = page).
//
// FRESH: the table holds nothing yet and its memory has not even been cleared (shk_reset leaves that to the first
// page pass when that pass covers every page and every lane).  The page is then not READ at all — tags start
// empty, counts start at zero — and written out whole at the end: every lane's counts, and the keys rebuilt from
// the tags (a tag and the page identify the key), EMPTY where no tag is.  What a reset would have written is
// written once, with the result in it, and a page in costs nothing.
//
// HIST (with FRESH): the page's share of EVERY histogram column and of the totals on the way out.  A fresh pass has
// each slot's counts of every chunk lane in its registers as it writes them — what k_histo would read back a moment
// later (4 B per slot and lane: a fifth of a ten-lane job on a 30 Mb genome).  Column l is the histogram of the
// clamped prefix sums over lanes 0..l (k_histo's comment; counting.rs:171-202, histogram.rs:51-85): a thread keeps
// the running sum of its sixteen slots across the lane loop, bins below FH_BINS go through LDS histograms (every
// wave's own, then idle, miss queue) into this page's row of `partial` — plain stores, k_hist_reduce sums the rows —
// and the few beyond straight into `hist`.  The host uses the result only if nothing else touches the table before
// the histogram is asked for (shk_ctx::fused_valid); otherwise k_histo runs as before.
constexpr uint32_t FH_BINS = 512;
struct FusedHist {
  uint32_t *partial;             // [page][col][FH_BINS]
  unsigned long long *ptot;      // [page][4]: occupied slots, Σ clamped sums, Σ lane counts, any saturated
  unsigned long long *hist;      // the context's histogram (bins ≥ FH_BINS)
  unsigned long long histo_max;
  uint32_t n_cols;
  uint32_t pad;
  unsigned long long *pspill;    // [page]: records this page's workgroup put on the spill list (TABLE = false only)
};
// (HIST = 2: the launch covers ONE chunk lane — no running sums to carry across a lane loop: the fold's sixteen
// registers and what they cost the record loop's code are not there)
//
// TABLE = false (with HIST): the histogram-only form.  Identical up to the end of a lane's record loop; then neither
// the lane's counts nor, at the end, the rebuilt keys are stored — the histogram rows, the totals, the spills and
// n_distinct are what the pass leaves.  The table is then DEFINED by the regions and cursors the launch read
// (shk_ctx::tb_virtual): whoever needs it runs k_pages32<true, 0> over them again.  A page's own spills are counted
// (pspill): that second pass spills for itself, so the host takes these off the list and keeps the scatter's.
template <bool FRESH, int HIST = 0, bool TABLE = true>
__global__ void __launch_bounds__(PG_WG, 4) k_pages32(TableRef tb, uint32_t lane_lo, uint32_t lane_hi,
                                                      uint32_t lane_stride, uint32_t n_regions_,
                                                      const unsigned int *__restrict__ cursor, uint32_t cap_p,
                                                      const uint32_t *__restrict__ part_buf,
                                                      DevStats *__restrict__ stats, SpillRef sp, uint32_t page0 = 0,
                                                      FusedHist fh = FusedHist{}, uint32_t segs = 1) {
  static_assert(!HIST || FRESH, "the fused histogram is a fresh pass's");
  static_assert(TABLE || HIST, "a pass that writes no table leaves the histogram");
  static_assert(FH_BINS == MQ32, "a wave bins into its own miss queue");
  __shared__ __attribute__((aligned(16))) uint32_t tags[PAGE_SLOTS];
  __shared__ __attribute__((aligned(16))) uint32_t dl[PAGE_SLOTS];  // this pass's count per slot
  __shared__ __attribute__((aligned(16))) uint32_t mqs[(PG_WG / 64) * MQ32];
  if (stats->bad != ~0ull) return;
  const uint32_t page = blockIdx.x + page0;
  // (lane l, segment s) of this page: region and cursor word (l·segs + s)·pages + page (k_scatter32's cursor segments;
  // lane_stride = pages or — one lane's regions — 0; segs = 1: l·lane_stride + page)
  const uint32_t seg_stride = segs > 1 ? 1u << tb.log_pages : 0u;
  auto region_of = [&](uint32_t l, uint32_t s) -> uint32_t { return l * lane_stride * segs + s * seg_stride + page; };
  if (!FRESH) {
    uint32_t any = 0;
    for (uint32_t l = lane_lo; l < lane_hi; ++l)
      for (uint32_t s = 0; s < segs; ++s) any |= cursor[region_of(l, s)];
    if (any == 0) return;  // nothing for this page in any lane: leave it untouched in HBM
  }
  uint32_t lane = lane_lo;
  const uint32_t bits = tb.key_bits, R = bits - (tb.log_pages + tb.owner_bits), fpb = R - 11;
  const uint32_t fpmask = (1u << fpb) - 1u;
  const uint64_t gpage = ((uint64_t)tb.owner_id << tb.log_pages) | page;  // page index in the virtual global table (owner share)
  uint64_t *gk = tb.keys + ((uint64_t)page << PAGE_LOG);
  uint32_t *gv = nullptr;  // this lane's counts of the page (set per lane below)
  // page keys → tags, counting occupied slots on the way
  uint32_t my_occ = 0;
  constexpr int LD = PAGE_SLOTS / 2 / PG_WG;  // 16-B loads per thread: all issued before the first is used
  if (FRESH) {
#pragma unroll
    for (int u = 0; u < LD; ++u) reinterpret_cast<uint2 *>(tags)[threadIdx.x + u * PG_WG] = make_uint2(TAG_EMPTY, TAG_EMPTY);
  } else {
  ulonglong2 pv[LD];
#pragma unroll
  for (int u = 0; u < LD; ++u) pv[u] = reinterpret_cast<const ulonglong2 *>(gk)[threadIdx.x + u * PG_WG];
#pragma unroll
  for (int u = 0; u < LD; ++u) {
    const uint32_t i = threadIdx.x + u * PG_WG;
    const ulonglong2 v = pv[u];
    const uint64_t kv[2] = {v.x, v.y};
    uint32_t tg[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      tg[q] = TAG_EMPTY;
      if (kv[q] != EMPTY) {
        const uint32_t rec = (uint32_t)mix_key(kv[q], bits) & (uint32_t)(0xFFFFFFFFull >> (32 - R));
        const uint32_t d = (((2 * i + q) >> 2) - (rec >> fpb)) & (PAGE_SLOTS / 4 - 1);
        tg[q] = ((rec & fpmask) << TAG_DB) | (d < TAG_FAR ? d : TAG_FAR);
        my_occ++;
      }
    }
    reinterpret_cast<uint2 *>(tags)[i] = make_uint2(tg[0], tg[1]);
  }
  }
  const uint32_t occ0 = FRESH ? 0u : pg_wg_sum(my_occ, dl);
  const uint32_t room = occ0 < PAGE_FILL_CAP ? (PAGE_FILL_CAP - occ0) / (PG_WG / 64) : 0u;
  for (uint32_t i = threadIdx.x; i < PAGE_SLOTS; i += PG_WG) dl[i] = 0;
  __syncthreads();
  uint32_t n = 0;        // records of the current lane's segments together (set per lane below)
  const uint64_t n_regions = n_regions_;
  const uint32_t wave = threadIdx.x >> 6, lane_id = threadIdx.x & 63;
  uint32_t *mq = mqs + wave * MQ32;
  uint32_t n_miss = 0;  // wave-uniform
  uint32_t n_new = 0;   // per thread
  bool may_insert = room > 0;
  auto update_may_insert = [&]() {
    uint32_t w = n_new;
    for (int off = 32; off > 0; off >>= 1) w += __shfl_xor(w, off, 64);
    may_insert = w < room;
  };
  uint32_t n_sp = 0;    // per thread (TABLE = false)
  auto spill = [&](uint32_t rec) {
    const uint64_t key = unmix_key((gpage << R) | rec, bits);
    if (!TABLE) ++n_sp;
    unsigned long long i = atomicAdd(&stats->spill_count, 1ull);
    if (i < sp.cap) {
      sp.keys[i] = key;
      sp.lanes[i] = lane;
      sp.counts[i] = 1u;
    }
  };
  // general probe of one record: find its (fp, d) tag or insert it, add one.  Bucket by bucket — ONE 16-B LDS read
  // brings the four tags of a bucket, which are then looked at in probe order in registers (a tag is written once,
  // from EMPTY: what was read as occupied stays what it is; what was read as EMPTY is claimed with a CAS, whose
  // answer is the slot's tag if somebody else was faster).  Slot by slot this was a chain of LDS round trips per
  // record: most of a many-lane page pass (10 lanes, 30 Mb genome: 10 k cycles per lane and page in the drains).
  auto insert = [&](uint32_t rec) {
    const uint32_t home = rec >> fpb, fp3 = (rec & fpmask) << TAG_DB;
    for (uint32_t d = 0; d < TAG_FAR;) {
      const uint32_t sl0 = ((home + d) & (PAGE_SLOTS / 4 - 1)) << 2, want = fp3 | d;
      const uint4 t4 = *reinterpret_cast<const uint4 *>(&tags[sl0]);
      // the first slot of the bucket, in probe order, that ends the search: this key's tag, an EMPTY slot, or a far
      // entry (low bits 7 — EMPTY has them too); one decision per bucket, the same code for every lane
      const uint32_t s0 = (t4.x == want) | ((t4.x & TAG_FAR) == TAG_FAR), s1 = (t4.y == want) | ((t4.y & TAG_FAR) == TAG_FAR),
                     s2 = (t4.z == want) | ((t4.z & TAG_FAR) == TAG_FAR), s3 = (t4.w == want) | ((t4.w & TAG_FAR) == TAG_FAR);
      if (!(s0 | s1 | s2 | s3)) {
        ++d;
        continue;
      }
      const uint32_t q = s0 ? 0u : s1 ? 1u : s2 ? 2u : 3u;
      const uint32_t cur = s0 ? t4.x : s1 ? t4.y : s2 ? t4.z : t4.w;
      if (cur == want) {
        atomicAdd(&dl[sl0 + q], 1u);
        return;
      }
      if (cur != TAG_EMPTY || !may_insert) break;  // a far entry (cannot tell whether it is this key), or this wave's share of the page's room is used up → spill
      const uint32_t prev = atomicCAS(&tags[sl0 + q], TAG_EMPTY, want);
      if (prev == TAG_EMPTY) {
        n_new++;
        if (!FRESH) gk[sl0 + q] = unmix_key((gpage << R) | rec, bits);
        atomicAdd(&dl[sl0 + q], 1u);
        return;
      }
      // somebody else took the slot: look at the bucket again (it may be this very key)
    }
    spill(rec);  // (or too far out for a tag)
  };
  auto drain = [&]() {
    for (uint32_t j = lane_id; j < n_miss; j += 64) insert(mq[j]);  // this wave's own queue
    n_miss = 0;
    update_may_insert();
  };
  // HIST: the running (clamped) sums of this thread's sixteen slots over the lanes so far, and its share of the totals
  constexpr int WBH = PAGE_SLOTS / 4 / PG_WG;
  uint32_t cum[HIST == 1 ? WBH * 4 : 1];
  uint32_t one_unique = 0, one_sat = 0;  // HIST = 2: the totals as the (only) lane's counts go by
  unsigned long long fh_lane = 0;
  uint32_t n_high = 0;  // sums this thread sent past the LDS bins (same-line global adds: a job full of them should leave the histogram to k_histo — the host looks)
  if (HIST == 1) {
#pragma unroll
    for (int i = 0; i < WBH * 4; ++i) cum[i] = 0;
  }
  // one lane's counts d (this thread's quads) folded into the sums; column `lane` of the page → partial.  Called by
  // every thread of the workgroup, the miss queues idle (between a lane's drain and the next lane's first record).
  auto fold_hist = [&](const uint4 (&d)[WBH]) {
    if (!HIST) return;
    // every wave bins into its OWN miss queue (MQ32 = FH_BINS words, idle since the wave's last drain): nothing to
    // agree on before, one barrier before the rows are summed, one before the queues are queues again
    const bool col = lane < fh.n_cols;
    if (col) {
      for (uint32_t i = lane_id; i < FH_BINS; i += 64) mq[i] = 0;
    }
    const unsigned long long hlen = fh.histo_max + 2;
    // bin of a sum cc: min(cc, histo_max + 1) — in 32 bits (histo_max ≥ 2^32 - 1: every sum is its own bin)
    const uint32_t top32 = fh.histo_max >= 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)fh.histo_max + 1u;
    uint32_t lsum = 0, lcarry = 0;  // Σ of this lane's sixteen counts
#pragma unroll
    for (int u = 0; u < WBH; ++u) {
      const uint32_t v[4] = {d[u].x, d[u].y, d[u].z, d[u].w};
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const uint32_t s1 = lsum + v[q];
        lcarry += s1 < lsum;
        lsum = s1;
        uint32_t cc;
        if (HIST == 1) {
          cc = sat_add_u32(cum[u * 4 + q], v[q]);
          cum[u * 4 + q] = cc;
        } else {
          cc = v[q];
          one_unique += cc != 0;
          one_sat |= cc == 0xFFFFFFFFu;
        }
        const uint32_t bin = cc < top32 ? cc : top32;
        if (col && cc) {
          if (bin < FH_BINS) atomicAdd(&mq[bin], 1u);
          else atomicAdd(&fh.hist[(unsigned long long)lane * hlen + bin], 1ull), ++n_high;
        }
      }
    }
    fh_lane += ((unsigned long long)lcarry << 32) | lsum;
    if (col) {
      lds_barrier();
      uint32_t *row = fh.partial + ((size_t)page * fh.n_cols + lane) * FH_BINS;
      for (uint32_t i = threadIdx.x; i < FH_BINS; i += PG_WG) {
        uint32_t sum = 0;
#pragma unroll
        for (int w = 0; w < PG_WG / 64; ++w) sum += mqs[w * MQ32 + i];
        row[i] = sum;
      }
      lds_barrier();  // (the next lane's misses go where the bins were)
    }
  };
  for (lane = lane_lo; lane < lane_hi; ++lane) {
    // (segment 0's fill level is read once; with one segment it is the region's, and the loop below is the single-region one)
    const uint32_t filled0 = cursor[region_of(lane, 0u)];
    const uint32_t fill0 = filled0 < cap_p ? filled0 : cap_p;
    auto seg_fill = [&](uint32_t s) -> uint32_t {  // records in segment s (wave-uniform)
      if (s == 0u) return fill0;
      const uint32_t filled = cursor[region_of(lane, s)];
      return filled < cap_p ? filled : cap_p;  // beyond cap_p: spilled
    };
    n = fill0;
    for (uint32_t s = 1; s < segs; ++s) n += seg_fill(s);
    gv = tb.vals + (uint64_t)lane * tb.cap + ((uint64_t)page << PAGE_LOG);
    if (n == 0) {  // (uniform across the workgroup)
      if (FRESH && TABLE) {
#pragma unroll
        for (int u = 0; u < PAGE_SLOTS / 4 / PG_WG; ++u)
          reinterpret_cast<uint4 *>(gv)[threadIdx.x + u * PG_WG] = make_uint4(0u, 0u, 0u, 0u);
      }
      if (HIST) {  // (the column still counts every slot whose sum so far is not zero)
        uint4 z[WBH];
#pragma unroll
        for (int u = 0; u < WBH; ++u) z[u] = make_uint4(0u, 0u, 0u, 0u);
        fold_hist(z);
      }
      continue;
    }
    // this lane's counts of the page: asked for NOW, needed when the lane's records have been counted — the
    // HBM round trip hides behind the record loop instead of standing between two lanes.  (A deeper pipeline —
    // every lane's fill level asked for up front, the next lane's first records in flight over this lane's drain
    // and write-out — was measured twice: ten lanes on a 30 Mb genome 3.04 → 2.91 ms before the drains were
    // made cheap, 1.81 → 1.86 ms after.  Not kept.)
    constexpr int WB = PAGE_SLOTS / 4 / PG_WG;
    uint4 gvv[WB];
    const bool prefetch = !FRESH && lane_hi - lane_lo > 1;  // (one lane: nothing stands between two lanes; the quads that did not change are then not read at all)
    if (prefetch) {
#pragma unroll
      for (int u = 0; u < WB; ++u) gvv[u] = reinterpret_cast<const uint4 *>(gv)[threadIdx.x + u * PG_WG];
    }
    // Main loop: one 16-B load = four records per thread per step, the next step's load in flight.
    // No barrier in here: queues are per wave, and a slot's count of this pass is a full 32-bit word
    // (a page sees < 2^31 records), so nothing has to be folded away mid-pass.
    // The lane's segments go into the same counts one after the other, ONE pipeline across them: first every segment's
    // whole steps (the load in flight may be the next segment's first), then what is left of all of them as one dense
    // run of quads — a thread finds its quad's (segment, offset) from the prefix sums — so that a page pays about as
    // many partial steps as there are records for, not one per segment.
    constexpr uint32_t STEP = P32_RPS * PG_WG;
    // (a region of at most two steps — a chunk lane's share of a page on a many-lane table — fits the miss queue
    // whole: one drain at the end instead of three, each of which is a chain of LDS round trips)
    const bool early = n > 2 * P32_RPS * PG_WG;
    auto load4 = [&](uint32_t s, uint32_t j) {  // four records from record j of segment s on (they share a block)
      return *reinterpret_cast<const uint4 *>(part_buf + rec_slot64(region_of(lane, s), n_regions, j));
    };
    // `nv` = how many of the lane's four records exist (4 in every step but a page's last, partial one)
    auto body = [&](uint32_t step, const uint4 &cur, uint32_t nv, auto partial) {
      const uint32_t rr[4] = {cur.x, cur.y, cur.z, cur.w};
      uint4 bk[4];
  #pragma unroll
      for (int q = 0; q < 4; ++q) bk[q] = *reinterpret_cast<const uint4 *>(&tags[(rr[q] >> fpb) << 2]);
      // Straight-line code on purpose (no ?: chains, which come out as nested exec-mask branches):
      // at most one of the four tags can match, so the matching index is a sum of the compare bits,
      // and a record that missed adds 0 to its bucket's first slot instead of skipping the add.
      bool missed[4];
  #pragma unroll
      for (int q = 0; q < 4; ++q) {
        const uint32_t want = (rr[q] & fpmask) << TAG_DB;
        const uint32_t e0 = bk[q].x == want, e1 = bk[q].y == want, e2 = bk[q].z == want, e3 = bk[q].w == want;
        const uint32_t idx = e1 + 2u * e2 + 3u * e3;
        uint32_t found = e0 | e1 | e2 | e3;
        bool exists = true;
        if (decltype(partial)::value) {
          exists = (uint32_t)q < nv;
          found &= (uint32_t)exists;
        }
        // (a lane past the end of the region adds its 0 to a slot of its own: left at record 0's bucket, the up
        // to 2047 of them in a page's last step queue up on ONE LDS address, and same-address atomics go one
        // by one — it shows on many-lane tables, where every lane of every page has such a step)
        uint32_t at = ((rr[q] >> fpb) << 2) + idx;
        if (decltype(partial)::value) at = exists ? at : threadIdx.x * 4u + (uint32_t)q;
        atomicAdd(&dl[at], found);
        missed[q] = exists && !found;
      }
  #pragma unroll
      for (int q = 0; q < 4; ++q) {
        const unsigned long long mm = __ballot(missed[q]);
        // (lanes below this one that missed: v_mbcnt_lo/hi take the mask as it is)
        if (missed[q]) mq[n_miss + __builtin_amdgcn_mbcnt_hi((uint32_t)(mm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mm, 0u))] = rr[q];
        n_miss += (uint32_t)__popcll(mm);
      }
      // drain when the next step might not fit (worst case: every record of it misses), and after
      // each of the first few steps: an empty page misses on every first occurrence and on its
      // repeats until it is inserted (measured: 4 early drains 0.232 ms, 0 → 0.240, 16 → 0.257)
      if (n_miss > MQ32 - 64 * P32_RPS || (step < P32_EARLY && early)) drain();
    };
    if (segs == 1) {  // one region per (lane, page): the loop as it has always been (every lane of a many-lane table comes through here)
      const uint32_t n_steps = n / STEP;
      uint4 nxt;
      if (n_steps) nxt = load4(0u, threadIdx.x * 4u);
      // the last, partial step's records are asked for now as well (a short region is two loads: both in flight)
      const uint32_t tail_j = (n_steps * PG_WG + threadIdx.x) * 4u;
      const uint32_t tail_nv = tail_j < n ? (n - tail_j < 4u ? n - tail_j : 4u) : 0u;
      uint4 tailv = make_uint4(0u, 0u, 0u, 0u);
      if (tail_nv) tailv = load4(0u, tail_j);  // (a quad never straddles a block; its tail past n is ignored)
      for (uint32_t step = 0; step < n_steps; ++step) {
        const uint4 cur = nxt;
        if (step + 1 < n_steps) nxt = load4(0u, ((step + 1) * PG_WG + threadIdx.x) * 4u);
        body(step, cur, 4u, std::false_type{});
      }
      if (n_steps * STEP < n)  // the page's last, partial step: lanes past the end sit it out
        body(n_steps, tailv, tail_nv, std::true_type{});
    } else {
      auto next_seg = [&](uint32_t s) -> uint32_t {  // the first segment from s on that has a whole step
        while (s < segs && seg_fill(s) < STEP) ++s;
        return s;
      };
      // this thread's quad of partial step t: its records (0: none), where they are
      auto tail_quad = [&](uint32_t t, uint32_t &qs, uint32_t &qj) -> uint32_t {
        const uint32_t q = t * PG_WG + threadIdx.x;
        uint32_t acc = 0, nv = 0;
        for (uint32_t s = 0; s < segs; ++s) {
          const uint32_t ns = seg_fill(s), left = ns & (STEP - 1u), quads = (left + 3u) >> 2;
          if (q - acc < quads) {  // (q < acc wraps: no)
            const uint32_t o = (q - acc) * 4u;
            nv = left - o < 4u ? left - o : 4u;
            qs = s;
            qj = (ns & ~(STEP - 1u)) + o;
          }
          acc += quads;
        }
        return nv;
      };
      uint32_t tail_quads = 0;
      for (uint32_t s = 0; s < segs; ++s) tail_quads += ((seg_fill(s) & (STEP - 1u)) + 3u) >> 2;
      const uint32_t tail_steps = (tail_quads + PG_WG - 1u) / PG_WG;
      uint4 nxt;
      uint32_t ls = next_seg(0), lj = 0;  // the load in flight: segment, step inside it
      uint32_t lw = ls < segs ? seg_fill(ls) / STEP : 0u;  // … and that segment's whole steps (no cursor is read inside the loop)
      if (ls < segs) nxt = load4(ls, threadIdx.x * 4u);
      // the first partial step's records are asked for now as well (a short region is two loads: both in flight)
      uint32_t qs = 0, qj = 0;
      uint32_t tail_nv = tail_quad(0, qs, qj);
      uint4 tailv = make_uint4(0u, 0u, 0u, 0u);
      if (tail_nv) tailv = load4(qs, qj);  // (a quad never straddles a block; its tail past the segment's end is ignored)
      uint32_t step = 0;  // steps of this lane so far (the early drains are for a page's first steps)
      while (ls < segs) {
        const uint4 cur = nxt;
        if (++lj == lw) {
          ls = next_seg(ls + 1), lj = 0;
          lw = ls < segs ? seg_fill(ls) / STEP : 0u;
        }
        if (ls < segs) nxt = load4(ls, (lj * PG_WG + threadIdx.x) * 4u);
        body(step++, cur, 4u, std::false_type{});
      }
      for (uint32_t t = 0; t < tail_steps; ++t) {  // partial steps: lanes past the end sit them out
        const uint4 cur = tailv;
        const uint32_t nv = tail_nv;
        if (t + 1 < tail_steps) {
          tail_nv = tail_quad(t + 1, qs, qj);
          if (tail_nv) tailv = load4(qs, qj);
        }
        body(step++, cur, nv, std::true_type{});
      }
    }
    drain();
    lds_barrier();
    // this pass's counts → the page's counts (saturating), four slots per lane and step; all of a
    // thread's loads are issued before the first is used, and the LDS counts go back to zero on the
    // way (the next chunk lane counts from zero)
    {
      uint4 d[WB];
#pragma unroll
      for (int u = 0; u < WB; ++u) d[u] = reinterpret_cast<const uint4 *>(dl)[threadIdx.x + u * PG_WG];
      if (FRESH) {  // counts start at zero: every quad is written, none is read
#pragma unroll
        for (int u = 0; u < WB; ++u) {
          if (TABLE) reinterpret_cast<uint4 *>(gv)[threadIdx.x + u * PG_WG] = d[u];
          if (d[u].x | d[u].y | d[u].z | d[u].w)
            reinterpret_cast<uint4 *>(dl)[threadIdx.x + u * PG_WG] = make_uint4(0u, 0u, 0u, 0u);
        }
        fold_hist(d);
      }
      if (!FRESH && !prefetch) {
#pragma unroll
        for (int u = 0; u < WB; ++u)
          if (d[u].x | d[u].y | d[u].z | d[u].w) gvv[u] = reinterpret_cast<const uint4 *>(gv)[threadIdx.x + u * PG_WG];
      }
#pragma unroll
      for (int u = 0; u < WB; ++u)
        if (!FRESH && (d[u].x | d[u].y | d[u].z | d[u].w)) {
          uint4 v = gvv[u];
          v.x = sat_add_u32(v.x, d[u].x);
          v.y = sat_add_u32(v.y, d[u].y);
          v.z = sat_add_u32(v.z, d[u].z);
          v.w = sat_add_u32(v.w, d[u].w);
          reinterpret_cast<uint4 *>(gv)[threadIdx.x + u * PG_WG] = v;
          reinterpret_cast<uint4 *>(dl)[threadIdx.x + u * PG_WG] = make_uint4(0u, 0u, 0u, 0u);
        }
    }
    lds_barrier();  // (the counts on their way to HBM are nobody's business in here: the next lane's are elsewhere)
  }
  __syncthreads();
  if (FRESH && TABLE) {  // the page's keys, rebuilt from the tags: home bucket = bucket - d, fingerprint = the tag's upper bits
#pragma unroll
    for (int u = 0; u < LD; ++u) {
      const uint32_t i = threadIdx.x + u * PG_WG;
      const uint2 tg = reinterpret_cast<const uint2 *>(tags)[i];
      const uint32_t t2[2] = {tg.x, tg.y};
      ulonglong2 kv;
      unsigned long long ko[2];
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        ko[q] = EMPTY;
        if (t2[q] != TAG_EMPTY) {
          const uint32_t home = (((2 * i + q) >> 2) - (t2[q] & TAG_FAR)) & (PAGE_SLOTS / 4 - 1);
          const uint32_t rec = (home << fpb) | (t2[q] >> TAG_DB);
          ko[q] = unmix_key((gpage << R) | rec, bits);
        }
      }
      kv.x = ko[0];
      kv.y = ko[1];
      reinterpret_cast<ulonglong2 *>(gk)[i] = kv;
    }
    __syncthreads();
  }
  const uint32_t nnew = pg_wg_sum(n_new, dl);
  if (nnew && threadIdx.x == 0) atomicAdd(&stats->n_distinct, (unsigned long long)nnew);
  if (!TABLE) {
    const uint32_t nsp = pg_wg_sum(n_sp, dl);
    if (threadIdx.x == 0) fh.pspill[page] = nsp;
  }
  if (HIST) {  // the page's share of the totals (k_histo's HistoTotals), one row of ptot
    unsigned long long t4[4] = {0, 0, fh_lane, 0};
    if (HIST == 1) {
#pragma unroll
      for (int i = 0; i < WBH * 4; ++i) {
        t4[0] += cum[i] != 0;
        t4[1] += cum[i];
        t4[3] += cum[i] == 0xFFFFFFFFu;
      }
    } else {  // (one lane: a slot's sum is its count)
      t4[0] = one_unique;
      t4[1] = fh_lane;
      t4[3] = one_sat;
    }
    t4[3] += (unsigned long long)n_high << 32;  // word 3: low half = saturated sums (a count here, a flag to the host), high half = adds past the LDS bins
    unsigned long long *red = reinterpret_cast<unsigned long long *>(dl);  // [wave][4]
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      unsigned long long v = t4[j];
      for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
      if ((threadIdx.x & 63) == 0) red[(threadIdx.x >> 6) * 4 + j] = v;
    }
    __syncthreads();
    if (threadIdx.x < 4) {
      unsigned long long v = 0;
      for (int w = 0; w < PG_WG / 64; ++w) v += red[w * 4 + threadIdx.x];
      fh.ptot[(size_t)page * 4 + threadIdx.x] = v;
    }
  }
}

// The rows of a fused page pass (k_pages32<true, true>) summed into the context's histogram and totals — what k_histo
// leaves there.  grid.x covers the (column, bin) pairs, grid.y slices the pages.
__global__ void __launch_bounds__(WG) k_hist_reduce(const uint32_t *__restrict__ partial, const unsigned long long *__restrict__ ptot,
                                                    uint32_t n_pages, uint32_t n_cols, unsigned long long hlen,
                                                    unsigned long long *__restrict__ hist, HistoTotals *__restrict__ tot) {
  const uint32_t per = (n_pages + gridDim.y - 1) / gridDim.y;
  const uint32_t p0 = blockIdx.y * per, p1 = p0 + per < n_pages ? p0 + per : n_pages;
  const uint32_t idx = blockIdx.x * WG + threadIdx.x, n_idx = n_cols * FH_BINS;
  if (idx < n_idx && p0 < p1) {
    const size_t stride = (size_t)n_idx;
    unsigned long long s = 0;
    uint32_t p = p0;
    for (; p + 8 <= p1; p += 8) {  // eight rows' loads in flight together
      uint32_t v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = partial[(size_t)(p + j) * stride + idx];
#pragma unroll
      for (int j = 0; j < 8; ++j) s += v[j];
    }
    for (; p < p1; ++p) s += partial[(size_t)p * stride + idx];
    const uint32_t col = idx / FH_BINS, bin = idx % FH_BINS;
    if (s && bin < hlen) atomicAdd(&hist[(unsigned long long)col * hlen + bin], s);
  }
  if (blockIdx.x == 0 && threadIdx.x < 4 && p0 < p1) {
    unsigned long long v = 0;
    for (uint32_t p = p0; p < p1; ++p) v += ptot[(size_t)p * 4 + threadIdx.x];
    if (v) {
      if (threadIdx.x == 0) atomicAdd(&tot->n_unique, v);
      if (threadIdx.x == 1) atomicAdd(&tot->n_hashed, v);
      if (threadIdx.x == 2) atomicAdd(&tot->n_lane_sum, v);
      if (threadIdx.x == 3) atomicAdd(&tot->any_saturated, v);  // (low half: saturated sums — non-zero is what counts; high half: adds past the LDS bins)
    }
  }
}

// ---- K_INFLATE: the members of a BGZF batch, one wave each ------------------------------------------
// comp: the batch's compressed bytes (4-byte aligned, INFLATE_PAD bytes allocated behind them); jobs[m]: where member
// m's raw DEFLATE body lies in comp and where its text goes in out (the host's prefix sum of ISIZE); status[m]: an
// InfCoreStatus.  A wave's work depends on no other wave's: nothing here waits, and a corrupt stream is a status.  The
// decode itself is shk_inflate_core.h — symbol decode the same in every lane, bytes moved by all 64.
// LDS: sizeof(InfCoreScratch) = 4384 bytes per wave, 17536 per workgroup of INFLATE_WAVES = 4 waves: nine workgroups —
// 36 waves — fit a CU's 160 KiB, so the tables do not hold occupancy under the 8 waves per CU asked for; the 140 VGPRs
// do, at 3 waves per SIMD: 12 waves per CU.
constexpr int INFLATE_WAVES = 4;
constexpr uint32_t INFLATE_PAD = 8;
struct InflateJob {
  unsigned long long in_offset, out_offset;
  uint32_t in_len, out_len;
};
__global__ __launch_bounds__(INFLATE_WAVES * 64) void k_inflate_members(const uint8_t *__restrict__ comp, const InflateJob *__restrict__ jobs,
                                                                         uint32_t n_members, uint8_t *out, uint32_t *__restrict__ status) {
  __shared__ InfCoreScratch scratch[INFLATE_WAVES];
  const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63u;  // (w: the same in the wave)
  const uint32_t m = blockIdx.x * INFLATE_WAVES + w;
  if (m >= n_members) return;  // (the whole wave)
  const InflateJob j = jobs[m];
  const uint32_t st = inflate_member<64>(scratch[w], lane, comp, j.in_offset, j.in_len, out + j.out_offset, j.out_len);
  if (lane == 0) status[m] = st;
}

// ---- K_FASTQ: FASTQ framing and CRC-32 over decoded text in HBM --------------------------------------
// The passes of shk_fastq_text_core.h, one launch each; every launch is done before the next one starts (one stream),
// no workgroup waits for another, plain vector stores, no inline assembly.  The control block is cleared by the host
// (anomaly: all ones) before the first launch.
struct FqCtrl {
  unsigned long long n_nl;     // '\n' in the text (the tile counts' total)
  unsigned long long anomaly;  // fq_anomaly_pack's minimum over the records looked at
  unsigned int any_high;       // a byte >= 0x80 somewhere in the text
  unsigned int ends_nl;        // the text's last byte is '\n'
  unsigned long long n_bases_look;  // the sequence lengths' total over the records looked at
  FqResultWords res;
};
constexpr int FQ_WAVES = 4;       // tiles per workgroup in the tile passes
constexpr int FQ_REC_WG = 256;    // records per workgroup in the record passes
constexpr int FQ_SCAN_WG = 1024;

// Pass 1.  tile_cnt[t]: the '\n' of tile t.
__global__ __launch_bounds__(FQ_WAVES * 64) void k_fq_count(const uint8_t *__restrict__ text, unsigned long long n, unsigned long long n_tiles,
                                                            unsigned long long *__restrict__ tile_cnt, FqCtrl *ctrl) {
  const unsigned long long t = (unsigned long long)blockIdx.x * FQ_WAVES + (threadIdx.x >> 6);
  if (t >= n_tiles) return;  // (the whole wave)
  const FqWave<64> W{threadIdx.x & 63u};
  bool high;
  const uint32_t cnt = fq_tile_count(W, text, n, t, &high);
  if (W.lane == 0) {
    tile_cnt[t] = cnt;
    if (high) atomicOr(&ctrl->any_high, 1u);
    if (t == n_tiles - 1) ctrl->ends_nl = text[n - 1] == '\n';
  }
}

// Exclusive scan of in[0, n) into out[0, n) and the total into *total, by ONE workgroup (n is a text's tiles, or a
// batch's records / FQ_REC_WG: tens of thousands at most).  out may be in.
__global__ __launch_bounds__(FQ_SCAN_WG) void k_fq_scan64(const unsigned long long *in, unsigned long long *out, unsigned long long n,
                                                          unsigned long long *total) {
  __shared__ unsigned long long wsum[FQ_SCAN_WG / 64];
  __shared__ unsigned long long carry_s;
  const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  if (threadIdx.x == 0) carry_s = 0;
  __syncthreads();
  for (unsigned long long i0 = 0; i0 < n; i0 += FQ_SCAN_WG) {
    const unsigned long long i = i0 + threadIdx.x;
    const unsigned long long v = i < n ? in[i] : 0ull;
    unsigned long long inc = v;  // inclusive within the wave
    for (int off = 1; off < 64; off <<= 1) {
      const unsigned long long u = __shfl_up(inc, off, 64);
      if ((int)lane >= off) inc += u;
    }
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    unsigned long long before = carry_s;
    for (uint32_t k = 0; k < w; ++k) before += wsum[k];
    if (i < n) out[i] = before + inc - v;
    __syncthreads();
    if (threadIdx.x == FQ_SCAN_WG - 1) carry_s = before + inc;
    __syncthreads();
  }
  if (threadIdx.x == 0) *total = carry_s;
}

// Pass 3.  line_end[L]: the position of the '\n' that ends line L.
__global__ __launch_bounds__(FQ_WAVES * 64) void k_fq_lines(const uint8_t *__restrict__ text, unsigned long long n, unsigned long long n_tiles,
                                                            const unsigned long long *__restrict__ tile_base, uint32_t *__restrict__ line_end,
                                                            unsigned long long n_lines_cap) {
  const unsigned long long t = (unsigned long long)blockIdx.x * FQ_WAVES + (threadIdx.x >> 6);
  if (t >= n_tiles) return;
  const FqWave<64> W{threadIdx.x & 63u};
  fq_tile_lines(W, text, n, t, tile_base[t], line_end, n_lines_cap);
}

// Pass 4.  Per record its sequence's start and length, the anomalies that need no look at the bases, and per workgroup
// the lengths' sum.
__global__ __launch_bounds__(FQ_REC_WG) void k_fq_records(const uint8_t *__restrict__ text, unsigned long long n, const uint32_t *__restrict__ line_end,
                                                          unsigned long long n_nl, unsigned long long n_look, unsigned long long first_record,
                                                          unsigned long long validate_every, FqCtrl *ctrl, uint32_t *__restrict__ seq_start,
                                                          uint32_t *__restrict__ seq_len, unsigned long long *__restrict__ blk_sum) {
  __shared__ unsigned long long wsum[FQ_REC_WG / 64];
  const unsigned long long j = (unsigned long long)blockIdx.x * FQ_REC_WG + threadIdx.x;
  uint32_t len = 0;
  if (j < n_look) {
    uint64_t s;
    const uint32_t kind = fq_record(text, n, line_end, n_nl, j, fq_validates(first_record + j, validate_every), ctrl->any_high != 0, &s, &len);
    seq_start[j] = (uint32_t)s;
    seq_len[j] = len;
    if (kind) atomicMin(&ctrl->anomaly, (unsigned long long)fq_anomaly_pack(j, kind));
  }
  unsigned long long v = len;
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  if ((threadIdx.x & 63u) == 0) wsum[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long s = 0;
    for (int k = 0; k < FQ_REC_WG / 64; ++k) s += wsum[k];
    blk_sum[blockIdx.x] = s;
  }
}

// offsets[j] = blk_base[workgroup] + the lengths in front of j within it; offsets[n_look]: the total.  (n_look == 0:
// one workgroup, which writes offsets[0] = 0.)
__global__ __launch_bounds__(FQ_REC_WG) void k_fq_offsets(const uint32_t *__restrict__ seq_len, const unsigned long long *__restrict__ blk_base,
                                                          unsigned long long n_look, unsigned long long *__restrict__ offsets) {
  __shared__ unsigned long long wsum[FQ_REC_WG / 64];
  const unsigned long long j = (unsigned long long)blockIdx.x * FQ_REC_WG + threadIdx.x;
  if (n_look == 0) {
    if (j == 0) offsets[0] = 0;
    return;  // (the whole grid)
  }
  const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  const unsigned long long v = j < n_look ? seq_len[j] : 0u;
  unsigned long long inc = v;
  for (int off = 1; off < 64; off <<= 1) {
    const unsigned long long u = __shfl_up(inc, off, 64);
    if ((int)lane >= off) inc += u;
  }
  if (lane == 63) wsum[w] = inc;
  __syncthreads();
  unsigned long long before = blk_base[blockIdx.x];
  for (uint32_t k = 0; k < w; ++k) before += wsum[k];
  if (j < n_look) {
    offsets[j] = before + inc - v;
    if (j == n_look - 1) offsets[n_look] = before + inc;
  }
}

// Pass 5.  FQ_COPY_LANES lanes per record copy its sequence and check its bases.
__global__ __launch_bounds__(256) void k_fq_copy(const uint8_t *__restrict__ text, const uint32_t *__restrict__ seq_start,
                                                 const uint32_t *__restrict__ seq_len, const unsigned long long *__restrict__ offsets,
                                                 unsigned long long n_look, uint8_t *__restrict__ bases, unsigned long long bases_cap, FqCtrl *ctrl) {
  const unsigned long long j = ((unsigned long long)blockIdx.x * 256 + threadIdx.x) / FQ_COPY_LANES;
  if (j >= n_look) return;
  const bool bad = fq_copy_sequence<FQ_COPY_LANES>(text, seq_start[j], seq_len[j], bases, offsets[j], bases_cap, threadIdx.x % FQ_COPY_LANES);
  if (bad) atomicMin(&ctrl->anomaly, (unsigned long long)fq_anomaly_pack(j, FQ_ANOMALY_BASE));
}

// Pass 6.
__global__ void k_fq_finish(unsigned long long n, const uint32_t *__restrict__ line_end, unsigned long long n_nl, unsigned long long n_look,
                            const unsigned long long *__restrict__ offsets, FqCtrl *ctrl) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    ctrl->n_bases_look = offsets[n_look];
    ctrl->res = fq_result(n, line_end, n_nl, n_look, (const uint64_t *)offsets, ctrl->anomaly);
  }
}

// CRC-32 of the members of a batch's decoded text, one wave each: crc[m] over text[jobs[m].offset, + jobs[m].len).
struct FqCrcJob {
  unsigned long long offset;
  uint32_t len, reserved;
};
__global__ __launch_bounds__(FQ_WAVES * 64) void k_crc_members(const uint8_t *__restrict__ text, const FqCrcJob *__restrict__ jobs, uint32_t n_members,
                                                               uint32_t *__restrict__ crc) {
  __shared__ uint32_t tab[256];
  tab[threadIdx.x] = fq_crc_table_entry(threadIdx.x);  // (FQ_WAVES * 64 == 256 threads: an entry each)
  __syncthreads();
  const uint32_t m = blockIdx.x * FQ_WAVES + (threadIdx.x >> 6);
  if (m >= n_members) return;  // (the whole wave)
  const FqWave<64> W{threadIdx.x & 63u};
  const FqCrcJob j = jobs[m];
  const uint32_t raw = W.bit_xor(fq_crc_share(tab, text + j.offset, j.len, W.lane));
  if (W.lane == 0) crc[m] = fq_crc_condition(raw, j.len);
}
static_assert(FQ_WAVES * 64 == 256 && FQ_CRC_SHARES == 64, "k_crc_members: a table entry per thread, a share per lane");

}  // namespace shk
