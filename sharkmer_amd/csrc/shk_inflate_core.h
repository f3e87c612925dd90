// shk_inflate_core.h — one BGZF member's raw DEFLATE body decoded into an output slot of exactly ISIZE bytes: the body of
// k_inflate_members (K_INFLATE in shk_device.hip.h).  Plain C++ that compiles for the host as well, with
// one lane in the place of the wave, so that a stand-alone driver can run it over damaged input under the sanitizers
// (tests/native/inflate_core_driver.cpp).
//
// One WAVE decodes one member.  Symbol decode is serial: the bit buffer, the positions and every branch are the same
// in all lanes (each lane computes them; the tables are read from LDS at one address, a broadcast).  The lanes differ
// only where bytes move: the compressed body comes in 256 bytes at a time (a dword per lane) into a two-half ring in
// LDS, literals gather in an LDS stage and leave 64 to a store, a match is copied 64 bytes to a step — its source lies
// in what the member has already put out, so an overlapping match (distance < length; distance 1 is a run of one byte)
// reads byte (i mod distance) of that and needs no second pass.
//
// What it promises for ARBITRARY input bytes:
//   * reads of the compressed bytes stay inside the dwords that hold [in_off, in_off + in_len) — at most
//     INFC_IN_SLACK bytes in front of and behind the extent (`base` is 4-byte aligned);
//   * writes stay inside [out, out + out_len); a match never reaches in front of `out` (the history is the member's own);
//   * it terminates: every pass of the symbol loop takes at least one input bit, and the bits taken are checked against
//     in_len after every symbol and every header; a block's table set-up is bounded by the alphabet sizes (≤ 320 code
//     lengths, ≤ 1024 + 256 table entries) and a block costs at least 10 bits.  There is no loop that waits for anything.
// A stream may decode "ok" to wrong bytes after damage: the member's CRC-32 (checked by the caller) is what catches that.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define SHK_HD __host__ __device__
#else
#define SHK_HD
#endif

#if defined(__HIP_DEVICE_COMPILE__)
// LDS and global accesses of one wave are performed in program order; this keeps the compiler from reordering them
#define SHK_INFC_SYNC()                                   \
  do {                                                    \
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); \
    __builtin_amdgcn_wave_barrier();                      \
  } while (0)
// What is read from LDS at one address by every lane is the same in every lane; saying so (the first lane's value) keeps
// the bit buffer, the positions and the branches of the symbol loop in scalar registers.  Only where all lanes run.
#define SHK_INFC_UNIFORM(x) ((uint32_t)__builtin_amdgcn_readfirstlane((int)(x)))
#else
#define SHK_INFC_SYNC() \
  do {                  \
  } while (0)
#define SHK_INFC_UNIFORM(x) ((uint32_t)(x))
#endif

#if defined(SHK_INFC_COUNT_STEPS)
#define SHK_INFC_STEP(n) (S.steps += (uint64_t)(n))
#else
#define SHK_INFC_STEP(n) ((void)0)
#endif

namespace shk {

enum InfCoreStatus : uint32_t {
  INFC_OK = 0,               // the final block ended in the body's last byte with exactly out_len bytes written
  INFC_CORRUPT = 1,          // not a DEFLATE stream (or a match that reaches in front of the member)
  INFC_INPUT_EXHAUSTED = 2,  // the stream wants more than in_len bytes
  INFC_OUTPUT_OVER = 3,      // the stream holds more than out_len bytes
  INFC_OUTPUT_SHORT = 4,     // the stream ended with fewer than out_len bytes
  INFC_INPUT_LEFT = 5,       // the stream ended in front of the body's last byte (the trailer is not where BSIZE says)
  INFC_NOT_RUN = 0xFFFFFFFFu // (what a caller fills the status words with: no wave has been there)
};

constexpr uint32_t INFC_IN_SLACK = 3;     // bytes in front of and behind a member's compressed extent that may be read
constexpr uint32_t INFC_MEMBER_MAX = 65536;  // BGZF: a member's body and its decoded text are at most this long
constexpr int INFC_LBITS = 10, INFC_DBITS = 8, INFC_PBITS = 7;

// One wave's working memory (LDS in the kernel, the stack in the host shim): 4384 bytes.
struct InfCoreScratch {
  uint32_t ring[128];     // two halves of 256 compressed bytes
  uint16_t lfast[1u << INFC_LBITS];  // first INFC_LBITS bits of the stream → symbol << 4 | code length (0: longer, or no code)
  uint16_t dfast[1u << INFC_DBITS];  // distances; the code length code (INFC_PBITS bits) while a dynamic header is read
  uint16_t lsym[288], dsym[32];      // symbols in canonical order (the codes longer than the fast tables' bits)
  uint16_t lcount[16], dcount[16];   // code words per length
  uint16_t offs[16];
  uint8_t lens[320];                 // a block's code lengths: 288 literal/length, 32 distance
  uint8_t stage[256];                // literals not stored yet
#if defined(SHK_INFC_COUNT_STEPS)
  uint64_t steps = 0;
#endif
};

template <int LANES>
struct InfCore {
  InfCoreScratch &S;
  const uint32_t lane;
  const uint32_t *in32;  // the dword that holds the member's first byte
  uint32_t lead;         // that byte's place in it
  uint32_t n_dw;         // dwords that hold the extent
  uint64_t in_bits;
  uint64_t bb = 0;
  uint32_t bc = 0, ip = 0;
  uint8_t *out;
  uint32_t out_len, opos = 0, nlit = 0;  // opos: bytes put out, the staged literals included
  bool fixed_built = false;

  SHK_HD InfCore(InfCoreScratch &s, uint32_t l, const uint8_t *base, uint64_t in_off, uint32_t in_len, uint8_t *o, uint32_t olen)
      : S(s), lane(l), in32((const uint32_t *)(base + (in_off & ~(uint64_t)3))), lead((uint32_t)(in_off & 3)),
        n_dw((uint32_t)(((uint64_t)(in_off & 3) + in_len + 3) >> 2)), in_bits((uint64_t)in_len * 8), out(o), out_len(olen) {}

  // ---- the compressed bytes ----------------------------------------------------------------------------------------
  SHK_HD void load_chunk(uint32_t c) {  // dwords [64c, 64c + 64) of the member → ring half c & 1 (zero behind the extent)
    for (uint32_t l = lane; l < 64; l += LANES) {
      const uint32_t d = c * 64 + l;
      S.ring[(c & 1) * 64 + l] = d < n_dw ? in32[d] : 0u;
    }
    SHK_INFC_STEP(1);
  }
  SHK_HD void refill() {  // afterwards bc > 32
    if (bc <= 32) {
      bb |= (uint64_t)SHK_INFC_UNIFORM(S.ring[ip & 127]) << bc;
      bc += 32;
      ++ip;
      if ((ip & 63) == 0) {  // entering a half: the one behind it is free for the chunk after this one
        SHK_INFC_SYNC();
        load_chunk((ip >> 6) + 1);
        SHK_INFC_SYNC();
      }
    }
  }
  SHK_HD void seek_byte(uint32_t pos) {  // pos: bytes from in32
    ip = pos >> 2;
    const uint32_t c = ip >> 6;
    SHK_INFC_SYNC();
    load_chunk(c);
    load_chunk(c + 1);
    SHK_INFC_SYNC();
    bb = 0;
    bc = 0;
    refill();
    drop((pos & 3) * 8);
  }
  SHK_HD uint64_t consumed() const { return (uint64_t)ip * 32 - (uint64_t)lead * 8 - bc; }
  SHK_HD bool exhausted() const { return consumed() > in_bits; }
  SHK_HD void drop(uint32_t n) {
    bb >>= n;
    bc -= n;
  }
  SHK_HD uint32_t take(uint32_t n) {  // n ≤ 16, bc ≥ n
    const uint32_t v = (uint32_t)bb & ((1u << n) - 1u);
    drop(n);
    return v;
  }

  // ---- code tables -------------------------------------------------------------------------------------------------
  static SHK_HD uint32_t bitrev(uint32_t v, uint32_t n) {
    uint32_t r = 0;
    for (uint32_t i = 0; i < n; ++i) r |= ((v >> i) & 1u) << (n - 1 - i);
    return r;
  }
  // Canonical code of lens[0, n) → count[], sym[] and the fast table of `fb` bits.  false: over-subscribed, or
  // incomplete with more than one code word in use (the rule of shk_inflate.cpp's build_table).
  SHK_HD bool build(const uint8_t *lens, uint32_t n, uint16_t *count, uint16_t *sym, uint16_t *fast, uint32_t fb) {
    for (uint32_t i = lane; i < (1u << fb); i += LANES) fast[i] = 0;
    for (uint32_t l = 0; l < 16; ++l) count[l] = 0;
    SHK_INFC_SYNC();
    uint32_t used = 0;
    for (uint32_t s = 0; s < n; ++s) {
      const uint32_t l = SHK_INFC_UNIFORM(lens[s]);
      count[l] = (uint16_t)(SHK_INFC_UNIFORM(count[l]) + 1);
      used += l != 0;
    }
    SHK_INFC_STEP(n + 32);
    int left = 1;
    for (uint32_t l = 1; l <= 15; ++l) {
      left <<= 1;
      left -= (int)SHK_INFC_UNIFORM(count[l]);
      if (left < 0) return false;
    }
    if (left > 0 && used > 1) return false;
    count[0] = 0;
    {
      uint32_t o = 0;
      for (uint32_t l = 1; l <= 15; ++l) {
        S.offs[l] = (uint16_t)o;
        o += SHK_INFC_UNIFORM(count[l]);
      }
    }
    for (uint32_t s = 0; s < n; ++s) {
      const uint32_t l = SHK_INFC_UNIFORM(lens[s]);
      if (l) {
        const uint32_t at = SHK_INFC_UNIFORM(S.offs[l]);
        sym[at] = (uint16_t)s;
        S.offs[l] = (uint16_t)(at + 1);
      }
    }
    SHK_INFC_STEP(n);
    // the fast table, in canonical order: at most 2^fb entries are written in all
    uint32_t code = 0, idx = 0;
    for (uint32_t l = 1; l <= fb; ++l) {
      const uint32_t cn = SHK_INFC_UNIFORM(count[l]);
      for (uint32_t k = 0; k < cn; ++k) {
        const uint32_t e = (SHK_INFC_UNIFORM(sym[idx++]) << 4) | l;
        for (uint32_t j = bitrev(code, l); j < (1u << fb); j += 1u << l) {
          fast[j] = (uint16_t)e;
          SHK_INFC_STEP(1);
        }
        ++code;
      }
      code <<= 1;
    }
    SHK_INFC_SYNC();
    return true;
  }
  // The next symbol (bc ≥ 15 … the caller has refilled), or -1 where no code word matches.
  SHK_HD int decode(const uint16_t *count, const uint16_t *sym, const uint16_t *fast, uint32_t fb) {
    const uint32_t e = SHK_INFC_UNIFORM(fast[(uint32_t)bb & ((1u << fb) - 1u)]);
    if (e & 15u) {
      drop(e & 15u);
      return (int)(e >> 4);
    }
    uint32_t code = 0, first = 0, index = 0;
    uint64_t b = bb;
    for (uint32_t l = 1; l <= 15; ++l) {  // (a code longer than fb bits: bit by bit, the canonical way)
      code |= (uint32_t)b & 1u;
      b >>= 1;
      const uint32_t cn = SHK_INFC_UNIFORM(count[l]);
      if (code < first + cn) {
        drop(l);
        return (int)SHK_INFC_UNIFORM(sym[index + (code - first)]);
      }
      index += cn;
      first = (first + cn) << 1;
      code <<= 1;
    }
    SHK_INFC_STEP(15);
    return -1;
  }

  // ---- the output ---------------------------------------------------------------------------------------------------
  SHK_HD void flush() {
    if (!nlit) return;
    SHK_INFC_SYNC();
    uint8_t *o = out + (opos - nlit);
    for (uint32_t i = lane; i < nlit; i += LANES) o[i] = S.stage[i];
    SHK_INFC_SYNC();
    nlit = 0;
  }

  SHK_HD uint32_t fixed_tables() {
    if (fixed_built) return INFC_OK;
    for (uint32_t i = lane; i < 320; i += LANES) S.lens[i] = i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : i < 288 ? 8 : 5;
    SHK_INFC_SYNC();
    build(S.lens, 288, S.lcount, S.lsym, S.lfast, INFC_LBITS);
    build(S.lens + 288, 32, S.dcount, S.dsym, S.dfast, INFC_DBITS);
    fixed_built = true;
    return INFC_OK;
  }
  SHK_HD uint32_t dynamic_tables() {
    fixed_built = false;
    refill();
    const uint32_t hlit = take(5) + 257, hdist = take(5) + 1, hclen = take(4) + 4;
    // the order in which the code length code's own lengths are sent, five bits each
    const uint64_t ord_lo = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 | 6ull << 35 | 10ull << 40 | 5ull << 45 |
                            11ull << 50 | 4ull << 55;
    const uint64_t ord_hi = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
    for (uint32_t i = lane; i < 320; i += LANES) S.lens[i] = 0;
    SHK_INFC_SYNC();
    for (uint32_t i = 0; i < hclen; ++i) {
      refill();
      const uint32_t s = (uint32_t)((i < 12 ? ord_lo >> (5 * i) : ord_hi >> (5 * (i - 12))) & 31u);
      S.lens[s] = (uint8_t)take(3);
    }
    SHK_INFC_STEP(hclen);
    SHK_INFC_SYNC();
    if (exhausted()) return INFC_INPUT_EXHAUSTED;
    if (!build(S.lens, 19, S.dcount, S.dsym, S.dfast, INFC_PBITS)) return INFC_CORRUPT;
    SHK_INFC_SYNC();
    for (uint32_t i = lane; i < 19; i += LANES) S.lens[i] = 0;
    SHK_INFC_SYNC();
    // literal/length lengths go to lens[0, hlit), distance lengths to lens[288, 288 + hdist): one run of hlit + hdist
    const uint32_t total = hlit + hdist;
    uint32_t i = 0, prev = 0;
    while (i < total) {
      refill();
      const int s = decode(S.dcount, S.dsym, S.dfast, INFC_PBITS);
      SHK_INFC_STEP(1);
      if (s < 0) return exhausted() ? INFC_INPUT_EXHAUSTED : INFC_CORRUPT;
      uint32_t rep = 1, v = (uint32_t)s;
      if (s == 16) {
        if (i == 0) return INFC_CORRUPT;
        rep = 3 + take(2);
        v = prev;
      } else if (s == 17) {
        rep = 3 + take(3);
        v = 0;
      } else if (s == 18) {
        rep = 11 + take(7);
        v = 0;
      }
      if (exhausted()) return INFC_INPUT_EXHAUSTED;
      if (i + rep > total) return INFC_CORRUPT;
      for (uint32_t k = 0; k < rep; ++k, ++i) S.lens[i < hlit ? i : 288 + (i - hlit)] = (uint8_t)v;
      SHK_INFC_STEP(rep);
      prev = v;
    }
    SHK_INFC_SYNC();
    if (!build(S.lens, 288, S.lcount, S.lsym, S.lfast, INFC_LBITS)) return INFC_CORRUPT;
    if (!build(S.lens + 288, 32, S.dcount, S.dsym, S.dfast, INFC_DBITS)) return INFC_CORRUPT;
    return INFC_OK;
  }

  SHK_HD uint32_t stored_block() {
    drop(bc & 7);
    refill();
    const uint32_t len = take(16), nlen = take(16);
    if (exhausted()) return INFC_INPUT_EXHAUSTED;
    if ((len ^ 0xFFFFu) != nlen) return INFC_CORRUPT;
    const uint32_t from = ip * 4 - (bc >> 3);  // bytes from in32
    if ((uint64_t)from - lead + len > in_bits / 8) return INFC_INPUT_EXHAUSTED;
    if (len > out_len - opos) return INFC_OUTPUT_OVER;
    flush();
    const uint8_t *src = (const uint8_t *)in32 + from;
    uint8_t *o = out + opos;
    for (uint32_t i = lane; i < len; i += LANES) o[i] = src[i];
    SHK_INFC_STEP(len / LANES + 1);
    opos += len;
    seek_byte(from + len);
    return INFC_OK;
  }

  SHK_HD uint32_t huffman_block() {
    for (;;) {
      refill();
      const int s = decode(S.lcount, S.lsym, S.lfast, INFC_LBITS);
      SHK_INFC_STEP(1);
      if (s < 0) return exhausted() ? INFC_INPUT_EXHAUSTED : INFC_CORRUPT;
      if (s < 256) {
        if (exhausted()) return INFC_INPUT_EXHAUSTED;
        if (opos >= out_len) return INFC_OUTPUT_OVER;
        S.stage[nlit++] = (uint8_t)s;
        ++opos;
        if (nlit == 256) flush();
        continue;
      }
      if (s == 256) return exhausted() ? INFC_INPUT_EXHAUSTED : INFC_OK;
      if (s >= 286) return INFC_CORRUPT;
      uint32_t len;
      {
        const uint32_t t = (uint32_t)s - 257;
        if (t < 8) len = 3 + t;
        else if (t == 28) len = 258;
        else {
          const uint32_t eb = (t >> 2) - 1;
          len = 3 + ((4 + (t & 3)) << eb) + take(eb);
        }
      }
      refill();
      const int d = decode(S.dcount, S.dsym, S.dfast, INFC_DBITS);
      if (d < 0) return exhausted() ? INFC_INPUT_EXHAUSTED : INFC_CORRUPT;
      if (d >= 30) return INFC_CORRUPT;
      uint32_t dist;
      if (d < 4) dist = 1 + (uint32_t)d;
      else {
        const uint32_t eb = ((uint32_t)d >> 1) - 1;
        dist = 1 + ((2 + ((uint32_t)d & 1)) << eb) + take(eb);
      }
      if (exhausted()) return INFC_INPUT_EXHAUSTED;
      if (dist > opos) return INFC_CORRUPT;  // (in front of the member: its history is its own)
      if (len > out_len - opos) return INFC_OUTPUT_OVER;
      flush();
      uint8_t *o = out + opos;
      const uint8_t *src = o - dist;
      if (dist >= len) {
        for (uint32_t i = lane; i < len; i += LANES) o[i] = src[i];
      } else {  // overlapping: the pattern of `dist` bytes repeats
        for (uint32_t i = lane; i < len; i += LANES) o[i] = src[i % dist];
      }
      SHK_INFC_SYNC();
      opos += len;
    }
  }

  SHK_HD uint32_t run() {
    seek_byte(lead);
    for (;;) {
      refill();
      const uint32_t last = take(1), type = take(2);
      if (exhausted()) return INFC_INPUT_EXHAUSTED;
      uint32_t st;
      if (type == 0) {
        st = stored_block();
      } else if (type == 1) {
        st = fixed_tables();
        if (st == INFC_OK) st = huffman_block();
      } else if (type == 2) {
        st = dynamic_tables();
        if (st == INFC_OK) st = huffman_block();
      } else {
        st = INFC_CORRUPT;
      }
      SHK_INFC_STEP(1);
      if (st != INFC_OK) {
        flush();  // (what was decoded in front of the damage: inside the slot, every staged byte was checked against out_len)
        return st;
      }
      if (last) break;
    }
    flush();
    if (opos != out_len) return INFC_OUTPUT_SHORT;
    return (consumed() + 7) / 8 == in_bits / 8 ? INFC_OK : INFC_INPUT_LEFT;
  }
};

// Decodes the DEFLATE stream in base[in_off, in_off + in_len) into out[0, out_len) with LANES lanes (every lane of the
// wave calls it with its own `lane` and the same everything else; LANES = 1, lane = 0: the host shim).  `base` is
// 4-byte aligned.  Returns an InfCoreStatus, the same in every lane.
template <int LANES>
SHK_HD inline uint32_t inflate_member(InfCoreScratch &S, uint32_t lane, const uint8_t *base, uint64_t in_off, uint32_t in_len, uint8_t *out,
                                      uint32_t out_len) {
  InfCore<LANES> c(S, lane, base, in_off, in_len, out, out_len);
  return c.run();
}

}  // namespace shk
