// shk_fastq_text_core.h — FASTQ framing and CRC-32 over text that lies in device memory: the bodies of the K_FASTQ
// kernels (shk_device.hip.h).  Plain C++ that compiles for the host as well, with one lane in the wave's
// place, so that a stand-alone driver can run it under the sanitizers (tests/native/fastq_text_driver.cpp).
//
// The framing restates read_fastq / BufRead::lines / validate_fastq_record (src/io.rs:161-198, 271-352) for a text of
// n bytes that holds whole lines:
//   * a line ends with '\n'; its content is what lies in front of that, without a '\r' directly in front of the '\n';
//     with `last` set an unterminated rest is a line too, and a '\r' at its end stays (lines() strips it only together
//     with a '\n');
//   * record j is lines 4j .. 4j + 3; its sequence is line 4j + 1;
//   * record j is an ANOMALY — something the host must decide about — when one of its four lines holds a byte >= 0x80,
//     when its sequence holds a byte outside ACGTN, or, for a record the cadence validates, when the header does not
//     start with '@', the separator not with '+' or the quality's length is not the sequence's.
// The passes: (1) per tile of FQ_TILE bytes the number of '\n' and whether a byte has its high bit set; (2) a scan of
// the tile counts; (3) per tile again, the position of every '\n' into the line table at its global line number;
// (4) per record its sequence's extent and the anomalies that need no look at the bases; a scan of the lengths;
// (5) the copy of the sequences, which also checks the bases; (6) the result words.  The scans are the caller's.
//
// Bounds: a tile reads 16-byte blocks that each hold at least one byte of the text (on the device: aligned 16-byte
// loads, which never leave the 4 KiB page of that byte; on the host: exactly the text's bytes); the line table is
// written below n_lines_cap only; the copy writes below bases_cap only.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define SHK_FQ_HD __host__ __device__
#else
#define SHK_FQ_HD
#endif

namespace shk {

constexpr uint32_t FQ_TILE = 4096;               // bytes of text per tile (one wave)
constexpr uint64_t FQ_TEXT_MAX = 1ull << 31;     // line ends are 32-bit positions
constexpr uint64_t FQ_NO_ANOMALY = ~0ull;
constexpr int FQ_COPY_LANES = 16;                // lanes that copy one sequence

enum FqAnomalyKind : uint32_t {  // (of several in one record the lowest is reported)
  FQ_ANOMALY_NONE = 0,
  FQ_ANOMALY_HIGH_BYTE = 1,   // a byte >= 0x80 in one of the record's four lines
  FQ_ANOMALY_HEADER = 2,      // validated record: the header does not start with '@'
  FQ_ANOMALY_SEPARATOR = 3,   // validated record: the separator does not start with '+'
  FQ_ANOMALY_QUALITY_LEN = 4, // validated record: quality length != sequence length
  FQ_ANOMALY_BASE = 5         // a sequence byte outside ACGTN
};
SHK_FQ_HD inline uint64_t fq_anomaly_pack(uint64_t record, uint32_t kind) { return record << 3 | kind; }

// The wave: lane, ballot and reductions.  LANES == 1 is the host's stand-in.
template <int LANES>
struct FqWave {
  uint32_t lane;
  SHK_FQ_HD uint64_t ballot(bool p) const {
#if defined(__HIP_DEVICE_COMPILE__)
    return __ballot(p);
#else
    return p ? 1ull : 0ull;
#endif
  }
  SHK_FQ_HD uint32_t sum(uint32_t v) const {
#if defined(__HIP_DEVICE_COMPILE__)
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
#endif
    return v;
  }
  SHK_FQ_HD uint32_t bit_xor(uint32_t v) const {
#if defined(__HIP_DEVICE_COMPILE__)
    for (int off = 32; off > 0; off >>= 1) v ^= __shfl_xor(v, off, 64);
#endif
    return v;
  }
};
SHK_FQ_HD inline uint32_t fq_popc32(uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return (uint32_t)__popc(v);
#else
  return (uint32_t)__builtin_popcount(v);
#endif
}
SHK_FQ_HD inline uint32_t fq_popc64(uint64_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return (uint32_t)__popcll(v);
#else
  return (uint32_t)__builtin_popcountll(v);
#endif
}

// ---- a tile's 16-byte blocks ------------------------------------------------------------------------------------------
// Tile t holds the text's bytes [lo, hi) = [t · FQ_TILE, min(n, (t + 1) · FQ_TILE)).  Its blocks are the 16-byte aligned
// blocks of memory that overlap it: block c starts `lead` bytes in front of text + lo, plus 16 c.
struct FqTile {
  uint64_t lo, hi;
  uint32_t lead, n_blocks;
};
SHK_FQ_HD inline FqTile fq_tile(const uint8_t *text, uint64_t n, uint64_t t) {
  FqTile T;
  T.lo = t * FQ_TILE;
  T.hi = T.lo + FQ_TILE < n ? T.lo + FQ_TILE : n;
  T.lead = (uint32_t)((uintptr_t)(text + T.lo) & 15u);
  T.n_blocks = T.hi > T.lo ? (uint32_t)((T.lead + (T.hi - T.lo) + 15) >> 4) : 0u;
  return T;
}
// Block c of the tile: nl — bit j set where byte j is a '\n' of the text; hi — where byte j has its high bit set; both
// only for bytes inside the tile.  *pos0: the text position of the block's byte 0 (may lie in front of the tile: signed).
SHK_FQ_HD inline void fq_block_masks(const uint8_t *text, const FqTile &T, uint32_t c, uint32_t *nl, uint32_t *hi, int64_t *pos0) {
  const int64_t p0 = (int64_t)T.lo - (int64_t)T.lead + 16 * (int64_t)c;
  const int64_t a = (int64_t)T.lo - p0, b = (int64_t)T.hi - p0;
  const uint32_t jlo = a > 0 ? (uint32_t)a : 0u, jhi = b < 16 ? (uint32_t)b : 16u;  // (jlo < jhi: the block overlaps the tile)
  const uint32_t valid = ((1u << jhi) - 1u) & ~((1u << jlo) - 1u);
  uint32_t w[4];
#if defined(__HIP_DEVICE_COMPILE__)
  const uint4 v = *(const uint4 *)(text + p0);  // 16-byte aligned; holds a byte of the text, so it is inside that byte's page
  w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
#else
  w[0] = w[1] = w[2] = w[3] = 0;
  for (uint32_t j = jlo; j < jhi; ++j) w[j >> 2] |= (uint32_t)text[p0 + j] << (8 * (j & 3));
#endif
  uint32_t m_nl = 0, m_hi = 0;
  for (int k = 0; k < 4; ++k) {
    const uint32_t x = w[k] ^ 0x0A0A0A0Au;
    const uint32_t z = ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);  // 0x80 exactly where a byte of x is 0
    const uint32_t h = w[k] & 0x80808080u;
    m_nl |= ((z >> 7 & 1u) | (z >> 14 & 2u) | (z >> 21 & 4u) | (z >> 28 & 8u)) << (4 * k);
    m_hi |= ((h >> 7 & 1u) | (h >> 14 & 2u) | (h >> 21 & 4u) | (h >> 28 & 8u)) << (4 * k);
  }
  *nl = m_nl & valid;
  *hi = m_hi & valid;
  *pos0 = p0;
}

// Pass 1: the tile's number of '\n' (the same in every lane) and whether any of its bytes has the high bit set.
template <int LANES>
SHK_FQ_HD inline uint32_t fq_tile_count(const FqWave<LANES> &W, const uint8_t *text, uint64_t n, uint64_t t, bool *any_high) {
  const FqTile T = fq_tile(text, n, t);
  uint32_t cnt = 0, high = 0;
  for (uint32_t c0 = 0; c0 < T.n_blocks; c0 += LANES) {
    const uint32_t c = c0 + W.lane;
    if (c < T.n_blocks) {
      uint32_t nl, hi;
      int64_t p0;
      fq_block_masks(text, T, c, &nl, &hi, &p0);
      cnt += fq_popc32(nl);
      high |= hi;
    }
  }
  *any_high = W.ballot(high != 0) != 0;
  return W.sum(cnt);
}

// Pass 3: every '\n' of the tile into line_end[] at its global line number (tile_base: the lines in front of the tile).
template <int LANES>
SHK_FQ_HD inline void fq_tile_lines(const FqWave<LANES> &W, const uint8_t *text, uint64_t n, uint64_t t, uint64_t tile_base, uint32_t *line_end,
                                    uint64_t n_lines_cap) {
  const FqTile T = fq_tile(text, n, t);
  uint64_t run = tile_base;  // lines in front of this round's blocks
  const uint64_t below = W.lane ? (~0ull >> (64 - W.lane)) : 0ull;
  for (uint32_t c0 = 0; c0 < T.n_blocks; c0 += LANES) {  // (every lane takes every round: the ballots are the wave's)
    const uint32_t c = c0 + W.lane;
    uint32_t nl = 0, hi;
    int64_t p0 = 0;
    if (c < T.n_blocks) fq_block_masks(text, T, c, &nl, &hi, &p0);
    // the blocks are in lane order, the bytes of a block in bit order: a '\n' comes behind all those of the lanes
    // below and the lower bits of its own block
    uint32_t before = 0, total = 0;
    for (int j = 0; j < 16; ++j) {
      const uint64_t b = W.ballot((nl >> j & 1u) != 0);
      before += fq_popc64(b & below);
      total += fq_popc64(b);
    }
    uint64_t L = run + before;
    for (uint32_t m = nl; m; m &= m - 1, ++L) {
      const uint32_t j = fq_popc32((m & (0u - m)) - 1u);
      if (L < n_lines_cap) line_end[L] = (uint32_t)(p0 + j);
    }
    run += total;
  }
}

// ---- lines and records ------------------------------------------------------------------------------------------------
// Line L of a text with n_nl terminated lines: its content is [*start, *end).  L == n_nl is the unterminated rest.
SHK_FQ_HD inline void fq_line(const uint8_t *text, uint64_t n, const uint32_t *line_end, uint64_t n_nl, uint64_t L, uint64_t *start, uint64_t *end) {
  const uint64_t s = L ? (uint64_t)line_end[L - 1] + 1 : 0;
  uint64_t e;
  if (L < n_nl) {
    e = line_end[L];
    if (e > s && text[e - 1] == '\r') --e;
  } else {
    e = n;
  }
  *start = s;
  *end = e;
}
SHK_FQ_HD inline bool fq_validates(uint64_t global_record, uint64_t validate_every) {
  return global_record == 0 || (validate_every && global_record % validate_every == 0);
}
// Pass 4, record j: the sequence's extent; returns the anomaly kind that needs no look at the bases (0: none).
// scan_high: pass 1 saw a byte >= 0x80 somewhere, so the record's four lines are looked through for one.
SHK_FQ_HD inline uint32_t fq_record(const uint8_t *text, uint64_t n, const uint32_t *line_end, uint64_t n_nl, uint64_t j, bool validate, bool scan_high,
                                    uint64_t *seq_start, uint32_t *seq_len) {
  uint64_t s1, e1;
  fq_line(text, n, line_end, n_nl, 4 * j + 1, &s1, &e1);
  *seq_start = s1;
  *seq_len = (uint32_t)(e1 - s1);
  uint32_t kind = FQ_ANOMALY_NONE;
  if (validate) {  // (highest kind first: the lowest one stays)
    uint64_t s, e;
    fq_line(text, n, line_end, n_nl, 4 * j + 3, &s, &e);
    if (e - s != e1 - s1) kind = FQ_ANOMALY_QUALITY_LEN;
    fq_line(text, n, line_end, n_nl, 4 * j + 2, &s, &e);
    if (e == s || text[s] != '+') kind = FQ_ANOMALY_SEPARATOR;
    fq_line(text, n, line_end, n_nl, 4 * j, &s, &e);
    if (e == s || text[s] != '@') kind = FQ_ANOMALY_HEADER;
  }
  if (scan_high) {
    const uint64_t a = j ? (uint64_t)line_end[4 * j - 1] + 1 : 0;
    const uint64_t b = 4 * j + 3 < n_nl ? (uint64_t)line_end[4 * j + 3] : n;
    for (uint64_t i = a; i < b; ++i)
      if (text[i] & 0x80) {
        kind = FQ_ANOMALY_HIGH_BYTE;
        break;
      }
  }
  return kind;
}
SHK_FQ_HD inline bool fq_is_acgtn(uint8_t c) { return c == 'A' || c == 'C' || c == 'G' || c == 'T' || c == 'N'; }
// Pass 5, record j by GROUP lanes (sub: this lane's index among them): the sequence to bases[off ..), below bases_cap
// only.  Returns whether this lane met a byte outside ACGTN.
template <int GROUP>
SHK_FQ_HD inline bool fq_copy_sequence(const uint8_t *text, uint64_t seq_start, uint32_t seq_len, uint8_t *bases, uint64_t off, uint64_t bases_cap,
                                       uint32_t sub) {
  bool bad = false;
  for (uint32_t i = sub; i < seq_len; i += GROUP) {
    const uint8_t ch = text[seq_start + i];
    bad |= !fq_is_acgtn(ch);
    if (off + i < bases_cap) bases[off + i] = ch;
  }
  return bad;
}

// Pass 6: what the call answers.  n_look: the records looked at, min(whole records, max_records); offsets[0 .. n_look]
// as scanned; anomaly: the packed minimum (FQ_NO_ANOMALY: none).
struct FqResultWords {
  uint64_t n_records, n_bases, bytes_consumed, anomaly_record;
  uint32_t anomaly_kind, reserved;
};
SHK_FQ_HD inline FqResultWords fq_result(uint64_t n, const uint32_t *line_end, uint64_t n_nl, uint64_t n_look, const uint64_t *offsets, uint64_t anomaly) {
  FqResultWords r;
  r.anomaly_record = anomaly == FQ_NO_ANOMALY ? FQ_NO_ANOMALY : anomaly >> 3;
  r.anomaly_kind = anomaly == FQ_NO_ANOMALY ? (uint32_t)FQ_ANOMALY_NONE : (uint32_t)(anomaly & 7u);
  r.reserved = 0;
  r.n_records = r.anomaly_record < n_look ? r.anomaly_record : n_look;
  r.n_bases = offsets[r.n_records] - offsets[0];
  r.bytes_consumed = r.n_records == 0 ? 0 : (4 * r.n_records - 1 < n_nl ? (uint64_t)line_end[4 * r.n_records - 1] + 1 : n);
  return r;
}
// The lines of a text with n_nl '\n' (last: an unterminated rest counts) and the records to look at.
SHK_FQ_HD inline uint64_t fq_n_lines(uint64_t n, uint64_t n_nl, bool last, bool ends_with_newline) {
  return n_nl + ((last && n && !ends_with_newline) ? 1 : 0);
}

// ---- CRC-32 (IEEE, reflected) -----------------------------------------------------------------------------------------
// A member's CRC from 64 contiguous shares: lane i computes the RAW remainder (register 0 at the start, no final
// inversion) of its share; raw(A ‖ B) = raw(A) · x^(8·|B|) ⊕ raw(B), so the member's raw remainder is the XOR of the
// shares' remainders, each multiplied by x^(8 · bytes behind the share) mod P.  The conditioning — the register starts
// as 0xFFFFFFFF and is inverted at the end — is crc = raw ⊕ 0xFFFFFFFF · x^(8·len) ⊕ 0xFFFFFFFF, applied once.
constexpr uint32_t FQ_CRC_POLY = 0xEDB88320u;
constexpr int FQ_CRC_SHARES = 64;
SHK_FQ_HD inline uint32_t fq_crc_table_entry(uint32_t i) {
  uint32_t c = i;
  for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ FQ_CRC_POLY : c >> 1;
  return c;
}
// a · b mod P (reflected: bit 31 is x^0)
SHK_FQ_HD inline uint32_t fq_crc_mul(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (uint32_t m = 1u << 31; m; m >>= 1) {
    if (a & m) p ^= b;
    b = (b & 1u) ? (b >> 1) ^ FQ_CRC_POLY : b >> 1;
  }
  return p;
}
SHK_FQ_HD inline uint32_t fq_crc_xpow8(uint64_t n_bytes) {  // x^(8 · n_bytes) mod P
  uint32_t r = 1u << 31, b = 1u << 23;  // x^0, x^8
  for (; n_bytes; n_bytes >>= 1) {
    if (n_bytes & 1) r = fq_crc_mul(r, b);
    b = fq_crc_mul(b, b);
  }
  return r;
}
SHK_FQ_HD inline uint32_t fq_crc_raw(const uint32_t *tab, const uint8_t *p, uint64_t len) {
  uint32_t c = 0;
  while (len && ((uintptr_t)p & 3u)) c = tab[(c ^ *p++) & 0xFFu] ^ (c >> 8), --len;
  for (; len >= 4; len -= 4, p += 4) {
    uint32_t w;
    __builtin_memcpy(&w, p, 4);  // (p is 4-byte aligned here: one dword load)
    c ^= w;
    for (int k = 0; k < 4; ++k) c = tab[c & 0xFFu] ^ (c >> 8);
  }
  while (len) c = tab[(c ^ *p++) & 0xFFu] ^ (c >> 8), --len;
  return c;
}
// Share `share` (of FQ_CRC_SHARES) of a member of len bytes at p: its part of the member's raw remainder.  tab: the 256
// entries of fq_crc_table_entry.
SHK_FQ_HD inline uint32_t fq_crc_share(const uint32_t *tab, const uint8_t *p, uint32_t len, uint32_t share) {
  const uint32_t per = (len + FQ_CRC_SHARES - 1) / FQ_CRC_SHARES;
  const uint64_t a = (uint64_t)per * share;
  if (a >= len) return 0;
  const uint64_t b = a + per < len ? a + per : len;
  return fq_crc_mul(fq_crc_raw(tab, p + a, b - a), fq_crc_xpow8(len - b));
}
SHK_FQ_HD inline uint32_t fq_crc_condition(uint32_t raw, uint32_t len) { return raw ^ fq_crc_mul(0xFFFFFFFFu, fq_crc_xpow8(len)) ^ 0xFFFFFFFFu; }

#if !defined(__HIP_DEVICE_COMPILE__)
// ---- the passes strung together, serially (the host's stand-in for the launches; the scans are plain loops) -----------
// line_end: room for n_lines_cap entries; bases: bases_cap bytes; offsets: offsets_cap entries.  Returns false, with
// r->n_records the records looked at, when a capacity is too small for them (nothing is written beyond any).
struct FqSerialParams {
  uint64_t first_record, validate_every, max_records;
  bool last;
};
inline bool fq_parse_serial(const uint8_t *text, uint64_t n, const FqSerialParams &p, uint32_t *line_end, uint64_t n_lines_cap, uint8_t *bases,
                            uint64_t bases_cap, uint64_t *offsets, uint64_t offsets_cap, FqResultWords *r) {
  const FqWave<1> W{0};
  const uint64_t n_tiles = (n + FQ_TILE - 1) / FQ_TILE;
  uint64_t n_nl = 0;
  bool any_high = false;
  for (uint64_t t = 0; t < n_tiles; ++t) {
    bool h;
    n_nl += fq_tile_count(W, text, n, t, &h);
    any_high |= h;
  }
  *r = FqResultWords{};
  r->anomaly_record = FQ_NO_ANOMALY;
  if (n_nl > n_lines_cap) return false;
  uint64_t base = 0;
  for (uint64_t t = 0; t < n_tiles; ++t) {
    bool h;
    const uint32_t cnt = fq_tile_count(W, text, n, t, &h);
    fq_tile_lines(W, text, n, t, base, line_end, n_lines_cap);
    base += cnt;
  }
  const uint64_t n_lines = fq_n_lines(n, n_nl, p.last, n && text[n - 1] == '\n');
  uint64_t n_look = n_lines / 4;
  if (p.max_records && n_look > p.max_records) n_look = p.max_records;
  r->n_records = n_look;
  if (n_look + 1 > offsets_cap) return false;
  uint64_t anomaly = FQ_NO_ANOMALY, off = 0;
  for (uint64_t j = 0; j < n_look; ++j) {
    uint64_t s;
    uint32_t len;
    const uint32_t kind = fq_record(text, n, line_end, n_nl, j, fq_validates(p.first_record + j, p.validate_every), any_high, &s, &len);
    if (kind && fq_anomaly_pack(j, kind) < anomaly) anomaly = fq_anomaly_pack(j, kind);
    offsets[j] = off;
    bool bad = false;
    for (uint32_t sub = 0; sub < (uint32_t)FQ_COPY_LANES; ++sub) bad |= fq_copy_sequence<FQ_COPY_LANES>(text, s, len, bases, off, bases_cap, sub);
    if (bad && fq_anomaly_pack(j, FQ_ANOMALY_BASE) < anomaly) anomaly = fq_anomaly_pack(j, FQ_ANOMALY_BASE);
    off += len;
  }
  offsets[n_look] = off;
  *r = fq_result(n, line_end, n_nl, n_look, offsets, anomaly);
  return r->n_bases <= bases_cap;
}
#endif

}  // namespace shk
