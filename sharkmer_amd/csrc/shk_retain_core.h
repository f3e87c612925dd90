// shk_retain_core.h — the retained read store's arithmetic: where a base lies, the loader of a wave step's planes and
// the decode back to ASCII (K_RETAIN, the plane walks of K_FILTER_PANEL and K_THREAD in shk_device.hip.h; DESIGN.md
// §17).  Plain C++ that compiles for the host as well, so a stand-alone driver can run it against a scalar model
// under the sanitizers (tests/native/retain_driver.cpp).
//
// The store is three arrays of 64-bit words, p0, p1 and nn: bit P % 64 of word P / 64 describes base P of the
// concatenation of every retained read — code bit 0, code bit 1 (code = ((c >> 1) ^ (c >> 2)) & 3: A 0, C 1, G 2, T 3;
// 00 where the base is N) and "is N".  Bits at and beyond the store's end are zero, and RETAIN_SLACK_WORDS words
// follow the word of the last base: the loader reads word + 1 of a step that may start up to 63 bases behind a read.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define SHK_HD __host__ __device__
#else
#define SHK_HD
#endif

namespace shk {

constexpr uint64_t RETAIN_SLACK_WORDS = 2;

// words of one plane of a store of n_bases bases, slack included: what the loader may read
SHK_HD inline uint64_t retain_words(uint64_t n_bases) { return (n_bases + 63) / 64 + RETAIN_SLACK_WORDS; }

// a base's code as the counting kernels and read_planes form it (valid for ACGT; N is coded 00 by its callers)
SHK_HD inline uint32_t retain_code(uint32_t c) { return ((c >> 1) ^ (c >> 2)) & 3u; }

// bits sh … sh + 63 of the 128-bit value hi:lo (sh < 64; sh = 0 shifts nothing by 64)
SHK_HD inline uint64_t retain_window(uint64_t lo, uint64_t hi, uint32_t sh) { return (lo >> sh) | ((hi << 1) << (63u - sh)); }

// The 64 bits of plane W from read position s of the read that starts at absolute bit b0 and has len bases: bit l is
// position s + l.  Positions at and beyond len read as 0 — code 00 and no N, what read_planes returns there.
// s <= len + 63: the two words lie within retain_words() of the store.
SHK_HD inline uint64_t retain_plane(const uint64_t *W, uint64_t b0, uint32_t s, uint32_t len) {
  const uint64_t A = b0 + s, w = A >> 6;
  const uint32_t left = len > s ? len - s : 0u;
  const uint64_t mask = left >= 64u ? ~0ull : (1ull << left) - 1ull;
  return retain_window(W[w], W[w + 1], (uint32_t)(A & 63u)) & mask;
}

// base j (j < 16) of 16-bit slices of the three planes, as ASCII
SHK_HD inline uint8_t retain_ascii(uint32_t p0, uint32_t p1, uint32_t nn, uint32_t j) {
  const uint32_t code = ((p0 >> j) & 1u) | (((p1 >> j) & 1u) << 1);
  return (nn >> j) & 1u ? (uint8_t)'N' : (uint8_t)(0x54474341u >> (8u * code));  // T G C A
}

}  // namespace shk
