// shk_dedup_core.h — "is the Levenshtein distance of two 2-bit packed sequences <= t" for one pair, the body of a
// K_DEDUP lane (shk_products_api.hip.h).  Plain C++ that compiles for the host as well, so a stand-alone driver can run
// it against the full matrix (tests/native/dedup_driver.cpp).
//
// Landau-Vishkin / Ukkonen: L[d] is the furthest row of a reached on diagonal d = j - i with e differences; level e
// takes each diagonal one difference further from its three neighbours and then slides along matching bases, 32 at a
// time (xor of two 64-bit windows, count of trailing zeros).  Work is O(t^2) slides plus the matched length / 32,
// where a banded DP — bit-parallel or not — pays for every column of a 2500-base record.  Exact for any
// lengths below 2^30 and any t the caller's slots hold: every stored row is a cell that e differences reach, and at
// level e only diagonals that can still come home to lb - la within t - e differences are advanced, which no
// alignment of at most t differences ever leaves.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define SHK_HD __host__ __device__
#else
#define SHK_HD
#endif

namespace shk {

constexpr uint32_t DEDUP_MAX_T = 31;             // 2t + 3 <= 65 slots per lane
constexpr uint32_t DEDUP_MAX_LEN = 1u << 30;     // rows are int32
constexpr int32_t DEDUP_NEG = -(1 << 30);        // "no cell reached"

// words a packed record of len bases takes: base p at bits 2(p & 31) of word p >> 5, zero bits above the last base,
// and room for the window that starts AT len
SHK_HD inline uint64_t dedup_words(uint64_t len) { return (len >> 5) + 2; }

// the 32 bases from position x (x <= len)
SHK_HD inline uint64_t dedup_window(const uint64_t *w, uint32_t x) {
  const uint32_t s = (x & 31u) * 2u;
  const uint64_t lo = w[x >> 5];
  return s ? (lo >> s) | (w[(x >> 5) + 1] << (64u - s)) : lo;
}

// from cell (i, i + d): the row after the run of equal bases
SHK_HD inline int32_t dedup_slide(const uint64_t *a, int32_t la, const uint64_t *b, int32_t lb, int32_t i, int32_t d) {
  int32_t room = la - i < lb - (i + d) ? la - i : lb - (i + d);
  while (room > 0) {
    const uint64_t x = dedup_window(a, (uint32_t)i) ^ dedup_window(b, (uint32_t)(i + d));
    const int32_t same = x ? (int32_t)(__builtin_ctzll(x) >> 1) : 32;
    if (same >= room) return i + room;
    if (same < 32) return i + same;
    i += 32, room -= 32;
  }
  return i;
}

// L: this pair's 2t + 3 slots, slot s at L[s * stride] (diagonal d in slot d + t + 1, a never-reached slot at either end)
SHK_HD inline bool dedup_within(const uint64_t *a, int32_t la, const uint64_t *b, int32_t lb, int32_t t, int32_t *L, uint32_t stride) {
  const int32_t D = lb - la;
  if (D > t || -D > t) return false;
  if (t >= (la > lb ? la : lb)) return true;
  for (int32_t s = 0; s < 2 * t + 3; ++s) L[(uint32_t)s * stride] = DEDUP_NEG;
  int32_t i = dedup_slide(a, la, b, lb, 0, 0);
  if (D == 0 && i == la) return true;
  L[(uint32_t)(t + 1) * stride] = i;
  for (int32_t e = 1; e <= t; ++e) {
    const int32_t rem = t - e;
    const int32_t d0 = -e > D - rem ? -e : D - rem, d1 = e < D + rem ? e : D + rem;
    int32_t left = L[(uint32_t)(d0 + t) * stride];  // diagonal d0 - 1 before this level
    for (int32_t d = d0; d <= d1; ++d) {
      const uint32_t s = (uint32_t)(d + t + 1);
      const int32_t mid = L[s * stride], right = L[(s + 1) * stride];
      i = mid + 1;                         // substitution
      if (left > i) i = left;              // a base of b alone: from diagonal d - 1, same row
      if (right + 1 > i) i = right + 1;    // a base of a alone: from diagonal d + 1, next row
      left = mid;
      const int32_t end = la < lb - d ? la : lb - d;
      if (i > end) i = end;
      if (i < 0) continue;                 // nothing reaches this diagonal yet (or it lies outside the matrix)
      i = dedup_slide(a, la, b, lb, i, d);
      L[s * stride] = i;
      if (d == D && i == la) return true;
    }
  }
  return false;
}

// Pair p of the row-major upper triangle of m records (m >= 2, p < m(m - 1) / 2) -> (i, j), i < j: row i starts at
// i(2m - i - 1) / 2; the root of the quadratic, put right by steps (at most 22 of them for any m below 2^31, where
// the doubles run out of bits)
SHK_HD inline uint64_t dedup_row_start(uint64_t i, uint64_t m) { return i * (2 * m - i - 1) / 2; }
SHK_HD inline void dedup_pair_of(uint64_t p, uint64_t m, uint64_t *pi, uint64_t *pj) {
  const double b = (double)(2 * m - 1);
  uint64_t i = (uint64_t)((b - sqrt(b * b - 8.0 * (double)p)) * 0.5);
  if (i > m - 2) i = m - 2;
  while (dedup_row_start(i, m) > p) --i;
  while (i + 2 < m && dedup_row_start(i + 1, m) <= p) ++i;
  *pi = i, *pj = i + 1 + (p - dedup_row_start(i, m));
}

}  // namespace shk
