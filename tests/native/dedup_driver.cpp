// dedup_driver.cpp — a native caller of the dedup's pair decision: shk_edit_within (the host route) and
// shk::dedup_within (the body of a K_DEDUP lane, compiled for the host) against the full Levenshtein matrix, built
// under AddressSanitizer and UBSan by `make -C sharkmer_amd/csrc dedup_driver`.  Exit status 0 and "ok" when every
// pair agrees.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../include/shk.h"
#include "../../sharkmer_amd/csrc/shk_dedup_core.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
  rng_state ^= rng_state << 13, rng_state ^= rng_state >> 7, rng_state ^= rng_state << 17;
  return rng_state;
}

static uint64_t full_distance(const std::string &a, const std::string &b) {
  std::vector<uint64_t> prev(b.size() + 1), cur(b.size() + 1);
  for (size_t j = 0; j <= b.size(); ++j) prev[j] = j;
  for (size_t i = 1; i <= a.size(); ++i) {
    cur[0] = i;
    for (size_t j = 1; j <= b.size(); ++j) cur[j] = std::min({prev[j - 1] + (a[i - 1] != b[j - 1]), prev[j] + 1, cur[j - 1] + 1});
    prev.swap(cur);
  }
  return prev[b.size()];
}

static std::vector<uint64_t> pack(const std::string &s) {
  std::vector<uint64_t> w(shk::dedup_words(s.size()), 0);  // exactly the words the kernel may read: ASan sees one more
  for (size_t p = 0; p < s.size(); ++p) {
    const uint64_t code = s[p] == 'A' ? 0 : s[p] == 'C' ? 1 : s[p] == 'G' ? 2 : 3;
    w[p >> 5] |= code << (2 * (p & 31));
  }
  return w;
}

static std::string random_seq(size_t n, unsigned alphabet) {
  std::string s(n, 'A');
  for (auto &ch : s) ch = "ACGT"[rnd() % alphabet];
  return s;
}

static std::string mutate(std::string s, unsigned edits) {
  for (unsigned e = 0; e < edits; ++e) {
    const unsigned kind = rnd() % 3;
    const size_t at = s.empty() ? 0 : rnd() % (s.size() + (kind == 1));
    if (kind == 0 && !s.empty())
      s[at] = "ACGT"[rnd() % 4];
    else if (kind == 1)
      s.insert(s.begin() + at, "ACGT"[rnd() % 4]);
    else if (!s.empty())
      s.erase(s.begin() + at);
  }
  return s;
}

static long checked = 0;
static int check(const std::string &a, const std::string &b, uint64_t t) {
  const uint64_t dist = full_distance(a, b);
  const int want = dist <= t;
  const int host = shk_edit_within((const uint8_t *)a.data(), a.size(), (const uint8_t *)b.data(), b.size(), (uint32_t)t);
  int bad = host != want;
  if (t <= shk::DEDUP_MAX_T) {
    const std::vector<uint64_t> pa = pack(a), pb = pack(b);
    const uint32_t stride = 3;  // (a stride as on the device, where the lanes' slots interleave)
    std::vector<int32_t> L((2 * t + 3) * stride, 0);
    const int dev = shk::dedup_within(pa.data(), (int32_t)a.size(), pb.data(), (int32_t)b.size(), (int32_t)t, L.data() + 1, stride);
    bad |= dev != want;
    if (dev != want) fprintf(stderr, "dedup_within %d, distance %llu, t %llu\n", dev, (unsigned long long)dist, (unsigned long long)t);
  }
  if (host != want) fprintf(stderr, "shk_edit_within %d, distance %llu, t %llu\n", host, (unsigned long long)dist, (unsigned long long)t);
  if (bad) fprintf(stderr, "  a=%s\n  b=%s\n", a.c_str(), b.c_str());
  ++checked;
  return bad;
}

int main() {
  int bad = 0;
  const size_t lens[] = {0, 1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129};
  const uint64_t ts[] = {0, 1, 2, 10, 31, 32, 4294967295ull};
  for (const size_t la : lens)
    for (const size_t lb : lens)
      for (const uint64_t t : ts)
        for (int rep = 0; rep < 3; ++rep) {
          const std::string a = random_seq(la, rep == 0 ? 1 : 4);
          bad += check(a, random_seq(lb, rep == 0 ? 1 : 4), t);
          bad += check(a, mutate(a, (unsigned)std::min<uint64_t>(t, 40)), t);
          bad += check(a, mutate(a, (unsigned)std::min<uint64_t>(t, 40) + 1), t);
        }
  for (int it = 0; it < 20000 && !bad; ++it) {
    const std::string a = random_seq(rnd() % 200, 1 + rnd() % 4);
    const unsigned edits = rnd() % 40;
    const std::string b = rnd() % 4 ? mutate(a, edits) : random_seq(rnd() % 200, 1 + rnd() % 4);
    bad += check(a, b, rnd() % 36);
    bad += check(a, b, full_distance(a, b));                                // exactly t
    if (full_distance(a, b)) bad += check(a, b, full_distance(a, b) - 1);   // t + 1
  }
  for (uint64_t t = 0; t <= 33; ++t) {  // t insertions at the head against t deletions at the tail; a length difference of t, t + 1
    const std::string core = random_seq(150, 4);
    bad += check(random_seq(t, 4) + core, core + random_seq(t, 4), t);
    bad += check(random_seq(t, 4) + core, core + random_seq(t, 4), 2 * t);
    bad += check(core, core + random_seq(t, 4), t);
    bad += check(core, core + random_seq(t + 1, 4), t);
  }
  for (int it = 0; it < 40 && !bad; ++it) {  // long records
    const std::string a = random_seq(2500 + rnd() % 10, 4);
    const std::string b = mutate(a, rnd() % 14);
    bad += check(a, b, 10);
  }
  for (uint64_t m = 2; m <= 400 && !bad; ++m) {  // the kernel's pair index -> (i, j): every pair of small sets
    uint64_t p = 0;
    for (uint64_t i = 0; i + 1 < m; ++i)
      for (uint64_t j = i + 1; j < m; ++j, ++p) {
        uint64_t gi, gj;
        shk::dedup_pair_of(p, m, &gi, &gj);
        bad += gi != i || gj != j;
      }
  }
  for (int it = 0; it < 300000 && !bad; ++it) {  // and of sets up to 2^31 records, the triangle's two ends among them
    const uint64_t m = 2 + rnd() % ((1ull << 31) - 3), n = m * (m - 1) / 2;
    const uint64_t p = it % 3 == 0 ? rnd() % n : it % 3 == 1 ? n - 1 - rnd() % 5 % n : rnd() % 5 % n;
    uint64_t gi, gj;
    shk::dedup_pair_of(p, m, &gi, &gj);
    bad += !(gi < gj && gj < m && shk::dedup_row_start(gi, m) + (gj - gi - 1) == p);
  }
  printf("%s: %ld pairs\n", bad ? "FAILED" : "ok", checked);
  return bad ? 1 : 0;
}
