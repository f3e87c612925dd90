// retain_driver — the retained read store's loader and decode (sharkmer_amd/csrc/shk_retain_core.h: retain_plane,
// retain_window, retain_ascii — the code the plane walks of K_FILTER_PANEL / K_THREAD and K_RETAINED_EXPORT run)
// compiled for the host and run against a scalar model, under AddressSanitizer and UBSan:
//   make -C sharkmer_amd/csrc retain_driver && sharkmer_amd/csrc/retain_driver
// Reads are packed with a plain loop into plane arrays allocated at EXACTLY retain_words() words — the two-word slack
// rule — so a load past what the rule allows is a heap overflow the sanitizer reports.  Every read is placed at every
// start alignment 0..63, last in the store and with reads behind it; every step s the contract allows (s <= len + 63) is
// loaded and compared with read_planes' definition over the ASCII bytes (position s + l: its code bits and N, zero at
// and beyond len); then the store is decoded back 16 bases at a time, as the export kernel does.
// Prints "ok <reads> <steps>" and exits 0, or the first difference and exits 1.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "shk_retain_core.h"

namespace {

struct Store {
  uint64_t n_bases = 0, n_words = 0;
  std::unique_ptr<uint64_t[]> p0, p1, nn;  // exactly retain_words(n_bases) words each
};

// the model of K_RETAIN: one base after the other
Store pack(const std::string &all) {
  Store st;
  st.n_bases = all.size();
  st.n_words = shk::retain_words(st.n_bases);
  st.p0.reset(new uint64_t[st.n_words]());
  st.p1.reset(new uint64_t[st.n_words]());
  st.nn.reset(new uint64_t[st.n_words]());
  for (uint64_t p = 0; p < all.size(); ++p) {
    const uint32_t c = (uint8_t)all[p];
    const uint64_t bit = 1ull << (p & 63);
    if (c == 'N') {
      st.nn[p >> 6] |= bit;
      continue;
    }
    uint32_t code = 0;
    switch (c) {  // (spelled out: the model does not share retain_code with the code under test)
      case 'A': code = 0; break;
      case 'C': code = 1; break;
      case 'G': code = 2; break;
      case 'T': code = 3; break;
      default: fprintf(stderr, "the driver packs ACGTN only\n"); exit(2);
    }
    if (code & 1) st.p0[p >> 6] |= bit;
    if (code & 2) st.p1[p >> 6] |= bit;
  }
  return st;
}

// read_planes' definition: bit l describes position s + l of the read; 'A' (code 00, no N) at and beyond len
void model_planes(const std::string &read, uint32_t s, uint64_t *m0, uint64_t *m1, uint64_t *mn) {
  *m0 = *m1 = *mn = 0;
  for (uint32_t l = 0; l < 64; ++l) {
    const uint64_t p = (uint64_t)s + l;
    const char c = p < read.size() ? read[p] : 'A';
    const uint64_t bit = 1ull << l;
    if (c == 'N') *mn |= bit;
    if (c == 'C' || c == 'T') *m0 |= bit;
    if (c == 'G' || c == 'T') *m1 |= bit;
  }
}

uint64_t n_reads_done = 0, n_steps_done = 0;

bool check(const std::string &filler, const std::string &read, const std::string &behind) {
  const std::string all = filler + read + behind;
  const Store st = pack(all);
  const uint64_t b0 = filler.size();
  const uint32_t len = (uint32_t)read.size();
  for (uint32_t s = 0; s <= len + 63; ++s) {
    uint64_t m0, m1, mn;
    model_planes(read, s, &m0, &m1, &mn);
    const uint64_t g0 = shk::retain_plane(st.p0.get(), b0, s, len), g1 = shk::retain_plane(st.p1.get(), b0, s, len),
                   gn = shk::retain_plane(st.nn.get(), b0, s, len);
    ++n_steps_done;
    if (g0 != m0 || g1 != m1 || gn != mn) {
      printf("planes differ: start bit %llu, len %u, step %u, %zu bases behind: got %016llx %016llx %016llx, want %016llx %016llx %016llx\n",
             (unsigned long long)b0, len, s, behind.size(), (unsigned long long)g0, (unsigned long long)g1, (unsigned long long)gn,
             (unsigned long long)m0, (unsigned long long)m1, (unsigned long long)mn);
      return false;
    }
  }
  // the export: bases [b0, b0 + len) back, 16 at a time (a group's window reads word + 1 as well)
  std::string back(len, '?');
  for (uint64_t q = 0; q < len; q += 16) {
    const uint64_t A = b0 + q, w = A >> 6;
    const uint32_t sh = (uint32_t)(A & 63);
    const uint32_t a0 = (uint32_t)shk::retain_window(st.p0[w], st.p0[w + 1], sh) & 0xFFFFu,
                   a1 = (uint32_t)shk::retain_window(st.p1[w], st.p1[w + 1], sh) & 0xFFFFu,
                   an = (uint32_t)shk::retain_window(st.nn[w], st.nn[w + 1], sh) & 0xFFFFu;
    for (uint32_t j = 0; j < 16 && q + j < len; ++j) back[q + j] = (char)shk::retain_ascii(a0, a1, an, j);
  }
  if (back != read) {
    printf("decode differs: start bit %llu, len %u: got %s, want %s\n", (unsigned long long)b0, len, back.c_str(), read.c_str());
    return false;
  }
  ++n_reads_done;
  return true;
}

}  // namespace

int main() {
  std::mt19937_64 rng(20261019);
  auto rand_seq = [&](size_t n, double p_n) {
    std::string s(n, 'A');
    for (auto &c : s) c = (rng() % 1000) < p_n * 1000 ? 'N' : "ACGT"[rng() % 4];
    return s;
  };
  std::vector<std::string> reads;
  // crafted: the lengths around a word and a wave step, one base repeated (every plane all ones or all zeros), N at the edges
  for (size_t len : {0, 1, 2, 20, 21, 22, 63, 64, 65, 84, 127, 128, 129, 149, 150, 192, 193, 300}) {
    reads.push_back(rand_seq(len, 0.0));
    reads.push_back(rand_seq(len, 0.1));
    for (char c : {'A', 'C', 'G', 'T', 'N'}) reads.push_back(std::string(len, c));
  }
  for (size_t at : {0, 1, 62, 63, 64, 65, 127, 128, 149}) {
    std::string s(150, 'T');
    s[at] = 'N';
    reads.push_back(s);
  }
  for (int i = 0; i < 60; ++i) reads.push_back(rand_seq(rng() % 260, (i % 3) * 0.05));
  for (const std::string &read : reads)
    for (size_t a = 0; a < 64; ++a) {
      const std::string filler = rand_seq(a + 64 * (rng() % 3), 0.05);
      // last in the store — once with the filler all T, so that bits of the read before leak into a wrong window as ones
      if (!check(filler, read, "")) return 1;
      if (!check(std::string(filler.size(), 'T'), read, "")) return 1;
      // reads behind it: what the tail mask has to hide
      if (!check(filler, read, std::string(1 + rng() % 200, 'T'))) return 1;
      if (!check(filler, read, rand_seq(1 + rng() % 200, 0.3))) return 1;
    }
  printf("ok %llu %llu\n", (unsigned long long)n_reads_done, (unsigned long long)n_steps_done);
  return 0;
}
