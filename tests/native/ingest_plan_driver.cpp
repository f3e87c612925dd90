// ingest_plan_driver — what a host-buffer ingest decides and runs without a device (sharkmer_amd/csrc/shk_ingest_plan.h:
// reads_within / slice_cuts, StageRing, PackedExtent, HostPackLayout, nmask_nonzero, HostPacker) against linear-scan
// models, as a stand-alone program under AddressSanitizer and UBSan, and under ThreadSanitizer for the packer thread:
//   make -C sharkmer_amd/csrc ingest_plan_driver ingest_plan_driver_tsan
//   sharkmer_amd/csrc/ingest_plan_driver && sharkmer_amd/csrc/ingest_plan_driver_tsan
// Every buffer the code under test writes is allocated at exactly the size its contract names, so a store past it is a
// heap overflow the sanitizer reports.  Prints "ok <checks>" and exits 0, or the first difference and exits 1.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "shk_ingest_plan.h"

namespace {

constexpr int NST = 6;  // shk_ctx::NST, the most staging sets a call takes
uint64_t n_checks = 0;

#define CHECK(cond, ...)                          \
  do {                                            \
    ++n_checks;                                   \
    if (!(cond)) {                                \
      fprintf(stdout, "FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); \
      fprintf(stdout, __VA_ARGS__);               \
      fprintf(stdout, "\n");                      \
      exit(1);                                    \
    }                                             \
  } while (0)

using U64 = unsigned long long;

std::vector<uint64_t> offsets_of(const std::vector<uint32_t> &lens, uint64_t first = 0) {
  std::vector<uint64_t> o{first};
  for (uint32_t l : lens) o.push_back(o.back() + l);
  return o;
}

// ---- the slice cuts ---------------------------------------------------------------------------------------------------
uint64_t first_limit(uint64_t slice_bases, bool quarter) { return quarter ? (slice_bases / 4 ? slice_bases / 4 : 1) : slice_bases; }

// the model: one read after the other, as long as the slice stays within its limit
std::vector<uint64_t> model_cuts(const std::vector<uint64_t> &o, uint64_t slice_bases, bool quarter) {
  const uint64_t n = o.size() - 1;
  std::vector<uint64_t> cut{0};
  while (cut.back() < n) {
    const uint64_t lo = cut.back(), limit = lo == 0 ? first_limit(slice_bases, quarter) : slice_bases;
    uint64_t hi = lo + 1;  // (at least one read)
    while (hi < n && o[hi + 1] - o[lo] <= limit) ++hi;
    cut.push_back(hi);
  }
  return cut;
}

void check_cuts(const char *family, const std::vector<uint64_t> &o) {
  const uint64_t n = o.size() - 1, total = o[n] - o[0];
  for (uint64_t slice_bases : {(uint64_t)1, (uint64_t)7, (uint64_t)1024, (uint64_t)65536, total + 1})
    for (bool quarter : {false, true}) {
      const std::vector<uint64_t> cut = shk::slice_cuts(o.data(), n, slice_bases, quarter);
      CHECK(cut.size() >= 2 && cut[0] == 0 && cut.back() == n, "%s slice %llu q%d", family, (U64)slice_bases, quarter);
      for (size_t i = 0; i + 1 < cut.size(); ++i) {
        const uint64_t lo = cut[i], hi = cut[i + 1], limit = lo == 0 ? first_limit(slice_bases, quarter) : slice_bases;
        CHECK(hi > lo, "%s slice %llu q%d: cut %zu not increasing", family, (U64)slice_bases, quarter, i);
        CHECK(o[hi] - o[lo] <= limit || hi == lo + 1, "%s slice %llu q%d: slice %zu over its limit", family, (U64)slice_bases, quarter, i);
        CHECK(hi == n || o[hi + 1] - o[lo] > limit, "%s slice %llu q%d: slice %zu not maximal", family, (U64)slice_bases, quarter, i);
        CHECK(shk::reads_within(o.data(), lo, n, limit) == hi, "%s reads_within", family);
      }
      CHECK(cut == model_cuts(o, slice_bases, quarter), "%s slice %llu q%d: not the model's cuts", family, (U64)slice_bases, quarter);
    }
}

void check_all_cuts() {
  std::mt19937_64 rng(20251);
  check_cuts("uniform", offsets_of(std::vector<uint32_t>(1000, 150)));
  {
    // empty reads in front, behind, and where the 1024-base limit falls (the reads before the run hold exactly 1024 and
    // 7 bases more than a multiple of it: the run sits on the limit of one slice size and inside another's)
    std::vector<uint32_t> lens(5, 0);
    for (int i = 0; i < 4; ++i) lens.push_back(256);
    for (int i = 0; i < 3; ++i) lens.push_back(0);
    lens.push_back(7);
    for (int i = 0; i < 4; ++i) lens.push_back(0);
    for (int i = 0; i < 1500; ++i) {
      lens.push_back((uint32_t)(rng() % 301));
      if (rng() % 16 == 0)
        for (int j = 0, m = 1 + (int)(rng() % 5); j < m; ++j) lens.push_back(0);
    }
    for (int i = 0; i < 6; ++i) lens.push_back(0);
    check_cuts("ragged", offsets_of(lens));
    check_cuts("ragged from 12345", offsets_of(lens, 12345));
  }
  {
    std::vector<uint32_t> lens{100, 0, 200000, 0, 0, 50, 70000, 3};  // reads longer than every slice size but the last
    check_cuts("long read", offsets_of(lens));
    check_cuts("long read first", offsets_of({300000, 10, 0}));
  }
  check_cuts("offsets[0] = 12345", offsets_of(std::vector<uint32_t>(300, 101), 12345));
  check_cuts("one base first", offsets_of({1, 0, 0, 5, 1, 1, 0, 3}));  // (a quarter of a tiny slice is one base, not none)
  check_cuts("one read", offsets_of({150}));
  check_cuts("one empty read", offsets_of({0}, 99));
  check_cuts("all empty", offsets_of(std::vector<uint32_t>(77, 0)));
  check_cuts("all empty from 12345", offsets_of(std::vector<uint32_t>(77, 0), 12345));
}

// ---- the ring of staging sets -------------------------------------------------------------------------------------------
void check_ring() {
  for (int max_sets = 2; max_sets <= NST; ++max_sets)
    for (int stage_last = -1; stage_last < NST; ++stage_last)
      for (size_t n_slices = 1; n_slices <= 9; ++n_slices) {
        const shk::StageRing ring(n_slices, stage_last, max_sets);
        const int want = (int)n_slices + 1 < max_sets ? (int)n_slices + 1 : max_sets;
        CHECK(ring.nst == want && ring.nst >= 2 && ring.nst <= NST, "nst %d for %zu slices of %d sets", ring.nst, n_slices, max_sets);
        CHECK(ring.set_of(0) == (int)ring.s0 && (int)ring.s0 != stage_last, "s0 %u after %d", ring.s0, stage_last);
        CHECK(stage_last < 0 || stage_last >= ring.nst || (int)ring.s0 == (stage_last + 1) % ring.nst, "s0 %u does not follow %d", ring.s0, stage_last);
        for (size_t i = 0; i < 3 * (size_t)NST; ++i) {
          CHECK(ring.set_of(i) >= 0 && ring.set_of(i) < ring.nst, "set_of(%zu) out of the ring", i);
          for (size_t j = i + 1; j < i + (size_t)ring.nst; ++j)  // slice i's set is not taken again by the nst − 1 slices queued behind it
            CHECK(ring.set_of(i) != ring.set_of(j), "slices %zu and %zu share a set (nst %d)", i, j, ring.nst);
        }
      }
}

// ---- a slice's extents in the packed streams; the host packer's staging -----------------------------------------------------
void check_extents_and_layout() {
  const uint64_t o_rels[] = {0, 1, 3, 31, 32, 33, 12345}, nbs[] = {1, 3, 4, 31, 32, 33, 65537};
  for (uint64_t o_rel : o_rels)
    for (uint64_t nb : nbs) {
      uint64_t b0 = ~0ull, b1 = 0, w0 = ~0ull, w1 = 0;  // the model: every base's byte and word
      for (uint64_t p = o_rel; p < o_rel + nb; ++p) {
        b0 = std::min(b0, p / 4), b1 = std::max(b1, p / 4 + 1);
        w0 = std::min(w0, p / 32), w1 = std::max(w1, p / 32 + 1);
      }
      const shk::PackedExtent x(o_rel, nb);
      CHECK(x.b0 == b0 && x.b1 == b1 && x.w0 == w0 && x.w1 == w1, "extent of %llu bases at %llu", (U64)nb, (U64)o_rel);
    }
  for (uint64_t first : {(uint64_t)0, (uint64_t)12345}) {  // a call whose slices are these sizes, one read each, with empty ones between
    std::vector<uint32_t> lens;
    std::vector<uint64_t> cut{0};
    for (uint64_t nb : nbs) lens.push_back((uint32_t)nb), lens.push_back(0), cut.push_back(lens.size());
    const std::vector<uint64_t> o = offsets_of(lens, first);
    const shk::HostPackLayout lay(o.data(), cut);
    const size_t n = cut.size() - 1;
    CHECK(lay.pk_off.size() == n && lay.nm_off.size() == n, "a stretch per slice");
    for (size_t j = 0; j < n; ++j) {
      uint64_t pb = 0, nw = 0;
      shk_packed_sizes(o[cut[j + 1]] - o[cut[j]], &pb, &nw);
      const size_t pk_end = j + 1 < n ? lay.pk_off[j + 1] : lay.pk_total, nm_end = j + 1 < n ? lay.nm_off[j + 1] : lay.nm_total;
      CHECK(lay.pk_off[j] % 64 == 0 && lay.nm_off[j] % 64 == 0, "slice %zu is not 64-byte aligned", j);
      CHECK(pk_end >= lay.pk_off[j] + pb && nm_end >= lay.nm_off[j] + nw * 4, "slice %zu's stretch is too short or overlaps the next", j);
    }
    CHECK(lay.pk_total % 64 == 0 && lay.nm_total % 64 == 0, "totals");
  }
}

// ---- the list form of a sparse N mask -----------------------------------------------------------------------------------
// the model: the function's contract spelled out one word at a time — a thread's share is [n·t/T, n·(t+1)/T), its
// segment cap/T pairs, T one thread per 2^18 words (at least one, at most eight)
size_t model_nonzero(const uint32_t *w, size_t n, size_t cap, std::vector<uint32_t> *pairs) {
  size_t T = n >> 18;
  T = T < 1 ? 1 : T > 8 ? 8 : T;
  pairs->clear();
  bool over = false;
  for (size_t t = 0; t < T; ++t) {
    size_t k = 0;
    for (size_t i = n * t / T; i < n * (t + 1) / T; ++i)
      if (w[i]) pairs->push_back((uint32_t)i), pairs->push_back(w[i]), ++k;
    over |= k > cap / T;
  }
  return over ? ~(size_t)0 : pairs->size() / 2;
}

void check_one_mask(const char *what, const std::vector<uint32_t> &words, size_t start, size_t n, size_t cap) {
  std::unique_ptr<uint32_t[]> buf(new uint32_t[start + n]);  // the mask ends where the allocation ends; start 1: not 8-byte aligned
  const uint32_t *w = buf.get() + start;
  if (n) memcpy(buf.get() + start, words.data() + start, n * 4);
  std::unique_ptr<uint32_t[]> pairs(new uint32_t[2 * cap]);
  std::vector<uint32_t> want;
  const size_t m = model_nonzero(w, n, cap, &want);
  const size_t got = shk::nmask_nonzero(w, n, pairs.get(), cap);
  CHECK(got == m, "%s: n %zu cap %zu: %zu pairs, the model has %zu", what, n, cap, got, m);
  if (m != ~(size_t)0 && m) CHECK(memcmp(pairs.get(), want.data(), m * 8) == 0, "%s: n %zu cap %zu: other pairs than the model's", what, n, cap);
}

void check_nmask() {
  std::mt19937_64 rng(77);
  const size_t sizes[] = {0, 1, 7, 8, 9, (1u << 18) - 1, 1u << 18, 3 * (1u << 18) + 5};
  const size_t longest = 3 * (1u << 18) + 5 + 1;
  std::vector<uint32_t> none(longest, 0), sparse(longest, 0), all(longest);
  for (auto &x : sparse)
    if (rng() % 50 == 0) x = (uint32_t)rng() | 1u;
  for (auto &x : all) x = (uint32_t)rng() | 1u;
  for (size_t n : sizes)
    for (size_t start : {(size_t)0, (size_t)1}) {  // (1: a slice that starts at an odd word of the caller's mask; the largest size
                                                   // gives its middle thread a share that starts at an odd index)
      const size_t cap = n / 16 + 64;              // what ingest_host gives it
      check_one_mask("none", none, start, n, cap);
      check_one_mask("sparse", sparse, start, n, cap);
      check_one_mask("all", all, start, n, cap);
      check_one_mask("all, room for all", all, start, n, n + 8);
      check_one_mask("sparse, no room", sparse, start, n, 0);
    }
  {
    // three threads, 100 pairs each: 150 non-zero words in the middle thread's share alone are fewer than cap and still
    // more than its segment holds
    const size_t n = 3 * (1u << 18) + 5;
    std::vector<uint32_t> w(n + 1, 0);
    for (size_t i = 0; i < 150; ++i) w[n / 2 + 3 * i] = 0x80000000u >> (i % 32);
    std::vector<uint32_t> want;
    CHECK(model_nonzero(w.data(), n, 300, &want) == ~(size_t)0 && want.size() == 300, "the case is not what it says");
    check_one_mask("one share overflows", w, 0, n, 300);
    check_one_mask("one share overflows by one pair", w, 0, n, 449);
    check_one_mask("one share just fits", w, 0, n, 450);
  }
}

// ---- the packer thread ------------------------------------------------------------------------------------------------------
struct Call {
  std::string bases;
  std::vector<uint64_t> offsets, cut;
  shk::HostPackLayout lay;
  size_t n_slices() const { return cut.size() - 1; }
  uint64_t o0(size_t j) const { return offsets[cut[j]]; }
  uint64_t nb(size_t j) const { return offsets[cut[j + 1]] - offsets[cut[j]]; }
};

// 40 slices as ingest_host cuts a host-packed call: 150-base reads from offsets[0] = 300 on, 150 000 bases a slice (more
// than shk_pack_reads hands to one thread), the first a quarter of that
Call make_call() {
  Call c;
  std::mt19937_64 rng(4242);
  const uint64_t n_reads = 250 + 39 * 1000;
  c.bases.resize(300 + n_reads * 150);
  for (auto &ch : c.bases) ch = rng() % 100 == 0 ? 'N' : "ACGT"[rng() & 3];
  c.offsets = offsets_of(std::vector<uint32_t>(n_reads, 150), 300);
  c.cut = shk::slice_cuts(c.offsets.data(), n_reads, 150000, true);
  c.lay = shk::HostPackLayout(c.offsets.data(), c.cut);
  return c;
}

struct Packed {
  int rc = SHK_OK;
  std::string text;
  std::vector<uint8_t> pk;
  std::vector<uint32_t> nm;
};

Packed pack_direct(const Call &c, size_t j) {
  Packed p;
  uint64_t pb = 0, nw = 0;
  shk_packed_sizes(c.nb(j), &pb, &nw);
  p.pk.resize(pb), p.nm.resize(nw);
  p.rc = shk_pack_reads((const uint8_t *)c.bases.data() + c.o0(j), c.nb(j), p.pk.data(), p.nm.data(), 0);
  p.text = shk_run_error();
  return p;
}

// consume slices [0, n_consume) in order, as ingest_host does, then let go of the packer wherever it is
void run_packer(const Call &c, size_t n_consume, size_t bad_slice) {
  std::unique_ptr<uint8_t[]> pk(new uint8_t[c.lay.pk_total]), nm(new uint8_t[c.lay.nm_total]);
  shk::HostPacker packer((const uint8_t *)c.bases.data(), c.offsets.data(), c.cut, c.lay, pk.get(), nm.get());
  for (size_t i = 0; i < n_consume; ++i) {
    const size_t have = packer.packed(i + 1);
    const Packed want = pack_direct(c, i);
    if (have < i + 1) {
      CHECK(i == bad_slice && have == i, "the packer gave up at slice %zu with %zu packed", i, have);
      CHECK(packer.code() == want.rc && want.rc == SHK_ERR_INVALID_CHAR, "code %d, the direct call's %d", packer.code(), want.rc);
      CHECK(packer.text() == want.text && !want.text.empty(), "text '%s', the direct call's '%s'", packer.text().c_str(), want.text.c_str());
      CHECK(packer.packed(0) == i && packer.packed(i + 1) == i, "a packer that has given up stays where it is");
      return;
    }
    CHECK(i != bad_slice && want.rc == SHK_OK, "slice %zu was packed, the direct call says %d", i, want.rc);
    CHECK(packer.packed(0) >= i + 1, "packed(0) went back");
    CHECK(memcmp(pk.get() + c.lay.pk_off[i], want.pk.data(), want.pk.size()) == 0, "slice %zu: 2-bit stream differs", i);
    CHECK(memcmp(nm.get() + c.lay.nm_off[i], want.nm.data(), want.nm.size() * 4) == 0, "slice %zu: N mask differs", i);
  }
  CHECK(bad_slice >= n_consume, "the packer did not report slice %zu", bad_slice);
}

void check_packer() {
  Call c = make_call();
  const size_t n = c.n_slices(), none = ~(size_t)0;
  CHECK(n == 40, "%zu slices", n);
  run_packer(c, n, none);
  for (size_t k : {(size_t)0, (size_t)1, (size_t)17, n - 1, n}) run_packer(c, k, none);  // let go after none, some, all
  for (size_t bad : {(size_t)0, n / 2, n - 1}) {
    const uint64_t at = c.o0(bad) + c.nb(bad) / 3;
    const char was = c.bases[at];
    c.bases[at] = 'x';
    run_packer(c, n, bad);
    run_packer(c, bad / 2, bad);  // … and let go before the consumer got there
    c.bases[at] = was;
  }
}

}  // namespace

int main() {
  check_all_cuts();
  check_ring();
  check_extents_and_layout();
  check_nmask();
  check_packer();
  printf("ok %llu\n", (U64)n_checks);
  return 0;
}
