// group_reads_driver — the run directory and the host merges of a multi-device context's retained reads
// (sharkmer_amd/csrc/shk_group_reads_core.h) brute-forced against linear models, under AddressSanitizer and UBSan:
//   make -C sharkmer_amd/csrc group_reads_driver && sharkmer_amd/csrc/group_reads_driver
// Random directories over D in {1, 2, 4, 64} shares: rounds deal every share a run of 0, 1 or a few reads (a round may
// deal nothing at all), up to thousands of rounds.  The model is the list owner[global] = (share, local) written one
// read at a time.  Checked: lookup and to_global of every global index and the refusal at total(); split of ranges
// that start and end at a run border - 1, + 0, + 1 — every pair of them in a small directory; from every one of them to
// the next few and some long ones in a large one — with the empty and the whole range and the refusals beyond the end,
// read by read against the model, pieces maximal within a run and in global order; group_merge_ascending against
// std::sort, repeats within and across lists kept; group_merge_links against a std::map, counts wrapping in 32 bits.
// Prints "ok <directories> <lookups> <splits>" and exits 0, or the first difference and exits 1.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <utility>
#include <vector>

#include "shk_group_reads_core.h"

namespace {

[[noreturn]] void die(const char *what, uint64_t a, uint64_t b, uint64_t c) {
  printf("FAIL %s: %llu %llu %llu\n", what, (unsigned long long)a, (unsigned long long)b, (unsigned long long)c);
  exit(1);
}

uint64_t n_lookups = 0, n_splits = 0;

void check_split(const shk::GroupReadsDir &dir, const std::vector<std::pair<uint32_t, uint64_t>> &owner, uint64_t first, uint64_t n) {
  std::vector<shk::GroupPiece> pieces;
  const uint64_t total = owner.size();
  const bool ok = dir.split(first, n, &pieces);
  if (first > total || n > total - first) {
    if (ok || !pieces.empty()) die("split accepted a range beyond the end", first, n, total);
    return;
  }
  if (!ok) die("split refused a range", first, n, total);
  ++n_splits;
  uint64_t at = first;
  for (size_t i = 0; i < pieces.size(); ++i) {
    const shk::GroupPiece &p = pieces[i];
    if (p.n_reads == 0 || p.global_first != at) die("split piece out of order or empty", first, n, i);
    for (uint64_t j = 0; j < p.n_reads; ++j)
      if (owner[at + j] != std::make_pair(p.share, p.local_first + j)) die("split piece differs from the model", first, n, at + j);
    // two pieces in a row never continue each other: a piece is as long as its run allows
    if (i && pieces[i - 1].share == p.share && pieces[i - 1].local_first + pieces[i - 1].n_reads == p.local_first)
      die("split cut a run in two", first, n, i);
    at += p.n_reads;
  }
  if (at != first + n) die("split covers another range", first, n, at);
}

void check_directory(std::mt19937_64 &rng, uint32_t D, uint32_t n_rounds, uint32_t max_run) {
  shk::GroupReadsDir dir;
  dir.init(D);
  std::vector<std::pair<uint32_t, uint64_t>> owner;  // the model
  std::vector<uint64_t> held(D, 0), borders{0};
  for (uint32_t r = 0; r < n_rounds; ++r) {
    const uint32_t kind = (uint32_t)(rng() % 8);  // 0: nobody gets a read; 1: one share gets one; else a run per share, many empty
    for (uint32_t d = 0; d < D; ++d) {
      uint64_t n = 0;
      if (kind == 1) n = d == rng() % D;
      else if (kind > 1) n = rng() % 3 == 0 ? 0 : 1 + rng() % max_run;
      dir.append(d, n);
      for (uint64_t j = 0; j < n; ++j) owner.emplace_back(d, held[d]++);
      if (n) borders.push_back(owner.size());
    }
    if (dir.total() != owner.size()) die("total", r, dir.total(), owner.size());
  }
  const uint64_t total = owner.size();
  for (uint32_t d = 0; d < D; ++d)
    if (dir.share_reads(d) != held[d]) die("share_reads", d, dir.share_reads(d), held[d]);
  if (dir.n_runs() > borders.size() - 1) die("more runs than appends", dir.n_runs(), borders.size(), 0);
  if (D == 1 && total && dir.n_runs() != 1) die("one share's runs were not joined", dir.n_runs(), total, 0);
  uint32_t share = 0;
  uint64_t local = 0;
  for (uint64_t i = 0; i < total; ++i, ++n_lookups) {
    if (!dir.lookup(i, &share, &local) || owner[i] != std::make_pair(share, local)) die("lookup", i, share, local);
    if (dir.to_global(share, local) != i) die("to_global", i, share, local);
  }
  if (dir.lookup(total, &share, &local) || dir.lookup(~0ull, &share, &local)) die("lookup beyond the end", total, 0, 0);
  // ranges between every pair of positions next to a run border (all pairs while they are few, else a random partner)
  std::vector<uint64_t> at;
  for (const uint64_t b : borders)
    for (int64_t o = -1; o <= 1; ++o)
      if ((int64_t)b + o >= 0 && b + o <= total + 1) at.push_back(b + o);
  std::sort(at.begin(), at.end());
  at.erase(std::unique(at.begin(), at.end()), at.end());
  for (size_t i = 0; i < at.size(); ++i) {
    if (at.size() <= 200) {
      for (size_t j = i; j < at.size(); ++j) check_split(dir, owner, at[i], at[j] - at[i]);
    } else {
      for (int t = 0; t < 4; ++t) {  // (a partner a few borders on: the check reads every read of the range)
        const size_t j = std::min(at.size() - 1, i + (size_t)(rng() % 12));
        check_split(dir, owner, at[i], at[j] - at[i]);
      }
      check_split(dir, owner, at[i], 0);
    }
  }
  for (int t = 0; t < 40 && at.size() > 200; ++t) {  // … and some long ones
    const size_t i = rng() % at.size(), j = i + rng() % (at.size() - i);
    check_split(dir, owner, at[i], at[j] - at[i]);
  }
  check_split(dir, owner, 0, total);
  check_split(dir, owner, 0, total + 1);
  check_split(dir, owner, total, 1);
  check_split(dir, owner, 1, ~0ull);  // (first + n wraps)
  dir.clear();
  if (dir.total() || dir.n_runs() || dir.share_reads(0) || dir.lookup(0, &share, &local)) die("clear", dir.total(), dir.n_runs(), 0);
  dir.append(D - 1, 2);  // … and goes on from zero
  if (!dir.lookup(1, &share, &local) || share != D - 1 || local != 1 || dir.total() != 2) die("append after clear", share, local, dir.total());
}

void check_merges(std::mt19937_64 &rng, uint32_t D) {
  std::vector<std::vector<uint64_t>> lists(D);
  std::vector<uint64_t> want, got;
  const uint64_t range = 1 + rng() % 50;  // small: repeats within and across lists
  for (auto &l : lists) {
    const uint64_t n = rng() % 4 == 0 ? 0 : rng() % 40;
    for (uint64_t i = 0; i < n; ++i) l.push_back(rng() % range);
    std::sort(l.begin(), l.end());
    want.insert(want.end(), l.begin(), l.end());
  }
  std::sort(want.begin(), want.end());
  shk::group_merge_ascending(lists, &got);
  if (got != want) die("group_merge_ascending", D, got.size(), want.size());

  std::vector<std::vector<shk::GroupLink>> links(D);
  std::map<std::pair<uint32_t, uint32_t>, uint32_t> sum;
  for (auto &l : links) {
    std::map<std::pair<uint32_t, uint32_t>, uint32_t> mine;  // (in, out) once per list, ascending
    const uint64_t n = rng() % 4 == 0 ? 0 : rng() % 30;
    for (uint64_t i = 0; i < n; ++i)
      mine[{(uint32_t)(rng() % 6), (uint32_t)(rng() % 6)}] = rng() % 5 == 0 ? 0xFFFFFFFFu - (uint32_t)(rng() % 3) : 1 + (uint32_t)(rng() % 9);
    for (const auto &kv : mine) {
      l.push_back(shk::GroupLink{kv.first.first, kv.first.second, kv.second});
      sum[kv.first] += kv.second;  // (32 bits: wraps as the merge's sum does)
    }
  }
  std::vector<shk::GroupLink> merged;
  shk::group_merge_links(links, &merged);
  if (merged.size() != sum.size()) die("group_merge_links size", D, merged.size(), sum.size());
  size_t i = 0;
  for (const auto &kv : sum) {
    const shk::GroupLink &m = merged[i++];
    if (m.in != kv.first.first || m.out != kv.first.second || m.count != kv.second) die("group_merge_links", D, m.in, m.out);
  }
}

}  // namespace

int main() {
  std::mt19937_64 rng(0x5eed);
  uint64_t n_dirs = 0;
  for (const uint32_t D : {1u, 2u, 4u, 64u}) {
    check_directory(rng, D, 0, 1);  // nothing appended
    ++n_dirs;
    for (int rep = 0; rep < 30; ++rep, ++n_dirs) check_directory(rng, D, 1 + (uint32_t)(rng() % 12), 1 + (uint32_t)(rng() % 3));
    for (int rep = 0; rep < 3; ++rep, ++n_dirs) check_directory(rng, D, D == 64 ? 1500 : 4000, 1 + (uint32_t)(rng() % 5));  // thousands of rounds
    for (int rep = 0; rep < 300; ++rep) check_merges(rng, D);
  }
  printf("ok %llu %llu %llu\n", (unsigned long long)n_dirs, (unsigned long long)n_lookups, (unsigned long long)n_splits);
  return 0;
}
