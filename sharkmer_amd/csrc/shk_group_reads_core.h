// shk_group_reads_core.h — the run directory of a multi-device context that retains reads (SHK_FLAG_GROUP_READS;
// DESIGN.md §22) and the host merges of its retained calls.  Plain C++17, no HIP: a stand-alone driver brute-forces it
// under the sanitizers (tests/native/group_reads_driver.cpp).
//
// Every exchange round appends one run of reads to every share's store, share 0's first.  A retained read's GLOBAL index
// is its ordinal in that order since retention was switched on or the context reset — the index it has on a one-device
// context fed the same calls; its LOCAL index is its place in its share's store.  The directory keeps, per share, the runs
// it appended as {global_first, n_reads, local_first} (local_first: the prefix sum of n_reads), and the same runs once
// more in global order.  A run of no reads leaves no entry; a run that continues its share's last one — globally and
// therefore locally — extends it.
#pragma once

#include <algorithm>
#include <cstdint>
#include <queue>
#include <utility>
#include <vector>

namespace shk {

struct GroupRun {
  uint64_t global_first, n_reads, local_first;
};
// [global_first, global_first + n_reads) = reads [local_first, local_first + n_reads) of share `share`
struct GroupPiece {
  uint32_t share;
  uint64_t global_first, local_first, n_reads;
};
struct GroupLink {
  uint32_t in, out, count;
};

class GroupReadsDir {
 public:
  void init(uint32_t n_shares) {
    runs_.assign(n_shares, {});
    clear();
  }
  void clear() {
    for (auto &r : runs_) r.clear();
    order_.clear();
    total_ = 0;
  }
  uint32_t n_shares() const { return (uint32_t)runs_.size(); }
  uint64_t total() const { return total_; }
  uint64_t share_reads(uint32_t share) const {
    const auto &r = runs_[share];
    return r.empty() ? 0 : r.back().local_first + r.back().n_reads;
  }
  size_t n_runs() const { return order_.size(); }

  // the next n_reads global indices are share's next n_reads local ones
  void append(uint32_t share, uint64_t n_reads) {
    if (!n_reads) return;
    auto &r = runs_[share];
    if (!order_.empty() && order_.back().first == share) {  // (then r.back() ends at total_)
      r.back().n_reads += n_reads;
    } else {
      r.push_back(GroupRun{total_, n_reads, share_reads(share)});
      order_.emplace_back(share, (uint32_t)(r.size() - 1));
    }
    total_ += n_reads;
  }

  // global < total() → its share and its index there
  bool lookup(uint64_t global, uint32_t *share, uint64_t *local) const {
    if (global >= total_) return false;
    const size_t i = run_of(global);
    const GroupRun &r = run(i);
    *share = order_[i].first;
    *local = r.local_first + (global - r.global_first);
    return true;
  }
  // local < share_reads(share) → its global index
  uint64_t to_global(uint32_t share, uint64_t local) const {
    const auto &r = runs_[share];
    size_t lo = 0, hi = r.size();  // the last run with local_first <= local
    while (hi - lo > 1) {
      const size_t mid = lo + (hi - lo) / 2;
      (r[mid].local_first <= local ? lo : hi) = mid;
    }
    return r[lo].global_first + (local - r[lo].local_first);
  }
  // [first, first + n) within [0, total()] as contiguous pieces, in global order
  bool split(uint64_t first, uint64_t n, std::vector<GroupPiece> *out) const {
    out->clear();
    if (first > total_ || n > total_ - first) return false;
    if (!n) return true;
    for (size_t i = run_of(first); i < order_.size() && run(i).global_first < first + n; ++i) {
      const GroupRun &r = run(i);
      const uint64_t a = std::max(first, r.global_first), b = std::min(first + n, r.global_first + r.n_reads);
      out->push_back(GroupPiece{order_[i].first, a, r.local_first + (a - r.global_first), b - a});
    }
    return true;
  }

 private:
  const GroupRun &run(size_t i) const { return runs_[order_[i].first][order_[i].second]; }
  size_t run_of(uint64_t global) const {  // the last run in global order with global_first <= global (global < total_)
    size_t lo = 0, hi = order_.size();
    while (hi - lo > 1) {
      const size_t mid = lo + (hi - lo) / 2;
      (run(mid).global_first <= global ? lo : hi) = mid;
    }
    return lo;
  }
  std::vector<std::vector<GroupRun>> runs_;            // per share, ascending
  std::vector<std::pair<uint32_t, uint32_t>> order_;   // (share, index in runs_[share]), ascending global_first
  uint64_t total_ = 0;
};

// Ascending lists → one ascending list, every entry kept (equal entries of different lists too).
inline void group_merge_ascending(const std::vector<std::vector<uint64_t>> &lists, std::vector<uint64_t> *out) {
  out->clear();
  size_t n = 0;
  for (const auto &l : lists) n += l.size();
  out->reserve(n);
  using Head = std::pair<uint64_t, size_t>;  // (value, list)
  std::priority_queue<Head, std::vector<Head>, std::greater<Head>> heads;
  std::vector<size_t> at(lists.size(), 0);
  for (size_t d = 0; d < lists.size(); ++d)
    if (!lists[d].empty()) heads.emplace(lists[d][0], d);
  while (!heads.empty()) {
    const Head h = heads.top();
    heads.pop();
    out->push_back(h.first);
    const size_t d = h.second;
    if (++at[d] < lists[d].size()) heads.emplace(lists[d][at[d]], d);
  }
}

// Link lists, each ascending by (in, out) without repeats → one such list, the counts of a pair added in 32 bits.
inline void group_merge_links(const std::vector<std::vector<GroupLink>> &lists, std::vector<GroupLink> *out) {
  out->clear();
  using Head = std::pair<uint64_t, size_t>;  // ((in, out), list)
  std::priority_queue<Head, std::vector<Head>, std::greater<Head>> heads;
  std::vector<size_t> at(lists.size(), 0);
  auto key = [](const GroupLink &l) { return (uint64_t)l.in << 32 | l.out; };
  for (size_t d = 0; d < lists.size(); ++d)
    if (!lists[d].empty()) heads.emplace(key(lists[d][0]), d);
  while (!heads.empty()) {
    const size_t d = heads.top().second;
    heads.pop();
    const GroupLink &l = lists[d][at[d]];
    if (!out->empty() && out->back().in == l.in && out->back().out == l.out)
      out->back().count += l.count;
    else
      out->push_back(l);
    if (++at[d] < lists[d].size()) heads.emplace(key(lists[d][at[d]]), d);
  }
}

}  // namespace shk
