// shk_ingest_plan.h — what a host-buffer ingest (ingest_host in shk_engine.hip, DESIGN.md §3 "Host staging") decides
// and runs without touching a device: where a call is cut into slices, which staging set a slice takes, which bytes of
// the packed streams a slice occupies, where the host packer puts a slice, the list form of a sparse N mask, and the
// packer thread itself.  Plain C++ with no HIP and no context in it, so a stand-alone driver runs all of it against
// linear-scan models under the sanitizers (tests/native/ingest_plan_driver.cpp).
#pragma once

#include <algorithm>
#include <condition_variable>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/shk.h"

namespace shk {

// The run of whole reads from read `lo` (< n_seqs) that holds at most max_bases bases: the largest hi with
// offsets[hi] ≤ offsets[lo] + max_bases, and at least one read (which may then be longer than max_bases).
inline uint64_t reads_within(const uint64_t *offsets, uint64_t lo, uint64_t n_seqs, uint64_t max_bases) {
  const uint64_t limit = offsets[lo] + max_bases;
  const uint64_t hi = (uint64_t)(std::upper_bound(offsets + lo, offsets + n_seqs + 1, limit) - offsets) - 1;
  return hi > lo ? hi : lo + 1;
}

// Slice boundaries at read boundaries, ≈ slice_bases each: slice i is reads [cut[i], cut[i + 1]).  quarter_first: the
// first slice a quarter of that (a packed or host-packed call: nothing overlaps the first slice's copy).
inline std::vector<uint64_t> slice_cuts(const uint64_t *offsets, uint64_t n_seqs, uint64_t slice_bases, bool quarter_first) {
  std::vector<uint64_t> cut{0};
  while (cut.back() < n_seqs) {
    const uint64_t lo = cut.back();
    cut.push_back(reads_within(offsets, lo, n_seqs, lo == 0 && quarter_first ? std::max<uint64_t>(slice_bases / 4, 1) : slice_bases));
  }
  return cut;
}

// The staging sets of a call, taken in turn across slices and across calls.  A call of few slices takes few sets (at
// least two: one may still be read by the previous call's last launch), and the set a call starts with is never the one
// the previous call's last slice took (stage_last, −1: none).
struct StageRing {
  int nst;      // sets in use: NST − 1 slices' copies are queued ahead of the count
  uint32_t s0;  // the first slice's
  StageRing(size_t n_slices, int stage_last, int max_sets)
      : nst((int)std::min<size_t>((size_t)max_sets, std::max<size_t>(n_slices + 1, 2))),
        s0(stage_last >= 0 ? (uint32_t)(stage_last + 1) % (uint32_t)nst : 0u) {}
  int set_of(size_t i) const { return (int)((s0 + i) % (uint32_t)nst); }
};

// The bytes [b0, b1) of a 2-bit stream and the words [w0, w1) of its N mask that hold bases [o_rel, o_rel + nb).
struct PackedExtent {
  uint64_t b0, b1, w0, w1;
  PackedExtent(uint64_t o_rel, uint64_t nb) : b0(o_rel >> 2), b1((o_rel + nb + 3) >> 2), w0(o_rel >> 5), w1((o_rel + nb + 31) >> 5) {}
};

// Host packing: every slice of the call has a stretch of its own in the call's two pinned staging buffers (2-bit
// streams; N masks), 64-byte aligned (no two slices share a cache line) and longer than shk_packed_sizes says.
struct HostPackLayout {
  std::vector<size_t> pk_off, nm_off;
  size_t pk_total = 0, nm_total = 0;
  HostPackLayout() = default;
  HostPackLayout(const uint64_t *offsets, const std::vector<uint64_t> &cut) {
    for (size_t j = 0; j + 1 < cut.size(); ++j) {
      const uint64_t nb = offsets[cut[j + 1]] - offsets[cut[j]];
      pk_off.push_back(pk_total);
      nm_off.push_back(nm_total);
      pk_total += (size_t)((nb / 4 + 64 + 63) & ~63ull);
      nm_total += (size_t)(((nb / 32 + 2) * 4 + 63) & ~63ull);
    }
  }
};

// The non-zero words of an N mask as (index, word) pairs — on a few threads: the caller is between two slices of
// a host-buffer ingest, with the link busy and nothing else to do.  Returns the number of pairs, or ~0 when
// there are more than `cap` (the mask then crosses the link as it is).
inline size_t nmask_nonzero(const uint32_t *w, size_t n, uint32_t *pairs, size_t cap) {
  const unsigned T = (unsigned)std::max(1, std::min(8, (int)(n >> 18)));  // ≥ 1 MiB of mask per thread
  std::vector<size_t> cnt(T, 0);
  const size_t seg = cap / T;
  auto work = [&](unsigned t) {
    const size_t a = n * t / T, b = n * (t + 1) / T;
    uint32_t *out = pairs + 2 * seg * t;
    size_t k = 0;
    size_t i = a;
    for (; i < b && (i & 1); ++i)
      if (w[i]) { if (k < seg) out[2 * k] = (uint32_t)i, out[2 * k + 1] = w[i]; ++k; }
    for (; i + 8 <= b; i += 8) {  // (64-bit loads: the mask is 4-byte aligned, i is even here — and the host tolerates the rest)
      uint64_t q[4];
      memcpy(q, w + i, 32);
      if ((q[0] | q[1] | q[2] | q[3]) == 0) continue;
      for (size_t j = i; j < i + 8; ++j)
        if (w[j]) { if (k < seg) out[2 * k] = (uint32_t)j, out[2 * k + 1] = w[j]; ++k; }
    }
    for (; i < b; ++i)
      if (w[i]) { if (k < seg) out[2 * k] = (uint32_t)i, out[2 * k + 1] = w[i]; ++k; }
    cnt[t] = k;
  };
  if (T == 1) {
    work(0);
  } else {
    std::vector<std::thread> th;
    for (unsigned t = 1; t < T; ++t) th.emplace_back(work, t);
    work(0);
    for (auto &x : th) x.join();
  }
  size_t total = 0;
  for (unsigned t = 0; t < T; ++t) {
    if (cnt[t] > seg) return ~(size_t)0;
    if (t && cnt[t]) memmove(pairs + 2 * total, pairs + 2 * seg * t, cnt[t] * 8);
    total += cnt[t];
  }
  return total;
}

// Host packing: ONE thread of its own packs the call's slices, in order, each into its own stretch of the call's
// staging (shk_pack_reads: all the host's cores per slice), and says how far it has come; the caller sends what is
// packed and counts what has arrived — a deferred page pass that holds the caller up does not hold the packing up.
// It starts on construction and stops at the first invalid byte; the destructor asks it to stop after the slice it is
// at and joins it, so every way out of the caller goes past it.
class HostPacker {
 public:
  HostPacker(const uint8_t *bases, const uint64_t *offsets, const std::vector<uint64_t> &cut, const HostPackLayout &lay, uint8_t *pk, uint8_t *nm)
      : thread_([=, &cut, &lay] {
          for (size_t j = 0; j + 1 < cut.size(); ++j) {
            {
              std::lock_guard<std::mutex> lk(m_);
              if (quit_) return;
            }
            const uint64_t o0 = offsets[cut[j]], nb = offsets[cut[j + 1]] - o0;
            int prc = SHK_OK;
            if (nb) prc = shk_pack_reads(bases + o0, nb, pk + lay.pk_off[j], (uint32_t *)(nm + lay.nm_off[j]), 0);
            std::lock_guard<std::mutex> lk(m_);
            if (prc != SHK_OK) {
              rc_ = prc;
              err_ = shk_run_error();  // (this thread's own message buffer)
              cv_.notify_all();
              return;
            }
            done_ = j + 1;
            cv_.notify_all();
          }
        }) {}
  ~HostPacker() {
    {
      std::lock_guard<std::mutex> lk(m_);
      quit_ = true;
    }
    thread_.join();
  }
  HostPacker(const HostPacker &) = delete;
  HostPacker &operator=(const HostPacker &) = delete;
  // Slices [0, n) are packed.  need > 0: wait for slice need − 1 first — or for the packer's error, which is the
  // caller's: n < need then, and code() and text() say what shk_pack_reads said.
  size_t packed(size_t need) {
    std::unique_lock<std::mutex> lk(m_);
    if (need) cv_.wait(lk, [&] { return done_ >= need || rc_ != SHK_OK; });
    return done_;
  }
  int code() {
    std::lock_guard<std::mutex> lk(m_);
    return rc_;
  }
  std::string text() {
    std::lock_guard<std::mutex> lk(m_);
    return err_;
  }

 private:
  std::mutex m_;
  std::condition_variable cv_;
  size_t done_ = 0;   // slices packed so far
  int rc_ = SHK_OK;   // … or the packer's error (an invalid byte: the run is over)
  std::string err_;
  bool quit_ = false;
  std::thread thread_;  // (last: it starts with everything above in place)
};

}  // namespace shk
