// gz_source_driver — the gzip source's parts below the level of a whole reader (sharkmer_amd/csrc/shk_gz_source.h), as a
// stand-alone program under AddressSanitizer and UBSan, and under ThreadSanitizer:
//   make -C sharkmer_amd/csrc gz_source_driver gz_source_driver_tsan
//   sharkmer_amd/csrc/gz_source_driver [STREAM EXPECTED_TEXT]...
//   * LineWindows against a linear model, from a fixed seed: random appends (the inflater's way and a batch's way),
//     rolls and a finish at a random cut;
//   * ParallelInflate over every STREAM (raw DEFLATE, whatever follows it included) at chunk sizes 512 B, 1 KiB and
//     16 KiB with 1, 2 and 5 workers against one Inflater in a plain loop, and with a sink that stops after its k-th
//     window.
// Links shk_inflate.cpp and nothing else.  Prints "ok <checks>" and exits 0, or the first difference and exits 1.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "shk_gz_source.h"

using namespace shk;
using namespace shk::gzsrc;

namespace {

uint64_t n_checks = 0;

#define CHECK(cond, ...)                                             \
  do {                                                               \
    ++n_checks;                                                      \
    if (!(cond)) {                                                   \
      fprintf(stdout, "FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); \
      fprintf(stdout, __VA_ARGS__);                                  \
      fprintf(stdout, "\n");                                         \
      exit(1);                                                       \
    }                                                                \
  } while (0)

using U64 = unsigned long long;
using Bytes = std::vector<uint8_t>;

// Takes every window apart as it arrives: a non-last one is whole lines and not empty, all of them continue `want`
// where the one before ended.  Stops after `stop_after` windows (−1: never) and must then get no more.
struct CheckSink final : WindowSink {
  const char *what;
  const Bytes *want;             // the text the windows are cut from (LineWindows: grows while they arrive)
  uint64_t got = 0, n_windows = 0;
  long stop_after = -1;
  bool saw_last = false;
  const uint64_t *appended = nullptr;  // LineWindows: bytes appended so far — HOLD_BACK of them lie behind a window
  explicit CheckSink(const char *w, const Bytes *t) : what(w), want(t) {}
  bool stopped() override { return stop_after >= 0 && n_windows >= (uint64_t)stop_after; }
  void emit(Window &&w) override {
    CHECK(!stopped(), "%s: a window after the sink had stopped", what);
    CHECK(!saw_last, "%s: a window behind the last one", what);
    ++n_windows;
    saw_last = w.last;
    if (!w.last) CHECK(w.n > 0 && w.p[w.n - 1] == '\n', "%s: window %llu (%zu bytes) is not whole lines", what, (U64)n_windows, w.n);
    CHECK(got + w.n <= want->size() && (w.n == 0 || memcmp(w.p, want->data() + got, w.n) == 0), "%s: window %llu differs from the text at %llu", what,
          (U64)n_windows, (U64)got);
    got += w.n;
    if (appended && !w.last) CHECK(*appended - got >= LineWindows::HOLD_BACK, "%s: only %llu bytes behind window %llu", what, (U64)(*appended - got), (U64)n_windows);
  }
};

// ---- LineWindows ----------------------------------------------------------------------------------------------------
void after_roll(const LineWindows &lw, const uint8_t *all, size_t n_all, const char *what) {  // all[0, n_all): what has been appended
  CHECK(lw.appended() == n_all, "%s: gone + pos = %llu, appended %zu", what, (U64)lw.appended(), n_all);
  const size_t h = std::min<size_t>(32768, n_all);
  CHECK(lw.pos >= h && memcmp(lw.data() + lw.pos - h, all + n_all - h, h) == 0, "%s: the %zu bytes in front of pos are not the stream's last", what, h);
  CHECK(lw.line0 <= lw.pos, "%s: line0 behind pos", what);
}

void line_windows_sequence(std::mt19937_64 &rng, size_t window, int family) {
  char what[96];
  snprintf(what, sizeof what, "LineWindows window %zu family %d", window, family);
  Bytes all;
  uint64_t appended = 0;
  CheckSink sink(what, &all);
  sink.appended = &appended;
  LineWindows lw(window);
  size_t line_left = 0;  // bytes until the next '\n'
  auto next_line = [&] {
    const unsigned r = (unsigned)(rng() % 100);
    if (family == 1) return (size_t)1 << 40;                                    // no '\n' at all
    if (family == 2 && r < 4) return (size_t)(40000 + rng() % 60000);           // longer than 32 KiB (and than the window)
    if (family >= 2 && r < 12) return (size_t)(window + 1 + rng() % (2 * window));  // longer than the window
    return (size_t)(1 + rng() % 200);
  };
  line_left = next_line();
  const int n_ops = 40 + (int)(rng() % 120);
  for (int op = 0; op < n_ops; ++op) {
    size_t n = (size_t)(rng() % 3 == 0 ? rng() % (3 * window) : rng() % 3000);
    const size_t at = all.size();
    for (size_t i = 0; i < n; ++i) {
      if (line_left == 0) {
        all.push_back('\n');
        line_left = next_line();
      } else {
        all.push_back((uint8_t)("ACGT@+IJ"[(all.size() * 0x9E3779B97F4A7C15ull) >> 61]));  // (a byte says where it lies)
        --line_left;
      }
    }
    if (rng() & 1) {  // a batch: room for all of it first
      lw.roll(n, sink);
      after_roll(lw, all.data(), at, what);
      CHECK(lw.room() >= n + Inflater::OUT_SLACK, "%s: roll(%zu) left %zu bytes of room", what, n, lw.room());
      memcpy(lw.data() + lw.pos, all.data() + at, n);
      lw.advance(n);
      appended += n;
    } else {  // the inflater: until fewer than OUT_SLACK bytes of room are left, then a roll
      size_t done = 0;
      while (done < n) {
        const size_t avail = lw.room() > Inflater::OUT_SLACK ? lw.room() - Inflater::OUT_SLACK : 0;
        if (!avail) {
          lw.roll(sink);
          after_roll(lw, all.data(), at + done, what);
          CHECK(lw.room() > Inflater::OUT_SLACK, "%s: a roll made no room", what);
          continue;
        }
        const size_t m = std::min(n - done, avail);
        memcpy(lw.data() + lw.pos, all.data() + at + done, m);
        lw.advance(m);
        appended += m;
        done += m;
      }
    }
    CHECK(lw.appended() == all.size(), "%s: gone + pos = %llu, appended %zu", what, (U64)lw.appended(), all.size());
  }
  // the last window at a random cut: anywhere in what was held back (a corrupt stream's cut), or the whole text
  const uint64_t unsent = all.size() - sink.got;
  const uint64_t back = rng() % 3 == 0 ? 0 : rng() % (std::min<uint64_t>(unsent, LineWindows::HOLD_BACK) + 1);
  all.resize(all.size() - back);
  sink.appended = nullptr;
  lw.finish(all.size(), sink);
  CHECK(sink.saw_last && sink.got == all.size(), "%s: the windows end at %llu, the cut is at %zu", what, (U64)sink.got, all.size());
}

// a line that ends exactly HOLD_BACK bytes in front of pos is not handed on yet: the window ends at the line before
void line_end_at_the_hold_back_border() {
  const char *what = "LineWindows, '\\n' at pos - HOLD_BACK";
  LineWindows lw(4096);
  const size_t full = lw.room() - Inflater::OUT_SLACK;  // where the inflater stops
  Bytes all(full, (uint8_t)'A');
  all[100] = '\n';
  all[full - LineWindows::HOLD_BACK] = '\n';
  uint64_t appended = full;
  CheckSink sink(what, &all);
  sink.appended = &appended;
  memcpy(lw.data(), all.data(), full);
  lw.advance(full);
  lw.roll(sink);
  after_roll(lw, all.data(), full, what);
  CHECK(sink.n_windows == 1 && sink.got == 101, "%s: %llu windows, %llu bytes", what, (U64)sink.n_windows, (U64)sink.got);
  all.push_back('C');  // one more byte behind it, and the line goes out
  memcpy(lw.data() + lw.pos, "C", 1);
  lw.advance(1);
  appended += 1;
  lw.roll(0, sink);  // (room enough: nothing happens)
  CHECK(sink.n_windows == 1, "%s: a roll with room enough cut a window", what);
  lw.roll(lw.room(), sink);
  after_roll(lw, all.data(), all.size(), what);
  CHECK(sink.n_windows == 2 && sink.got == full - LineWindows::HOLD_BACK + 1, "%s: %llu windows, %llu bytes", what, (U64)sink.n_windows, (U64)sink.got);
}

void check_line_windows() {
  line_end_at_the_hold_back_border();
  std::mt19937_64 rng(20261020);
#ifdef __SANITIZE_THREAD__
  const int rounds = 2;  // (one thread: ThreadSanitizer has nothing to find here, and takes five times as long over it)
#else
  const int rounds = 12;
#endif
  for (int round = 0; round < rounds; ++round)
    for (size_t window : {(size_t)4096, (size_t)20000, (size_t)65536})
      for (int family : {0, 1, 2, 3})
        if (window == 4096 || round < 3) line_windows_sequence(rng, window, family);
}

// ---- ParallelInflate --------------------------------------------------------------------------------------------------
Bytes slurp(const char *path) {
  FILE *f = fopen(path, "rb");
  CHECK(f != nullptr, "cannot open %s", path);
  Bytes b;
  uint8_t buf[65536];
  for (size_t r; (r = fread(buf, 1, sizeof buf, f)) > 0;) b.insert(b.end(), buf, buf + r);
  fclose(f);
  return b;
}

struct Sequential {
  Bytes out;
  InflateStatus status;
  const uint8_t *after = nullptr;
  uint64_t bit = 0;
};
Sequential inflate_in_a_plain_loop(const Bytes &z) {
  Sequential s;
  Inflater inf;
  inf.reset(z.data(), z.data() + z.size());
  Bytes buf(1u << 16);
  size_t pos = 0;
  while ((s.status = inf.run(buf.data(), &pos, buf.size())) == INF_OUTPUT_FULL) buf.resize(buf.size() * 2);
  buf.resize(pos);
  s.out = std::move(buf);
  s.bit = inf.bit_position(z.data());
  if (s.status == INF_STREAM_END) s.after = inf.input_after_stream();
  return s;
}

void check_stream(const char *path, const Bytes &z, const Bytes &text) {
  const Sequential seq = inflate_in_a_plain_loop(z);
  CHECK(seq.out.size() <= text.size() && (seq.out.empty() || memcmp(seq.out.data(), text.data(), seq.out.size()) == 0), "%s: the plain loop's bytes are no prefix of the text", path);
  if (seq.status == INF_STREAM_END) CHECK(seq.out.size() == text.size(), "%s: the plain loop gives %zu bytes of %zu", path, seq.out.size(), text.size());
  for (size_t chunk : {(size_t)512, (size_t)1024, (size_t)16384})
    for (uint32_t workers : {1u, 2u, 5u}) {
      char what[512];
      snprintf(what, sizeof what, "%s chunk %zu workers %u", path, chunk, workers);
      // a corrupt stream is cut where the callback says: at the last multiple of 8192 (inside what is held back)
      uint64_t n_ok_seen = ~0ull, cut_at = ~0ull;
      const uint8_t *fail_seen = nullptr;
      Bytes want = seq.out;
      CheckSink sink(what, &want);
      ParallelInflate par(z.data(), z.data() + z.size(), workers, chunk, sink, [&](uint64_t n_ok, const uint8_t *fail) {
        n_ok_seen = n_ok;
        fail_seen = fail;
        return cut_at = n_ok / 8192 * 8192;
      });
      ParallelInflate::Result r = par.run();
      CHECK(!r.stopped, "%s: stopped", what);
      CHECK(r.status == seq.status, "%s: status %d, the plain loop's %d", what, (int)r.status, (int)seq.status);
      if (seq.status == INF_STREAM_END) CHECK(r.after == seq.after && r.verified_bit == seq.bit, "%s: the stream ends at bit %llu, the plain loop's at %llu", what, (U64)r.verified_bit, (U64)seq.bit);
      if (seq.status == INF_CORRUPT) {
        CHECK(n_ok_seen == seq.out.size(), "%s: %llu bytes in front of the damage, the plain loop has %zu", what, (U64)n_ok_seen, seq.out.size());
        CHECK(fail_seen == z.data() + (seq.bit >> 3), "%s: damage at byte %lld, the plain loop's at %llu", what, (long long)(fail_seen - z.data()), (U64)(seq.bit >> 3));
        want.resize((size_t)cut_at);
      } else {
        CHECK(n_ok_seen == ~0ull, "%s: asked for a corrupt stream's cut", what);
      }
      CHECK(r.last.last, "%s: no last window", what);
      sink.emit(std::move(r.last));
      CHECK(sink.got == want.size(), "%s: %llu bytes handed on, %zu expected", what, (U64)sink.got, want.size());
    }
  // a sink that stops after its k-th window gets no further one (CheckSink::emit), and the call comes back
  for (long k : {0L, 1L, 3L})
    for (uint32_t workers : {2u, 5u}) {
      char what[512];
      snprintf(what, sizeof what, "%s stopped after %ld windows, workers %u", path, k, workers);
      CheckSink sink(what, &seq.out);
      sink.stop_after = k;
      ParallelInflate par(z.data(), z.data() + z.size(), workers, 512, sink);
      ParallelInflate::Result r = par.run();
      CHECK(sink.n_windows <= (uint64_t)k, "%s: %llu windows", what, (U64)sink.n_windows);
      CHECK(r.stopped || r.last.last, "%s: neither stopped nor at the end", what);
    }
}

}  // namespace

int main(int argc, char **argv) {
  check_line_windows();
  if ((argc - 1) % 2) {
    fprintf(stdout, "usage: gz_source_driver [STREAM EXPECTED_TEXT]...\n");
    return 2;
  }
  for (int i = 1; i + 1 < argc; i += 2) check_stream(argv[i], slurp(argv[i]), slurp(argv[i + 1]));
  printf("ok %llu\n", (U64)n_checks);
  return 0;
}
