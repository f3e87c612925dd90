// shk_gz_source.h — the FASTQ reader's windows of text and the parts a gzip source is made of:
//   * Buf / UBuf / Window / Source: what every source hands to the parse;
//   * LineWindows: the rolling output buffer of a decoder — whole lines leave as windows, the decoder's 32 KiB of
//     history and the unfinished line move on into the next block;
//   * ParallelInflate: one DEFLATE stream decoded by many threads (speculative chunks, verified in order).
// Host only: included by shk_front.cpp and by tests/native/gz_source_driver.cpp, by nothing on the HIP side.
#pragma once
#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <functional>
#include <memory>
#include <mutex>
#include <new>
#include <thread>
#include <utility>
#include <vector>

#include "shk_inflate.h"

namespace shk {
namespace gzsrc {

// A window's bytes when they are not the mapped file's: a block that is neither zero-filled (std::vector would: 16 MiB
// per inflated window, a tenth of the inflate thread's time) nor handed back to the allocator after every window (a block
// this large comes from mmap: thousands of page faults each time) — a few blocks of each size in use are kept for reuse.
struct Buf {
  struct Bytes {
    uint8_t *p = nullptr;
    size_t n = 0;
    uint8_t *data() const { return p; }
    size_t size() const { return n; }
    void resize(size_t m) {  // (contents are NOT kept: every caller copies what it needs itself)
      release(p, n);
      p = acquire(m);
      n = m;
    }
    ~Bytes() { release(p, n); }
    Bytes() = default;
    Bytes(const Bytes &) = delete;
    Bytes &operator=(const Bytes &) = delete;
  } v;
  // a fresh block of `cap` bytes that begins with src[0, n): the same bytes in a bigger block, a tail carried over
  static std::shared_ptr<Buf> block(size_t cap, const uint8_t *src = nullptr, size_t n = 0) {
    auto b = std::make_shared<Buf>();
    b->v.resize(cap);
    if (n) memcpy(b->v.data(), src, n);
    return b;
  }

 private:
  struct Cache {
    std::mutex m;
    std::vector<std::pair<size_t, uint8_t *>> blocks;
    ~Cache() {
      for (auto &b : blocks) free(b.second);
    }
  };
  static Cache &cache() {
    static Cache c;
    return c;
  }
  static uint8_t *acquire(size_t n) {
    if (!n) return nullptr;
    {
      Cache &c = cache();
      std::lock_guard<std::mutex> lk(c.m);
      for (size_t i = 0; i < c.blocks.size(); ++i)
        if (c.blocks[i].first == n) {
          uint8_t *p = c.blocks[i].second;
          c.blocks.erase(c.blocks.begin() + (long)i);
          return p;
        }
    }
    uint8_t *p = (uint8_t *)malloc(n);
    if (!p) throw std::bad_alloc();
    return p;
  }
  static void release(uint8_t *p, size_t n) {
    if (!p) return;
    Cache &c = cache();
    {
      std::lock_guard<std::mutex> lk(c.m);
      if (c.blocks.size() < 12) {
        c.blocks.emplace_back(n, p);
        return;
      }
    }
    free(p);
  }
};
struct Window {
  std::shared_ptr<Buf> hold;  // what keeps the bytes alive (null: the producer's mapping)
  const char *p = nullptr;
  size_t n = 0;
  bool last = false;  // the file's last window (any other ends with '\n')
};

// An array that is not value-initialised (the line tables of a 128 MiB window are megabytes: zero-filling them, by one
// thread, was a third of the window's parse).
template <class T>
struct UBuf {
  std::unique_ptr<T[]> p;
  size_t n = 0, cap = 0;
  void resize_discard(size_t m) {  // (contents are lost when it has to grow)
    if (m > cap) {
      p.reset(new T[m]);
      cap = m;
    }
    n = m;
  }
  void grow(size_t m, size_t keep) {  // the first `keep` entries in an array of m
    std::unique_ptr<T[]> q(new T[m]);
    memcpy(q.get(), p.get(), keep * sizeof(T));
    p = std::move(q);
    n = cap = m;
  }
  T *data() { return p.get(); }
  const T *data() const { return p.get(); }
  size_t size() const { return n; }
  T &operator[](size_t i) { return p[i]; }
  const T &operator[](size_t i) const { return p[i]; }
};

struct Source {
  size_t window = 128u << 20;
  virtual ~Source() {}
  virtual bool next(Window *w) = 0;  // false: no window is left
  // What reading on behind the last byte reports (IO_NONE: a clean end of file), given the CRC-32 and the length of
  // all the windows' bytes.  Valid once the window with `last` set has been handed out.
  virtual IoError finish(uint32_t, uint64_t) { return IoError(); }
  virtual bool wants_crc() const { return false; }
  virtual void cancel() {}
};

// where a decoder's windows go (GzSource: its queue to the parse)
struct WindowSink {
  virtual ~WindowSink() {}
  virtual void emit(Window &&w) = 0;  // may block; drops the window once stopped
  virtual bool stopped() = 0;        // nobody wants any more windows: the decoder returns
};

// ---- the rolling output buffer of a decoder ------------------------------------------------------------------------
// The decoder writes behind `pos`; [line0, pos) has not been handed on yet; `gone` bytes of the stream have left the
// block's front, so stream offset s lies at s − gone.  A roll hands the whole lines in front of pos − HOLD_BACK on as a
// window and starts a fresh block with the last max(32 KiB, unfinished line) bytes: the decoder's history, and every
// window is whole lines.
struct LineWindows {
  // no window is handed on while fewer than this many decoded bytes lie behind its end: the cut of a corrupt stream
  // (GzSource::reference_has_seen) then never has to take anything back
  static constexpr size_t HOLD_BACK = 8192;
  size_t window;  // text a block takes before it rolls
  std::shared_ptr<Buf> b;
  size_t pos = 0, line0 = 0;
  uint64_t gone = 0;
  explicit LineWindows(size_t window_) : window(window_), b(Buf::block(cap())) {}
  size_t cap() const { return window + 32768 + Inflater::OUT_SLACK; }  // a block's least size
  uint8_t *data() const { return b->v.data(); }
  size_t room() const { return b->v.size() - pos; }  // behind data() + pos
  void advance(size_t n) { pos += n; }
  uint64_t appended() const { return gone + pos; }  // the stream offset of pos
  InflateStatus inflate(Inflater &inf) { return inf.run(data(), &pos, b->v.size()); }

  // The inflater has run out of room.  (A line longer than the block: a block twice as large, everything moves along.)
  void roll(WindowSink &sink) {
    const size_t cut = line_end();
    if (cut == line0) b = Buf::block(b->v.size() * 2, data(), pos);
    else carry(cut, std::max(cap(), keep_behind(cut) + window + Inflater::OUT_SLACK), sink);
  }
  // Room for `need` more bytes behind pos.  (Sizes in steps of 8 MiB: Buf keeps blocks for reuse by their exact size.)
  void roll(size_t need, WindowSink &sink) {
    if (room() >= need + Inflater::OUT_SLACK) return;
    const size_t cut = line_end(), step = 8u << 20;
    carry(cut, std::max(cap(), (keep_behind(cut) + std::max(need, window) + Inflater::OUT_SLACK + step - 1) & ~(step - 1)), sink);
  }
  // The last window: everything not handed on yet in front of stream offset `stream_end` (≥ the offset of line0: the
  // last HOLD_BACK bytes are never handed on before).
  void finish(uint64_t stream_end, WindowSink &sink) {
    sink.emit(Window{b, (const char *)data() + line0, (size_t)(stream_end - gone) - line0, true});
  }

 private:
  size_t line_end() const {  // behind the last '\n' in front of pos − HOLD_BACK (line0: no line ends there)
    const size_t held = std::min(pos - line0, HOLD_BACK);
    const void *nl = memrchr(data() + line0, '\n', pos - held - line0);
    return nl ? (size_t)((const uint8_t *)nl - data()) + 1 : line0;
  }
  size_t keep_behind(size_t cut) const { return std::min(pos, std::max<size_t>(32768, pos - cut)); }
  void carry(size_t cut, size_t block_size, WindowSink &sink) {
    const size_t keep = keep_behind(cut);
    auto nb = Buf::block(block_size, data() + pos - keep, keep);
    if (cut > line0) sink.emit(Window{b, (const char *)data() + line0, cut - line0, false});
    line0 = keep - (pos - cut);
    gone += pos - keep;
    pos = keep;
    b = std::move(nb);
  }
};

// ---- one member, many threads -------------------------------------------------------------------------------------
// A DEFLATE stream is one long dependency chain (every block's matches reach into the 32 KiB before it), and one
// thread inflates ≈1.2 GB/s of FASTQ — 0.6 Gbases/s, three orders of magnitude under the counting rate.  The
// two-pass scheme of parallel gzip readers (pugz, rapidgzip) breaks the chain:
//   1. the compressed bytes are cut into chunks; a worker per chunk FINDS a block boundary behind its cut (a bit
//      position where a dynamic-Huffman header parses, its block decodes and another header follows) and decodes from
//      there SPECULATIVELY into 16-bit symbols — a byte, or "byte w of the 32 KiB in front of my entry point, which I
//      do not know" (Inflater::run_symbols) — up to the first block boundary behind the next cut;
//   2. the caller's thread goes through the chunks in order.  A chunk's result counts only if its entry point is
//      EXACTLY where the verified decoding before it ended; what lies between (a stored or fixed block the finder does
//      not look for, a chunk whose speculation failed) is decoded there, the ordinary way.  With the window in front of
//      a chunk known, its symbols become bytes — any of them independently of the others, so the last 32 KiB (the next
//      chunk's window) at once, and all of them by the workers, chunks side by side.
// What comes out — bytes, their order, the final status and where the stream ended — is the sequential decoder's:
// nothing speculative is ever handed on unverified, and an error is only ever reported by a verified position.
struct SpecResult {
  UBuf<uint16_t> sym;
  size_t n = 0;
  bool found = false, ready = false;
  uint64_t start_bit = 0, end_bit = 0;
  InflateStatus status = INF_CORRUPT;
  const uint8_t *after = nullptr;
  double seconds = 0, find_seconds = 0;  // (debug: the worker's time on this chunk, and of it the search for the entry point)
};
struct Workers {  // a small two-priority pool of the decoder's own
  std::vector<std::thread> th;
  std::mutex m;
  std::condition_variable cv;
  std::deque<std::function<void()>> hi, lo;
  bool quit = false;
  // n threads take whatever there is, urgent work first; n_urgent more take urgent work only — a chunk's bytes are
  // wanted NOW (the windows go out in order), and a worker deep in a 10 ms speculative decode is no help with that
  Workers(uint32_t n, uint32_t n_urgent) {
    for (uint32_t i = 0; i < n + n_urgent; ++i)
      th.emplace_back([this, only_urgent = i >= n] {
        for (;;) {
          std::function<void()> f;
          {
            std::unique_lock<std::mutex> lk(m);
            cv.wait(lk, [&] { return quit || !hi.empty() || (!only_urgent && !lo.empty()); });
            if (hi.empty() && (only_urgent || lo.empty())) {
              if (quit) return;
              continue;
            }
            auto &q = hi.empty() ? lo : hi;
            f = std::move(q.front());
            q.pop_front();
          }
          f();
        }
      });
  }
  void post(bool urgent, std::function<void()> f) {
    {
      std::lock_guard<std::mutex> lk(m);
      (urgent ? hi : lo).emplace_back(std::move(f));
    }
    cv.notify_all();
  }
  ~Workers() {
    {
      std::lock_guard<std::mutex> lk(m);
      quit = true;
      lo.clear();  // (speculation nobody will look at)
    }
    cv.notify_all();
    for (auto &t : th) t.join();
  }
};
inline double now_seconds() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
inline bool plausible_header_at(const uint8_t *origin, const uint8_t *end, uint64_t bit) {
  // BFINAL = 0, BTYPE = 2 (bits 0, 0, 1), HLIT ≤ 29, HDIST ≤ 29: what an encoder's dynamic, non-final block starts with
  const uint8_t *p = origin + (bit >> 3);
  if (end - p < 4) return false;
  uint32_t w;
  memcpy(&w, p, 4);
  w >>= (uint32_t)(bit & 7);
  return (w & 7u) == 4u && ((w >> 3) & 31u) <= 29u && ((w >> 8) & 31u) <= 29u;
}
// The speculative decode of a chunk: entry point at or behind bit lo, output up to the first block boundary at or
// behind bit hi.
inline void speculate(SpecResult *r, const uint8_t *origin, const uint8_t *end, uint64_t lo, uint64_t hi, size_t guess) {
  const double t_begin = now_seconds();
  struct Note {
    SpecResult *r;
    double t0;
    ~Note() { r->seconds = now_seconds() - t0; }
  } note{r, t_begin};
  Inflater inf;
  r->sym.resize_discard(guess + 65536);
  // whole blocks up to the first boundary at or behind `to`, in a symbol buffer that grows as they need
  auto run_to = [&](size_t *pos, uint64_t to, bool *between) {
    for (;;) {
      const InflateStatus st = inf.run_symbols(r->sym.data(), pos, r->sym.size(), origin, to, between);
      if (st != INF_OUTPUT_FULL || *between) return st;
      r->sym.grow(r->sym.size() * 2, *pos);
    }
  };
  const uint64_t total_bits = (uint64_t)(end - origin) * 8;
  for (uint64_t p = lo; p < hi && p + 64 < total_bits; ++p) {
    if (!plausible_header_at(origin, end, p)) continue;
    inf.seek(origin, end, p);
    if (inf.read_block_header() != INF_OUTPUT_FULL || inf.state != 2 || inf.last_block || !inf.hdr_plausible) continue;
    // its block must decode, and a header must follow it
    size_t pos = 0;
    bool between = false;
    InflateStatus st = run_to(&pos, p + 1, &between);
    if (st != INF_OUTPUT_FULL || !between) continue;
    {
      Inflater peek = inf;
      if (peek.read_block_header() == INF_CORRUPT) continue;
    }
    // accepted: go on to the first block boundary at or behind `hi`
    r->found = true;
    r->start_bit = p;
    r->find_seconds = now_seconds() - t_begin;
    st = run_to(&pos, hi, &between);
    r->n = pos;
    r->status = st;
    r->end_bit = inf.bit_position(origin);
    if (st == INF_STREAM_END) r->after = inf.input_after_stream();
    return;
  }
}
// Symbols as bytes, with the window in front of their entry point known: win[0, w_len), w_len ≤ 32768.  Symbol 256 + w
// means byte w of a FULL 32 KiB window; with less decoded so far the window's first 32768 − w_len places do not exist:
// a reference to one is no valid stream (the ordinary decoder says "distance too far back"), a chunk entered at a
// verified position never has any (symbols_in_window says so before anything of it is used), and it gives 0 here.
inline void symbols_to_bytes(const uint16_t *sym, size_t n, const uint8_t *win, size_t w_len, uint8_t *out) {
  const size_t shift = 32768 - w_len;
  for (size_t j = 0; j < n; ++j) {
    const uint16_t s = sym[j];
    out[j] = s < 256 ? (uint8_t)s : ((size_t)(s - 256) >= shift ? win[(size_t)(s - 256) - shift] : (uint8_t)0);
  }
}
inline bool symbols_in_window(const uint16_t *sym, size_t n, size_t w_len) {
  const size_t shift = 32768 - w_len;
  for (size_t j = 0; shift && j < n; ++j)
    if (sym[j] >= 256 && (size_t)(sym[j] - 256) < shift) return false;
  return true;
}

struct ParallelInflate {
  struct Result {
    InflateStatus status = INF_TRUNCATED;  // the sequential decoder's
    const uint8_t *after = nullptr;        // INF_STREAM_END: the first input byte behind the stream
    uint64_t verified_bit = 0;             // everything in front of it has been decoded and checked
    bool stopped = false;                  // the sink said so: nothing below counts
    Window last;                           // the stream's last window, for the caller to hand on once it has taken the rest
  };
  // the stream's bytes a reader is to get when the stream is corrupt, given the n_ok bytes in front of the damage and
  // the input byte the decoder stood at (GzSource::reference_has_seen); none: all of them
  using SeenOfCorrupt = std::function<uint64_t(uint64_t n_ok, const uint8_t *fail)>;

  ParallelInflate(const uint8_t *origin_, const uint8_t *end_, uint32_t n_threads_, size_t chunk_bytes_, WindowSink &sink_, SeenOfCorrupt seen_ = nullptr)
      : origin(origin_), end(end_), n_threads(n_threads_), chunk_bytes(chunk_bytes_), n_chunks(((size_t)(end_ - origin_) + chunk_bytes_ - 1) / chunk_bytes_),
        sink(sink_), seen(std::move(seen_)), spec(n_chunks), pool(n_threads_, std::max(2u, n_threads_ / 4)) {}

  // chunk 0, then chunk after chunk; every window but the last goes to the sink
  Result run() {
    issue_up_to(ahead());
    decode_here((uint64_t)chunk_bytes * 8);
    size_t next = 1;
    while (status == INF_OUTPUT_FULL && !cancelled && !(cancelled = sink.stopped())) {
      drain(6);
      if (next >= n_chunks) {  // behind the last cut: the rest of the stream, the ordinary way
        decode_here(~0ull);
        continue;
      }
      issue_up_to(next + ahead());
      SpecResult &r = spec[next];
      {
        const double t0 = now_seconds();
        std::unique_lock<std::mutex> lk(rm);
        rcv.wait(lk, [&] { return r.ready; });
        dbg.wait_spec += now_seconds() - t0;
        dbg.workers += r.seconds;
        dbg.find += r.find_seconds;
      }
      const uint64_t chunk_end_bit = (uint64_t)(next + 1) * chunk_bytes * 8;
      if (r.found && r.start_bit == verified && symbols_in_window(r.sym.data(), r.n, W.size())) {
        resolve(r);
      } else if (r.found && r.start_bit > verified) {  // something the finder does not look for lies in between
        decode_here(r.start_bit);
        if (verified == r.start_bit) continue;  // (else it was no block boundary after all: that chunk's result is void)
      } else if (r.found && r.start_bit == verified) {
        decode_here(chunk_end_bit);  // (a symbol in front of everything decoded: the ordinary decoder says what is wrong)
      } else if (chunk_end_bit > verified) {
        // no entry point found in this chunk, or one in front of where the stream really stands: the ordinary way
        decode_here(chunk_end_bit);
      }
      // A chunk whose speculation is passed over gives its symbol buffer back at once (12 MB or more each, touched by
      // the worker): a member where the finder keeps missing — stored or fixed blocks, false block starts — would
      // otherwise hold one per chunk until its end, memory growing with the file.  (resolve() has moved it away.)
      r.sym = UBuf<uint16_t>();
      r.n = 0;
      ++next;
    }
    Result res;
    if (!cancelled) finish(&res);
    res.stopped = cancelled;
    if (getenv("SHK_FASTQ_DEBUG"))
      fprintf(stderr, "[gzip member, %u threads, %zu chunks of %zu KiB] %zu chunks (%.1f MB) from the workers, %zu stretches (%.1f MB) decoded in order\n",
              n_threads, n_chunks, chunk_bytes >> 10, dbg.n_spec_used, dbg.bytes_spec / 1e6, dbg.n_here, dbg.bytes_here / 1e6),
          fprintf(stderr, "   workers %.0f ms in all (%.0f ms of it looking for entry points); this thread waited %.0f ms for chunks, %.0f ms for their bytes, %.0f ms handing windows on\n",
                  dbg.workers * 1e3, dbg.find * 1e3, dbg.wait_spec * 1e3, dbg.wait_resolve * 1e3, dbg.emit * 1e3);
    return res;
    // (the workers are joined by ~Workers: what is still queued of the speculation is dropped)
  }

 private:
  // a piece of output on its way out: [window w_len][n bytes] in one block; `pending` jobs still write into it
  // (a count the workers take down and this thread sleeps on — it used to spin with yield())
  struct Pending {
    std::mutex m;
    std::condition_variable cv;
    int n = 0;
    void set(int k) {
      std::lock_guard<std::mutex> lk(m);
      n = k;
    }
    void done() {
      std::lock_guard<std::mutex> lk(m);
      if (--n <= 0) cv.notify_all();
    }
    void wait() {
      std::unique_lock<std::mutex> lk(m);
      cv.wait(lk, [&] { return n <= 0; });
    }
  };
  struct Piece {
    std::shared_ptr<Buf> buf;
    size_t w_len = 0, n = 0;
    std::shared_ptr<Pending> pending;
  };
  struct Debug {  // SHK_FASTQ_DEBUG's report
    size_t n_spec_used = 0, n_here = 0;  // chunks taken from the workers / stretches decoded by this thread
    uint64_t bytes_spec = 0, bytes_here = 0;
    double workers = 0, find = 0, wait_spec = 0, wait_resolve = 0, emit = 0;
  };

  const uint8_t *const origin, *const end;
  const uint32_t n_threads;
  const size_t chunk_bytes, n_chunks;
  WindowSink &sink;
  SeenOfCorrupt seen;
  std::vector<SpecResult> spec;
  std::mutex rm;  // spec[i].ready
  std::condition_variable rcv;
  size_t issued = 1;  // (chunk 0 starts at the stream's start: decoded by run(), the ordinary way)
  std::deque<Piece> out_q;
  std::vector<uint8_t> W;      // the last ≤ 32 KiB of everything decoded so far
  std::vector<uint8_t> carry;  // the bytes of the last, unfinished line (they are also the tail of W when they fit)
  uint64_t verified = 0;       // bit position everything in front of which has been decoded and checked
  InflateStatus status = INF_OUTPUT_FULL;
  const uint8_t *after = nullptr;
  uint64_t emitted_out = 0;  // bytes of the pieces that have left out_q
  bool cancelled = false;
  Debug dbg;
  Workers pool;  // (the last member: joined before anything its jobs point to goes)

  size_t ahead() const { return (size_t)n_threads + 2; }
  void issue_up_to(size_t upto) {
    for (; issued < n_chunks && issued <= upto; ++issued) {
      const size_t i = issued;
      pool.post(false, [this, i] {
        speculate(&spec[i], origin, end, (uint64_t)i * chunk_bytes * 8, (uint64_t)(i + 1) * chunk_bytes * 8, chunk_bytes * 6);
        {
          std::lock_guard<std::mutex> lk(rm);
          spec[i].ready = true;
        }
        rcv.notify_all();
      });
    }
  }
  // the front piece as a window of whole lines (its last line's beginning is carried into the next); n = 0 and not
  // last: no line ends in it, all of it is carried on
  Window take_front(bool last) {
    Piece pc = std::move(out_q.front());
    out_q.pop_front();
    const double t0 = now_seconds();
    if (pc.pending) pc.pending->wait();
    dbg.wait_resolve += now_seconds() - t0;
    uint8_t *base = pc.buf->v.data();
    size_t a = pc.w_len, b = pc.w_len + pc.n;
    if (!carry.empty()) {  // the line begun in the piece before: it lies right in front of this piece's bytes
      if (carry.size() <= pc.w_len && memcmp(base + pc.w_len - carry.size(), carry.data(), carry.size()) == 0) {
        a = pc.w_len - carry.size();
      } else {  // (longer than the window in front: a block of its own)
        auto nb = Buf::block(carry.size() + pc.n + 64, carry.data(), carry.size());
        memcpy(nb->v.data() + carry.size(), base + pc.w_len, pc.n);
        pc.buf = nb;
        base = nb->v.data();
        a = 0;
        b = carry.size() + pc.n;
      }
    }
    size_t cut = b;
    if (!last) {
      const void *nl = b > a ? memrchr(base + a, '\n', b - a) : nullptr;
      cut = nl ? (size_t)((const uint8_t *)nl - base) + 1 : a;
    }
    carry.assign(base + cut, base + b);
    return Window{pc.buf, (const char *)base + a, cut - a, last};
  }
  void emit_front() {
    Window w = take_front(false);
    const double t0 = now_seconds();
    if (w.n && !(cancelled = sink.stopped())) sink.emit(std::move(w));
    dbg.emit += now_seconds() - t0;
  }
  std::shared_ptr<Buf> new_piece_block(size_t n) { return Buf::block(W.size() + n + Inflater::OUT_SLACK + 64, W.data(), W.size()); }
  void roll_window(const uint8_t *bytes, size_t n) {  // W := last 32 KiB of W ++ bytes
    if (n >= 32768) {
      W.assign(bytes + n - 32768, bytes + n);
    } else {
      const size_t keep = std::min(W.size(), (size_t)32768 - n);
      std::vector<uint8_t> nw(W.end() - (long)keep, W.end());
      nw.insert(nw.end(), bytes, bytes + n);
      W.swap(nw);
    }
  }
  // the ordinary decoder from the verified position on, up to the first block boundary at or behind `to_bit`
  void decode_here(uint64_t to_bit) {
    Inflater inf;
    inf.seek(origin, end, verified);
    inf.stop_origin = origin;
    inf.stop_bit = to_bit;
    size_t cap = std::max<size_t>(chunk_bytes * 6, 1u << 20);
    auto b = new_piece_block(cap);
    const size_t w_len = W.size();
    size_t pos = w_len;
    InflateStatus st;
    while ((st = inf.run(b->v.data(), &pos, w_len + cap)) == INF_OUTPUT_FULL && !inf.stopped_between_blocks) {  // more room
      cap *= 2;
      b = Buf::block(w_len + cap + Inflater::OUT_SLACK + 64, b->v.data(), pos);
      if ((cancelled = sink.stopped())) break;
    }
    Piece pc;
    pc.buf = b;
    pc.w_len = w_len;
    pc.n = pos - w_len;
    roll_window(b->v.data() + w_len, pc.n);
    ++dbg.n_here;
    dbg.bytes_here += pc.n;
    out_q.emplace_back(std::move(pc));
    verified = inf.bit_position(origin);
    if (st != INF_OUTPUT_FULL) {
      status = st;
      if (st == INF_STREAM_END) after = inf.input_after_stream();
    }
  }
  // a verified chunk: its window is known now — the next chunk's window at once, its bytes by the workers
  void resolve(SpecResult &r) {
    const size_t n = r.n, w_len = W.size();
    ++dbg.n_spec_used;
    dbg.bytes_spec += n;
    verified = r.end_bit;
    if (r.status != INF_OUTPUT_FULL) {
      status = r.status;
      after = r.after;
    }
    Piece pc;
    pc.buf = new_piece_block(n);
    pc.w_len = w_len;
    pc.n = n;
    pc.pending = std::make_shared<Pending>();
    // the next window first (the last 32 KiB of this chunk's bytes), by this thread
    {
      const size_t t0 = n > 32768 ? n - 32768 : 0;
      std::vector<uint8_t> tail(n - t0);
      symbols_to_bytes(r.sym.data() + t0, n - t0, pc.buf->v.data(), w_len, tail.data());
      roll_window(tail.data(), tail.size());
    }
    // all of it, in slices, by the workers
    const size_t slice = 1u << 20;
    const size_t n_slices = (n + slice - 1) / slice;
    pc.pending->set((int)n_slices);
    auto keep = std::make_shared<SpecResult>(std::move(r));
    for (size_t sl = 0; sl < n_slices; ++sl) {
      const size_t j0 = sl * slice, j1 = std::min(n, j0 + slice);
      pool.post(true, [keep, b = pc.buf, w_len, j0, j1, pend = pc.pending] {
        symbols_to_bytes(keep->sym.data() + j0, j1 - j0, b->v.data(), w_len, b->v.data() + w_len + j0);
        pend->done();
      });
    }
    out_q.emplace_back(std::move(pc));
  }
  // (a piece goes out only while HOLD_BACK decoded bytes lie behind it: see GzSource::reference_has_seen)
  void drain(size_t keep_n) {
    while (out_q.size() > keep_n && !cancelled) {
      size_t behind = 0;
      for (size_t i = 1; i < out_q.size() && behind < LineWindows::HOLD_BACK; ++i) behind += out_q[i].n;
      if (behind < LineWindows::HOLD_BACK) break;
      emitted_out += out_q.front().n;
      emit_front();
    }
  }
  // the stream has ended: what is left goes out, cut where a reader of a corrupt stream stops seeing it
  void finish(Result *res) {
    if (out_q.empty()) {  // (nothing at all was decoded)
      Piece pc;
      pc.buf = Buf::block(64);
      out_q.emplace_back(std::move(pc));
    }
    res->status = status == INF_OUTPUT_FULL ? INF_TRUNCATED : status;
    res->after = after;
    res->verified_bit = verified;
    if (res->status == INF_CORRUPT && seen) {
      uint64_t n_ok = emitted_out;
      for (const Piece &pc : out_q) n_ok += pc.n;
      uint64_t cut = n_ok - seen(n_ok, origin + (verified >> 3));
      while (cut && !out_q.empty()) {  // (off the tail: resolved pieces first — their bytes are being written by workers)
        Piece &pc = out_q.back();
        const size_t t = (size_t)std::min<uint64_t>(cut, pc.n);
        pc.n -= t;
        cut -= t;
        if (pc.n == 0 && out_q.size() > 1) {
          if (pc.pending) pc.pending->wait();
          out_q.pop_back();
        } else if (pc.n == 0) {
          break;
        }
      }
    }
    while (out_q.size() > 1 && !cancelled) emit_front();
    if (!cancelled) res->last = take_front(true);
  }
};

}  // namespace gzsrc
}  // namespace shk
