// shk_fastq_api.hip.h — FASTQ text framed on the device: shk_fastq_parse_device and
// shk_crc32_members_device over K_FASTQ, and shk_ingest_fastq_files_device, the route that strings K_INFLATE, the CRC-32
// and the framing together so that a bgzip'd file's text never leaves device memory.  Included at the end of
// shk_engine.hip.
#include "shk_inflate.h"

#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

namespace {

struct FastqDeviceTotals {
  std::atomic<uint64_t> batches{0}, records{0}, give_ups{0}, up{0}, down{0}, kernel_ns{0};
};
static FastqDeviceTotals &fq_totals() {
  static FastqDeviceTotals t;
  return t;
}
static_assert(sizeof(FqResultWords) == sizeof(shk_fastq_text_result) && offsetof(FqResultWords, anomaly_kind) == offsetof(shk_fastq_text_result, anomaly_kind),
              "the kernels' result words are the ABI's");
static_assert(sizeof(FqCrcJob) == sizeof(shk_crc_job) && offsetof(FqCrcJob, len) == offsetof(shk_crc_job, len), "the kernel's CRC jobs are the ABI's");

// Where a parse puts its output once the records to look at are known: the callee answers pointers and the capacity of
// the bases (offsets: room for n_look + 1), or an SHK_* code.
struct FqOut {
  uint8_t *bases = nullptr;
  uint64_t bases_cap = 0;
  uint64_t *offsets = nullptr;
};

// The passes over d_text on the context's stream; returns once the result words are back.  get_out is called between
// the two halves, with the number of records that will be looked at.  *down and *kernel_ns: the bytes this call brought
// down and its kernels' time, also where it fails — added to fq_totals() here, to a caller's own statistics by the caller.
template <typename GetOut>
static int fq_parse_core(shk_ctx *c, const uint8_t *d_text, uint64_t n, const shk_fastq_text_params &p, GetOut get_out, shk_fastq_text_result *res,
                         uint64_t *n_look_out, uint64_t *down, uint64_t *kernel_ns, bool *ends_nl_out = nullptr) {
  *down = *kernel_ns = 0;
  if (n > FQ_TEXT_MAX) return fail(c, SHK_ERR_BAD_ARG, "shk_fastq_parse_device takes at most %llu bytes of text", (unsigned long long)FQ_TEXT_MAX);
  hipStream_t st = c->stream;
  for (hipEvent_t &e : c->fq_ev)
    if (!e) HIPC(c, hipEventCreate(&e));
  const uint64_t n_tiles = (n + FQ_TILE - 1) / FQ_TILE;
  HIPC(c, c->fq_ctrl.ensure(sizeof(FqCtrl)));
  HIPC(c, c->fq_hctrl.ensure(sizeof(FqCtrl)));
  HIPC(c, c->fq_tiles.ensure((n_tiles + 1) * 8));
  FqCtrl *ctrl = (FqCtrl *)c->fq_ctrl.p, *h = (FqCtrl *)c->fq_hctrl.p;
  unsigned long long *tiles = (unsigned long long *)c->fq_tiles.p;  // counts, then (in place) the lines in front of each tile
  HIPC(c, hipMemsetAsync(ctrl, 0, sizeof(FqCtrl), st));
  HIPC(c, hipMemsetAsync(&ctrl->anomaly, 0xFF, sizeof ctrl->anomaly, st));
  HIPC(c, hipEventRecord(c->fq_ev[0], st));
  if (n_tiles) {
    k_fq_count<<<dim3((uint32_t)((n_tiles + FQ_WAVES - 1) / FQ_WAVES)), dim3(FQ_WAVES * 64), 0, st>>>(d_text, n, n_tiles, tiles, ctrl);
    k_fq_scan64<<<dim3(1), dim3(FQ_SCAN_WG), 0, st>>>(tiles, tiles, n_tiles, &ctrl->n_nl);
    HIPC(c, hipGetLastError());
  }
  HIPC(c, hipEventRecord(c->fq_ev[1], st));
  HIPC(c, hipMemcpyAsync(h, ctrl, offsetof(FqCtrl, n_bases_look), hipMemcpyDeviceToHost, st));
  HIPC(c, hipStreamSynchronize(st));
  fq_totals().down += offsetof(FqCtrl, n_bases_look);
  *down = offsetof(FqCtrl, n_bases_look);
  const uint64_t n_nl = h->n_nl;
  const uint64_t n_lines = fq_n_lines(n, n_nl, p.last != 0, h->ends_nl != 0);
  uint64_t n_look = n_lines / 4;
  if (p.max_records && n_look > p.max_records) n_look = p.max_records;
  *n_look_out = n_look;
  if (ends_nl_out) *ends_nl_out = h->ends_nl != 0;
  FqOut o;
  SHK_TRY(get_out(n_look, &o));
  const uint64_t n_blocks = (n_look + FQ_REC_WG - 1) / FQ_REC_WG;
  HIPC(c, c->fq_lines.ensure((n_nl + 1) * 4));
  Scratch m{c->fq_recs};
  const size_t o_start = m.take<uint32_t>(n_look + 1), o_len = m.take<uint32_t>(n_look + 1), o_blk = m.take<unsigned long long>(n_blocks + 1);
  HIPC(c, m.ensure());
  uint32_t *line_end = (uint32_t *)c->fq_lines.p, *seq_start = m.at<uint32_t>(o_start), *seq_len = m.at<uint32_t>(o_len);
  unsigned long long *blk = m.at<unsigned long long>(o_blk);
  HIPC(c, hipEventRecord(c->fq_ev[2], st));
  if (n_tiles)
    k_fq_lines<<<dim3((uint32_t)((n_tiles + FQ_WAVES - 1) / FQ_WAVES)), dim3(FQ_WAVES * 64), 0, st>>>(d_text, n, n_tiles, tiles, line_end, n_nl);
  if (n_look) {
    k_fq_records<<<dim3((uint32_t)n_blocks), dim3(FQ_REC_WG), 0, st>>>(d_text, n, line_end, n_nl, n_look, p.first_record, p.validate_every, ctrl, seq_start,
                                                                      seq_len, blk);
    k_fq_scan64<<<dim3(1), dim3(FQ_SCAN_WG), 0, st>>>(blk, blk, n_blocks, &ctrl->n_bases_look);
  }
  k_fq_offsets<<<dim3((uint32_t)std::max<uint64_t>(1, n_blocks)), dim3(FQ_REC_WG), 0, st>>>(seq_len, blk, n_look, (unsigned long long *)o.offsets);
  if (n_look)
    k_fq_copy<<<dim3((uint32_t)((n_look * FQ_COPY_LANES + 255) / 256)), dim3(256), 0, st>>>(d_text, seq_start, seq_len, (const unsigned long long *)o.offsets,
                                                                                           n_look, o.bases, o.bases_cap, ctrl);
  k_fq_finish<<<dim3(1), dim3(64), 0, st>>>(n, line_end, n_nl, n_look, (const unsigned long long *)o.offsets, ctrl);
  HIPC(c, hipGetLastError());
  HIPC(c, hipEventRecord(c->fq_ev[3], st));
  HIPC(c, hipMemcpyAsync(&h->res, &ctrl->res, sizeof(FqResultWords), hipMemcpyDeviceToHost, st));
  HIPC(c, hipStreamSynchronize(st));
  fq_totals().down += sizeof(FqResultWords);
  *down += sizeof(FqResultWords);
  float ms0 = 0, ms1 = 0;
  if (hipEventElapsedTime(&ms0, c->fq_ev[0], c->fq_ev[1]) == hipSuccess && hipEventElapsedTime(&ms1, c->fq_ev[2], c->fq_ev[3]) == hipSuccess)
    fq_totals().kernel_ns += *kernel_ns = (uint64_t)(((double)ms0 + (double)ms1) * 1e6);
  else
    (void)hipGetLastError();
  memcpy(res, &h->res, sizeof *res);
  return SHK_OK;
}

// ---- the route --------------------------------------------------------------------------------------------------------
constexpr uint64_t FQ_CARRY_ROOM = 4ull << 20;  // text in front of a batch's own: the record a batch border cuts (longer: give up)

struct MappedFile {
  const uint8_t *p = nullptr;
  size_t n = 0;
  ~MappedFile() {
    if (p) munmap((void *)p, n);
  }
};

// The route's run over its files: two slots, and the batches of all files as one sequence — the next one is planned and
// queued before this one is waited for.  Each step answers a give-up reason, 0: go on.
struct FastqRoute {
  struct Slot : DecodeSlot {  // up: [inflate jobs | crc jobs | compressed bytes | pad]; down: [n statuses | n crcs], 8 bytes per member and no more
    hipEvent_t passed = nullptr;  // the engine stream behind this slot's ingest (k0, k1: round the CRC kernel)
    bool passed_set = false;
    DevBuf d_text, d_bases, d_offs;
    shk::BgzfBatch b;
    bool last_of_file = false;
    ~Slot() {  // (the caller has waited for the engine stream where it had been given any of these)
      if (st) (void)hipStreamSynchronize(st);
      d_text.release();
      d_bases.release();
      d_offs.release();
      if (passed) (void)hipEventDestroy(passed);
    }
  } slot[2];
  shk_ctx *c;
  const std::vector<MappedFile> &files;
  uint64_t budget, max_reads, validate_every;
  shk_fastq_device_stats *stats;
  uint32_t f_next = 0;
  const uint8_t *p_next;
  bool input_done = false, reached_max = false;
  uint64_t carry = 0;  // bytes of text in front of the current slot's own, already in its carry room
  uint64_t n_reads = 0, n_bases = 0;

  static uint32_t own(hipError_t e) {  // a HIP call of the route's own: 0, or the reason with the error taken off
    if (e == hipSuccess) return 0;
    (void)hipGetLastError();
    return SHK_FASTQ_GIVEUP_OWN;
  }
  uint32_t open() {
    for (Slot &s : slot)
      if (!s.open() || own(hipEventCreateWithFlags(&s.passed, hipEventDisableTiming))) return SHK_FASTQ_GIVEUP_OWN;
    return 0;
  }

  // The batch feed: the next batch of the next file into s — upload, K_INFLATE, the CRCs, statuses and CRCs down, queued
  // on the slot's stream behind the engine stream's last use of the slot.  At the input's end: input_done, nothing queued.
  uint32_t feed(Slot &s) {
    while (f_next < files.size() && p_next == files[f_next].p + files[f_next].n)
      if (++f_next < files.size()) p_next = files[f_next].p;
    if (f_next >= files.size()) {
      input_done = true;
      return 0;
    }
    const uint8_t *file_end = files[f_next].p + files[f_next].n;
    if (!shk::bgzf_plan_batch(p_next, file_end, budget, &s.b)) return SHK_FASTQ_GIVEUP_MEMBER;
    s.last_of_file = s.b.end == file_end;
    const uint32_t n = (uint32_t)s.b.ms.size();
    const size_t down = (size_t)n * 8;
    if (!s.ensure_down(down) || own(s.d_text.ensure_step(FQ_CARRY_ROOM + s.b.out_bytes + 16, STAGE_STEP))) return SHK_FASTQ_GIVEUP_OWN;
    uint8_t *text = (uint8_t *)s.d_text.p + FQ_CARRY_ROOM;
    uint32_t *d_status = (uint32_t *)s.d_down.p;
    // (the ingest that read this slot's buffers last, and the carry copied out of it)
    if (s.passed_set && hipStreamWaitEvent(s.st, s.passed, 0) != hipSuccess) {
      s.drain();
      return SHK_FASTQ_GIVEUP_OWN;
    }
    auto crc_jobs = [&](uint8_t *h) {
      for (uint32_t i = 0; i < n; ++i) ((FqCrcJob *)h)[i] = FqCrcJob{s.b.jobs[i].out_offset, s.b.jobs[i].out_len, 0};
    };
    const uint8_t *d_cj = nullptr;
    const size_t up = stage_queue_inflate(s, s.b.begin, (size_t)(s.b.end - s.b.begin), s.b.jobs.data(), n, s.b.out_bytes, stage_round256((size_t)n * sizeof(FqCrcJob)),
                                          crc_jobs, &d_cj, text, d_status, down, false);  // (0xFF: INFC_NOT_RUN; no CRC yet)
    if (!up) return SHK_FASTQ_GIVEUP_OWN;
    bool ok = hipEventRecord(s.k0, s.st) == hipSuccess;
    if (ok) {
      k_crc_members<<<dim3((n + FQ_WAVES - 1) / FQ_WAVES), dim3(FQ_WAVES * 64), 0, s.st>>>(text, (const FqCrcJob *)d_cj, n, d_status + n);
      ok = hipGetLastError() == hipSuccess;
    }
    ok = ok && hipEventRecord(s.k1, s.st) == hipSuccess;
    ok = ok && hipMemcpyAsync(s.h_down.p, d_status, down, hipMemcpyDeviceToHost, s.st) == hipSuccess;
    if (!ok) {
      s.drain();
      return SHK_FASTQ_GIVEUP_OWN;
    }
    s.queued = true;
    p_next = s.b.end;
    stats->bytes_up += up;
    stats->bytes_down += down;  // (exactly what the copy above brings down)
    stats->n_members += n;
    stats->n_batches += 1;
    return 0;
  }

  // The slot's stream waited for; every member's status and CRC-32.
  uint32_t wait_and_check(Slot &s) {
    s.queued = false;
    if (own(hipStreamSynchronize(s.st))) return SHK_FASTQ_GIVEUP_OWN;
    float ms = 0;
    if (hipEventElapsedTime(&ms, s.k0, s.k1) == hipSuccess) {
      stats->kernel_ns += (uint64_t)((double)ms * 1e6);
      fq_totals().kernel_ns += (uint64_t)((double)ms * 1e6);
    }
    const uint32_t n = (uint32_t)s.b.ms.size();
    const uint32_t *status = (const uint32_t *)s.h_down.p, *crc = status + n;
    for (uint32_t i = 0; i < n; ++i) {
      if (status[i] != INFC_OK) return SHK_FASTQ_GIVEUP_DECODE;
      if (crc[i] != s.b.ms[i].crc) return SHK_FASTQ_GIVEUP_CRC;
    }
    return 0;
  }

  // The framing over carry + text and the ingest, on the engine stream (the slot's stream has been waited for), and the
  // text behind the last record to the front of nx's.
  uint32_t frame_ingest_carry(Slot &s, Slot &nx) {
    const uint64_t n_text = carry + s.b.out_bytes;
    const uint8_t *text = (const uint8_t *)s.d_text.p + FQ_CARRY_ROOM - carry;
    shk_fastq_text_params p{};
    p.first_record = n_reads;
    p.validate_every = validate_every;
    p.max_records = max_reads ? max_reads - n_reads : 0;
    p.last = s.last_of_file;
    auto get_out = [&](uint64_t n_look, FqOut *o) -> int {
      if (own(s.d_bases.ensure_step(n_text + 64, STAGE_STEP)) || own(s.d_offs.ensure_step((n_look + 1) * 8, STAGE_STEP))) return SHK_ERR_NOMEM;
      *o = FqOut{(uint8_t *)s.d_bases.p, n_text, (uint64_t *)s.d_offs.p};  // (the sequences are part of the text: never more bytes than it has)
      return SHK_OK;
    };
    shk_fastq_text_result r{};
    uint64_t n_look = 0;
    uint64_t down = 0, ns = 0;
    bool ends_nl = false;
    const int prc = fq_parse_core(c, text, n_text, p, get_out, &r, &n_look, &down, &ns, &ends_nl);
    stats->bytes_down += down;
    stats->kernel_ns += ns;
    if (prc != SHK_OK) return SHK_FASTQ_GIVEUP_OWN;
    if (r.anomaly_record != FQ_NO_ANOMALY) return SHK_FASTQ_GIVEUP_ANOMALY;
    // a file whose last line is not terminated ends inside a record, or may: the host decides
    if (s.last_of_file && n_text && !ends_nl) return SHK_FASTQ_GIVEUP_TEXT_LEFT;
    if (r.n_records && shk_ingest_reads_device(c, s.d_bases.p, s.d_offs.p, r.n_records, r.n_bases) != SHK_OK) return SHK_FASTQ_GIVEUP_OWN;
    n_reads += r.n_records;
    n_bases += r.n_bases;
    reached_max = max_reads && n_reads >= max_reads;
    if (reached_max) return 0;
    const uint64_t left = n_text - r.bytes_consumed;
    if (s.last_of_file) {
      carry = 0;
      return left ? SHK_FASTQ_GIVEUP_TEXT_LEFT : 0;
    }
    if (left > FQ_CARRY_ROOM || !nx.queued) return SHK_FASTQ_GIVEUP_OWN;  // (a batch that does not end its file has one behind it)
    if (left && own(hipMemcpyAsync((uint8_t *)nx.d_text.p + FQ_CARRY_ROOM - left, text + r.bytes_consumed, left, hipMemcpyDeviceToDevice, c->stream)))
      return SHK_FASTQ_GIVEUP_OWN;
    carry = left;
    return 0;
  }

  // The hand-back: this slot's buffers are free again once the engine stream has passed the ingest (and the copy of the carry).
  uint32_t hand_back(Slot &s) {
    if (own(hipEventRecord(s.passed, c->stream))) return SHK_FASTQ_GIVEUP_OWN;
    s.passed_set = true;
    return 0;
  }
};

// Maps the files; every one a regular, non-empty file whose first member is a BGZF one.  0, or NOT_ELIGIBLE.
static uint32_t fq_route_map(const char *const *paths, uint32_t n_paths, std::vector<MappedFile> *files) {
  files->resize(n_paths);
  for (uint32_t f = 0; f < n_paths; ++f) {
    struct stat sb;
    const int fd = paths[f] ? open(paths[f], O_RDONLY | O_CLOEXEC) : -1;
    if (fd < 0) return SHK_FASTQ_GIVEUP_NOT_ELIGIBLE;
    if (fstat(fd, &sb) != 0 || !S_ISREG(sb.st_mode) || sb.st_size <= 0) {
      close(fd);
      return SHK_FASTQ_GIVEUP_NOT_ELIGIBLE;
    }
    void *m = mmap(nullptr, (size_t)sb.st_size, PROT_READ, MAP_PRIVATE, fd, 0);
    close(fd);
    if (m == MAP_FAILED) return SHK_FASTQ_GIVEUP_NOT_ELIGIBLE;
    MappedFile &mf = (*files)[f];
    mf.p = (const uint8_t *)m;
    mf.n = (size_t)sb.st_size;
    std::vector<shk::BgzfMember> first;
    if (shk::bgzf_scan(mf.p, mf.p + mf.n, 0, &first) == mf.p) return SHK_FASTQ_GIVEUP_NOT_ELIGIBLE;
  }
  return 0;
}

}  // namespace

extern "C" {

void shk_fastq_parse_geometry(uint32_t *tile_bytes) {
  if (tile_bytes) *tile_bytes = FQ_TILE;
}

int shk_fastq_device_totals(uint64_t *n_batches, uint64_t *n_records, uint64_t *n_give_ups, uint64_t *bytes_up, uint64_t *bytes_down, uint64_t *kernel_ns) {
  FastqDeviceTotals &t = fq_totals();
  if (n_batches) *n_batches = t.batches.load();
  if (n_records) *n_records = t.records.load();
  if (n_give_ups) *n_give_ups = t.give_ups.load();
  if (bytes_up) *bytes_up = t.up.load();
  if (bytes_down) *bytes_down = t.down.load();
  if (kernel_ns) *kernel_ns = t.kernel_ns.load();
  return SHK_OK;
}

int shk_fastq_parse_device(shk_ctx *c, const void *d_text, uint64_t n_bytes, const shk_fastq_text_params *params, void *d_bases, uint64_t bases_cap,
                           void *d_offsets, uint64_t offsets_cap, shk_fastq_text_result *out) {
  SHK_TRY(xs_closed(c));
  SHK_TRY(single_device_only(c));
  if (!params || !out || (n_bytes && !d_text)) return fail(c, SHK_ERR_BAD_ARG, "shk_fastq_parse_device: a null argument");
  HIPC(c, hipSetDevice(c->cfg.device));
  bool short_offsets = false;
  auto get_out = [&](uint64_t n_look, FqOut *o) -> int {
    if (n_look + 1 > offsets_cap || !d_offsets) {  // the offsets go to scratch and no base anywhere: the call still says what the text needs
      short_offsets = true;
      HIPC(c, c->fq_offs.ensure((n_look + 1) * 8));
      *o = FqOut{nullptr, 0, (uint64_t *)c->fq_offs.p};
    } else {
      *o = FqOut{(uint8_t *)d_bases, d_bases ? bases_cap : 0, (uint64_t *)d_offsets};
    }
    return SHK_OK;
  };
  uint64_t n_look = 0;
  uint64_t down = 0, ns = 0;
  SHK_TRY(fq_parse_core(c, (const uint8_t *)d_text, n_bytes, *params, get_out, out, &n_look, &down, &ns));
  fq_totals().records += out->n_records;
  if (short_offsets) {
    const uint64_t need = out->n_records;
    return fail(c, SHK_ERR_BAD_ARG, "shk_fastq_parse_device: offsets_cap %llu, the text needs %llu", (unsigned long long)offsets_cap, (unsigned long long)need + 1);
  }
  if (out->n_bases > (d_bases ? bases_cap : 0))
    return fail(c, SHK_ERR_BAD_ARG, "shk_fastq_parse_device: bases_cap %llu, the text needs %llu", (unsigned long long)bases_cap, (unsigned long long)out->n_bases);
  return SHK_OK;
}

int shk_crc32_members_device(shk_ctx *c, const void *d_text, const void *d_jobs, uint32_t n, void *d_crc) {
  SHK_TRY(xs_closed(c));
  SHK_TRY(single_device_only(c));
  if (n && (!d_jobs || !d_crc)) return fail(c, SHK_ERR_BAD_ARG, "shk_crc32_members_device: a null argument");
  if (!n) return SHK_OK;
  HIPC(c, hipSetDevice(c->cfg.device));
  for (hipEvent_t &e : c->fq_ev)
    if (!e) HIPC(c, hipEventCreate(&e));
  HIPC(c, hipEventRecord(c->fq_ev[0], c->stream));
  k_crc_members<<<dim3((n + FQ_WAVES - 1) / FQ_WAVES), dim3(FQ_WAVES * 64), 0, c->stream>>>((const uint8_t *)d_text, (const FqCrcJob *)d_jobs, n, (uint32_t *)d_crc);
  HIPC(c, hipGetLastError());
  HIPC(c, hipEventRecord(c->fq_ev[1], c->stream));
  HIPC(c, hipStreamSynchronize(c->stream));
  float ms = 0;
  if (hipEventElapsedTime(&ms, c->fq_ev[0], c->fq_ev[1]) == hipSuccess) fq_totals().kernel_ns += (uint64_t)((double)ms * 1e6);
  return SHK_OK;
}

int shk_ingest_fastq_files_device(shk_ctx *c, const char *const *paths, uint32_t n_paths, uint64_t max_reads, uint64_t validate_every,
                                  shk_fastq_device_stats *out) {
  SHK_TRY(xs_closed(c));
  if (!c || !out) return SHK_ERR_BAD_ARG;
  *out = shk_fastq_device_stats{};
  auto not_eligible = [&] {
    out->gave_up = 2;
    out->give_up_reason = SHK_FASTQ_GIVEUP_NOT_ELIGIBLE;
    fq_totals().give_ups += 1;
    return SHK_OK;
  };
  if (c->group || !n_paths || !paths) return not_eligible();
  if (c->poisoned) return fail(c, c->poison_code, "%s", c->err.c_str());
  if (c->n_reads_read || c->n_bases_read || c->n_inserted || c->retain.n_reads)
    return fail(c, SHK_ERR_STATE, "shk_ingest_fastq_files_device: the context holds reads already; the route starts on an empty one (shk_create or shk_reset)");
  std::vector<MappedFile> files;
  if (fq_route_map(paths, n_paths, &files)) return not_eligible();
  HIPC(c, hipSetDevice(c->cfg.device));
  const uint64_t budget = std::min<uint64_t>(shk::bgzf_batch_budget((uint64_t)128 << 20), (uint64_t)1 << 30);
  uint32_t reason = 0;
  uint64_t n_reads = 0, n_bases = 0;
  {
    FastqRoute R{{}, c, files, budget, max_reads, validate_every, out};
    R.p_next = files[0].p;
    reason = R.open();
    if (!reason) reason = R.feed(R.slot[0]);
    for (int cur = 0; !reason && R.slot[cur].queued; cur ^= 1) {
      FastqRoute::Slot &s = R.slot[cur], &nx = R.slot[cur ^ 1];
      if (!R.input_done) reason = R.feed(nx);
      if (!reason) reason = R.wait_and_check(s);
      if (!reason) reason = R.frame_ingest_carry(s, nx);
      if (reason || R.reached_max) break;
      reason = R.hand_back(s);
    }
    n_reads = R.n_reads;
    n_bases = R.n_bases;
    // the engine stream may still read a slot's buffers (the last ingests): it is waited for before they go back
    if (FastqRoute::own(hipStreamSynchronize(c->stream)) && !reason) reason = SHK_FASTQ_GIVEUP_OWN;
  }
  fq_totals().batches += out->n_batches;
  fq_totals().up += out->bytes_up;
  fq_totals().down += out->n_members * 8;  // (the statuses' and CRCs' copies, exactly; the parses' words are counted where they come down)
  if (reason) {
    (void)hipGetLastError();
    out->gave_up = 1;
    out->give_up_reason = reason;
    fq_totals().give_ups += 1;
    return shk_reset(c);  // (retention stays as it was; the store is emptied)
  }
  out->n_records = n_reads;
  out->n_bases = n_bases;
  fq_totals().records += n_reads;
  return SHK_OK;
}

}  // extern "C"
