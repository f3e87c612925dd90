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
// the two halves, with the number of records that will be looked at.
template <typename GetOut>
static int fq_parse_core(shk_ctx *c, const uint8_t *d_text, uint64_t n, const shk_fastq_text_params &p, GetOut get_out, shk_fastq_text_result *res,
                         uint64_t *n_look_out, bool *ends_nl_out = nullptr) {
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
  float ms0 = 0, ms1 = 0;
  if (hipEventElapsedTime(&ms0, c->fq_ev[0], c->fq_ev[1]) == hipSuccess && hipEventElapsedTime(&ms1, c->fq_ev[2], c->fq_ev[3]) == hipSuccess)
    fq_totals().kernel_ns += (uint64_t)(((double)ms0 + (double)ms1) * 1e6);
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

struct FastqRoute {
  struct Slot {
    hipStream_t st = nullptr;
    hipEvent_t k0 = nullptr, k1 = nullptr, passed = nullptr;  // round the CRC kernel; the engine stream behind this slot's ingest
    bool passed_set = false;
    // up: [inflate jobs | crc jobs | compressed bytes | pad]; down: [n statuses | n crcs], 8 bytes per member and no more
    uint8_t *h_in = nullptr, *d_in = nullptr, *h_out = nullptr, *d_out = nullptr, *d_text = nullptr, *d_bases = nullptr, *d_offs = nullptr;
    size_t h_in_cap = 0, d_in_cap = 0, h_out_cap = 0, d_out_cap = 0, d_text_cap = 0, d_bases_cap = 0, d_offs_cap = 0;
    std::vector<shk::BgzfMember> ms;
    uint64_t out_bytes = 0;
    bool live = false, last_of_file = false;
  } slot[2];
  bool grow(uint8_t **p, size_t *cap, size_t need, bool pinned) {  // (as InflateDecoder::grow: steps of 4 MiB, the block cache matches sizes)
    if (*cap >= need) return true;
    if (*p) pinned ? host_free(*p, *cap) : dev_free(*p, *cap);
    *p = nullptr;
    *cap = 0;
    const size_t ask = (need + (((size_t)4 << 20) - 1)) & ~(((size_t)4 << 20) - 1);
    size_t got = 0;
    void *q = nullptr;
    if ((pinned ? host_alloc(&q, ask, &got) : dev_alloc(&q, ask, &got)) != hipSuccess) {
      (void)hipGetLastError();
      return false;
    }
    *p = (uint8_t *)q;
    *cap = ask;
    return true;
  }
  bool open() {
    for (Slot &s : slot)
      if (hipStreamCreateWithFlags(&s.st, hipStreamNonBlocking) != hipSuccess || hipEventCreate(&s.k0) != hipSuccess || hipEventCreate(&s.k1) != hipSuccess ||
          hipEventCreateWithFlags(&s.passed, hipEventDisableTiming) != hipSuccess) {
        (void)hipGetLastError();
        return false;
      }
    return true;
  }
  ~FastqRoute() {  // (the caller has waited for the engine stream where it had been given any of these)
    for (Slot &s : slot) {
      if (s.st) (void)hipStreamSynchronize(s.st);
      host_free(s.h_in, s.h_in_cap);
      host_free(s.h_out, s.h_out_cap);
      dev_free(s.d_in, s.d_in_cap);
      dev_free(s.d_out, s.d_out_cap);
      dev_free(s.d_text, s.d_text_cap);
      dev_free(s.d_bases, s.d_bases_cap);
      dev_free(s.d_offs, s.d_offs_cap);
      if (s.k0) (void)hipEventDestroy(s.k0);
      if (s.k1) (void)hipEventDestroy(s.k1);
      if (s.passed) (void)hipEventDestroy(s.passed);
      if (s.st) (void)hipStreamDestroy(s.st);
    }
  }
};

// Upload, K_INFLATE, the CRCs, statuses and CRCs down: queued on the slot's stream behind the engine stream's last use
// of the slot.  false: a failure of the route's own.
static bool fq_route_submit(FastqRoute &R, FastqRoute::Slot &s, const uint8_t *from, const uint8_t *end, shk_fastq_device_stats *stats) {
  const uint32_t n = (uint32_t)s.ms.size();
  const size_t comp_len = (size_t)(end - from);
  const size_t jobs_bytes = ((size_t)n * sizeof(InflateJob) + 255) & ~(size_t)255, cjobs_bytes = ((size_t)n * sizeof(FqCrcJob) + 255) & ~(size_t)255;
  const size_t up = jobs_bytes + cjobs_bytes + ((comp_len + 3) & ~(size_t)3) + INFLATE_PAD, down = (size_t)n * 8;
  uint64_t out_bytes = 0;
  for (const shk::BgzfMember &x : s.ms) out_bytes += x.isize;
  s.out_bytes = out_bytes;
  if (!R.grow(&s.h_in, &s.h_in_cap, up, true) || !R.grow(&s.d_in, &s.d_in_cap, up, false) || !R.grow(&s.h_out, &s.h_out_cap, down, true) ||
      !R.grow(&s.d_out, &s.d_out_cap, down, false) || !R.grow(&s.d_text, &s.d_text_cap, FQ_CARRY_ROOM + out_bytes + 16, false))
    return false;
  InflateJob *ij = (InflateJob *)s.h_in;
  FqCrcJob *cj = (FqCrcJob *)(s.h_in + jobs_bytes);
  uint64_t at = 0;
  for (uint32_t i = 0; i < n; ++i) {
    const shk::BgzfMember &x = s.ms[i];
    // every job inside the batch: the kernels read and write what the jobs say (bgzf_scan has held body and ISIZE to 65536)
    const uint64_t in_off = (uint64_t)(x.header - from) + x.body_off;
    if (x.body_len > INFC_MEMBER_MAX || x.isize > INFC_MEMBER_MAX || in_off + x.body_len > comp_len) return false;
    ij[i] = InflateJob{in_off, at, x.body_len, x.isize};
    cj[i] = FqCrcJob{at, x.isize, 0};
    at += x.isize;
  }
  memcpy(s.h_in + jobs_bytes + cjobs_bytes, from, comp_len);
  memset(s.h_in + jobs_bytes + cjobs_bytes + comp_len, 0, up - jobs_bytes - cjobs_bytes - comp_len);
  uint8_t *text = s.d_text + FQ_CARRY_ROOM;
  bool ok = true;
  if (s.passed_set) ok = hipStreamWaitEvent(s.st, s.passed, 0) == hipSuccess;  // (the ingest that read this slot's buffers last, and the carry copied out of it)
  ok = ok && hipMemcpyAsync(s.d_in, s.h_in, up, hipMemcpyHostToDevice, s.st) == hipSuccess;
  ok = ok && hipMemsetAsync(s.d_out, 0xFF, down, s.st) == hipSuccess;  // INFC_NOT_RUN; no CRC yet
  if (ok) {
    k_inflate_members<<<dim3((n + INFLATE_WAVES - 1) / INFLATE_WAVES), dim3(INFLATE_WAVES * 64), 0, s.st>>>(s.d_in + jobs_bytes + cjobs_bytes, (const InflateJob *)s.d_in, n,
                                                                                                        text, (uint32_t *)s.d_out);
    ok = hipGetLastError() == hipSuccess;
  }
  ok = ok && hipEventRecord(s.k0, s.st) == hipSuccess;
  if (ok) {
    k_crc_members<<<dim3((n + FQ_WAVES - 1) / FQ_WAVES), dim3(FQ_WAVES * 64), 0, s.st>>>(text, (const FqCrcJob *)(s.d_in + jobs_bytes), n, (uint32_t *)s.d_out + n);
    ok = hipGetLastError() == hipSuccess;
  }
  ok = ok && hipEventRecord(s.k1, s.st) == hipSuccess;
  ok = ok && hipMemcpyAsync(s.h_out, s.d_out, down, hipMemcpyDeviceToHost, s.st) == hipSuccess;
  if (!ok) {
    (void)hipGetLastError();
    (void)hipStreamSynchronize(s.st);
    return false;
  }
  s.live = true;
  stats->bytes_up += up;
  stats->bytes_down += down;  // (exactly what the copy above brings down)
  stats->n_members += n;
  stats->n_batches += 1;
  return true;
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
  SHK_TRY(fq_parse_core(c, (const uint8_t *)d_text, n_bytes, *params, get_out, out, &n_look));
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
  std::vector<MappedFile> files(n_paths);
  for (uint32_t f = 0; f < n_paths; ++f) {
    struct stat sb;
    const int fd = paths[f] ? open(paths[f], O_RDONLY | O_CLOEXEC) : -1;
    if (fd < 0) return not_eligible();
    if (fstat(fd, &sb) != 0 || !S_ISREG(sb.st_mode) || sb.st_size <= 0) {
      close(fd);
      return not_eligible();
    }
    void *m = mmap(nullptr, (size_t)sb.st_size, PROT_READ, MAP_PRIVATE, fd, 0);
    close(fd);
    if (m == MAP_FAILED) return not_eligible();
    files[f].p = (const uint8_t *)m;
    files[f].n = (size_t)sb.st_size;
    std::vector<shk::BgzfMember> first;
    if (shk::bgzf_scan(files[f].p, files[f].p + files[f].n, 0, &first) == files[f].p) return not_eligible();
  }
  HIPC(c, hipSetDevice(c->cfg.device));
  const uint64_t budget = [] {
    const char *e = getenv("SHK_BGZF_BATCH_KB");  // (the BGZF routes' test hook: batch borders in tiny files)
    const uint64_t b = e ? std::max<uint64_t>(1, (uint64_t)atoll(e)) << 10 : (uint64_t)128 << 20;
    return std::min<uint64_t>(b, (uint64_t)1 << 30);
  }();
  uint32_t reason = 0;
  uint64_t n_reads = 0, n_bases = 0;
  {
    FastqRoute R;
    if (!R.open()) reason = SHK_FASTQ_GIVEUP_OWN;
    // the batches of all files as one sequence: the next one is scanned and submitted before this one is waited for
    uint32_t f_next = 0;
    const uint8_t *p_next = files[0].p;
    bool input_done = false;
    auto submit_next = [&](FastqRoute::Slot &s) {  // false with reason == 0: the input's end
      while (f_next < n_paths && p_next == files[f_next].p + files[f_next].n) {
        ++f_next;
        if (f_next < n_paths) p_next = files[f_next].p;
      }
      if (f_next >= n_paths) {
        input_done = true;
        return false;
      }
      const uint8_t *file_end = files[f_next].p + files[f_next].n;
      s.ms.clear();
      const uint8_t *end = shk::bgzf_scan(p_next, file_end, budget, &s.ms);
      if (end == p_next || s.ms.empty()) {
        reason = SHK_FASTQ_GIVEUP_MEMBER;
        return false;
      }
      s.last_of_file = end == file_end;
      if (!fq_route_submit(R, s, p_next, end, out)) {
        reason = SHK_FASTQ_GIVEUP_OWN;
        return false;
      }
      p_next = end;
      return true;
    };
    int cur = 0;
    uint64_t carry = 0;  // bytes of text in front of slot[cur]'s own, already in its carry room
    bool reached_max = false;
    if (!reason) (void)submit_next(R.slot[0]);
    while (!reason && R.slot[cur].live) {
      FastqRoute::Slot &s = R.slot[cur], &nx = R.slot[cur ^ 1];
      if (!input_done) (void)submit_next(nx);
      if (reason) break;
      s.live = false;
      if (hipStreamSynchronize(s.st) != hipSuccess) {
        (void)hipGetLastError();
        reason = SHK_FASTQ_GIVEUP_OWN;
        break;
      }
      float ms = 0;
      if (hipEventElapsedTime(&ms, s.k0, s.k1) == hipSuccess) {
        out->kernel_ns += (uint64_t)((double)ms * 1e6);
        fq_totals().kernel_ns += (uint64_t)((double)ms * 1e6);
      }
      const uint32_t n = (uint32_t)s.ms.size();
      const uint32_t *status = (const uint32_t *)s.h_out, *crc = status + n;
      for (uint32_t i = 0; i < n && !reason; ++i) {
        if (status[i] != INFC_OK) reason = SHK_FASTQ_GIVEUP_DECODE;
        else if (crc[i] != s.ms[i].crc) reason = SHK_FASTQ_GIVEUP_CRC;
      }
      if (reason) break;
      // the framing over carry + text, on the engine stream (the slot's stream has been waited for)
      const uint64_t n_text = carry + s.out_bytes;
      const uint8_t *text = s.d_text + FQ_CARRY_ROOM - carry;
      shk_fastq_text_params p{};
      p.first_record = n_reads;
      p.validate_every = validate_every;
      p.max_records = max_reads ? max_reads - n_reads : 0;
      p.last = s.last_of_file;
      auto get_out = [&](uint64_t n_look, FqOut *o) -> int {
        if (!R.grow(&s.d_bases, &s.d_bases_cap, n_text + 64, false) || !R.grow(&s.d_offs, &s.d_offs_cap, (n_look + 1) * 8, false)) return SHK_ERR_NOMEM;
        *o = FqOut{s.d_bases, n_text, (uint64_t *)s.d_offs};  // (the sequences are part of the text: never more bytes than it has)
        return SHK_OK;
      };
      shk_fastq_text_result r{};
      uint64_t n_look = 0;
      const uint64_t down0 = fq_totals().down.load(), ns0 = fq_totals().kernel_ns.load();
      bool ends_nl = false;
      const int prc = fq_parse_core(c, text, n_text, p, get_out, &r, &n_look, &ends_nl);
      out->bytes_down += fq_totals().down.load() - down0;
      out->kernel_ns += fq_totals().kernel_ns.load() - ns0;
      if (prc != SHK_OK) {
        reason = SHK_FASTQ_GIVEUP_OWN;
        break;
      }
      if (r.anomaly_record != FQ_NO_ANOMALY) {
        reason = SHK_FASTQ_GIVEUP_ANOMALY;
        break;
      }
      if (s.last_of_file && n_text && !ends_nl) {  // a file whose last line is not terminated ends inside a record, or may: the host decides
        reason = SHK_FASTQ_GIVEUP_TEXT_LEFT;
        break;
      }
      if (r.n_records && shk_ingest_reads_device(c, s.d_bases, s.d_offs, r.n_records, r.n_bases) != SHK_OK) {
        reason = SHK_FASTQ_GIVEUP_OWN;
        break;
      }
      n_reads += r.n_records;
      n_bases += r.n_bases;
      reached_max = max_reads && n_reads >= max_reads;
      const uint64_t left = n_text - r.bytes_consumed;
      if (reached_max) break;
      if (s.last_of_file) {
        if (left) {
          reason = SHK_FASTQ_GIVEUP_TEXT_LEFT;
          break;
        }
        carry = 0;
      } else {
        if (left > FQ_CARRY_ROOM || !nx.live) {  // (a batch that does not end its file has one behind it)
          reason = SHK_FASTQ_GIVEUP_OWN;
          break;
        }
        // the text behind the last record, to the front of the next batch's text
        if (left && hipMemcpyAsync(nx.d_text + FQ_CARRY_ROOM - left, text + r.bytes_consumed, left, hipMemcpyDeviceToDevice, c->stream) != hipSuccess) {
          (void)hipGetLastError();
          reason = SHK_FASTQ_GIVEUP_OWN;
          break;
        }
        carry = left;
      }
      // this slot's buffers are free again once the engine stream has passed the ingest (and the copy of the carry)
      if (hipEventRecord(s.passed, c->stream) != hipSuccess) {
        (void)hipGetLastError();
        reason = SHK_FASTQ_GIVEUP_OWN;
        break;
      }
      s.passed_set = true;
      cur ^= 1;
    }
    // the engine stream may still read a slot's buffers (the last ingests): it is waited for before they go back
    if (hipStreamSynchronize(c->stream) != hipSuccess) {
      (void)hipGetLastError();
      if (!reason) reason = SHK_FASTQ_GIVEUP_OWN;
    }
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
