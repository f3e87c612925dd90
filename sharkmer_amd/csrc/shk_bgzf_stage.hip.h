// shk_bgzf_stage.hip.h — the decode stage under the BGZF device decoder (shk_inflate_api.hip.h) and the
// file-to-ingest route (shk_fastq_api.hip.h, §20): a slot — a stream of its own, two events, a pinned and a device block
// each way, all from and back to the process-wide block cache — and the one function that lays a batch of members out in
// a slot's up pair and queues upload, status fill and K_INFLATE on its stream.  What comes down, and where the events
// stand, is the caller's.  Included at the end of shk_engine.hip, in front of the two.

namespace {

constexpr size_t STAGE_STEP = (size_t)4 << 20;  // a slot's blocks are asked in steps of 4 MiB: the cache matches sizes

struct DecodeSlot {
  hipStream_t st = nullptr;
  hipEvent_t k0 = nullptr, k1 = nullptr;  // round what the caller times
  HostBuf h_up, h_down;
  DevBuf d_up, d_down;
  bool queued = false;
  bool open() {
    const bool ok = hipStreamCreateWithFlags(&st, hipStreamNonBlocking) == hipSuccess && hipEventCreate(&k0) == hipSuccess && hipEventCreate(&k1) == hipSuccess;
    if (!ok) (void)hipGetLastError();
    return ok;
  }
  bool ensure_down(size_t bytes) {
    const bool ok = h_down.ensure_step(bytes, STAGE_STEP) == hipSuccess && d_down.ensure_step(bytes, STAGE_STEP) == hipSuccess;
    if (!ok) (void)hipGetLastError();
    return ok;
  }
  void drain() {  // a queueing step failed: what did get queued runs out before the blocks are touched again
    (void)hipGetLastError();
    (void)hipStreamSynchronize(st);
  }
  ~DecodeSlot() {
    if (st) (void)hipStreamSynchronize(st);
    h_up.release();
    h_down.release();
    d_up.release();
    d_down.release();
    if (k0) (void)hipEventDestroy(k0);
    if (k1) (void)hipEventDestroy(k1);
    if (st) (void)hipStreamDestroy(st);
  }
};

static size_t stage_round256(size_t x) { return (x + 255) & ~(size_t)255; }

static_assert(sizeof(shk::MemberJob) == sizeof(InflateJob) && offsetof(shk::MemberJob, in_len) == offsetof(InflateJob, in_len) &&
                  offsetof(shk::MemberJob, out_offset) == offsetof(InflateJob, out_offset),
              "the front-end's jobs are the kernel's");

// A batch on slot s: its up pair laid out as [jobs | extra | compressed bytes | pad] (jobs rounded to 256 bytes; extra_bytes
// is the caller's, 256-rounded, filled through fill_extra(host pointer) before it goes up, *d_extra: where it is on the
// device), then on the slot's stream the upload, 0xFF (INFC_NOT_RUN) over d_status[0, status_fill), k0 where the caller
// times K_INFLATE alone, and K_INFLATE: text to d_text[0, out_bytes), a status word per member to d_status.  Every job
// is held inside the batch first: the kernel reads and writes what the jobs say.  Returns the bytes that go up; 0: a job
// outside the batch, no memory, or a step that failed (the stream has been waited for).
template <typename FillExtra>
static size_t stage_queue_inflate(DecodeSlot &s, const uint8_t *comp, size_t comp_len, const shk::MemberJob *jobs, uint32_t n, uint64_t out_bytes, size_t extra_bytes,
                                  FillExtra fill_extra, const uint8_t **d_extra, uint8_t *d_text, uint32_t *d_status, size_t status_fill, bool k0_before_kernel) {
  if (!n || !shk::bgzf_jobs_inside(jobs, n, comp_len, out_bytes)) return 0;
  const size_t jobs_bytes = stage_round256((size_t)n * sizeof(InflateJob)), at_comp = jobs_bytes + extra_bytes;
  const size_t up = at_comp + ((comp_len + 3) & ~(size_t)3) + INFLATE_PAD;
  if (s.h_up.ensure_step(up, STAGE_STEP) != hipSuccess || s.d_up.ensure_step(up, STAGE_STEP) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  uint8_t *h = (uint8_t *)s.h_up.p, *d = (uint8_t *)s.d_up.p;
  memcpy(h, jobs, (size_t)n * sizeof(InflateJob));
  fill_extra(h + jobs_bytes);
  memcpy(h + at_comp, comp, comp_len);
  memset(h + at_comp + comp_len, 0, up - at_comp - comp_len);
  if (d_extra) *d_extra = d + jobs_bytes;
  bool ok = hipMemcpyAsync(d, h, up, hipMemcpyHostToDevice, s.st) == hipSuccess;
  ok = ok && hipMemsetAsync(d_status, 0xFF, status_fill, s.st) == hipSuccess;
  if (k0_before_kernel) ok = ok && hipEventRecord(s.k0, s.st) == hipSuccess;
  if (ok) {
    k_inflate_members<<<dim3((n + INFLATE_WAVES - 1) / INFLATE_WAVES), dim3(INFLATE_WAVES * 64), 0, s.st>>>(d + at_comp, (const InflateJob *)d, n, d_text, d_status);
    ok = hipGetLastError() == hipSuccess;
  }
  if (!ok) s.drain();
  return ok ? up : 0;
}

}  // namespace
