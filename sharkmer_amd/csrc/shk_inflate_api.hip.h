// shk_inflate_api.hip.h — the device backend of the BGZF batched route: K_INFLATE behind the front-end's
// MemberDecoderOps (shk_front.h), registered when the library is loaded.  Included at the end of shk_engine.hip.
//
// A decoder belongs to one gzip source (one file being read) and to one device.  It has two slots, each with a stream
// of its own, a pinned pair (compressed bytes + jobs up, text + statuses down) and a device pair, so that batch n + 1
// goes up while batch n's text comes back; all of them from, and back to, the process-wide block cache.  submit()
// copies the batch's compressed bytes into the slot's pinned block and queues upload, kernel and download on the
// slot's stream; collect() waits for that stream alone and copies the text out of the pinned block.

namespace {

struct InflateTotals {
  std::atomic<uint64_t> members{0}, kernel_ns{0}, up{0}, down{0};
};
static InflateTotals &inflate_totals() {
  static InflateTotals t;
  return t;
}

struct InflateDecoder {
  int dev = 0;
  struct Slot {
    hipStream_t st = nullptr;
    hipEvent_t k0 = nullptr, k1 = nullptr;
    uint8_t *h_in = nullptr, *h_out = nullptr, *d_in = nullptr, *d_out = nullptr;
    size_t h_in_cap = 0, h_out_cap = 0, d_in_cap = 0, d_out_cap = 0;  // (the sizes they were asked at)
    // the layout of a pair, up: [jobs | compressed bytes | pad], down: [statuses | text]
    size_t jobs_bytes = 0, comp_len = 0, status_bytes = 0;
    uint64_t out_bytes = 0;
    uint32_t n = 0;
    bool queued = false;
  } slot[2];
  bool grow(uint8_t **p, size_t *cap, size_t need, bool pinned) {
    if (*cap >= need) return true;
    if (*p) pinned ? host_free(*p, *cap) : dev_free(*p, *cap);
    *p = nullptr;
    *cap = 0;
    const size_t ask = (need + (((size_t)4 << 20) - 1)) & ~(((size_t)4 << 20) - 1);  // (steps of 4 MiB: the cache matches sizes)
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
  ~InflateDecoder() {
    (void)hipSetDevice(dev);
    for (Slot &s : slot) {
      if (s.st) (void)hipStreamSynchronize(s.st);
      host_free(s.h_in, s.h_in_cap);
      host_free(s.h_out, s.h_out_cap);
      dev_free(s.d_in, s.d_in_cap);
      dev_free(s.d_out, s.d_out_cap);
      if (s.k0) (void)hipEventDestroy(s.k0);
      if (s.k1) (void)hipEventDestroy(s.k1);
      if (s.st) (void)hipStreamDestroy(s.st);
    }
  }
};

static bool inflate_probe(int device, std::string *why) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
    (void)hipGetLastError();
    *why = "no HIP device is visible";
    return false;
  }
  if (device < 0 || device >= n || hipSetDevice(device) != hipSuccess) {
    (void)hipGetLastError();
    *why = shk::fmt("%d device(s) visible", n);
    return false;
  }
  return true;
}
static void *inflate_open(int device) {
  if (hipSetDevice(device) != hipSuccess) {
    (void)hipGetLastError();
    return nullptr;
  }
  auto *d = new InflateDecoder();
  d->dev = device;
  for (auto &s : d->slot)
    if (hipStreamCreateWithFlags(&s.st, hipStreamNonBlocking) != hipSuccess || hipEventCreate(&s.k0) != hipSuccess ||
        hipEventCreate(&s.k1) != hipSuccess) {
      (void)hipGetLastError();
      delete d;
      return nullptr;
    }
  return d;
}
static int inflate_submit(void *dec, int si, const uint8_t *comp, size_t comp_len, const shk::MemberJob *jobs, uint32_t n, uint64_t out_bytes) {
  auto *d = (InflateDecoder *)dec;
  auto &s = d->slot[si];
  if (s.queued || !n) return -1;
  if (hipSetDevice(d->dev) != hipSuccess) return -1;
  static_assert(sizeof(shk::MemberJob) == sizeof(InflateJob) && offsetof(shk::MemberJob, in_len) == offsetof(InflateJob, in_len) &&
                    offsetof(shk::MemberJob, out_offset) == offsetof(InflateJob, out_offset),
                "the front-end's jobs are the kernel's");
  // every job inside the batch: the kernel reads and writes what the jobs say
  for (uint32_t i = 0; i < n; ++i)
    if (jobs[i].in_len > INFC_MEMBER_MAX || jobs[i].out_len > INFC_MEMBER_MAX || jobs[i].in_offset + jobs[i].in_len > comp_len ||
        jobs[i].out_offset + jobs[i].out_len > out_bytes)
      return -1;
  s.jobs_bytes = ((size_t)n * sizeof(InflateJob) + 255) & ~(size_t)255;
  s.status_bytes = ((size_t)n * 4 + 255) & ~(size_t)255;
  s.comp_len = comp_len;
  s.out_bytes = out_bytes;
  s.n = n;
  const size_t up = s.jobs_bytes + ((comp_len + 3) & ~(size_t)3) + INFLATE_PAD, down = s.status_bytes + (size_t)out_bytes;
  if (!d->grow(&s.h_in, &s.h_in_cap, up, true) || !d->grow(&s.d_in, &s.d_in_cap, up, false) || !d->grow(&s.h_out, &s.h_out_cap, down, true) ||
      !d->grow(&s.d_out, &s.d_out_cap, down, false))
    return -1;
  memcpy(s.h_in, jobs, (size_t)n * sizeof(InflateJob));
  memcpy(s.h_in + s.jobs_bytes, comp, comp_len);
  memset(s.h_in + s.jobs_bytes + comp_len, 0, up - s.jobs_bytes - comp_len);
  bool ok = hipMemcpyAsync(s.d_in, s.h_in, up, hipMemcpyHostToDevice, s.st) == hipSuccess;
  ok = ok && hipMemsetAsync(s.d_out, 0xFF, s.status_bytes, s.st) == hipSuccess;  // INFC_NOT_RUN
  ok = ok && hipEventRecord(s.k0, s.st) == hipSuccess;
  if (ok) {
    k_inflate_members<<<dim3((n + INFLATE_WAVES - 1) / INFLATE_WAVES), dim3(INFLATE_WAVES * 64), 0, s.st>>>(
        s.d_in + s.jobs_bytes, (const InflateJob *)s.d_in, n, s.d_out + s.status_bytes, (uint32_t *)s.d_out);
    ok = hipGetLastError() == hipSuccess;
  }
  ok = ok && hipEventRecord(s.k1, s.st) == hipSuccess;
  ok = ok && hipMemcpyAsync(s.h_out, s.d_out, down, hipMemcpyDeviceToHost, s.st) == hipSuccess;
  if (!ok) {
    (void)hipGetLastError();
    (void)hipStreamSynchronize(s.st);
    return -1;
  }
  s.queued = true;
  inflate_totals().up += up;
  inflate_totals().down += down;
  return 0;
}
static int inflate_collect(void *dec, int si, uint8_t *dst, uint32_t *status) {
  auto *d = (InflateDecoder *)dec;
  auto &s = d->slot[si];
  if (!s.queued) return -1;
  s.queued = false;
  if (hipSetDevice(d->dev) != hipSuccess || hipStreamSynchronize(s.st) != hipSuccess) {
    (void)hipGetLastError();
    return -1;
  }
  float ms = 0;
  if (hipEventElapsedTime(&ms, s.k0, s.k1) == hipSuccess) inflate_totals().kernel_ns += (uint64_t)((double)ms * 1e6);
  inflate_totals().members += s.n;
  if (dst) {
    memcpy(status, s.h_out, (size_t)s.n * 4);
    memcpy(dst, s.h_out + s.status_bytes, (size_t)s.out_bytes);
  }
  return 0;
}
static void inflate_close(void *dec) { delete (InflateDecoder *)dec; }

static const shk::MemberDecoderOps INFLATE_DEVICE_OPS = {inflate_probe, inflate_open, inflate_submit, inflate_collect, inflate_close};
static const bool inflate_registered = (shk::shk_front_set_member_decoder(&INFLATE_DEVICE_OPS), true);

}  // namespace

extern "C" int shk_bgzf_device_totals(uint64_t *n_members, uint64_t *kernel_ns, uint64_t *bytes_up, uint64_t *bytes_down) {
  InflateTotals &t = inflate_totals();
  if (n_members) *n_members = t.members.load();
  if (kernel_ns) *kernel_ns = t.kernel_ns.load();
  if (bytes_up) *bytes_up = t.up.load();
  if (bytes_down) *bytes_down = t.down.load();
  return SHK_OK;
}
