// shk_inflate_api.hip.h — the device backend of the BGZF batched route: K_INFLATE behind the front-end's
// MemberDecoderOps (shk_front.h), registered when the library is loaded.  Included at the end of shk_engine.hip.
//
// A decoder belongs to one gzip source (one file being read) and to one device.  It has two DecodeSlots
// (shk_bgzf_stage.hip.h), so that batch n + 1 goes up while batch n's text comes back.  submit() has the stage lay the
// batch out and queue upload and kernel, and queues the download of [statuses | text] behind them; collect() waits for
// that stream alone and copies the text out of the pinned block.

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
  struct Slot : DecodeSlot {
    // the layout of the down pair: [statuses | text]
    size_t status_bytes = 0;
    uint64_t out_bytes = 0;
    uint32_t n = 0;
  } slot[2];
  ~InflateDecoder() { (void)hipSetDevice(dev); }  // (in front of the slots' own)
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
    if (!s.open()) {
      delete d;
      return nullptr;
    }
  return d;
}
static int inflate_submit(void *dec, int si, const uint8_t *comp, size_t comp_len, const shk::MemberJob *jobs, uint32_t n, uint64_t out_bytes) {
  auto *d = (InflateDecoder *)dec;
  auto &s = d->slot[si];
  if (s.queued) return -1;
  if (hipSetDevice(d->dev) != hipSuccess) return -1;
  s.status_bytes = stage_round256((size_t)n * 4);
  s.out_bytes = out_bytes;
  s.n = n;
  const size_t down = s.status_bytes + (size_t)out_bytes;
  if (!s.ensure_down(down)) return -1;
  uint8_t *d_down = (uint8_t *)s.d_down.p;
  const size_t up = stage_queue_inflate(s, comp, comp_len, jobs, n, out_bytes, 0, [](uint8_t *) {}, nullptr, d_down + s.status_bytes, (uint32_t *)d_down,
                                        s.status_bytes, true);
  if (!up) return -1;
  if (hipEventRecord(s.k1, s.st) != hipSuccess || hipMemcpyAsync(s.h_down.p, d_down, down, hipMemcpyDeviceToHost, s.st) != hipSuccess) {
    s.drain();
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
    memcpy(status, s.h_down.p, (size_t)s.n * 4);
    memcpy(dst, (const uint8_t *)s.h_down.p + s.status_bytes, (size_t)s.out_bytes);
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
