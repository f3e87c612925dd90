// shk_products_api.hip.h — shk_pcr_dedup_panel and shk_pcr_products_panel (included by shk_engine.hip, same translation
// unit): the last stage of sPCR after shk_thread_reads_panel.  The paths, sequences and scores are the
// host's (shk_products.cpp).  The dedup's arithmetic — is pair (i, j) of a gene's sorted records within the gene's edit
// threshold, for ALL pairs — is K_DEDUP's: one lane per pair, the pair derived from its index, Landau-Vishkin over 2-bit
// packed words (shk_dedup_core.h), the answers written 64 at a time from a ballot.  The host then runs the reference's
// greedy order over the bit matrix.  The table is not read.
namespace shk {

constexpr int DEDUP_WG = 128;  // two waves; (2t + 3) int32 slots per lane of LDS: 33 280 bytes at t = 31

struct DedupGene {
  uint64_t rec;    // the gene's first record in rec_word / rec_len (sorted order)
  uint64_t bits;   // the gene's first word of pair bits
  uint32_t m, t;   // records, threshold
};
struct DedupBlock {
  uint64_t first;  // the block's first pair index in its gene, a multiple of DEDUP_WG
  uint32_t gene, pad;
};

__global__ void __launch_bounds__(DEDUP_WG) k_dedup_panel(const DedupGene *__restrict__ genes, const DedupBlock *__restrict__ blocks,
                                                          const uint64_t *__restrict__ rec_word, const uint32_t *__restrict__ rec_len,
                                                          const uint64_t *__restrict__ text, uint64_t *__restrict__ bits) {
  extern __shared__ int32_t dedup_slots[];
  const DedupBlock bk = blocks[blockIdx.x];
  const DedupGene g = genes[bk.gene];
  const uint64_t m = g.m, n_pairs = m * (m - 1) / 2;
  const uint64_t p = bk.first + threadIdx.x;
  bool within = false;
  if (p < n_pairs) {
    uint64_t i, j;
    dedup_pair_of(p, m, &i, &j);
    within = dedup_within(text + rec_word[g.rec + i], (int32_t)rec_len[g.rec + i], text + rec_word[g.rec + j], (int32_t)rec_len[g.rec + j],
                          (int32_t)g.t, dedup_slots + threadIdx.x, DEDUP_WG);
  }
  const uint64_t word = __ballot(within);
  if ((threadIdx.x & 63) == 0 && p < n_pairs) bits[g.bits + (p >> 6)] = word;
}

}  // namespace shk

namespace {

// f64::total_cmp as an integer order
int64_t total_order_key(double x) {
  int64_t b;
  memcpy(&b, &x, sizeof b);
  return b ^ (int64_t)((uint64_t)(b >> 63) >> 1);
}

uint64_t env_u64_or(const char *name, uint64_t dflt) {
  const char *s = getenv(name);
  return s && *s ? strtoull(s, nullptr, 10) : dflt;
}

constexpr uint64_t DEDUP_DEVICE_PAIRS = 0;  // default of SHK_DEDUP_DEVICE_PAIRS: always the device

}  // namespace

extern "C" int shk_pcr_dedup_panel(shk_ctx *c, const uint8_t *seqs, const uint64_t *seq_offsets, const uint64_t *record_offsets,
                                   const double *scores, const uint32_t *thresholds, uint32_t n_genes, shk_pcr_dedup_out *out) {
  SHK_TRY(xs_closed(c));
  using ull = unsigned long long;
  if (c && c->group)
    return on_any_device(c, [&](shk_ctx *d) { return shk_pcr_dedup_panel(d, seqs, seq_offsets, record_offsets, scores, thresholds, n_genes, out); });
  if (!c || !out) return SHK_ERR_BAD_ARG;
  out->device_ms = 0.0;
  out->pairs_device = out->pairs_host = out->pairs_prefiltered = 0;
  // everything that is refused, before the device is touched
  if (n_genes > SHK_PCR_MAX_GENES) return fail(c, SHK_ERR_BAD_ARG, "n_genes %u above SHK_PCR_MAX_GENES (%u)", n_genes, (unsigned)SHK_PCR_MAX_GENES);
  if (out->pair_offsets) out->pair_offsets[0] = 0;
  if (n_genes == 0) return SHK_OK;
  if (!record_offsets || !thresholds) return fail(c, SHK_ERR_BAD_ARG, "shk_pcr_dedup_panel: record_offsets or thresholds is missing");
  for (uint32_t g = 0; g < n_genes; ++g) {
    if (record_offsets[g + 1] < record_offsets[g])
      return fail(c, SHK_ERR_BAD_ARG, "gene %u: record_offsets decrease (%llu after %llu)", g, (ull)record_offsets[g + 1], (ull)record_offsets[g]);
    if (record_offsets[g + 1] - record_offsets[g] >= (1ull << 31)) return fail(c, SHK_ERR_BAD_ARG, "gene %u: 2^31 records or more", g);
  }
  const uint64_t r0 = record_offsets[0], nr = record_offsets[n_genes] - r0;
  if (nr && (!seq_offsets || !scores)) return fail(c, SHK_ERR_BAD_ARG, "shk_pcr_dedup_panel: seq_offsets or scores is missing");
  for (uint32_t g = 0; g < n_genes; ++g)
    for (uint64_t r = record_offsets[g]; r < record_offsets[g + 1]; ++r) {
      if (seq_offsets[r + 1] < seq_offsets[r])
        return fail(c, SHK_ERR_BAD_ARG, "gene %u: record %llu: seq_offsets decrease (%llu after %llu)", g, (ull)(r - record_offsets[g]),
                    (ull)seq_offsets[r + 1], (ull)seq_offsets[r]);
      if (seq_offsets[r + 1] > seq_offsets[r] && !seqs) return fail(c, SHK_ERR_BAD_ARG, "shk_pcr_dedup_panel: seqs is missing");
      for (uint64_t x = seq_offsets[r]; x < seq_offsets[r + 1]; ++x)
        if (seqs[x] != 'A' && seqs[x] != 'C' && seqs[x] != 'G' && seqs[x] != 'T')
          return fail(c, SHK_ERR_BAD_ARG, "gene %u: record %llu: byte %u at base %llu is none of ACGT", g, (ull)(r - record_offsets[g]), seqs[x],
                      (ull)(x - seq_offsets[r]));
    }
  auto len_of = [&](uint64_t r) { return seq_offsets[r + 1] - seq_offsets[r]; };

  // per gene: the sorted order, the pair-bit layout, the prefilter count, the route
  std::vector<uint32_t> order(nr);           // sorted position -> input index, local to the gene
  std::vector<uint64_t> poff(n_genes + 1, 0);  // words
  std::vector<uint8_t> on_device(n_genes, 0);
  std::vector<uint64_t> need(n_genes, 0), lens;
  uint64_t need_device = 0;
  for (uint32_t g = 0; g < n_genes; ++g) {
    const uint64_t ra = record_offsets[g], m = record_offsets[g + 1] - ra, t = thresholds[g];
    uint32_t *ord = order.data() + (ra - r0);
    for (uint64_t i = 0; i < m; ++i) ord[i] = (uint32_t)i;
    std::sort(ord, ord + m, [&](uint32_t x, uint32_t y) {  // score descending (total_cmp), then bytes ascending; input order last
      const int64_t kx = total_order_key(scores[ra + x]), ky = total_order_key(scores[ra + y]);
      if (kx != ky) return kx > ky;
      const uint64_t lx = len_of(ra + x), ly = len_of(ra + y);
      const int cmp = std::min(lx, ly) ? memcmp(seqs + seq_offsets[ra + x], seqs + seq_offsets[ra + y], std::min(lx, ly)) : 0;
      if (cmp) return cmp < 0;
      return lx != ly ? lx < ly : x < y;
    });
    const uint64_t pairs = m * (m ? m - 1 : 0) / 2;
    poff[g + 1] = poff[g] + (pairs + 63) / 64;
    // pairs no alignment decides: |la - lb| > t over the sorted lengths, and both lengths <= t (the two never overlap)
    lens.resize(m);
    bool fits = t <= DEDUP_MAX_T;
    for (uint64_t i = 0; i < m; ++i) {
      lens[i] = len_of(ra + i);
      fits = fits && lens[i] < DEDUP_MAX_LEN;
    }
    std::sort(lens.begin(), lens.end());
    uint64_t far = 0, small = 0;
    for (uint64_t i = 0, lo = 0; i < m; ++i) {
      while (lens[i] - lens[lo] > t) ++lo;
      far += lo;
      small += lens[i] <= t;
    }
    const uint64_t pre = far + small * (small ? small - 1 : 0) / 2;
    out->pairs_prefiltered += pre;
    need[g] = pairs - pre;
    on_device[g] = fits && pairs > 0;
    if (on_device[g]) need_device += need[g];
  }
  if (out->pair_offsets) std::copy(poff.begin(), poff.end(), out->pair_offsets);
  if (out->pair_words && poff[n_genes] > out->pair_cap)
    return fail(c, SHK_ERR_BAD_ARG, "pair bits of %llu words do not fit pair_cap %llu", (ull)poff[n_genes], (ull)out->pair_cap);
  const uint64_t knob = env_u64_or("SHK_DEDUP_DEVICE_PAIRS", DEDUP_DEVICE_PAIRS);
  if (knob && need_device < knob) std::fill(on_device.begin(), on_device.end(), (uint8_t)0);
  for (uint32_t g = 0; g < n_genes; ++g) (on_device[g] ? out->pairs_device : out->pairs_host) += need[g];

  // the device's genes: packed text in sorted order, one block per DEDUP_WG pairs
  std::vector<uint64_t> bits;  // the device's pair words, gene after gene
  std::vector<uint64_t> dev_bits_at(n_genes, 0);
  {
    std::vector<DedupGene> dg;
    std::vector<DedupBlock> blocks;
    std::vector<uint64_t> rec_word, text;
    std::vector<uint32_t> rec_len;
    uint64_t n_words = 0;
    uint32_t tmax = 0;
    for (uint32_t g = 0; g < n_genes; ++g) {
      if (!on_device[g]) continue;
      const uint64_t ra = record_offsets[g], m = record_offsets[g + 1] - ra;
      const uint32_t *ord = order.data() + (ra - r0);
      const uint64_t pairs = m * (m - 1) / 2;
      dev_bits_at[g] = n_words;
      dg.push_back(DedupGene{(uint64_t)rec_word.size(), n_words, (uint32_t)m, thresholds[g]});
      n_words += (pairs + 63) / 64;
      tmax = std::max(tmax, thresholds[g]);
      for (uint64_t p = 0; p < pairs; p += DEDUP_WG) blocks.push_back(DedupBlock{p, (uint32_t)(dg.size() - 1), 0u});
      for (uint64_t i = 0; i < m; ++i) {
        const uint64_t r = ra + ord[i], len = len_of(r), at = text.size();
        rec_word.push_back(at), rec_len.push_back((uint32_t)len);
        text.resize(at + dedup_words(len), 0);
        const uint8_t *s = seqs + seq_offsets[r];
        for (uint64_t x = 0; x < len; ++x) text[at + (x >> 5)] |= (uint64_t)(((s[x] >> 1) & 3u) ^ ((s[x] >> 2) & 1u)) << (2 * (x & 31));
      }
    }
    if (blocks.size() >= (1ull << 31)) return fail(c, SHK_ERR_NOMEM, "%llu dedup workgroups: the launch cannot be had", (ull)blocks.size());
    if (!blocks.empty()) {
      bits.resize(n_words);
      HIPC(c, hipSetDevice(c->cfg.device));
      SHK_TRY(settle(c));  // (the table is not read; the scratch may still feed a counting launch)
      Scratch m{c->misc};
      const size_t o_g = m.take<DedupGene>(dg.size()), o_b = m.take<DedupBlock>(blocks.size()), o_w = m.take<uint64_t>(rec_word.size()),
                   o_l = m.take<uint32_t>(rec_len.size()), o_t = m.take<uint64_t>(text.size()), o_bits = m.take<uint64_t>(n_words);
      HIPC(c, m.ensure());
      hipEvent_t ev0 = nullptr, ev1 = nullptr;
      HIPC(c, hipEventCreate(&ev0));
      if (hipError_t e_ = hipEventCreate(&ev1); e_ != hipSuccess) {
        (void)hipEventDestroy(ev0);
        HIPC(c, e_);
      }
      auto run = [&]() -> int {
        HIPC(c, hipMemcpyAsync(m.at<DedupGene>(o_g), dg.data(), dg.size() * sizeof(DedupGene), hipMemcpyHostToDevice, c->stream));
        HIPC(c, hipMemcpyAsync(m.at<DedupBlock>(o_b), blocks.data(), blocks.size() * sizeof(DedupBlock), hipMemcpyHostToDevice, c->stream));
        HIPC(c, hipMemcpyAsync(m.at<uint64_t>(o_w), rec_word.data(), rec_word.size() * 8, hipMemcpyHostToDevice, c->stream));
        HIPC(c, hipMemcpyAsync(m.at<uint32_t>(o_l), rec_len.data(), rec_len.size() * 4, hipMemcpyHostToDevice, c->stream));
        HIPC(c, hipMemcpyAsync(m.at<uint64_t>(o_t), text.data(), text.size() * 8, hipMemcpyHostToDevice, c->stream));
        const size_t lds = (size_t)(2 * tmax + 3) * DEDUP_WG * sizeof(int32_t);
        HIPC(c, hipEventRecord(ev0, c->stream));
        hipLaunchKernelGGL(k_dedup_panel, dim3((uint32_t)blocks.size()), dim3(DEDUP_WG), lds, c->stream, m.at<DedupGene>(o_g), m.at<DedupBlock>(o_b),
                           m.at<uint64_t>(o_w), m.at<uint32_t>(o_l), m.at<uint64_t>(o_t), m.at<uint64_t>(o_bits));
        HIPC(c, hipEventRecord(ev1, c->stream));
        HIPC(c, hipGetLastError());
        HIPC(c, hipMemcpyAsync(bits.data(), m.at<uint64_t>(o_bits), n_words * 8, hipMemcpyDeviceToHost, c->stream));
        HIPC(c, hipStreamSynchronize(c->stream));  // (also keeps the uploads alive until their copies ran)
        float ms = 0;
        HIPC(c, hipEventElapsedTime(&ms, ev0, ev1));
        out->device_ms = ms;
        return SHK_OK;
      };
      const int rc = run();
      (void)hipEventDestroy(ev0);
      (void)hipEventDestroy(ev1);
      SHK_TRY(rc);
    }
  }
  if (getenv("SHK_TRACE"))  // (read at each call: the tests look for this line)
    fprintf(stderr, "[shk] pcr_dedup_panel: %u genes, %llu pairs on the device, %llu pairs on the host, %llu pairs decided by the prefilters\n",
            n_genes, (ull)out->pairs_device, (ull)out->pairs_host, (ull)out->pairs_prefiltered);

  // the greedy pass in the reference's order; a host gene aligns what the pass asks for, or every pair when the caller
  // wants the bits
  std::vector<uint64_t> host_bits;
  std::vector<uint32_t> kept;
  for (uint32_t g = 0; g < n_genes; ++g) {
    const uint64_t ra = record_offsets[g], m = record_offsets[g + 1] - ra, t = thresholds[g];
    const uint32_t *ord = order.data() + (ra - r0);
    auto aligned = [&](uint64_t i, uint64_t j) -> bool {
      const uint64_t a = ra + ord[i], b = ra + ord[j];
      return shk_edit_within(seqs + seq_offsets[a], len_of(a), seqs + seq_offsets[b], len_of(b), (uint32_t)t) != 0;
    };
    const uint64_t *gene_bits = on_device[g] ? bits.data() + dev_bits_at[g] : nullptr;
    if (!on_device[g] && out->pair_words) {
      host_bits.assign(poff[g + 1] - poff[g], 0);
      for (uint64_t i = 0, p = 0; i < m; ++i)
        for (uint64_t j = i + 1; j < m; ++j, ++p)
          if (aligned(i, j)) host_bits[p >> 6] |= 1ull << (p & 63);
      gene_bits = host_bits.data();
    }
    if (out->pair_words && poff[g + 1] > poff[g]) memcpy(out->pair_words + poff[g], gene_bits, (poff[g + 1] - poff[g]) * 8);
    kept.clear();
    for (uint64_t j = 0; j < m; ++j) {
      bool duplicate = false;
      for (const uint32_t i : kept) {
        const uint64_t p = dedup_row_start(i, m) + (j - i - 1);
        duplicate = gene_bits ? (gene_bits[p >> 6] >> (p & 63)) & 1 : aligned(i, j);
        if (duplicate) break;
      }
      if (!duplicate) kept.push_back((uint32_t)j);
    }
    const uint32_t ret = (uint32_t)std::min<size_t>(kept.size(), SHK_PCR_MAX_AMPLICONS);
    if (out->generated) out->generated[g] = (uint32_t)m;
    if (out->retained) out->retained[g] = (uint32_t)kept.size();
    if (out->returned) out->returned[g] = ret;
    if (out->kept)
      for (uint32_t i = 0; i < ret; ++i) out->kept[(size_t)SHK_PCR_MAX_AMPLICONS * g + i] = ord[kept[i]];
  }
  if (out->order && nr) std::copy(order.begin(), order.end(), out->order + r0);
  return SHK_OK;
}

extern "C" int shk_pcr_products_panel(shk_ctx *c, const shk_pcr_graphs *graphs, const shk_pcr_paths_params *params, const uint32_t *thresholds,
                                      shk_pcr_records *out, uint32_t *retained, double *device_ms) {
  SHK_TRY(xs_closed(c));
  if (c && c->group) return on_any_device(c, [&](shk_ctx *d) { return shk_pcr_products_panel(d, graphs, params, thresholds, out, retained, device_ms); });
  if (!c || !out || !out->record_offsets) return SHK_ERR_BAD_ARG;
  if (device_ms) *device_ms = 0.0;
  out->n_records = out->n_seq_bytes = 0;
  out->record_offsets[0] = 0;
  std::string err;
  std::vector<PcrGeneRecords> records;
  try {
    if (const int rc = pcr_paths_panel_run((uint32_t)c->cfg.k, graphs, params, &records, &err); rc != SHK_OK) return fail(c, rc, "%s", err.c_str());
    const uint32_t ng = (uint32_t)records.size();
    if (ng && !thresholds) return fail(c, SHK_ERR_BAD_ARG, "shk_pcr_products_panel: thresholds is missing");
    // the records as one panel of the dedup
    std::vector<uint64_t> roff(ng + 1, 0), soff(1, 0);
    std::vector<uint8_t> seqs;
    std::vector<double> scores;
    for (uint32_t g = 0; g < ng; ++g) {
      const PcrGeneRecords &r = records[g];
      roff[g + 1] = roff[g] + r.size();
      const uint64_t base = seqs.size();
      seqs.insert(seqs.end(), r.seqs.begin(), r.seqs.end());
      for (size_t i = 1; i < r.seq_offsets.size(); ++i) soff.push_back(base + r.seq_offsets[i]);
      scores.insert(scores.end(), r.score.begin(), r.score.end());
    }
    std::vector<uint32_t> kept((size_t)SHK_PCR_MAX_AMPLICONS * std::max(ng, 1u)), returned(std::max(ng, 1u), 0u);
    shk_pcr_dedup_out d{};
    d.kept = kept.data(), d.returned = returned.data(), d.retained = retained;
    SHK_TRY(shk_pcr_dedup_panel(c, seqs.data(), soff.data(), roff.data(), scores.data(), thresholds, ng, &d));
    if (device_ms) *device_ms = d.device_ms;
    std::vector<std::vector<uint32_t>> pick(ng);
    for (uint32_t g = 0; g < ng; ++g) pick[g].assign(kept.begin() + (size_t)SHK_PCR_MAX_AMPLICONS * g, kept.begin() + (size_t)SHK_PCR_MAX_AMPLICONS * g + returned[g]);
    const int rc = pcr_records_store(records, &pick, out, &err);
    return rc == SHK_OK ? rc : fail(c, rc, "%s", err.c_str());
  } catch (...) {  // no exception leaves the C ABI
    return fail(c, SHK_ERR_NOMEM, "shk_pcr_products_panel: out of host memory");
  }
}
