// shk_prune_api.hip.h — shk_pcr_prune_panel (included by shk_engine.hip, same translation unit): the pruning stage of sPCR
// between shk_pcr_extend_panel and shk_thread_reads_panel.  The host checks the graphs, takes the first
// median, turns the f64 threshold into an integer one and builds every gene's two CSR sides by counting sort; K_PRUNE
// (shk_device.hip.h) runs the tip rounds and the two searches, one workgroup per gene; the host compacts, renumbers,
// takes the second median and divides, so that every double is the reference's own.  The table is not read.
namespace {

// median_via_select (src/pcr/graph.rs:82-103) of u32 counts; false when there are none
bool prune_median(std::vector<uint32_t> &v, double *median) {
  if (v.empty()) return false;
  const size_t mid = v.size() / 2;
  std::nth_element(v.begin(), v.begin() + mid, v.end());
  if (v.size() % 2 == 0)
    *median = ((double)*std::max_element(v.begin(), v.begin() + mid) + (double)v[mid]) / 2.0;
  else
    *median = (double)v[mid];
  return true;
}

// A u32 count c passes `(c as f64) >= min_tip_count` (pruning.rs:64, :80) iff c >= this; 2^32 when none can.
uint64_t prune_threshold(double median, double fraction) {
  const double x = median * fraction;
  const double min_tip = x > 1.0 ? x : 1.0;  // f64::max(1.0): a NaN product (0 × inf) gives 1.0 as well
  const double up = std::ceil(min_tip);
  return up > 4294967295.0 ? (1ull << 32) : (uint64_t)up;
}

// One side of a gene's adjacency by counting sort: node v's list is nbr[first[v] .. first[v + 1]), in ascending edge
// index; bit j of heavy: the edge at list position j has count >= thr.
void prune_csr_side(const uint32_t *at, const uint32_t *other, const uint32_t *counts, uint32_t n, uint32_t e, uint64_t thr,
                    uint32_t *first, uint32_t *nbr, uint32_t *heavy) {
  std::fill(first, first + n + 1, 0u);
  for (uint32_t i = 0; i < e; ++i) first[at[i] + 1] += 1;
  for (uint32_t v = 0; v < n; ++v) first[v + 1] += first[v];
  std::vector<uint32_t> fill(first, first + n);
  for (uint32_t i = 0; i < e; ++i) {
    const uint32_t j = fill[at[i]]++;
    nbr[j] = other[i];
    if (counts[i] >= thr) heavy[j >> 5] |= 1u << (j & 31);
  }
}

}  // namespace

extern "C" int shk_pcr_prune_panel(shk_ctx *c, const uint64_t *node_sub_kmers, const uint8_t *node_flags, const uint64_t *node_offsets,
                                   const uint32_t *edge_src, const uint32_t *edge_tgt, const uint32_t *edge_counts, const uint64_t *edge_offsets,
                                   uint32_t n_genes, const shk_pcr_prune_params *params, shk_pcr_prune_out *out) {
  SHK_TRY(xs_closed(c));
  using ull = unsigned long long;
  if (c && c->group)
    return on_any_device(c, [&](shk_ctx *d) {
      return shk_pcr_prune_panel(d, node_sub_kmers, node_flags, node_offsets, edge_src, edge_tgt, edge_counts, edge_offsets, n_genes, params, out);
    });
  if (!c || !out) return SHK_ERR_BAD_ARG;
  out->device_ms = 0.0;
  // everything that is refused, before the device is touched
  if (n_genes > SHK_PCR_MAX_GENES) return fail(c, SHK_ERR_BAD_ARG, "n_genes %u above SHK_PCR_MAX_GENES (%u)", n_genes, (unsigned)SHK_PCR_MAX_GENES);
  if (out->out_node_offsets) out->out_node_offsets[0] = 0;
  if (out->out_edge_offsets) out->out_edge_offsets[0] = 0;
  if (n_genes == 0) return SHK_OK;
  if (!node_offsets || !edge_offsets || !params) return fail(c, SHK_ERR_BAD_ARG, "shk_pcr_prune_panel: an offsets array or params is missing");
  for (uint32_t g = 0; g < n_genes; ++g) {
    if (node_offsets[g + 1] < node_offsets[g])
      return fail(c, SHK_ERR_BAD_ARG, "gene %u: node_offsets decrease (%llu after %llu)", g, (ull)node_offsets[g + 1], (ull)node_offsets[g]);
    if (edge_offsets[g + 1] < edge_offsets[g])
      return fail(c, SHK_ERR_BAD_ARG, "gene %u: edge_offsets decrease (%llu after %llu)", g, (ull)edge_offsets[g + 1], (ull)edge_offsets[g]);
    if (params[g].tip_coverage_fraction != params[g].tip_coverage_fraction)
      return fail(c, SHK_ERR_BAD_ARG, "gene %u: tip_coverage_fraction is NaN", g);
    if (params[g].stages > 3) return fail(c, SHK_ERR_BAD_ARG, "gene %u: stages %u (bit 0 tips, bit 1 reachability)", g, params[g].stages);
  }
  const uint64_t v0 = node_offsets[0], e0 = edge_offsets[0];
  const uint64_t nn = node_offsets[n_genes] - v0, ne = edge_offsets[n_genes] - e0;
  if (nn >= (1ull << 32) || ne >= (1ull << 32))
    return fail(c, SHK_ERR_BAD_ARG, "a panel of %llu nodes and %llu edges (gene 0 to gene %u): both totals must be below 2^32", (ull)nn, (ull)ne,
                n_genes - 1);
  if ((nn && (!node_flags || !out->node_keep)) || (ne && (!edge_src || !edge_tgt || !edge_counts)))
    return fail(c, SHK_ERR_BAD_ARG, "shk_pcr_prune_panel: a graph array or node_keep is missing");
  for (uint32_t g = 0; g < n_genes; ++g) {
    const uint64_t n = node_offsets[g + 1] - node_offsets[g];
    for (uint64_t v = node_offsets[g]; v < node_offsets[g + 1]; ++v)
      if (node_flags[v] > 3)
        return fail(c, SHK_ERR_BAD_ARG, "gene %u: node %llu has flags %u (1 is_start, 2 is_end)", g, (ull)(v - node_offsets[g]), node_flags[v]);
    for (uint64_t i = edge_offsets[g]; i < edge_offsets[g + 1]; ++i)
      if (edge_src[i] >= n || edge_tgt[i] >= n)
        return fail(c, SHK_ERR_BAD_ARG, "gene %u: edge %llu: endpoint (%u, %u) outside the gene's %llu nodes", g, (ull)(i - edge_offsets[g]),
                    edge_src[i], edge_tgt[i], (ull)n);
  }
  if (nn > (1ull << 32) - 2 * PRUNE_WG || ne > (1ull << 32) - 2 * PRUNE_WG)  // (the kernel's 32-bit strides)
    return fail(c, SHK_ERR_NOMEM, "a panel of %llu nodes and %llu edges: its device state cannot be had", (ull)nn, (ull)ne);

  // per gene: the first median and its threshold, the CSR sides, the descriptor
  const int lds_nodes = env_int("SHK_PRUNE_LDS_NODES", PRUNE_LDS_NODES);
  std::vector<uint8_t> up;
  auto put = [&up](size_t bytes) {  // (16-byte aligned, zeroed)
    const size_t at = up.size();
    up.resize(at + ((bytes + 15) & ~(size_t)15), 0);
    return at;
  };
  std::vector<PruneGene> desc(n_genes);
  std::vector<uint32_t> tmp;
  size_t lds = 0;
  uint64_t work_words = 0;
  uint32_t n_lds = 0, n_global = 0;
  for (uint32_t g = 0; g < n_genes; ++g) {
    const uint64_t va = node_offsets[g], ea = edge_offsets[g];
    const uint32_t n = (uint32_t)(node_offsets[g + 1] - va), e = (uint32_t)(edge_offsets[g + 1] - ea);
    PruneGene &d = desc[g];
    d = PruneGene{};
    d.n = n, d.e = e, d.keep = va - v0;
    d.stages = params[g].stages ? params[g].stages : 3u;
    if (!n) continue;
    tmp.assign(edge_counts + ea, edge_counts + ea + e);
    double median = 1.0;  // global_median_edge_count(..).unwrap_or(1.0)
    prune_median(tmp, &median);
    const uint64_t thr = prune_threshold(median, params[g].tip_coverage_fraction);
    const size_t words = (e + 31) / 32;
    d.in_first = put(4 * ((size_t)n + 1)), d.out_first = put(4 * ((size_t)n + 1));
    d.in_nbr = put(4 * (size_t)e), d.out_nbr = put(4 * (size_t)e);
    d.in_heavy = put(4 * words), d.out_heavy = put(4 * words);
    d.flags = put(n);
    uint8_t *b = up.data();  // (taken after the last put of this gene)
    prune_csr_side(edge_tgt + ea, edge_src + ea, edge_counts + ea, n, e, thr, (uint32_t *)(b + d.in_first), (uint32_t *)(b + d.in_nbr),
                   (uint32_t *)(b + d.in_heavy));
    prune_csr_side(edge_src + ea, edge_tgt + ea, edge_counts + ea, n, e, thr, (uint32_t *)(b + d.out_first), (uint32_t *)(b + d.out_nbr),
                   (uint32_t *)(b + d.out_heavy));
    memcpy(b + d.flags, node_flags + va, n);
    const size_t gene_lds = prune_lds_bytes(n, e);
    d.lds = (int64_t)n <= (int64_t)lds_nodes && gene_lds <= PRUNE_LDS_MAX;
    if (d.lds) {
      lds = std::max(lds, gene_lds);
      ++n_lds;
    } else {
      d.work = work_words;
      work_words += 4 * (uint64_t)n;
      ++n_global;
    }
  }
  std::vector<PruneCounters> cnt(n_genes, PruneCounters{0, 0, 0, 0});
  uint8_t *keep = out->node_keep ? out->node_keep + v0 : nullptr;
  if (nn) {
    const size_t o_desc_up = put(desc.size() * sizeof(PruneGene));
    memcpy(up.data() + o_desc_up, desc.data(), desc.size() * sizeof(PruneGene));
    HIPC(c, hipSetDevice(c->cfg.device));
    SHK_TRY(settle(c));  // (not table_read_begin: the table is not read; the scratch may still feed a counting launch)
    Scratch m{c->misc};
    const size_t o_up = m.take<uint8_t>(up.size()), o_work = m.take<uint32_t>(work_words), o_keep = m.take<uint8_t>(nn),
                 o_cnt = m.take<PruneCounters>(n_genes);
    HIPC(c, m.ensure());
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    HIPC(c, hipEventCreate(&ev0));
    if (hipError_t e_ = hipEventCreate(&ev1); e_ != hipSuccess) {
      (void)hipEventDestroy(ev0);
      HIPC(c, e_);
    }
    auto run = [&]() -> int {
      HIPC(c, hipMemcpyAsync(m.at<uint8_t>(o_up), up.data(), up.size(), hipMemcpyHostToDevice, c->stream));
      if (getenv("SHK_TRACE"))  // (read at each call, like SHK_PRUNE_LDS_NODES: the tests look for this line)
        fprintf(stderr, "[shk] pcr_prune_panel: %u genes, %u genes in LDS (%zu bytes), %u genes in global memory\n", n_genes, n_lds, lds, n_global);
      if (lds > (64u << 10) && !c->lds_attr_prune) {  // > 64 KiB of dynamic LDS has to be asked for once
        HIPC(c, hipFuncSetAttribute(reinterpret_cast<const void *>(&k_prune_panel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)PRUNE_LDS_MAX));
        c->lds_attr_prune = true;
      }
      HIPC(c, hipEventRecord(ev0, c->stream));
      hipLaunchKernelGGL(k_prune_panel, dim3(n_genes), dim3(PRUNE_WG), lds, c->stream, (const PruneGene *)(m.at<uint8_t>(o_up) + o_desc_up),
                         (const uint8_t *)m.at<uint8_t>(o_up), m.at<uint32_t>(o_work), m.at<uint8_t>(o_keep), m.at<PruneCounters>(o_cnt),
                         (uint32_t)c->cfg.k);
      HIPC(c, hipEventRecord(ev1, c->stream));
      HIPC(c, hipGetLastError());
      HIPC(c, hipMemcpyAsync(keep, m.at<uint8_t>(o_keep), nn, hipMemcpyDeviceToHost, c->stream));
      HIPC(c, hipMemcpyAsync(cnt.data(), m.at<PruneCounters>(o_cnt), (size_t)n_genes * sizeof(PruneCounters), hipMemcpyDeviceToHost, c->stream));
      HIPC(c, hipStreamSynchronize(c->stream));  // (also keeps the upload alive until its copy ran)
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

  // the compacted graphs: survivors in ascending original index, endpoints renumbered, the second median, the ratios
  std::vector<uint64_t> noff(n_genes + 1, 0), eoff(n_genes + 1, 0);
  for (uint32_t g = 0; g < n_genes; ++g) {
    const uint64_t va = node_offsets[g], ea = edge_offsets[g];
    uint64_t kn = 0, ke = 0;
    for (uint64_t v = va; v < node_offsets[g + 1]; ++v) kn += out->node_keep[v] != 0;
    for (uint64_t i = ea; i < edge_offsets[g + 1]; ++i) ke += out->node_keep[va + edge_src[i]] && out->node_keep[va + edge_tgt[i]];
    noff[g + 1] = noff[g] + kn, eoff[g + 1] = eoff[g] + ke;
    if (out->tip_rounds) out->tip_rounds[g] = cnt[g].tip_rounds;
    if (out->tips_removed) out->tips_removed[g] = cnt[g].tips_removed;
    if (out->unreachable_removed) out->unreachable_removed[g] = cnt[g].unreachable_removed;
  }
  if (out->out_node_offsets) std::copy(noff.begin(), noff.end(), out->out_node_offsets);
  if (out->out_edge_offsets) std::copy(eoff.begin(), eoff.end(), out->out_edge_offsets);
  const bool want_nodes = out->node_sub_kmers || out->node_flags || out->node_index;
  const bool want_edges = out->edge_src || out->edge_tgt || out->edge_counts || out->edge_index || out->coverage_ratio;
  const bool fits = (!want_nodes || noff[n_genes] <= out->node_cap) && (!want_edges || eoff[n_genes] <= out->edge_cap);
  std::vector<uint32_t> renum;
  for (uint32_t g = 0; g < n_genes; ++g) {
    const uint64_t va = node_offsets[g], ea = edge_offsets[g];
    const uint32_t n = desc[g].n, e = desc[g].e;
    // the pruned graph's median (annotate_coverage_ratios, graph.rs:533-546): needs no room in the caller's arrays
    tmp.clear();
    for (uint32_t i = 0; i < e; ++i)
      if (out->node_keep[va + edge_src[ea + i]] && out->node_keep[va + edge_tgt[ea + i]]) tmp.push_back(edge_counts[ea + i]);
    double median = 0.0;
    const bool annotated = prune_median(tmp, &median) && median > 0.0;
    if (out->median) out->median[g] = median;
    if (!fits) continue;
    renum.assign(n, 0u);
    uint64_t at = noff[g];
    for (uint32_t v = 0; v < n; ++v) {
      if (!out->node_keep[va + v]) continue;
      renum[v] = (uint32_t)(at - noff[g]);
      if (out->node_sub_kmers && node_sub_kmers) out->node_sub_kmers[at] = node_sub_kmers[va + v];
      if (out->node_flags) out->node_flags[at] = node_flags[va + v];
      if (out->node_index) out->node_index[at] = v;
      ++at;
    }
    at = eoff[g];
    for (uint32_t i = 0; i < e; ++i) {
      const uint32_t s = edge_src[ea + i], t = edge_tgt[ea + i];
      if (!out->node_keep[va + s] || !out->node_keep[va + t]) continue;
      if (out->edge_src) out->edge_src[at] = renum[s];
      if (out->edge_tgt) out->edge_tgt[at] = renum[t];
      if (out->edge_counts) out->edge_counts[at] = edge_counts[ea + i];
      if (out->edge_index) out->edge_index[at] = i;
      if (out->coverage_ratio) out->coverage_ratio[at] = annotated ? (double)edge_counts[ea + i] / median : 0.0;
      ++at;
    }
  }
  if (!fits)
    return fail(c, SHK_ERR_BAD_ARG, "pruned panel of %llu nodes and %llu edges does not fit node_cap %llu / edge_cap %llu", (ull)noff[n_genes],
                (ull)eoff[n_genes], (ull)out->node_cap, (ull)out->edge_cap);
  return SHK_OK;
}
