// shk_retain_api.hip.h — the retained reads' calls of the C ABI (included by shk_engine.hip, same translation unit, behind
// shk_reads_api.hip.h whose plans and cores it runs): the switch, what the store holds, the export back to ASCII, and
// the panel filter and the panel threading over every retained read.  The store itself and its appends are the
// ingest's (RetainStore, retain_reserve, retain_append next to ingest_core; K_RETAIN in shk_device.hip.h).
namespace {

// What opens every retained call: one device, retention on, the context settled — so an invalid byte of a queued batch
// has poisoned it by now — and not poisoned.
int retained_begin(shk_ctx *c, const char *who) {
  SHK_TRY(single_device_only(c));
  if (!c->retain.on) return fail(c, SHK_ERR_STATE, "%s: reads are not retained (shk_retain_reads)", who);
  HIPC(c, hipSetDevice(c->cfg.device));
  if (c->poisoned) return fail(c, c->poison_code, "%s", c->err.c_str());
  SHK_TRY(settle(c));  // (not table_read_begin: the table is not read)
  if (c->poisoned) return fail(c, c->poison_code, "%s", c->err.c_str());
  return SHK_OK;
}

// Every retained read as a batch (n_reads > 0), as batch_from_device opens one: the offsets copied back — behind every
// queued append, which the context's stream orders — and checked.
int batch_from_retained(shk_ctx *c, const char *who, ReadBatch *b) {
  const RetainStore &st = c->retain;
  std::vector<uint64_t> h_off(st.n_reads + 1);
  HIPC(c, hipMemcpyAsync(h_off.data(), st.offsets, (st.n_reads + 1) * 8, hipMemcpyDeviceToHost, c->stream));
  HIPC(c, hipStreamSynchronize(c->stream));
  *b = ReadBatch{nullptr, nullptr, st.n_reads, st.n_bases, 0, PlaneReads{st.p0(), st.p1(), st.nn(), st.offsets}};
  return batch_check_offsets(c, h_off.data(), st.n_reads, st.n_bases, who, &b->max_len);
}

// The two halves of an export from one store (opened by retained_begin): the store's offsets of reads [first, first + n]
// (n > 0, inside the store), checked; and bases [B0, B0 + need) (need > 0) as ASCII into host memory.
int retained_export_offsets(shk_ctx *c, uint64_t first, uint64_t n, std::vector<uint64_t> *h_off) {
  const RetainStore &st = c->retain;
  h_off->resize(n + 1);
  HIPC(c, hipMemcpyAsync(h_off->data(), st.offsets + first, (n + 1) * 8, hipMemcpyDeviceToHost, c->stream));
  HIPC(c, hipStreamSynchronize(c->stream));
  for (uint64_t i = 0; i < n; ++i)
    if ((*h_off)[i + 1] < (*h_off)[i] || (*h_off)[i + 1] > st.n_bases) return fail(c, SHK_ERR_BAD_ARG, "offsets must be non-decreasing");
  return SHK_OK;
}
int retained_export_bases(shk_ctx *c, uint64_t B0, uint64_t need, uint8_t *bases) {
  const RetainStore &st = c->retain;
  Scratch m{c->misc};
  const size_t o_out = m.take<uint8_t>(need + 16);
  HIPC(c, m.ensure());
  hipLaunchKernelGGL(k_retained_export, dim3((uint32_t)((need + 16ull * WG - 1) / (16ull * WG))), dim3(WG), 0, c->stream,
                     (const uint64_t *)st.p0(), (const uint64_t *)st.p1(), (const uint64_t *)st.nn(), B0, need, m.at<uint8_t>(o_out));
  HIPC(c, hipGetLastError());
  HIPC(c, hipMemcpyAsync(bases, m.at<uint8_t>(o_out), need, hipMemcpyDeviceToHost, c->stream));
  HIPC(c, hipStreamSynchronize(c->stream));
  return SHK_OK;
}

// ---- a multi-device context with SHK_FLAG_GROUP_READS: every share walks its own store, the host stitches ----

// Whether the retained calls answer on this multi-device context (without the flag: single_device_only's refusal).
bool group_reads(const shk_ctx *c) { return c && c->group && (c->cfg.flags & SHK_FLAG_GROUP_READS) != 0; }
bool retain_is_on(const shk_ctx *c) { return c->group ? c->group->retain_on : c->retain.on; }

// f(d) on every share's worker at once; a share's failure → the context's error.
template <class F>
int group_each(shk_ctx *top, F f) {
  uint32_t who = 0;
  const int rc = top->group->run(f, &who);
  return rc == SHK_OK ? rc : group_fail(top, top->group, rc, who);
}

// retained_begin on the group: retention on, no round failed under it, and every share opened as a one-device context is.
int group_retained_begin(shk_ctx *top, const char *who) {
  shk_group *g = top->group;
  if (!g->retain_on) return fail(top, SHK_ERR_STATE, "%s: reads are not retained (shk_retain_reads)", who);
  if (g->retain_rc != SHK_OK) return fail(top, g->retain_rc, "%s", g->retain_err.c_str());
  return group_each(top, [&](uint32_t d) { return retained_begin(g->ctx[d], who); });
}

int group_retain_switch(shk_ctx *top, int on, uint64_t capacity_bases_hint) {
  shk_group *g = top->group;
  const uint32_t D = g->D;
  if (!on) {
    for (uint32_t d = 0; d < D; ++d) {
      const int rc = shk_retain_reads(g->ctx[d], 0, 0);
      if (rc != SHK_OK) return group_fail(top, g, rc, d);
    }
    g->retain_on = false;
    g->reads_dir.clear();
    g->retain_rc = SHK_OK;
    return SHK_OK;
  }
  if (g->retain_on) return g->reads_dir.total() ? fail(top, SHK_ERR_STATE, "reads are being retained already") : SHK_OK;
  uint64_t given = 0;  // the one-device condition, over all shares
  for (uint32_t d = 0; d < D; ++d) {
    given += g->ctx[d]->n_reads_read + g->ctx[d]->n_bases_read;
    for (const uint64_t n : g->ctx[d]->lane_reads) given += n;
  }
  if (given) return fail(top, SHK_ERR_STATE, "shk_retain_reads: the context holds reads already; switch retention on after shk_create or shk_reset");
  for (uint32_t d = 0; d < D; ++d) {
    const int rc = shk_retain_reads(g->ctx[d], 1, (capacity_bases_hint + D - 1) / D);
    if (rc != SHK_OK) {
      for (uint32_t e = 0; e < d; ++e) (void)shk_retain_reads(g->ctx[e], 0, 0);
      return group_fail(top, g, rc, d);
    }
  }
  g->retain_on = true;
  g->reads_dir.clear();
  g->retain_rc = SHK_OK;
  return SHK_OK;
}

int group_retained_export(shk_ctx *top, uint64_t first_read, uint64_t n_reads, uint8_t *bases, uint64_t bases_cap, uint64_t *offsets,
                          uint64_t *n_bases) {
  shk_group *g = top->group;
  const uint32_t D = g->D;
  std::vector<shk::GroupPiece> pieces;
  if (!g->reads_dir.split(first_read, n_reads, &pieces))
    return fail(top, SHK_ERR_BAD_ARG, "reads %llu to %llu are outside the %llu retained reads", (unsigned long long)first_read,
                (unsigned long long)(first_read + n_reads), (unsigned long long)g->reads_dir.total());
  offsets[0] = 0;
  if (n_reads == 0) return SHK_OK;
  // a share's pieces of one global range are consecutive runs of its store: one local range [lo, hi) per share
  std::vector<uint64_t> lo(D, 0), hi(D, 0);
  for (const shk::GroupPiece &p : pieces) {
    if (hi[p.share] == 0) lo[p.share] = p.local_first;
    hi[p.share] = p.local_first + p.n_reads;
  }
  std::vector<std::vector<uint64_t>> h_off(D);
  SHK_TRY(group_each(top, [&](uint32_t d) { return hi[d] > lo[d] ? retained_export_offsets(g->ctx[d], lo[d], hi[d] - lo[d], &h_off[d]) : SHK_OK; }));
  uint64_t need = 0;
  for (uint32_t d = 0; d < D; ++d)
    if (hi[d] > lo[d]) need += h_off[d].back() - h_off[d][0];
  *n_bases = need;
  if (need > bases_cap || (need && !bases))
    return fail(top, SHK_ERR_BAD_ARG, "%llu bases do not fit bases_cap %llu", (unsigned long long)need, (unsigned long long)bases_cap);
  std::vector<std::vector<uint8_t>> part(D);
  SHK_TRY(group_each(top, [&](uint32_t d) {
    const uint64_t nb = hi[d] > lo[d] ? h_off[d].back() - h_off[d][0] : 0;
    part[d].resize(nb);
    return nb ? retained_export_bases(g->ctx[d], h_off[d][0], nb, part[d].data()) : SHK_OK;
  }));
  uint64_t at = 0, r = 0;  // the pieces in global order
  for (const shk::GroupPiece &p : pieces) {
    const uint64_t *o = h_off[p.share].data() + (p.local_first - lo[p.share]);
    const uint64_t nb = o[p.n_reads] - o[0];
    if (nb) memcpy(bases + at, part[p.share].data() + (o[0] - h_off[p.share][0]), nb);
    for (uint64_t i = 1; i <= p.n_reads; ++i) offsets[r + i] = at + (o[i] - o[0]);
    at += nb, r += p.n_reads;
  }
  return SHK_OK;
}

// The panel filter over every share's store (opened by group_retained_begin; match_offsets zero, *n_matches 0; the plan
// not empty): each share's records come back whole, so the caller's match_cap costs no share a second walk.
int group_filter_retained(shk_ctx *top, const HostKeyRuns &pl, uint32_t n_genes, uint64_t *match_offsets, uint64_t *match_reads,
                          uint64_t match_cap, uint64_t *n_matches) {
  shk_group *g = top->group;
  const uint32_t D = g->D;
  std::vector<std::vector<uint64_t>> recs(D);
  SHK_TRY(group_each(top, [&](uint32_t d) {
    shk_ctx *c = g->ctx[d];
    if (c->retain.n_reads == 0) return (int)SHK_OK;  // (nothing to walk: nothing is launched)
    ReadBatch b;
    SHK_TRY(batch_from_retained(c, "shk_filter_reads_panel", &b));
    return panel_records(c, pl, n_genes, b, &recs[d]);
  }));
  // a share's records are sorted by (gene, local read), and local order is global order within a share: per gene D
  // ascending lists of global indices, merged
  std::vector<size_t> at(D, 0);
  std::vector<std::vector<uint64_t>> lists(D);
  std::vector<uint64_t> merged, all;
  for (uint32_t gene = 0; gene < n_genes; ++gene) {
    for (uint32_t d = 0; d < D; ++d) {
      lists[d].clear();
      for (; at[d] < recs[d].size() && (recs[d][at[d]] >> FILTER_READ_BITS) == gene; ++at[d])
        lists[d].push_back(g->reads_dir.to_global(d, recs[d][at[d]] & ((1ull << FILTER_READ_BITS) - 1)));
    }
    shk::group_merge_ascending(lists, &merged);
    all.insert(all.end(), merged.begin(), merged.end());
    match_offsets[gene + 1] = all.size();
  }
  const uint64_t nt = all.size();
  *n_matches = nt;
  if (nt > match_cap || (nt && !match_reads))
    return fail(top, SHK_ERR_BAD_ARG, "%llu matches do not fit match_cap %llu", (unsigned long long)nt, (unsigned long long)match_cap);
  std::copy(all.begin(), all.end(), match_reads);
  return SHK_OK;
}

// The panel threading over the shares' stores (opened by group_retained_begin; the plan made against the total retained
// count, res's supports zero): every gene's list is split by owner share in list order, each share with listed reads
// threads its local lists, and the host adds the supports, merge-sums the links, puts read_edges back at their list
// positions and counts the pairs over them — so a pair whose mates lie on two shares counts as on one device.
int group_thread_retained(shk_ctx *top, const ThreadPanelPlan &pp, uint32_t n_genes, const uint64_t *list_offsets, const uint64_t *list_reads,
                          const uint64_t *read_index, const uint8_t *mate, bool mate_rule, ThreadPanelResult *res) {
  shk_group *g = top->group;
  const uint32_t D = g->D;
  res->link_off.assign(n_genes + 1, 0);
  res->n_paired.assign(n_genes, 0);
  if (pp.n_edges == 0 || pp.n_listed == 0) return SHK_OK;  // (the outputs are zero already)
  const bool pairs = mate || mate_rule, want_re = res->read_edges || pairs;
  struct Share {
    std::vector<uint64_t> loff, lreads, pos;  // its lists (local indices) and their positions in the caller's, from pp.l0
    std::vector<uint32_t> tot, una, re;
    ThreadPanelResult res{};
  };
  std::vector<Share> sh(D);
  for (Share &s : sh) s.loff.assign(n_genes + 1, 0);
  for (uint32_t gene = 0; gene < n_genes; ++gene) {
    for (uint64_t p = list_offsets[gene]; p < list_offsets[gene + 1]; ++p) {
      uint32_t d = 0;
      uint64_t local = 0;
      if (!g->reads_dir.lookup(list_reads[p], &d, &local)) return fail(top, SHK_ERR_INVARIANT, "retained read %llu is in no share's store", (unsigned long long)list_reads[p]);
      sh[d].lreads.push_back(local), sh[d].pos.push_back(p - pp.l0);
    }
    for (Share &s : sh) s.loff[gene + 1] = s.lreads.size();
  }
  SHK_TRY(group_each(top, [&](uint32_t d) {
    Share &s = sh[d];
    if (s.lreads.empty()) return (int)SHK_OK;  // (no listed reads: nothing is launched)
    shk_ctx *c = g->ctx[d];
    s.tot.assign(pp.n_edges, 0), s.una.assign(pp.n_edges, 0);
    if (want_re) s.re.assign(s.lreads.size(), 0);
    s.res = ThreadPanelResult{s.tot.data(), s.una.data(), want_re ? s.re.data() : nullptr, {}, {}, {}, {}, {}};
    ReadBatch b;
    SHK_TRY(batch_from_retained(c, "shk_thread_reads_panel", &b));
    const ThreadListSpan span{0, s.lreads.size()};
    return thread_panel_core(c, pp, n_genes, b, s.loff.data(), s.lreads.data(), nullptr, nullptr, &s.res, false, &span);
  }));
  std::vector<uint32_t> re_own;
  uint32_t *re = res->read_edges;
  if (!re && pairs) {
    re_own.assign(pp.n_listed, 0);
    re = re_own.data();
  }
  for (const Share &s : sh) {
    if (s.lreads.empty()) continue;
    for (uint64_t e = 0; e < pp.n_edges; ++e) res->support_total[e] += s.tot[e], res->support_unambiguous[e] += s.una[e];
    for (size_t j = 0; re && j < s.pos.size(); ++j) re[s.pos[j]] = s.re[j];
  }
  std::vector<std::vector<shk::GroupLink>> lists(D);
  std::vector<shk::GroupLink> merged;
  for (uint32_t gene = 0; gene < n_genes; ++gene) {
    for (uint32_t d = 0; d < D; ++d) {
      lists[d].clear();
      const ThreadPanelResult &r = sh[d].res;
      for (uint64_t i = r.link_off.empty() ? 0 : r.link_off[gene]; !r.link_off.empty() && i < r.link_off[gene + 1]; ++i)
        lists[d].push_back(shk::GroupLink{r.link_in[i], r.link_out[i], r.link_counts[i]});
    }
    shk::group_merge_links(lists, &merged);
    for (const shk::GroupLink &l : merged) res->link_in.push_back(l.in), res->link_out.push_back(l.out), res->link_counts.push_back(l.count);
    res->link_off[gene + 1] = res->link_in.size();
    const uint64_t l_at = list_offsets[gene] - pp.l0, n_list = list_offsets[gene + 1] - list_offsets[gene];
    if (pairs) res->n_paired[gene] = thread_paired_links(list_reads + list_offsets[gene], n_list, mate ? read_index : nullptr, mate, re + l_at);
  }
  return SHK_OK;
}

}  // namespace

extern "C" {

int shk_retain_reads(shk_ctx *c, int on, uint64_t capacity_bases_hint) {
  SHK_TRY(xs_closed(c));
  if (group_reads(c)) return group_retain_switch(c, on, capacity_bases_hint);
  SHK_TRY(single_device_only(c));
  HIPC(c, hipSetDevice(c->cfg.device));
  RetainStore &st = c->retain;
  if (!on) {
    if (st.planes || st.offsets) HIPC(c, hipStreamSynchronize(c->stream));  // (an append may still be queued)
    dev_free(st.planes, st.planes_alloc);
    dev_free(st.offsets, st.offsets_alloc);
    st = RetainStore{};
    return SHK_OK;
  }
  if (st.on) return st.n_reads ? fail(c, SHK_ERR_STATE, "reads are being retained already") : SHK_OK;
  uint64_t given = c->n_reads_read + c->n_bases_read;
  for (const uint64_t n : c->lane_reads) given += n;
  if (given) return fail(c, SHK_ERR_STATE, "shk_retain_reads: the context holds reads already; switch retention on after shk_create or shk_reset");
  st.on = true;
  st.hint_bases = capacity_bases_hint;
  return SHK_OK;
}

int shk_retained_info(shk_ctx *c, uint64_t *n_reads, uint64_t *n_bases, uint64_t *device_bytes) {
  SHK_TRY(xs_closed(c));
  if (group_reads(c)) {  // summed over the shares
    uint64_t r = 0, b = 0, bytes = 0;
    for (const shk_ctx *d : c->group->ctx) r += d->retain.n_reads, b += d->retain.n_bases, bytes += d->retain.planes_alloc + d->retain.offsets_alloc;
    if (n_reads) *n_reads = r;
    if (n_bases) *n_bases = b;
    if (device_bytes) *device_bytes = bytes;
    return SHK_OK;
  }
  SHK_TRY(single_device_only(c));
  const RetainStore &st = c->retain;
  if (n_reads) *n_reads = st.n_reads;
  if (n_bases) *n_bases = st.n_bases;
  if (device_bytes) *device_bytes = st.planes_alloc + st.offsets_alloc;
  return SHK_OK;
}

int shk_retained_export(shk_ctx *c, uint64_t first_read, uint64_t n_reads, uint8_t *bases, uint64_t bases_cap, uint64_t *offsets,
                        uint64_t *n_bases) {
  SHK_TRY(xs_closed(c));
  if (c && (!c->group || group_reads(c)) && (!offsets || !n_bases)) return SHK_ERR_BAD_ARG;
  if (group_reads(c)) {
    SHK_TRY(group_retained_begin(c, "shk_retained_export"));
    *n_bases = 0;
    return group_retained_export(c, first_read, n_reads, bases, bases_cap, offsets, n_bases);
  }
  SHK_TRY(retained_begin(c, "shk_retained_export"));
  const RetainStore &st = c->retain;
  *n_bases = 0;
  if (first_read > st.n_reads || n_reads > st.n_reads - first_read)
    return fail(c, SHK_ERR_BAD_ARG, "reads %llu to %llu are outside the %llu retained reads", (unsigned long long)first_read,
                (unsigned long long)(first_read + n_reads), (unsigned long long)st.n_reads);
  offsets[0] = 0;
  if (n_reads == 0) return SHK_OK;
  std::vector<uint64_t> h_off;
  SHK_TRY(retained_export_offsets(c, first_read, n_reads, &h_off));
  const uint64_t B0 = h_off[0], need = h_off[n_reads] - B0;
  *n_bases = need;
  if (need > bases_cap || (need && !bases))
    return fail(c, SHK_ERR_BAD_ARG, "%llu bases do not fit bases_cap %llu", (unsigned long long)need, (unsigned long long)bases_cap);
  for (uint64_t i = 0; i <= n_reads; ++i) offsets[i] = h_off[i] - B0;
  return need ? retained_export_bases(c, B0, need, bases) : SHK_OK;
}

int shk_filter_reads_panel_retained(shk_ctx *c, const uint64_t *primer_kmers, const uint64_t *gene_offsets, uint32_t n_genes,
                                    uint64_t *match_offsets, uint64_t *match_reads, uint64_t match_cap, uint64_t *n_matches) {
  SHK_TRY(xs_closed(c));
  if (c && (!c->group || group_reads(c)) && (!match_offsets || !n_matches)) return SHK_ERR_BAD_ARG;
  if (!group_reads(c)) SHK_TRY(single_device_only(c));
  if (!retain_is_on(c)) return fail(c, SHK_ERR_STATE, "shk_filter_reads_panel_retained: reads are not retained (shk_retain_reads)");
  HostKeyRuns pl;
  SHK_TRY(panel_plan(c, primer_kmers, gene_offsets, n_genes, &pl));
  std::fill(match_offsets, match_offsets + n_genes + 1, 0ull);
  *n_matches = 0;
  if (c->group) {  // one plan, every share's store walked at once
    SHK_TRY(group_retained_begin(c, "shk_filter_reads_panel_retained"));
    if (c->group->reads_dir.total() == 0 || pl.items.empty()) return SHK_OK;
    return group_filter_retained(c, pl, n_genes, match_offsets, match_reads, match_cap, n_matches);
  }
  SHK_TRY(retained_begin(c, "shk_filter_reads_panel_retained"));
  if (c->retain.n_reads == 0) return SHK_OK;
  ReadBatch b;
  SHK_TRY(batch_from_retained(c, "shk_filter_reads_panel", &b));
  if (pl.items.empty()) return SHK_OK;
  return panel_core(c, pl, n_genes, b, match_offsets, match_reads, match_cap, n_matches);
}

int shk_thread_reads_panel_retained(shk_ctx *c, const uint64_t *node_sub_kmers, const uint64_t *node_offsets, const uint32_t *edge_src,
                                    const uint32_t *edge_tgt, const uint64_t *edge_offsets, uint32_t n_genes, const uint64_t *list_offsets,
                                    const uint64_t *list_reads, const uint64_t *read_index, const uint8_t *mate, shk_thread_panel_out *out) {
  SHK_TRY(xs_closed(c));
  if (c && (!c->group || group_reads(c)) && !out) return SHK_ERR_BAD_ARG;
  if (!group_reads(c)) SHK_TRY(single_device_only(c));
  if (!retain_is_on(c)) return fail(c, SHK_ERR_STATE, "shk_thread_reads_panel_retained: reads are not retained (shk_retain_reads)");
  const uint64_t n_seqs = c->group ? c->group->reads_dir.total() : c->retain.n_reads;
  ThreadPanelPlan pp;
  SHK_TRY(thread_panel_plan(c, node_sub_kmers, node_offsets, edge_src, edge_tgt, edge_offsets, n_genes, n_seqs, list_offsets, list_reads, read_index,
                            mate, out, &pp));
  thread_panel_out_zero(out, pp, n_genes);
  if (c->group) {  // every share threads the listed reads it holds, the host combines
    SHK_TRY(group_retained_begin(c, "shk_thread_reads_panel_retained"));
    if (n_seqs == 0 || n_genes == 0) return SHK_OK;
    ThreadPanelResult res{out->support_total + pp.e0, out->support_unambiguous + pp.e0, out->read_edges ? out->read_edges + pp.l0 : nullptr,
                          {}, {}, {}, {}, {}};
    SHK_TRY(group_thread_retained(c, pp, n_genes, list_offsets, list_reads, read_index, mate, false, &res));
    return thread_panel_finish(c, res, n_genes, out);
  }
  SHK_TRY(retained_begin(c, "shk_thread_reads_panel_retained"));
  if (n_seqs == 0 || n_genes == 0) return SHK_OK;
  ReadBatch b;
  SHK_TRY(batch_from_retained(c, "shk_thread_reads_panel", &b));
  return thread_panel_run(c, pp, n_genes, b, list_offsets, list_reads, read_index, mate, out);
}

}  // extern "C"
