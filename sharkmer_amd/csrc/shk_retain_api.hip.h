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

}  // namespace

extern "C" {

int shk_retain_reads(shk_ctx *c, int on, uint64_t capacity_bases_hint) {
  SHK_TRY(xs_closed(c));
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
  if (c && !c->group && (!offsets || !n_bases)) return SHK_ERR_BAD_ARG;
  SHK_TRY(retained_begin(c, "shk_retained_export"));
  const RetainStore &st = c->retain;
  *n_bases = 0;
  if (first_read > st.n_reads || n_reads > st.n_reads - first_read)
    return fail(c, SHK_ERR_BAD_ARG, "reads %llu to %llu are outside the %llu retained reads", (unsigned long long)first_read,
                (unsigned long long)(first_read + n_reads), (unsigned long long)st.n_reads);
  offsets[0] = 0;
  if (n_reads == 0) return SHK_OK;
  std::vector<uint64_t> h_off(n_reads + 1);
  HIPC(c, hipMemcpyAsync(h_off.data(), st.offsets + first_read, (n_reads + 1) * 8, hipMemcpyDeviceToHost, c->stream));
  HIPC(c, hipStreamSynchronize(c->stream));
  const uint64_t B0 = h_off[0], need = h_off[n_reads] - B0;
  for (uint64_t i = 0; i < n_reads; ++i)
    if (h_off[i + 1] < h_off[i] || h_off[i + 1] > st.n_bases) return fail(c, SHK_ERR_BAD_ARG, "offsets must be non-decreasing");
  *n_bases = need;
  if (need > bases_cap || (need && !bases))
    return fail(c, SHK_ERR_BAD_ARG, "%llu bases do not fit bases_cap %llu", (unsigned long long)need, (unsigned long long)bases_cap);
  for (uint64_t i = 0; i <= n_reads; ++i) offsets[i] = h_off[i] - B0;
  if (need == 0) return SHK_OK;
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

int shk_filter_reads_panel_retained(shk_ctx *c, const uint64_t *primer_kmers, const uint64_t *gene_offsets, uint32_t n_genes,
                                    uint64_t *match_offsets, uint64_t *match_reads, uint64_t match_cap, uint64_t *n_matches) {
  SHK_TRY(xs_closed(c));
  if (c && !c->group && (!match_offsets || !n_matches)) return SHK_ERR_BAD_ARG;
  SHK_TRY(single_device_only(c));
  if (!c->retain.on) return fail(c, SHK_ERR_STATE, "shk_filter_reads_panel_retained: reads are not retained (shk_retain_reads)");
  HostKeyRuns pl;
  SHK_TRY(panel_plan(c, primer_kmers, gene_offsets, n_genes, &pl));
  std::fill(match_offsets, match_offsets + n_genes + 1, 0ull);
  *n_matches = 0;
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
  if (c && !c->group && !out) return SHK_ERR_BAD_ARG;
  SHK_TRY(single_device_only(c));
  if (!c->retain.on) return fail(c, SHK_ERR_STATE, "shk_thread_reads_panel_retained: reads are not retained (shk_retain_reads)");
  const uint64_t n_seqs = c->retain.n_reads;
  ThreadPanelPlan pp;
  SHK_TRY(thread_panel_plan(c, node_sub_kmers, node_offsets, edge_src, edge_tgt, edge_offsets, n_genes, n_seqs, list_offsets, list_reads, read_index,
                            mate, out, &pp));
  thread_panel_out_zero(out, pp, n_genes);
  SHK_TRY(retained_begin(c, "shk_thread_reads_panel_retained"));
  if (n_seqs == 0 || n_genes == 0) return SHK_OK;
  ReadBatch b;
  SHK_TRY(batch_from_retained(c, "shk_thread_reads_panel", &b));
  return thread_panel_run(c, pp, n_genes, b, list_offsets, list_reads, read_index, mate, out);
}

}  // extern "C"
