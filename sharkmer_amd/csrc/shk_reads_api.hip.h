// shk_reads_api.hip.h — the read-side calls of the C ABI (included by shk_engine.hip, same translation unit): a batch of
// reads walked against a lookup set the host builds (shk_filter_reads, shk_filter_reads_panel, shk_thread_reads[_panel]), decoded
// (shk_kmers_from_reads) or copied (shk_gather_reads_device).  None reads the table.  What they share comes first: the
// host side of set_find / KeyRuns (shk_device.hip.h), the two openers of a batch, the LDS-or-global launch, the forward.
namespace {

// A call that keeps no state on its device, on a multi-device context: any device will do.
template <class F>
int on_any_device(shk_ctx *c, F call) {
  const int rc = call(c->group->ctx[0]);
  return rc == SHK_OK ? rc : group_fail(c, c->group, rc, 0);
}

// slots for n keys at load ≤ 1/2
uint64_t set_capacity(uint64_t n) {
  uint64_t cap = 16;
  while (cap < 2 * n) cap <<= 1;
  return cap;
}
// key's slot in an open-addressing set (2^n slots, EMPTY where free), taken now if the key was new: set_find's probe rule
uint64_t set_insert(std::vector<uint64_t> &keys, uint64_t key) {
  const uint64_t mask = keys.size() - 1;
  for (uint64_t s = set_hash(key) & mask;; s = (s + 1) & mask) {
    if (keys[s] == EMPTY) keys[s] = key;
    if (keys[s] == key) return s;
  }
}

// KeyRuns (shk_device.hip.h) on the host, from (key, item) pairs sorted by (key, item).
struct HostKeyRuns {
  std::vector<uint64_t> keys;                // open addressing by set_hash, EMPTY where free, load ≤ 1/2
  std::vector<uint32_t> start, items, last;  // a key's first item; items by (key, item); bit i: items[i] ends its key's run
  uint64_t n_keys = 0;
};
void key_runs_build(const std::vector<std::pair<uint64_t, uint32_t>> &pairs, HostKeyRuns *r) {
  const uint32_t n = (uint32_t)pairs.size();
  for (uint32_t i = 0; i < n; ++i) r->n_keys += i == 0 || pairs[i].first != pairs[i - 1].first;
  r->keys.assign(set_capacity(r->n_keys), EMPTY);
  r->start.assign(r->keys.size(), 0);
  r->items.resize(n);
  r->last.assign((n + 31) / 32, 0);
  for (uint32_t i = 0; i < n; ++i) {
    const uint64_t key = pairs[i].first;
    r->items[i] = pairs[i].second;
    if (i + 1 == n || pairs[i + 1].first != key) r->last[i >> 5] |= 1u << (i & 31);
    if (i == 0 || pairs[i - 1].first != key) r->start[set_insert(r->keys, key)] = i;
  }
}
// Its place in a call's Scratch (before ensure()), and the copies there (after it) → the device's KeyRuns.
struct KeyRunsAt { size_t keys, start, items, last; };
KeyRunsAt key_runs_take(Scratch &m, const HostKeyRuns &r) {
  return KeyRunsAt{m.take<uint64_t>(r.keys.size()), m.take<uint32_t>(r.start.size()), m.take<uint32_t>(r.items.size()), m.take<uint32_t>(r.last.size())};
}
int key_runs_upload(shk_ctx *c, const Scratch &m, const KeyRunsAt &at, const HostKeyRuns &r, KeyRuns *d) {
  *d = KeyRuns{m.at<uint64_t>(at.keys), m.at<uint32_t>(at.start), m.at<uint32_t>(at.items), m.at<uint32_t>(at.last), (uint32_t)r.keys.size() - 1,
               (uint32_t)r.items.size()};
  HIPC(c, hipMemcpyAsync((void *)d->keys, r.keys.data(), r.keys.size() * 8, hipMemcpyHostToDevice, c->stream));
  HIPC(c, hipMemcpyAsync((void *)d->start, r.start.data(), r.start.size() * 4, hipMemcpyHostToDevice, c->stream));
  HIPC(c, hipMemcpyAsync((void *)d->items, r.items.data(), r.items.size() * 4, hipMemcpyHostToDevice, c->stream));
  HIPC(c, hipMemcpyAsync((void *)d->last, r.last.data(), r.last.size() * 4, hipMemcpyHostToDevice, c->stream));
  return SHK_OK;
}

// A batch of reads in front of a kernel: resident, the context settled, its stream idle but for the batch's own copies.
// Either ASCII plus offsets, or (planes.p0 set) every read of the retained store (batch_from_retained, shk_retain_api.hip.h).
struct ReadBatch {
  const uint8_t *d_bases; const uint64_t *d_offsets;
  uint64_t n_seqs, n_bases, max_len;  // (max_len: 0 where the caller never looked)
  PlaneReads planes;
};

// offsets as a batch of reads over n_bases bytes (a read's length is a 31-bit number in the wave-per-read kernels)
int batch_check_offsets(shk_ctx *c, const uint64_t *offsets, uint64_t n_seqs, uint64_t n_bases, const char *who, uint64_t *max_len) {
  *max_len = 0;
  for (uint64_t i = 0; i < n_seqs; ++i) {
    if (offsets[i + 1] < offsets[i]) return fail(c, SHK_ERR_BAD_ARG, "offsets must be non-decreasing");
    *max_len = std::max(*max_len, offsets[i + 1] - offsets[i]);
  }
  if (offsets[n_seqs] > n_bases)
    return fail(c, SHK_ERR_BAD_ARG, "offsets end at %llu, beyond the %llu bases", (unsigned long long)offsets[n_seqs], (unsigned long long)n_bases);
  if (*max_len >= (1ull << 31)) return fail(c, SHK_ERR_BAD_ARG, "a read of %llu bases: %s takes reads below 2^31", (unsigned long long)*max_len, who);
  return SHK_OK;
}

// Host buffers (n_seqs > 0, whatever the caller checks of them already checked) staged into the context's input buffers.
int batch_from_host(shk_ctx *c, const uint8_t *bases, const uint64_t *offsets, uint64_t n_seqs, uint64_t max_len, ReadBatch *b) {
  const uint64_t n_bases = offsets[n_seqs];
  HIPC(c, hipSetDevice(c->cfg.device));
  SHK_TRY(settle(c));  // (not table_read_begin: the table is not read; the staging buffers may still feed a counting launch)
  HIPC(c, hipStreamSynchronize(c->stream));
  HIPC(c, c->in_bases.ensure(n_bases + 16));
  HIPC(c, c->in_offsets.ensure((n_seqs + 2) * 8));
  if (n_bases) HIPC(c, hipMemcpyAsync(c->in_bases.p, bases, n_bases, hipMemcpyHostToDevice, c->stream));
  HIPC(c, hipMemcpyAsync(c->in_offsets.p, offsets, (n_seqs + 1) * 8, hipMemcpyHostToDevice, c->stream));
  *b = ReadBatch{(const uint8_t *)c->in_bases.p, (const uint64_t *)c->in_offsets.p, n_seqs, n_bases, max_len};
  return SHK_OK;
}

// A batch that lies on the context's device (n_seqs > 0): its offsets copied back and checked against n_bases.
int batch_from_device(shk_ctx *c, const void *d_bases, const void *d_offsets, uint64_t n_seqs, uint64_t n_bases, const char *who, ReadBatch *b) {
  HIPC(c, hipSetDevice(c->cfg.device));
  SHK_TRY(settle(c));  // (not table_read_begin: the table is not read)
  std::vector<uint64_t> h_off(n_seqs + 1);
  HIPC(c, hipMemcpyAsync(h_off.data(), d_offsets, (n_seqs + 1) * 8, hipMemcpyDeviceToHost, c->stream));
  HIPC(c, hipStreamSynchronize(c->stream));
  *b = ReadBatch{(const uint8_t *)d_bases, (const uint64_t *)d_offsets, n_seqs, n_bases, 0};
  return batch_check_offsets(c, h_off.data(), n_seqs, n_bases, who, &b->max_len);
}

// The call's SHK_K_LOOKUP launch with the set in LDS (k_lds; > 64 KiB of dynamic LDS has to be asked for once: *asked) or not.
template <class K, class... A>
int launch_lds_or_global(shk_ctx *c, K k_lds, K k_global, bool use_lds, bool *asked, size_t lds_max, uint64_t blocks, int wg, size_t lds_bytes,
                         A... args) {
  ScopedTimer t(c, SHK_K_LOOKUP);
  if (use_lds && !*asked) {
    HIPC(c, hipFuncSetAttribute(reinterpret_cast<const void *>(k_lds), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_max));
    *asked = true;
  }
  const K kernel = use_lds ? k_lds : k_global;
  hipLaunchKernelGGL(kernel, dim3((uint32_t)blocks), dim3(wg), lds_bytes, c->stream, args...);
  return SHK_OK;
}

}  // namespace

extern "C" {

int shk_filter_reads(shk_ctx *c, const uint8_t *bases, const uint64_t *offsets, uint64_t n_seqs,
                     const uint64_t *primer_kmers, uint64_t n_kmers, uint8_t *out_matches) {
  SHK_TRY(xs_closed(c));
  if (c && c->group)
    return on_any_device(c, [&](shk_ctx *d) { return shk_filter_reads(d, bases, offsets, n_seqs, primer_kmers, n_kmers, out_matches); });
  if (!c || (n_seqs && (!offsets || !out_matches))) return SHK_ERR_BAD_ARG;
  if (n_seqs == 0) return SHK_OK;
  HIPC(c, hipSetDevice(c->cfg.device));
  const uint32_t k = c->cfg.k;
  // the union of the primer k-mers (read_filter.rs:24-41) as an open-addressing set at load ≤ 1/2
  const uint64_t cap = set_capacity(n_kmers);
  if (cap > (1ull << 31)) return fail(c, SHK_ERR_BAD_ARG, "primer k-mer set too large");
  std::vector<uint64_t> set(cap, EMPTY);
  for (uint64_t j = 0; j < n_kmers; ++j) {
    const uint64_t key = primer_kmers[j];
    if (2 * k < 64 && (key >> (2 * k)) != 0)
      return fail(c, SHK_ERR_BAD_ARG, "primer k-mer %llu does not fit %u bases", (unsigned long long)key, k);
    set_insert(set, key);
  }
  Scratch m{c->misc};
  const size_t o_set = m.take<uint64_t>(cap), o_out = m.take<uint8_t>(n_seqs);
  HIPC(c, m.ensure());
  uint64_t *dset = m.at<uint64_t>(o_set);
  uint8_t *dout = m.at<uint8_t>(o_out);
  ReadBatch b;
  SHK_TRY(batch_from_host(c, bases, offsets, n_seqs, 0, &b));  // (offsets[n_seqs] is taken as it is)
  HIPC(c, hipMemcpyAsync(dset, set.data(), cap * 8, hipMemcpyHostToDevice, c->stream));
  {
    ScopedTimer t(c, SHK_K_LOOKUP);
    hipLaunchKernelGGL(k_filter_reads, dim3((uint32_t)((n_seqs + WG - 1) / WG)), dim3(WG), 0, c->stream, b.d_bases, b.d_offsets, n_seqs, (int)k,
                       (const uint64_t *)dset, (uint32_t)(cap - 1), dout);
  }
  HIPC(c, hipMemcpyAsync(out_matches, dout, n_seqs, hipMemcpyDeviceToHost, c->stream));
  HIPC(c, hipStreamSynchronize(c->stream));  // (also keeps `set` alive until its copy ran)
  return SHK_OK;
}

int shk_kmers_from_reads(shk_ctx *c, const uint8_t *bases, const uint64_t *offsets, uint64_t n_seqs,
                         uint64_t *kmers, uint64_t kmers_cap, uint32_t *n_kmers, uint8_t *bad_byte) {
  SHK_TRY(xs_closed(c));
  if (c && c->group)
    return on_any_device(c, [&](shk_ctx *d) { return shk_kmers_from_reads(d, bases, offsets, n_seqs, kmers, kmers_cap, n_kmers, bad_byte); });
  if (!c || (n_seqs && (!offsets || !n_kmers || !bad_byte))) return SHK_ERR_BAD_ARG;
  if (n_seqs == 0) return SHK_OK;
  HIPC(c, hipSetDevice(c->cfg.device));
  const uint32_t k = c->cfg.k;
  // koff(i): every read gets room for the most k-mers it can yield
  std::vector<uint64_t> koff(n_seqs + 1);
  koff[0] = 0;
  for (uint64_t i = 0; i < n_seqs; ++i) {
    if (offsets[i + 1] < offsets[i]) return fail(c, SHK_ERR_BAD_ARG, "offsets must be non-decreasing");
    const uint64_t len = offsets[i + 1] - offsets[i];
    koff[i + 1] = koff[i] + (len >= k ? len - k + 1 : 0);
  }
  const uint64_t n_total = koff[n_seqs];
  if (n_total > kmers_cap || (n_total && !kmers))
    return fail(c, SHK_ERR_BAD_ARG, "kmers_cap %llu is below the %llu k-mers these reads can yield",
                (unsigned long long)kmers_cap, (unsigned long long)n_total);
  Scratch m{c->misc};
  const size_t o_koff = m.take<uint64_t>(n_seqs + 1), o_kmers = m.take<uint64_t>(n_total + 1), o_n = m.take<uint32_t>(n_seqs),
               o_bad = m.take<uint8_t>(n_seqs);
  HIPC(c, m.ensure());
  uint64_t *dkoff = m.at<uint64_t>(o_koff), *dkm = m.at<uint64_t>(o_kmers);
  uint32_t *dnk = m.at<uint32_t>(o_n);
  uint8_t *dbad = m.at<uint8_t>(o_bad);
  ReadBatch b;
  SHK_TRY(batch_from_host(c, bases, offsets, n_seqs, 0, &b));  // (offsets[n_seqs] is taken as it is)
  HIPC(c, hipMemcpyAsync(dkoff, koff.data(), (n_seqs + 1) * 8, hipMemcpyHostToDevice, c->stream));
  {
    ScopedTimer t(c, SHK_K_LOOKUP);
    hipLaunchKernelGGL(k_kmers_from_reads, dim3((uint32_t)((n_seqs + WG - 1) / WG)), dim3(WG), 0, c->stream, b.d_bases, b.d_offsets,
                       (const uint64_t *)dkoff, n_seqs, (int)k, dkm, dnk, dbad);
  }
  // a read's span is copied back whole; only its first n_kmers[i] entries mean anything
  if (n_total) HIPC(c, hipMemcpyAsync(kmers, dkm, n_total * 8, hipMemcpyDeviceToHost, c->stream));
  HIPC(c, hipMemcpyAsync(n_kmers, dnk, n_seqs * 4, hipMemcpyDeviceToHost, c->stream));
  HIPC(c, hipMemcpyAsync(bad_byte, dbad, n_seqs, hipMemcpyDeviceToHost, c->stream));
  HIPC(c, hipStreamSynchronize(c->stream));  // (also keeps `koff` alive until its copy ran)
  return SHK_OK;
}

namespace {

// A graph as k_thread_panel wants it: the lookup set of build_edge_lookup (threading.rs:203-220), the
// per-edge facts find_contiguous_runs / record_branch_links ask the graph for, and a dense slot for every branch link.
struct ThreadPlan {
  HostKeyRuns runs;                 // canonical edge k-mer → its candidates, edges ascending
  std::vector<uint4> meta;          // {src, tgt, link base or TH_NONE, out rank}
  std::vector<uint64_t> out_first;  // CSR of the out-edges by source node, ascending edge index (link decoding)
  std::vector<uint32_t> out_list;
  uint64_t n_slots = 0;             // Σ over branch nodes of in_deg · out_deg
};

// Everything shk_thread_reads refuses before the device is touched, and the plan of a non-empty graph.
int thread_plan(shk_ctx *c, const uint64_t *node_sub_kmers, uint64_t n_nodes, const uint32_t *edge_src, const uint32_t *edge_tgt,
                uint64_t n_edges, uint64_t n_seqs, const uint64_t *read_index, const uint8_t *mate, const shk_thread_out *out,
                ThreadPlan *pl) {
  const uint32_t k = c->cfg.k;
  if (k < 2) return fail(c, SHK_ERR_BAD_ARG, "shk_thread_reads needs k >= 2 (a node is a (k-1)-mer), got k=%u", k);
  if (n_nodes >= (1ull << 32) || n_edges >= (1ull << 32))
    return fail(c, SHK_ERR_BAD_ARG, "graph of %llu nodes and %llu edges: both must be below 2^32", (unsigned long long)n_nodes,
                (unsigned long long)n_edges);
  if ((n_nodes && !node_sub_kmers) || (n_edges && (!edge_src || !edge_tgt || !out->support_total || !out->support_unambiguous)))
    return fail(c, SHK_ERR_BAD_ARG, "shk_thread_reads: a graph array or a support array is missing");
  if ((read_index == nullptr) != (mate == nullptr))
    return fail(c, SHK_ERR_BAD_ARG, "read_index and mate go together: both (thread_reads_paired) or neither (thread_reads)");
  for (uint64_t i = 0; mate && i < n_seqs; ++i)
    if (mate[i] > 2) return fail(c, SHK_ERR_BAD_ARG, "mate[%llu] = %u: 0 unpaired, 1 R1, 2 R2", (unsigned long long)i, mate[i]);
  const uint64_t nmask = ~0ull >> (64 - 2 * (k - 1));
  for (uint64_t v = 0; v < n_nodes; ++v)
    if (node_sub_kmers[v] > nmask) return fail(c, SHK_ERR_BAD_ARG, "node %llu: sub_kmer is not a %u-mer", (unsigned long long)v, k - 1);
  for (uint64_t e = 0; e < n_edges; ++e)
    if (edge_src[e] >= n_nodes || edge_tgt[e] >= n_nodes)
      return fail(c, SHK_ERR_BAD_ARG, "edge %llu: endpoint (%u, %u) outside the %llu nodes", (unsigned long long)e, edge_src[e], edge_tgt[e],
                  (unsigned long long)n_nodes);
  if (!n_edges) return SHK_OK;
  if (n_edges > (1ull << 30)) return fail(c, SHK_ERR_NOMEM, "graph of %llu edges: the lookup set would not fit", (unsigned long long)n_edges);
  const uint32_t E = (uint32_t)n_edges;
  auto revcomp = [k](uint64_t x) {
    uint64_t r = 0;
    for (uint32_t i = 0; i < k; ++i, x >>= 2) r = (r << 2) | (3 - (x & 3));
    return r;
  };
  // edge k-mer (reconstruct_edge_kmer, graph.rs:127-134) → canonical key; candidates ascending by (key, edge)
  std::vector<std::pair<uint64_t, uint32_t>> pairs(E);
  for (uint32_t e = 0; e < E; ++e) {
    const uint64_t x = (node_sub_kmers[edge_src[e]] << 2) | (node_sub_kmers[edge_tgt[e]] & 3);
    pairs[e] = {std::min(x, revcomp(x)), e};
  }
  std::sort(pairs.begin(), pairs.end());
  key_runs_build(pairs, &pl->runs);
  // degrees as edge counts (neighbors_directed(..).count(), threading.rs:329-330), ranks among a node's in- and out-edges
  std::vector<uint32_t> in_deg(n_nodes, 0), out_deg(n_nodes, 0), in_rank(E), out_rank(E);
  for (uint32_t e = 0; e < E; ++e) in_rank[e] = in_deg[edge_tgt[e]]++, out_rank[e] = out_deg[edge_src[e]]++;
  pl->out_first.assign(n_nodes + 1, 0);
  for (uint64_t v = 0; v < n_nodes; ++v) pl->out_first[v + 1] = pl->out_first[v] + out_deg[v];
  pl->out_list.resize(E);
  for (uint32_t e = 0; e < E; ++e) pl->out_list[pl->out_first[edge_src[e]] + out_rank[e]] = e;
  // a branch node v (either degree above 1) owns in_deg · out_deg link slots: (a, b) ↦ base[v] + in_rank(a) · out_deg + out_rank(b)
  std::vector<uint64_t> base(n_nodes, 0);
  uint64_t n_slots = 0;
  for (uint64_t v = 0; v < n_nodes; ++v) {
    if (in_deg[v] <= 1 && out_deg[v] <= 1) continue;
    base[v] = n_slots;
    n_slots += (uint64_t)in_deg[v] * out_deg[v];
    if (n_slots > (1ull << 31))
      return fail(c, SHK_ERR_BAD_ARG, "the branch nodes of this graph have more than 2^31 (incoming, outgoing) edge pairs");
  }
  pl->n_slots = n_slots;
  pl->meta.resize(E);
  for (uint32_t e = 0; e < E; ++e) {
    const uint32_t v = edge_tgt[e];
    const bool branch = in_deg[v] > 1 || out_deg[v] > 1;
    pl->meta[e] = make_uint4(edge_src[e], v, branch ? (uint32_t)(base[v] + (uint64_t)in_rank[e] * out_deg[v]) : TH_NONE, out_rank[e]);
  }
  return SHK_OK;
}

void thread_out_zero(shk_thread_out *out, uint64_t n_edges, uint64_t n_seqs) {
  if (n_edges) std::fill(out->support_total, out->support_total + n_edges, 0u);
  if (n_edges) std::fill(out->support_unambiguous, out->support_unambiguous + n_edges, 0u);
  if (out->read_edges) std::fill(out->read_edges, out->read_edges + n_seqs, 0u);
  out->n_links = out->n_paired_links = 0;
}

// What follows a launch, per gene.
// paired_links.len() (threading.rs:166-189): pairs of which an R1 and an R2 read each mapped to some edge.  Position i
// of the n walked is read reads[i] of the batch (reads == NULL: read i) and mapped to re[i] edges.
// mate == NULL: the rule of interleaved pairs (reread_sequences, io.rs:831-898) — read r is R1 when r is even, R2 when
// odd, its index r — so that nothing the size of the batch has to exist (shk_pcr_run over retained reads).
uint64_t thread_paired_links(const uint64_t *reads, uint64_t n, const uint64_t *read_index, const uint8_t *mate, const uint32_t *re) {
  std::unordered_map<uint64_t, uint8_t> seen;
  uint64_t n_pairs = 0;
  for (uint64_t i = 0; i < n; ++i) {
    const uint64_t r = reads ? reads[i] : i;
    const uint8_t m = mate ? mate[r] : (uint8_t)(1 + (r & 1));
    if (m && re[i]) {
      uint8_t &s = seen[(mate ? read_index[r] : r) / 2];
      if (s != 3 && (s |= m) == 3) ++n_pairs;
    }
  }
  return n_pairs;
}
// the links that were seen: the slots that are not 0 …
uint64_t thread_links_count(const uint32_t *slots, uint64_t n_slots) {
  uint64_t n_links = 0;
  for (uint64_t i = 0; i < n_slots; ++i) n_links += slots[i] != 0;
  return n_links;
}
// … ascending by (in, out): edge a's slots are its target's out-edges in ascending order
void thread_links_decode(const ThreadPlan &pl, const uint32_t *slots, uint64_t n_links, uint32_t *link_in, uint32_t *link_out,
                         uint32_t *link_counts) {
  const uint32_t E = (uint32_t)pl.meta.size();
  uint64_t at = 0;
  for (uint32_t a = 0; a < E && at < n_links; ++a) {
    if (pl.meta[a].z == TH_NONE) continue;
    const uint64_t o0 = pl.out_first[pl.meta[a].y], o1 = pl.out_first[pl.meta[a].y + 1];
    for (uint64_t j = o0; j < o1; ++j)
      if (const uint32_t n = slots[pl.meta[a].z + (j - o0)]) {
        link_in[at] = a, link_out[at] = pl.out_list[j], link_counts[at] = n;
        ++at;
      }
  }
}

// A panel of graphs as k_thread_panel wants it: one ThreadPlan per gene, by thread_plan.
struct ThreadPanelPlan {
  std::vector<ThreadPlan> genes;
  uint64_t e0 = 0, n_edges = 0, l0 = 0, n_listed = 0, n_slots = 0;  // the panel's first edge and list position; its totals
};

// Everything shk_thread_reads_panel refuses before the device is touched (the read offsets apart), and the genes' plans.
int thread_panel_plan(shk_ctx *c, const uint64_t *node_sub_kmers, const uint64_t *node_offsets, const uint32_t *edge_src, const uint32_t *edge_tgt,
                      const uint64_t *edge_offsets, uint32_t n_genes, uint64_t n_seqs, const uint64_t *list_offsets, const uint64_t *list_reads,
                      const uint64_t *read_index, const uint8_t *mate, const shk_thread_panel_out *out, ThreadPanelPlan *pp) {
  if (n_genes > SHK_THREAD_MAX_GENES) return fail(c, SHK_ERR_BAD_ARG, "n_genes %u is above the limit of %u", n_genes, SHK_THREAD_MAX_GENES);
  if ((read_index == nullptr) != (mate == nullptr))
    return fail(c, SHK_ERR_BAD_ARG, "read_index and mate go together: both (thread_reads_paired) or neither (thread_reads)");
  for (uint64_t i = 0; mate && i < n_seqs; ++i)
    if (mate[i] > 2) return fail(c, SHK_ERR_BAD_ARG, "mate[%llu] = %u: 0 unpaired, 1 R1, 2 R2", (unsigned long long)i, mate[i]);
  if (!n_genes) return SHK_OK;
  if (!node_offsets || !edge_offsets || !list_offsets) return fail(c, SHK_ERR_BAD_ARG, "shk_thread_reads_panel: an offsets array is missing");
  for (uint32_t g = 0; g < n_genes; ++g) {
    if (node_offsets[g + 1] < node_offsets[g]) return fail(c, SHK_ERR_BAD_ARG, "gene %u: node_offsets must be non-decreasing", g);
    if (edge_offsets[g + 1] < edge_offsets[g]) return fail(c, SHK_ERR_BAD_ARG, "gene %u: edge_offsets must be non-decreasing", g);
    if (list_offsets[g + 1] < list_offsets[g]) return fail(c, SHK_ERR_BAD_ARG, "gene %u: list_offsets must be non-decreasing", g);
  }
  pp->e0 = edge_offsets[0], pp->n_edges = edge_offsets[n_genes] - pp->e0;
  pp->l0 = list_offsets[0], pp->n_listed = list_offsets[n_genes] - pp->l0;
  if (pp->n_edges >= (1ull << 32))
    return fail(c, SHK_ERR_BAD_ARG, "a panel of %llu edges (gene 0 to gene %u): the total must be below 2^32", (unsigned long long)pp->n_edges,
                n_genes - 1);
  if (pp->n_listed && !list_reads) return fail(c, SHK_ERR_BAD_ARG, "shk_thread_reads_panel: list_reads is missing");
  for (uint32_t g = 0; g < n_genes; ++g)
    for (uint64_t p = list_offsets[g]; p < list_offsets[g + 1]; ++p)
      if (list_reads[p] >= n_seqs)
        return fail(c, SHK_ERR_BAD_ARG, "gene %u: list_reads[%llu] = %llu is outside the %llu reads", g, (unsigned long long)p,
                    (unsigned long long)list_reads[p], (unsigned long long)n_seqs);
  // the graphs, each by shk_thread_reads' own rules (read_index / mate are checked above, once: no reads go in)
  const shk_thread_out one{out->support_total, out->support_unambiguous, nullptr, nullptr, nullptr, 0, 0, nullptr, 0};
  pp->genes.resize(n_genes);
  for (uint32_t g = 0; g < n_genes; ++g) {
    const uint64_t v0 = node_offsets[g], e0 = edge_offsets[g];
    const int rc = thread_plan(c, node_sub_kmers ? node_sub_kmers + v0 : nullptr, node_offsets[g + 1] - v0, edge_src ? edge_src + e0 : nullptr,
                               edge_tgt ? edge_tgt + e0 : nullptr, edge_offsets[g + 1] - e0, 0, read_index, mate, &one, &pp->genes[g]);
    if (rc != SHK_OK) {
      const std::string why = c->err;
      return fail(c, rc, "gene %u: %s", g, why.c_str());
    }
    pp->n_slots += pp->genes[g].n_slots;
    if (pp->n_slots > (1ull << 31))
      return fail(c, SHK_ERR_BAD_ARG, "gene %u: the panel's branch nodes have more than 2^31 (incoming, outgoing) edge pairs up to this gene", g);
  }
  return SHK_OK;
}

void thread_panel_out_zero(shk_thread_panel_out *out, const ThreadPanelPlan &pp, uint32_t n_genes) {
  if (pp.n_edges) std::fill(out->support_total + pp.e0, out->support_total + pp.e0 + pp.n_edges, 0u);
  if (pp.n_edges) std::fill(out->support_unambiguous + pp.e0, out->support_unambiguous + pp.e0 + pp.n_edges, 0u);
  if (out->read_edges && pp.n_listed) std::fill(out->read_edges + pp.l0, out->read_edges + pp.l0 + pp.n_listed, 0u);
  if (out->link_offsets) std::fill(out->link_offsets, out->link_offsets + n_genes + 1, 0ull);
  if (out->n_paired_links) std::fill(out->n_paired_links, out->n_paired_links + n_genes, 0ull);
  out->n_links = 0;
}

// What thread_panel_core leaves, for shk_thread_reads_panel's shk_thread_panel_out and shk_thread_reads' shk_thread_out
// alike.  The large arrays are written where the caller wants them: the supports of the panel's edges (gene after gene)
// and, where asked for, read_edges by list position.
struct ThreadPanelResult {
  uint32_t *support_total, *support_unambiguous, *read_edges;  // in: the destinations (read_edges: or nullptr)
  std::vector<uint32_t> link_in, link_out, link_counts;        // the links seen, gene after gene: gene g's from link_off[g]
  std::vector<uint64_t> link_off, n_paired;                    // n_genes + 1; n_genes (zero without mates)
};

// The links of a result into a caller's arrays of link_cap entries.
int thread_links_out(shk_ctx *c, const ThreadPanelResult &res, uint64_t link_cap, uint32_t *link_in, uint32_t *link_out, uint32_t *link_counts) {
  const uint64_t n_links = res.link_off.back();
  if (n_links > link_cap || (n_links && (!link_in || !link_out || !link_counts)))
    return fail(c, SHK_ERR_BAD_ARG, "%llu branch links do not fit link_cap %llu", (unsigned long long)n_links, (unsigned long long)link_cap);
  std::copy(res.link_in.begin(), res.link_in.end(), link_in);
  std::copy(res.link_out.begin(), res.link_out.end(), link_out);
  std::copy(res.link_counts.begin(), res.link_counts.end(), link_counts);
  return SHK_OK;
}

struct ThreadListSpan { uint64_t l0, n_listed; };  // list_reads[l0 … l0 + n_listed) are the panel's lists

// The launch over an opened batch (its offsets checked) and what follows it.  list_reads == nullptr: list position i (from
// pp.l0) is read i — the one gene of shk_thread_reads, which lists every read.
int thread_panel_core(shk_ctx *c, const ThreadPanelPlan &pp, uint32_t n_genes, const ReadBatch &b, const uint64_t *list_offsets,
                      const uint64_t *list_reads, const uint64_t *read_index, const uint8_t *mate, ThreadPanelResult *res,
                      bool mate_rule = false /* no arrays: pairs by thread_paired_links' rule (needs list_reads) */,
                      const ThreadListSpan *span = nullptr /* the lists' extent where it is not the plan's (a share's lists) */) {
  const uint32_t k = c->cfg.k;
  const uint64_t l0 = span ? span->l0 : pp.l0, n_listed = span ? span->n_listed : pp.n_listed;
  res->link_off.assign(n_genes + 1, 0);
  res->n_paired.assign(n_genes, 0);
  const int lds_edges = env_int("SHK_THREAD_LDS_EDGES", THREAD_LDS_EDGES);
  const uint64_t job_reads = (uint64_t)std::max(env_int("SHK_THREAD_PANEL_JOB", THREAD_PANEL_JOB), 1);
  const int block_cap = env_int("SHK_THREAD_PANEL_BLOCKS", 0);
  // the upload: every gene's meta, keys, start, items, last (16-byte aligned each), then the descriptors
  std::vector<uint8_t> up;
  std::vector<ThreadGene> desc(n_genes);
  std::vector<ThreadJob> jobs;
  auto put = [&up](const void *p, size_t bytes) {
    const size_t at = up.size();
    up.resize(at + ((bytes + 15) & ~(size_t)15), 0);
    if (bytes) memcpy(up.data() + at, p, bytes);
    return (uint64_t)at;
  };
  size_t lds = 0;
  uint32_t n_lds = 0, n_global = 0;
  uint64_t e_at = 0, slot_at = 0, n_walked = 0;
  for (uint32_t g = 0; g < n_genes; ++g) {
    const ThreadPlan &pl = pp.genes[g];
    const uint32_t E = (uint32_t)pl.runs.items.size();
    const uint64_t n_list = list_offsets[g + 1] - list_offsets[g];
    ThreadGene &d = desc[g];
    d = ThreadGene{};
    d.cnt_base = (uint32_t)e_at, d.link_base = (uint32_t)slot_at;
    e_at += E, slot_at += pl.n_slots;
    if (!E) continue;  // no set, no jobs: its reads map to nothing
    const uint32_t cap = (uint32_t)pl.runs.keys.size();
    const size_t gene_lds = thread_lds_bytes(cap, E);
    d.lds = (int64_t)E <= (int64_t)lds_edges && gene_lds <= THREAD_LDS_MAX;
    if (d.lds) lds = std::max(lds, gene_lds);
    ++(d.lds ? n_lds : n_global);
    d.meta = put(pl.meta.data(), (size_t)E * 16);
    d.keys = put(pl.runs.keys.data(), (size_t)cap * 8), d.start = put(pl.runs.start.data(), (size_t)cap * 4);
    d.items = put(pl.runs.items.data(), (size_t)E * 4), d.last = put(pl.runs.last.data(), pl.runs.last.size() * 4);
    d.mask = cap - 1, d.n_edges = E;
    for (uint64_t at = 0; at < n_list; at += job_reads)  // (gene, slice) order
      jobs.push_back(ThreadJob{list_offsets[g] - l0 + at, g, (uint32_t)std::min(job_reads, n_list - at)});
    n_walked += n_list;
  }
  if (jobs.empty()) return SHK_OK;  // (the outputs are zero already)
  if (jobs.size() >= (1ull << 32)) return fail(c, SHK_ERR_BAD_ARG, "%zu jobs: raise SHK_THREAD_PANEL_JOB", jobs.size());
  const size_t o_desc_up = put(desc.data(), desc.size() * sizeof(ThreadGene));
  // blocks: a wave per read up to the device's workgroups (one per CU when a set fills its LDS), the
  // waves bounded by 256 MiB of scratch, whose stride the longest read of the BATCH sets — and never more than the jobs
  const uint64_t max_win = b.max_len >= k ? b.max_len - k + 1 : 0;
  const uint64_t stride = std::max<uint64_t>(THREAD_TILE, (max_win + THREAD_TILE - 1) / THREAD_TILE * THREAD_TILE);
  const uint64_t wpb = THREAD_WG / 64;
  uint64_t blocks = std::min<uint64_t>((n_walked + wpb - 1) / wpb, (uint64_t)c->n_cus * (n_lds ? 1 : 2));
  blocks = std::min<uint64_t>(blocks, ((256ull << 20) / 8) / (stride * wpb));
  if (block_cap > 0) blocks = std::min<uint64_t>(blocks, (uint64_t)block_cap);
  blocks = std::max<uint64_t>(1, std::min<uint64_t>(blocks, jobs.size()));
  Scratch m{c->misc};
  const size_t o_up = m.take<uint8_t>(up.size()), o_jobs = m.take<ThreadJob>(jobs.size()), o_list = m.take<uint64_t>(list_reads ? n_listed : 0);
  const size_t n_cnt = 2 * (size_t)pp.n_edges + pp.n_slots + n_listed;  // ONE block, cleared as one: [total][unambiguous][link slots][read_edges]
  const size_t o_cnt = m.take<uint32_t>(n_cnt), o_scr = m.take<uint2>(blocks * wpb * stride);
  HIPC(c, m.ensure());
  uint32_t *dtot = m.at<uint32_t>(o_cnt), *dun = dtot + pp.n_edges, *dlinks = dun + pp.n_edges, *dre = dlinks + pp.n_slots;
  HIPC(c, hipMemcpyAsync(m.at<uint8_t>(o_up), up.data(), up.size(), hipMemcpyHostToDevice, c->stream));
  HIPC(c, hipMemcpyAsync(m.at<ThreadJob>(o_jobs), jobs.data(), jobs.size() * sizeof(ThreadJob), hipMemcpyHostToDevice, c->stream));
  const uint64_t *dlist = list_reads ? m.at<uint64_t>(o_list) : nullptr;
  if (list_reads) HIPC(c, hipMemcpyAsync(m.at<uint64_t>(o_list), list_reads + l0, n_listed * 8, hipMemcpyHostToDevice, c->stream));
  HIPC(c, hipMemsetAsync(dtot, 0, n_cnt * 4, c->stream));
  if (getenv("SHK_TRACE"))  // (read at each call, like the knobs: the tests look for this line)
    fprintf(stderr, "[shk] thread_reads_panel: %u genes, %zu jobs, %llu blocks, %u genes in LDS, %u genes in global memory%s\n", n_genes, jobs.size(),
            (unsigned long long)blocks, n_lds, n_global, b.planes.p0 ? ", retained reads" : "");
  {
    ScopedTimer t(c, SHK_K_LOOKUP);
    if (lds > (64u << 10) && !c->lds_attr_thread_panel) {  // > 64 KiB of dynamic LDS has to be asked for once
      HIPC(c, hipFuncSetAttribute(reinterpret_cast<const void *>(&k_thread_panel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)THREAD_LDS_MAX));
      c->lds_attr_thread_panel = true;
    }
    if (lds > (64u << 10) && b.planes.p0 && !c->lds_attr_thread_retained) {
      HIPC(c, hipFuncSetAttribute(reinterpret_cast<const void *>(&k_thread_panel_retained), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)THREAD_LDS_MAX));
      c->lds_attr_thread_retained = true;
    }
    if (b.planes.p0)
      hipLaunchKernelGGL(k_thread_panel_retained, dim3((uint32_t)blocks), dim3(THREAD_WG), lds, c->stream, b.planes, dlist,
                         (const ThreadGene *)(m.at<uint8_t>(o_up) + o_desc_up), (const ThreadJob *)m.at<ThreadJob>(o_jobs), (uint32_t)jobs.size(),
                         (const uint8_t *)m.at<uint8_t>(o_up), (int)k, m.at<uint2>(o_scr), (uint32_t)stride, dtot, dun, dlinks, dre);
    else
      hipLaunchKernelGGL(k_thread_panel, dim3((uint32_t)blocks), dim3(THREAD_WG), lds, c->stream, b.d_bases, b.d_offsets,
                         dlist, (const ThreadGene *)(m.at<uint8_t>(o_up) + o_desc_up),
                         (const ThreadJob *)m.at<ThreadJob>(o_jobs), (uint32_t)jobs.size(), (const uint8_t *)m.at<uint8_t>(o_up), (int)k,
                         m.at<uint2>(o_scr), (uint32_t)stride, dtot, dun, dlinks, dre);
  }
  HIPC(c, hipGetLastError());
  std::vector<uint32_t> slots(pp.n_slots), re_own;
  uint32_t *re = res->read_edges;
  if (!re && (mate || mate_rule)) {
    re_own.resize(n_listed);
    re = re_own.data();
  }
  HIPC(c, hipMemcpyAsync(res->support_total, dtot, (size_t)pp.n_edges * 4, hipMemcpyDeviceToHost, c->stream));
  HIPC(c, hipMemcpyAsync(res->support_unambiguous, dun, (size_t)pp.n_edges * 4, hipMemcpyDeviceToHost, c->stream));
  if (pp.n_slots) HIPC(c, hipMemcpyAsync(slots.data(), dlinks, pp.n_slots * 4, hipMemcpyDeviceToHost, c->stream));
  if (re) HIPC(c, hipMemcpyAsync(re, dre, n_listed * 4, hipMemcpyDeviceToHost, c->stream));
  HIPC(c, hipStreamSynchronize(c->stream));  // (also keeps the upload and the jobs alive until their copies ran)
  for (uint32_t g = 0; g < n_genes; ++g) {
    const uint64_t l_at = list_offsets[g] - l0, n_list = list_offsets[g + 1] - list_offsets[g];
    if (mate_rule && !mate)
      res->n_paired[g] = thread_paired_links(list_reads + list_offsets[g], n_list, nullptr, nullptr, re + l_at);
    else if (mate)
      res->n_paired[g] = list_reads ? thread_paired_links(list_reads + list_offsets[g], n_list, read_index, mate, re + l_at)
                                    : thread_paired_links(nullptr, n_list, read_index + l_at, mate + l_at, re + l_at);
    res->link_off[g + 1] = res->link_off[g] + thread_links_count(slots.data() + desc[g].link_base, pp.genes[g].n_slots);
  }
  const uint64_t n_links = res->link_off[n_genes];
  res->link_in.resize(n_links), res->link_out.resize(n_links), res->link_counts.resize(n_links);
  for (uint32_t g = 0; g < n_genes; ++g)
    thread_links_decode(pp.genes[g], slots.data() + desc[g].link_base, res->link_off[g + 1] - res->link_off[g],
                        res->link_in.data() + res->link_off[g], res->link_out.data() + res->link_off[g], res->link_counts.data() + res->link_off[g]);
  return SHK_OK;
}

// shk_thread_reads[_device] after their checks and early returns: the panel of one gene that lists every read of the
// opened batch, in the batch's order (no list is uploaded).
int thread_one_gene(shk_ctx *c, ThreadPlan &&pl, uint64_t n_edges, const ReadBatch &b, const uint64_t *read_index, const uint8_t *mate,
                    shk_thread_out *out) {
  ThreadPanelPlan pp;
  pp.n_edges = n_edges, pp.n_listed = b.n_seqs, pp.n_slots = pl.n_slots;
  pp.genes.push_back(std::move(pl));
  const uint64_t list_offsets[2] = {0, b.n_seqs};
  ThreadPanelResult res{out->support_total, out->support_unambiguous, out->read_edges, {}, {}, {}, {}, {}};
  SHK_TRY(thread_panel_core(c, pp, 1, b, list_offsets, nullptr, read_index, mate, &res));
  out->n_paired_links = res.n_paired[0];
  out->n_links = res.link_off[1];
  return thread_links_out(c, res, out->link_cap, out->link_in, out->link_out, out->link_counts);
}

// A result into shk_thread_reads_panel's out (the large arrays are where the result put them).
int thread_panel_finish(shk_ctx *c, const ThreadPanelResult &res, uint32_t n_genes, shk_thread_panel_out *out) {
  if (out->n_paired_links) std::copy(res.n_paired.begin(), res.n_paired.end(), out->n_paired_links);
  if (out->link_offsets) std::copy(res.link_off.begin(), res.link_off.end(), out->link_offsets);
  out->n_links = res.link_off[n_genes];
  return thread_links_out(c, res, out->link_cap, out->link_in, out->link_out, out->link_counts);
}

// shk_thread_reads_panel[_device] after theirs.
int thread_panel_run(shk_ctx *c, const ThreadPanelPlan &pp, uint32_t n_genes, const ReadBatch &b, const uint64_t *list_offsets,
                     const uint64_t *list_reads, const uint64_t *read_index, const uint8_t *mate, shk_thread_panel_out *out) {
  ThreadPanelResult res{out->support_total + pp.e0, out->support_unambiguous + pp.e0, out->read_edges ? out->read_edges + pp.l0 : nullptr,
                        {}, {}, {}, {}, {}};
  SHK_TRY(thread_panel_core(c, pp, n_genes, b, list_offsets, list_reads, read_index, mate, &res));
  return thread_panel_finish(c, res, n_genes, out);
}

}  // namespace

int shk_thread_reads_device(shk_ctx *c, const uint64_t *node_sub_kmers, uint64_t n_nodes, const uint32_t *edge_src, const uint32_t *edge_tgt,
                            uint64_t n_edges, const void *d_bases, const void *d_offsets, uint64_t n_seqs, uint64_t n_bases,
                            const uint64_t *read_index, const uint8_t *mate, shk_thread_out *out) {
  SHK_TRY(xs_closed(c));
  if (c && c->group)
    return on_any_device(c, [&](shk_ctx *d) {
      return shk_thread_reads_device(d, node_sub_kmers, n_nodes, edge_src, edge_tgt, n_edges, d_bases, d_offsets, n_seqs, n_bases, read_index, mate, out);
    });
  if (!c || !out || (n_seqs && !d_offsets)) return SHK_ERR_BAD_ARG;
  ThreadPlan pl;
  SHK_TRY(thread_plan(c, node_sub_kmers, n_nodes, edge_src, edge_tgt, n_edges, n_seqs, read_index, mate, out, &pl));
  thread_out_zero(out, n_edges, n_seqs);
  if (n_seqs == 0) return SHK_OK;
  ReadBatch b;
  SHK_TRY(batch_from_device(c, d_bases, d_offsets, n_seqs, n_bases, "shk_thread_reads", &b));
  if (n_edges == 0) return SHK_OK;
  return thread_one_gene(c, std::move(pl), n_edges, b, read_index, mate, out);
}

int shk_thread_reads(shk_ctx *c, const uint64_t *node_sub_kmers, uint64_t n_nodes, const uint32_t *edge_src, const uint32_t *edge_tgt,
                     uint64_t n_edges, const uint8_t *bases, const uint64_t *offsets, uint64_t n_seqs, const uint64_t *read_index,
                     const uint8_t *mate, shk_thread_out *out) {
  SHK_TRY(xs_closed(c));
  if (c && c->group)
    return on_any_device(c, [&](shk_ctx *d) {
      return shk_thread_reads(d, node_sub_kmers, n_nodes, edge_src, edge_tgt, n_edges, bases, offsets, n_seqs, read_index, mate, out);
    });
  if (!c || !out || (n_seqs && !offsets)) return SHK_ERR_BAD_ARG;
  ThreadPlan pl;
  SHK_TRY(thread_plan(c, node_sub_kmers, n_nodes, edge_src, edge_tgt, n_edges, n_seqs, read_index, mate, out, &pl));
  thread_out_zero(out, n_edges, n_seqs);
  if (n_seqs == 0) return SHK_OK;
  uint64_t max_len = 0;
  SHK_TRY(batch_check_offsets(c, offsets, n_seqs, offsets[n_seqs], "shk_thread_reads", &max_len));
  if (n_edges == 0) return SHK_OK;
  if (offsets[n_seqs] && !bases) return SHK_ERR_BAD_ARG;
  // the device form's launch over the staged batch (its offsets are already here: no copy back)
  ReadBatch b;
  SHK_TRY(batch_from_host(c, bases, offsets, n_seqs, max_len, &b));
  return thread_one_gene(c, std::move(pl), n_edges, b, read_index, mate, out);
}

int shk_thread_reads_panel_device(shk_ctx *c, const uint64_t *node_sub_kmers, const uint64_t *node_offsets, const uint32_t *edge_src,
                                  const uint32_t *edge_tgt, const uint64_t *edge_offsets, uint32_t n_genes, const void *d_bases, const void *d_offsets,
                                  uint64_t n_seqs, uint64_t n_bases, const uint64_t *list_offsets, const uint64_t *list_reads,
                                  const uint64_t *read_index, const uint8_t *mate, shk_thread_panel_out *out) {
  SHK_TRY(xs_closed(c));
  if (c && c->group)
    return on_any_device(c, [&](shk_ctx *d) {
      return shk_thread_reads_panel_device(d, node_sub_kmers, node_offsets, edge_src, edge_tgt, edge_offsets, n_genes, d_bases, d_offsets, n_seqs,
                                           n_bases, list_offsets, list_reads, read_index, mate, out);
    });
  if (!c || !out || (n_seqs && !d_offsets)) return SHK_ERR_BAD_ARG;
  ThreadPanelPlan pp;
  SHK_TRY(thread_panel_plan(c, node_sub_kmers, node_offsets, edge_src, edge_tgt, edge_offsets, n_genes, n_seqs, list_offsets, list_reads, read_index,
                            mate, out, &pp));
  thread_panel_out_zero(out, pp, n_genes);
  if (n_seqs == 0 || n_genes == 0) return SHK_OK;
  ReadBatch b;
  SHK_TRY(batch_from_device(c, d_bases, d_offsets, n_seqs, n_bases, "shk_thread_reads_panel", &b));  // (the offsets come back once)
  return thread_panel_run(c, pp, n_genes, b, list_offsets, list_reads, read_index, mate, out);
}

int shk_thread_reads_panel(shk_ctx *c, const uint64_t *node_sub_kmers, const uint64_t *node_offsets, const uint32_t *edge_src,
                           const uint32_t *edge_tgt, const uint64_t *edge_offsets, uint32_t n_genes, const uint8_t *bases, const uint64_t *offsets,
                           uint64_t n_seqs, const uint64_t *list_offsets, const uint64_t *list_reads, const uint64_t *read_index,
                           const uint8_t *mate, shk_thread_panel_out *out) {
  SHK_TRY(xs_closed(c));
  if (c && c->group)
    return on_any_device(c, [&](shk_ctx *d) {
      return shk_thread_reads_panel(d, node_sub_kmers, node_offsets, edge_src, edge_tgt, edge_offsets, n_genes, bases, offsets, n_seqs, list_offsets,
                                    list_reads, read_index, mate, out);
    });
  if (!c || !out || (n_seqs && !offsets)) return SHK_ERR_BAD_ARG;
  ThreadPanelPlan pp;
  SHK_TRY(thread_panel_plan(c, node_sub_kmers, node_offsets, edge_src, edge_tgt, edge_offsets, n_genes, n_seqs, list_offsets, list_reads, read_index,
                            mate, out, &pp));
  thread_panel_out_zero(out, pp, n_genes);
  if (n_seqs == 0 || n_genes == 0) return SHK_OK;
  uint64_t max_len = 0;
  SHK_TRY(batch_check_offsets(c, offsets, n_seqs, offsets[n_seqs], "shk_thread_reads_panel", &max_len));
  if (pp.n_edges == 0 || pp.n_listed == 0) return SHK_OK;
  if (offsets[n_seqs] && !bases) return SHK_ERR_BAD_ARG;
  // the device form's launch over the staged batch (its offsets are already here: no copy back)
  ReadBatch b;
  SHK_TRY(batch_from_host(c, bases, offsets, n_seqs, max_len, &b));
  return thread_panel_run(c, pp, n_genes, b, list_offsets, list_reads, read_index, mate, out);
}

namespace {

// Everything the panel filter refuses before the device is touched, and a panel that has k-mers as k_filter_panel wants
// it: the distinct k-mers of all genes, each with the run of genes that hold it, every (k-mer, gene) once.
int panel_plan(shk_ctx *c, const uint64_t *primer_kmers, const uint64_t *gene_offsets, uint32_t n_genes, HostKeyRuns *pl) {
  const uint32_t k = c->cfg.k;
  if (n_genes > FILTER_MAX_GENES) return fail(c, SHK_ERR_BAD_ARG, "n_genes %u is above the limit of %u", n_genes, FILTER_MAX_GENES);
  if (!n_genes) return SHK_OK;
  if (!gene_offsets) return SHK_ERR_BAD_ARG;
  for (uint32_t g = 0; g < n_genes; ++g)
    if (gene_offsets[g + 1] < gene_offsets[g]) return fail(c, SHK_ERR_BAD_ARG, "gene_offsets must be non-decreasing");
  const uint64_t k0 = gene_offsets[0], k1 = gene_offsets[n_genes];
  if (k1 > k0 && !primer_kmers) return SHK_ERR_BAD_ARG;
  if (k1 - k0 > (1ull << 30)) return fail(c, SHK_ERR_NOMEM, "panel of %llu k-mers: the lookup set would not fit", (unsigned long long)(k1 - k0));
  std::vector<std::pair<uint64_t, uint32_t>> pairs;
  pairs.reserve(k1 - k0);
  for (uint32_t g = 0; g < n_genes; ++g)
    for (uint64_t j = gene_offsets[g]; j < gene_offsets[g + 1]; ++j) {
      const uint64_t key = primer_kmers[j];
      if ((key >> (2 * k)) != 0)  // (k ≤ 31)
        return fail(c, SHK_ERR_BAD_ARG, "primer k-mer %llu does not fit %u bases", (unsigned long long)key, k);
      pairs.emplace_back(key, g);
    }
  std::sort(pairs.begin(), pairs.end());
  pairs.erase(std::unique(pairs.begin(), pairs.end()), pairs.end());
  if (!pairs.empty()) key_runs_build(pairs, pl);
  return SHK_OK;
}

// One k_filter_panel pass with room for `room` records: *n_total = the records the batch has; recs = all of them when
// they fit (else empty).  The batch is opened, its offsets checked.
int panel_pass(shk_ctx *c, const HostKeyRuns &pl, uint32_t n_genes, const ReadBatch &b, uint64_t room, std::vector<uint64_t> *recs,
               uint64_t *n_total) {
  const uint32_t cap = (uint32_t)pl.keys.size(), P = (uint32_t)pl.items.size();
  const uint64_t n_seqs = b.n_seqs;
  const int lds_keys = env_int("SHK_FILTER_LDS_KEYS", FILTER_LDS_KEYS);
  const size_t bitmaps = filter_bitmap_bytes(n_genes), lds = bitmaps + filter_set_bytes(cap, P);
  const bool use_lds = (int64_t)pl.n_keys <= (int64_t)lds_keys && lds <= FILTER_LDS_MAX;
  const uint64_t wpb = FILTER_WG / 64;
  const uint64_t blocks = std::max<uint64_t>(1, std::min<uint64_t>((n_seqs + wpb - 1) / wpb, (uint64_t)c->n_cus * (use_lds ? 1 : 2)));
  Scratch m{c->misc};
  const KeyRunsAt o_runs = key_runs_take(m, pl);
  const size_t o_n = m.take<unsigned long long>(1), o_rec = m.take<unsigned long long>(room);
  HIPC(c, m.ensure());
  unsigned long long *dn = m.at<unsigned long long>(o_n), *drec = m.at<unsigned long long>(o_rec);
  PanelSet set{{}, n_genes};
  SHK_TRY(key_runs_upload(c, m, o_runs, pl, &set.runs));
  HIPC(c, hipMemsetAsync(dn, 0, 8, c->stream));
  if (getenv("SHK_TRACE"))  // (read at each call, like SHK_FILTER_LDS_KEYS: the tests look for this line)
    fprintf(stderr, "[shk] filter_panel: %u genes, %llu keys, set of %zu bytes in %s, room %llu, %llu blocks%s\n", n_genes,
            (unsigned long long)pl.n_keys, lds - bitmaps, use_lds ? "LDS" : "global memory", (unsigned long long)room, (unsigned long long)blocks,
            b.planes.p0 ? ", retained reads" : "");
  if (b.planes.p0)
    SHK_TRY(launch_lds_or_global(c, &k_filter_panel_retained<true>, &k_filter_panel_retained<false>, use_lds, &c->lds_attr_filter_retained,
                                 FILTER_LDS_MAX, blocks, FILTER_WG, use_lds ? lds : bitmaps, b.planes, n_seqs, (int)c->cfg.k, set, drec, room, dn));
  else
    SHK_TRY(launch_lds_or_global(c, &k_filter_panel<true>, &k_filter_panel<false>, use_lds, &c->lds_attr_filter, FILTER_LDS_MAX, blocks, FILTER_WG,
                                 use_lds ? lds : bitmaps, b.d_bases, b.d_offsets, n_seqs, (int)c->cfg.k, set, drec, room, dn));
  HIPC(c, hipGetLastError());
  unsigned long long nt = 0;
  HIPC(c, hipMemcpyAsync(&nt, dn, 8, hipMemcpyDeviceToHost, c->stream));
  HIPC(c, hipStreamSynchronize(c->stream));  // (also keeps the plan alive until its copies ran)
  *n_total = nt;
  recs->clear();
  if (nt && nt <= room) {
    recs->resize(nt);
    HIPC(c, hipMemcpy(recs->data(), drec, nt * 8, hipMemcpyDeviceToHost));
  }
  return SHK_OK;
}

// The passes: every record of the batch, (gene << FILTER_READ_BITS | read), sorted.  Same preconditions as panel_pass.
int panel_records(shk_ctx *c, const HostKeyRuns &pl, uint32_t n_genes, const ReadBatch &b, std::vector<uint64_t> *recs) {
  if (b.n_seqs >> FILTER_READ_BITS) return fail(c, SHK_ERR_BAD_ARG, "a batch of %llu reads", (unsigned long long)b.n_seqs);
  const uint64_t room = (uint64_t)std::max(env_int("SHK_FILTER_CANDIDATES", 1 << 20), 1);
  uint64_t nt = 0;
  SHK_TRY(panel_pass(c, pl, n_genes, b, room, recs, &nt));
  if (nt > room) {  // the list overflowed: the pass counted what there is, so the second one has room for exactly that
    uint64_t n2 = 0;
    SHK_TRY(panel_pass(c, pl, n_genes, b, nt, recs, &n2));
    if (n2 != nt)
      return fail(c, SHK_ERR_INVARIANT, "panel filter rerun produced %llu records, expected %llu", (unsigned long long)n2, (unsigned long long)nt);
  }
  std::sort(recs->begin(), recs->end());  // arrival order is not part of the result
  return SHK_OK;
}

// The passes and what follows them: the records sorted by (gene, read) are the answer.
int panel_core(shk_ctx *c, const HostKeyRuns &pl, uint32_t n_genes, const ReadBatch &b, uint64_t *match_offsets, uint64_t *match_reads,
               uint64_t match_cap, uint64_t *n_matches) {
  std::vector<uint64_t> recs;
  SHK_TRY(panel_records(c, pl, n_genes, b, &recs));
  const uint64_t nt = recs.size();
  for (const uint64_t r : recs) ++match_offsets[(r >> FILTER_READ_BITS) + 1];
  for (uint32_t g = 0; g < n_genes; ++g) match_offsets[g + 1] += match_offsets[g];
  *n_matches = nt;
  if (nt > match_cap || (nt && !match_reads))
    return fail(c, SHK_ERR_BAD_ARG, "%llu matches do not fit match_cap %llu", (unsigned long long)nt, (unsigned long long)match_cap);
  for (uint64_t i = 0; i < nt; ++i) match_reads[i] = recs[i] & ((1ull << FILTER_READ_BITS) - 1);
  return SHK_OK;
}

}  // namespace

int shk_filter_reads_panel_device(shk_ctx *c, const void *d_bases, const void *d_offsets, uint64_t n_seqs, uint64_t n_bases,
                                  const uint64_t *primer_kmers, const uint64_t *gene_offsets, uint32_t n_genes, uint64_t *match_offsets,
                                  uint64_t *match_reads, uint64_t match_cap, uint64_t *n_matches) {
  SHK_TRY(xs_closed(c));
  if (c && c->group)
    return on_any_device(c, [&](shk_ctx *d) {
      return shk_filter_reads_panel_device(d, d_bases, d_offsets, n_seqs, n_bases, primer_kmers, gene_offsets, n_genes, match_offsets, match_reads,
                                           match_cap, n_matches);
    });
  if (!c || !match_offsets || !n_matches || (n_seqs && !d_offsets)) return SHK_ERR_BAD_ARG;
  HostKeyRuns pl;
  SHK_TRY(panel_plan(c, primer_kmers, gene_offsets, n_genes, &pl));
  std::fill(match_offsets, match_offsets + n_genes + 1, 0ull);
  *n_matches = 0;
  if (n_seqs == 0) return SHK_OK;
  ReadBatch b;
  SHK_TRY(batch_from_device(c, d_bases, d_offsets, n_seqs, n_bases, "shk_filter_reads_panel", &b));
  if (pl.items.empty()) return SHK_OK;
  return panel_core(c, pl, n_genes, b, match_offsets, match_reads, match_cap, n_matches);
}

int shk_filter_reads_panel(shk_ctx *c, const uint8_t *bases, const uint64_t *offsets, uint64_t n_seqs, const uint64_t *primer_kmers,
                           const uint64_t *gene_offsets, uint32_t n_genes, uint64_t *match_offsets, uint64_t *match_reads, uint64_t match_cap,
                           uint64_t *n_matches) {
  SHK_TRY(xs_closed(c));
  if (c && c->group)
    return on_any_device(c, [&](shk_ctx *d) {
      return shk_filter_reads_panel(d, bases, offsets, n_seqs, primer_kmers, gene_offsets, n_genes, match_offsets, match_reads, match_cap, n_matches);
    });
  if (!c || !match_offsets || !n_matches || (n_seqs && !offsets)) return SHK_ERR_BAD_ARG;
  HostKeyRuns pl;
  SHK_TRY(panel_plan(c, primer_kmers, gene_offsets, n_genes, &pl));
  std::fill(match_offsets, match_offsets + n_genes + 1, 0ull);
  *n_matches = 0;
  if (n_seqs == 0) return SHK_OK;
  uint64_t max_len = 0;
  SHK_TRY(batch_check_offsets(c, offsets, n_seqs, offsets[n_seqs], "shk_filter_reads_panel", &max_len));
  if (pl.items.empty()) return SHK_OK;
  if (offsets[n_seqs] && !bases) return SHK_ERR_BAD_ARG;
  // the device form's passes over the staged batch (its offsets are already here: no copy back)
  ReadBatch b;
  SHK_TRY(batch_from_host(c, bases, offsets, n_seqs, max_len, &b));
  return panel_core(c, pl, n_genes, b, match_offsets, match_reads, match_cap, n_matches);
}

int shk_gather_reads_device(shk_ctx *c, const void *d_bases, const void *d_offsets, uint64_t n_seqs, const uint64_t *read_ids, uint64_t n_ids,
                            void *d_out_bases, uint64_t out_bases_cap, void *d_out_offsets, uint64_t *n_out_bases) {
  SHK_TRY(xs_closed(c));
  if (c && c->group)
    return on_any_device(c, [&](shk_ctx *d) {
      return shk_gather_reads_device(d, d_bases, d_offsets, n_seqs, read_ids, n_ids, d_out_bases, out_bases_cap, d_out_offsets, n_out_bases);
    });
  if (!c || !n_out_bases || (n_ids && !read_ids) || (n_seqs && !d_offsets)) return SHK_ERR_BAD_ARG;
  *n_out_bases = 0;
  for (uint64_t j = 0; j < n_ids; ++j)
    if (read_ids[j] >= n_seqs)
      return fail(c, SHK_ERR_BAD_ARG, "read_ids[%llu] = %llu is outside the %llu reads", (unsigned long long)j, (unsigned long long)read_ids[j],
                  (unsigned long long)n_seqs);
  HIPC(c, hipSetDevice(c->cfg.device));
  // (not batch_from_device: no n_bases to hold the offsets to, no 2^31 limit on a read, and n_seqs may be 0)
  SHK_TRY(settle(c));  // (the call's scratch and stream are the context's)
  std::vector<uint64_t> h_off(n_seqs + 1, 0), out_off(n_ids + 1, 0);
  if (n_seqs) HIPC(c, hipMemcpyAsync(h_off.data(), d_offsets, (n_seqs + 1) * 8, hipMemcpyDeviceToHost, c->stream));
  HIPC(c, hipStreamSynchronize(c->stream));
  for (uint64_t i = 0; i < n_seqs; ++i)
    if (h_off[i + 1] < h_off[i]) return fail(c, SHK_ERR_BAD_ARG, "offsets must be non-decreasing");
  for (uint64_t j = 0; j < n_ids; ++j) out_off[j + 1] = out_off[j] + (h_off[read_ids[j] + 1] - h_off[read_ids[j]]);
  const uint64_t need = out_off[n_ids];
  *n_out_bases = need;
  if (need > out_bases_cap)
    return fail(c, SHK_ERR_BAD_ARG, "%llu bases do not fit out_bases_cap %llu", (unsigned long long)need, (unsigned long long)out_bases_cap);
  if (!d_out_offsets || (need && (!d_out_bases || !d_bases))) return SHK_ERR_BAD_ARG;
  HIPC(c, hipMemcpyAsync(d_out_offsets, out_off.data(), (n_ids + 1) * 8, hipMemcpyHostToDevice, c->stream));
  if (need) {
    Scratch m{c->misc};
    const size_t o_ids = m.take<uint64_t>(n_ids);
    HIPC(c, m.ensure());
    HIPC(c, hipMemcpyAsync(m.at<uint64_t>(o_ids), read_ids, n_ids * 8, hipMemcpyHostToDevice, c->stream));
    const uint64_t wpb = WG / 64;
    const uint64_t blocks = std::max<uint64_t>(1, std::min<uint64_t>((n_ids + wpb - 1) / wpb, (uint64_t)c->n_cus * 8));
    ScopedTimer t(c, SHK_K_LOOKUP);
    hipLaunchKernelGGL(k_gather_reads, dim3((uint32_t)blocks), dim3(WG), 0, c->stream, (const uint8_t *)d_bases, (const uint64_t *)d_offsets,
                       (const uint64_t *)m.at<uint64_t>(o_ids), n_ids, (const uint64_t *)d_out_offsets, (uint8_t *)d_out_bases);
  }
  HIPC(c, hipGetLastError());
  HIPC(c, hipStreamSynchronize(c->stream));  // (keeps out_off and read_ids alive until their copies ran; the batch is complete on return)
  return SHK_OK;
}

}  // extern "C"
