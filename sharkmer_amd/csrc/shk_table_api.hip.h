// The part of the C ABI that reads the table or hands it to a peer: export, lookup, the sPCR scans (neighborhood, extend,
// find_oligos, primer_kmers — each of the first two and the last with its depth form as a second caller of ONE body:
// nb_panel_call, pcr_extend_panel_call, primer_scan), the read filters, and the owner exchange (geometry, merge, counts,
// compaction, owned ranges).
// Included at the end of shk_engine.hip (one translation unit: the context, settle and the helpers beside HIPC are there).
//
// A call that reads the table begins with table_read_begin; one that does not says why where it departs.

// What the table-read and owner-exchange entry points share.
namespace {

// A scan of a multi-device context that appends to (kmers, counts): the shares are disjoint, so one after the other,
// each with the room those before it left.  call(share, kmers, counts, room, &n) is the scan of one share.
template <typename F>
int each_share_appends(shk_ctx *c, uint64_t *kmers, uint32_t *counts, uint64_t cap, uint64_t *n_out, F call) {
  uint64_t at = 0;
  for (uint32_t d = 0; d < c->group->D; ++d) {
    uint64_t n = 0;
    const uint64_t room = at < cap ? cap - at : 0;
    const int rc = call(c->group->ctx[d], kmers ? kmers + std::min(at, cap) : nullptr, counts ? counts + std::min(at, cap) : nullptr, room, &n);
    if (rc != SHK_OK) return group_fail(c, c->group, rc, d);
    at += n;
  }
  if (n_out) *n_out = at;
  return SHK_OK;
}

// The end of an appending scan: *n_out = the entries it found (dn; may exceed cap), and the first min(*n_out, cap) of
// them for the arrays the caller gave.  (The wait also keeps the caller's host sources alive until their copies ran.)
int fetch_appended(shk_ctx *c, const unsigned long long *dn, const uint64_t *dk, const uint32_t *dc, uint64_t cap, uint64_t *kmers,
                   uint32_t *counts, uint64_t *n_out) {
  unsigned long long n = 0;
  HIPC(c, hipMemcpyAsync(&n, dn, 8, hipMemcpyDeviceToHost, c->stream));
  HIPC(c, hipStreamSynchronize(c->stream));
  *n_out = n;
  const uint64_t m = std::min<uint64_t>(n, cap);
  if (m && kmers) HIPC(c, hipMemcpy(kmers, dk, m * 8, hipMemcpyDeviceToHost));
  if (m && counts) HIPC(c, hipMemcpy(counts, dc, m * 4, hipMemcpyDeviceToHost));
  return SHK_OK;
}

// An owner is a run of whole pages: the page count has to split evenly.
int owner_split_check(shk_ctx *c, uint32_t n_owners) {
  const uint64_t n_pages = 1ull << c->tb.log_pages;
  if (n_pages % n_owners) return fail(c, SHK_ERR_BAD_ARG, "%llu pages do not split over %u owners",
                                      (unsigned long long)n_pages, n_owners);
  return SHK_OK;
}
uint32_t owner_blocks(uint32_t n_owners) { return std::min<uint32_t>(1024, std::max<uint32_t>(16, 2048 / n_owners)); }  // blocks per owner

// The k_compact_owners launch of the three shk_compact_owners* calls.  device: [seg offsets (entries) × W][cursors × W]
// [counts × W].  h_off: where each owner's entries start in the destination; h_cnt: how many it was promised (the packed
// layouts; nullptr: separate key and count arrays); header_bytes: what a piece keeps in front of its entries; fullest:
// the word that takes the fullest owner range's entries (nullptr: nobody asks).
int compact_owners_launch(shk_ctx *c, uint32_t n_owners, const uint64_t *h_off, const uint64_t *h_cnt, void *d_keys, void *d_vals,
                          uint64_t vals_lane_stride, int32_t skip_owner, unsigned long long header_bytes, unsigned long long *fullest) {
  using ull = unsigned long long;
  Scratch m{c->misc};
  const size_t o_off = m.take<ull>(n_owners), o_cur = m.take<ull>(n_owners), o_cnt = m.take<ull>(h_cnt ? n_owners : 0);
  HIPC(c, m.ensure());
  ull *doff = m.at<ull>(o_off), *dcur = m.at<ull>(o_cur), *dcnt = h_cnt ? m.at<ull>(o_cnt) : nullptr;
  HIPC(c, hipMemcpyAsync(doff, h_off, (size_t)n_owners * 8, hipMemcpyHostToDevice, c->stream));
  if (h_cnt) HIPC(c, hipMemcpyAsync(dcnt, h_cnt, (size_t)n_owners * 8, hipMemcpyHostToDevice, c->stream));
  HIPC(c, hipMemsetAsync(dcur, 0, (size_t)n_owners * 8, c->stream));
  const uint32_t bpo = owner_blocks(n_owners);
  hipLaunchKernelGGL(k_compact_owners, dim3(n_owners * bpo), dim3(WG), 0, c->stream, c->tb, c->tb.cap / n_owners,
                     (const ull *)doff, dcur, (uint64_t *)d_keys, (uint32_t *)d_vals, vals_lane_stride,
                     skip_owner < 0 ? ~0u : (uint32_t)skip_owner, bpo, (const ull *)dcnt, header_bytes, fullest);
  return SHK_OK;
}

// "The table" of a neighbourhood call: the context's own TableRef, or — a multi-device context under
// SHK_FLAG_GROUP_GRAPH — the share directory, TableRef[2^owner_bits] in the lead share's scratch (rebuilt at every call:
// shares grow on their own).
struct NbTableArg {
  TableRef one{};
  NbShards shards{nullptr, 0};
  bool depths = false;  // every job's probe stops at its NbRef::lanes (the *_depth kernels; one table only)
  bool sharded() const { return shards.dir != nullptr; }
};

// The one launch site of the two kernels that probe the table.  wide == nullptr: k_nb_narrow_panel, one workgroup for
// each of the n_jobs jobs at (drefs, dctl); else k_nb_wide, the level of h->cur_n entries in list h->cur_sel of job
// (*wide, dctl).
void nb_launch(shk_ctx *c, const NbTableArg &tb, const NbRef *drefs, NbCtl *dctl, uint32_t n_jobs, const NbRef *wide, const NbCtl *h) {
  ScopedTimer t(c, SHK_K_EXTEND);
  const dim3 grid(wide ? (uint32_t)((h->cur_n * 4 + WG - 1) / WG) : n_jobs), block(wide ? WG : NB_WG);
  if (tb.depths) {
    if (wide)
      hipLaunchKernelGGL(k_nb_wide_depth, grid, block, 0, c->stream, tb.one, *wide, dctl, h->cur_sel, (uint64_t)h->cur_n);
    else
      hipLaunchKernelGGL(k_nb_narrow_panel_depth, grid, block, 0, c->stream, tb.one, drefs, dctl);
  } else if (wide) {
    if (tb.sharded())
      hipLaunchKernelGGL(k_nb_wide<true>, grid, block, 0, c->stream, tb.shards, *wide, dctl, h->cur_sel, (uint64_t)h->cur_n);
    else
      hipLaunchKernelGGL(k_nb_wide<false>, grid, block, 0, c->stream, tb.one, *wide, dctl, h->cur_sel, (uint64_t)h->cur_n);
  } else {
    if (tb.sharded())
      hipLaunchKernelGGL(k_nb_narrow_panel<true>, grid, block, 0, c->stream, tb.shards, drefs, dctl);
    else
      hipLaunchKernelGGL(k_nb_narrow_panel<false>, grid, block, 0, c->stream, tb.one, drefs, dctl);
  }
}

// The level loop of a neighbourhood job that outgrew its workgroup (nb_panel_core: status NB_WIDE): from the state h
// (which dctl holds too; nb is the host's copy of *dref) until the job stops — complete, at max_levels, or before a
// level that does not fit.  A narrow launch is k_nb_narrow_panel on this job alone.  Its guard (status NB_RUN, 0 <
// cur_n <= NB_NARROW) holds at each: the loop comes in with a level wider than NB_NARROW, so a narrow launch always
// follows a wide level, after which the host uploaded h with status NB_RUN and the cur_n tested here.
int nb_run_levels(shk_ctx *c, const NbTableArg &tb, const NbRef &nb, const NbRef *dref, NbCtl *dctl, NbCtl &h) {
  // level after level: the narrow kernel while a level fits one workgroup, else one wide launch and a look at its fills
  while (h.status == NB_RUN || h.status == NB_WIDE) {
    if (h.cur_n == 0) {
      h.status = NB_COMPLETE;
      break;
    }
    if (nb.max_levels && h.levels_done >= nb.max_levels) {
      h.status = NB_LIMIT;
      break;
    }
    if (h.cur_n <= NB_NARROW) {
      nb_launch(c, tb, dref, dctl, 1, nullptr, nullptr);
      HIPC(c, hipGetLastError());
      HIPC(c, hipMemcpyAsync(&h, dctl, sizeof h, hipMemcpyDeviceToHost, c->stream));
      HIPC(c, hipStreamSynchronize(c->stream));
      continue;
    }
    const unsigned long long k_start = h.k_n;
    nb_launch(c, tb, nullptr, dctl, 1, &nb, &h);
    HIPC(c, hipGetLastError());
    NbCtl r{};
    HIPC(c, hipMemcpyAsync(&r, dctl, sizeof r, hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipStreamSynchronize(c->stream));
    if (r.set_full || r.k_n > nb.cap || r.next_n > nb.fringe_cap) {  // the level did not fit: the k-mer list back to its start
      h.k_n = k_start;
      h.status = NB_OVERFLOW;
      break;
    }
    h.k_n = r.k_n;
    h.cur_n = r.next_n;
    h.cur_sel ^= 1u;
    h.levels_done += 1;
    h.next_n = 0;
    h.status = NB_RUN;
    HIPC(c, hipMemcpyAsync(dctl, &h, sizeof h, hipMemcpyHostToDevice, c->stream));
    HIPC(c, hipStreamSynchronize(c->stream));  // (h is a pageable source: the copy has read it)
  }
  return SHK_OK;
}

// Sizes of a job's two sets.  An accepted k-mer has two orientations and an orientation one successor per dir: through
// a level that fits, the visited set never holds more than the seeds and 4·cap entries, the k-mer set cap.  Both at
// most half full then; a set that fills up (probes are bounded) belongs to a level that does not fit and is dropped.
uint64_t nb_pow2_above(uint64_t n) {
  uint64_t s = 16;
  while (s < n) s <<= 1;
  return s;
}
uint64_t nb_vis_slots(uint64_t n_seeds, uint64_t cap) { return nb_pow2_above(2 * (n_seeds + 4 * cap) + 2); }
uint64_t nb_kset_slots(uint64_t cap) { return nb_pow2_above(2 * cap + 2); }

// A call's (or a job's) seeds as level 0: the distinct (node, dir) pairs as entries node << 1 | (0 forward, 1 reverse),
// ascending.  `who`: what an error text starts with ("" or "job 7: ").
int nb_level0(shk_ctx *c, const char *who, const uint64_t *nodes, const uint8_t *dirs, uint64_t n_seeds, uint32_t k,
              uint64_t fringe_cap, std::vector<uint64_t> *seeds) {
  const uint64_t node_mask = (1ull << (2 * (k - 1))) - 1ull;
  seeds->clear();
  seeds->reserve(n_seeds);
  for (uint64_t i = 0; i < n_seeds; ++i) {
    if (dirs[i] == 0 || dirs[i] > 3) return fail(c, SHK_ERR_BAD_ARG, "%sseed %llu: dir %u is not 1 (forward), 2 (reverse) or 3 (both)", who, (unsigned long long)i, dirs[i]);
    if (nodes[i] > node_mask) return fail(c, SHK_ERR_BAD_ARG, "%sseed %llu: node 0x%llx is not a %u-mer", who, (unsigned long long)i, (unsigned long long)nodes[i], k - 1);
    if (dirs[i] & 1) seeds->push_back(nodes[i] << 1);
    if (dirs[i] & 2) seeds->push_back(nodes[i] << 1 | 1ull);
  }
  std::sort(seeds->begin(), seeds->end());
  seeds->erase(std::unique(seeds->begin(), seeds->end()), seeds->end());
  if (seeds->size() > fringe_cap)
    return fail(c, SHK_ERR_BAD_ARG, "%s%llu distinct seeds do not fit fringe_cap %llu", who, (unsigned long long)seeds->size(), (unsigned long long)fringe_cap);
  return SHK_OK;
}

// The arrival order of the appends is not part of the result: (hk, hc) ascending by k-mer into (kmers, counts), the
// entries hf ascending into (fringe_nodes, fringe_dirs).
void nb_sorted_out(const uint64_t *hk, const uint32_t *hc, uint64_t nk, uint64_t *hf, uint64_t nf, uint64_t *kmers,
                   uint32_t *counts, uint64_t *fringe_nodes, uint8_t *fringe_dirs) {
  std::vector<uint32_t> order(nk);
  for (uint64_t i = 0; i < nk; ++i) order[i] = (uint32_t)i;
  std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return hk[a] < hk[b]; });
  for (uint64_t i = 0; i < nk; ++i) {
    kmers[i] = hk[order[i]];
    counts[i] = hc[order[i]];
  }
  std::sort(hf, hf + nf);
  for (uint64_t i = 0; i < nf; ++i) {
    fringe_nodes[i] = hf[i] >> 1;
    fringe_dirs[i] = (uint8_t)(1u << (hf[i] & 1ull));
  }
}

// The device part of shk_neighborhood_panel, and of shk_neighborhood as its one-job case, after every job's arguments
// were checked: job j starts from level 0 seeds[j] (nb_level0's) under min_counts[j], caps[j] and fringe_caps[j]; its
// k-mers go to (kmers, counts) + out_at[j], its fringe to (fringe_nodes, fringe_dirs) + fr_at[j], its figures to
// n_out[j], n_fringe[j] and levels_done[j].
// g == nullptr: c is the context and the table its own.  Else c is the lead share (share 0) of the multi-device context
// g: every share is settled on its own device and its stream drained, the directory of their tables goes up with the
// call's one upload, and the job logic runs as it is on c — its scratch, stream and timing slots; *who: the share whose
// error text is the call's.
// job_lanes (or nullptr): job j reads the table at depth job_lanes[j] (g == nullptr then).
int nb_panel_run(shk_ctx *c, shk_group *g, uint32_t *who, const std::vector<uint64_t> *seeds, uint32_t n_jobs, const uint32_t *min_counts, const uint32_t *job_lanes, uint32_t max_levels,
                  const uint64_t *caps, const uint64_t *fringe_caps, const uint64_t *out_at, const uint64_t *fr_at, uint64_t *kmers,
                  uint32_t *counts, uint64_t *n_out, uint64_t *fringe_nodes, uint8_t *fringe_dirs, uint64_t *n_fringe,
                  uint32_t *levels_done) {
  const uint32_t k = c->cfg.k;
  uint64_t n_all_seeds = 0;
  for (uint32_t j = 0; j < n_jobs; ++j) n_all_seeds += seeds[j].size();
  std::fill(n_out, n_out + n_jobs, 0ull);
  std::fill(n_fringe, n_fringe + n_jobs, 0ull);
  std::fill(levels_done, levels_done + n_jobs, 0u);
  if (n_all_seeds == 0) return SHK_OK;
  const uint32_t n_shares = g ? g->D : 0;
  std::vector<TableRef> shares(n_shares);
  if (g) {
    for (uint32_t d = 0; d < n_shares; ++d) {  // (a share's table is final once its stream is idle; nothing writes it during the call)
      *who = d;
      SHK_TRY(table_read_begin(g->ctx[d]));
      HIPC(g->ctx[d], hipStreamSynchronize(g->ctx[d]->stream));
      shares[d] = g->ctx[d]->tb;
    }
    *who = 0;
    HIPC(c, hipSetDevice(c->cfg.device));
  } else {
    SHK_TRY(table_read_begin(c));
  }
  // Device layout: every job's two sets in one region (one clear), then what is uploaded in one copy (NbRef, NbCtl,
  // seed starts, seeds, their jobs), then the lists.  A job without seeds gets no room: it is not run.  The packed
  // copies are for a panel: one job's lists are fetched from where they are.
  const bool packed = n_jobs > 1;
  std::vector<uint64_t> capj(n_jobs), fcj(n_jobs), set_at(n_jobs + 1, 0), l_at(n_jobs + 1, 0), k_at(n_jobs + 1, 0);
  for (uint32_t j = 0; j < n_jobs; ++j) {
    const bool live = !seeds[j].empty();
    capj[j] = live ? caps[j] : 0;
    fcj[j] = live ? fringe_caps[j] : 0;
    set_at[j + 1] = set_at[j] + (live ? nb_vis_slots(seeds[j].size(), capj[j]) + nb_kset_slots(capj[j]) : 0);
    l_at[j + 1] = l_at[j] + std::max<uint64_t>(fcj[j], 1);
    k_at[j + 1] = k_at[j] + std::max<uint64_t>(capj[j], 1);
  }
  const uint64_t n_pk = packed ? k_at[n_jobs] : 0, n_pf = packed ? l_at[n_jobs] : 0;
  Scratch m{c->misc};
  const size_t o_sets = m.take<uint64_t>(set_at[n_jobs]);
  const size_t o_refs = m.take<NbRef>(n_jobs), o_ctl = m.take<NbCtl>(n_jobs), o_start = m.take<uint64_t>(n_jobs + 1);
  const size_t o_seeds = m.take<uint64_t>(n_all_seeds), o_sjob = m.take<uint32_t>(n_all_seeds);
  const size_t o_dir = m.take<TableRef>(n_shares);  // the share directory (a multi-device context's)
  const size_t o_pack = m.take<NbPack>(n_jobs);  // (ends the uploaded block)
  const size_t o_l0 = m.take<uint64_t>(l_at[n_jobs]), o_l1 = m.take<uint64_t>(l_at[n_jobs]);
  const size_t o_km = m.take<uint64_t>(k_at[n_jobs]), o_ct = m.take<uint32_t>(k_at[n_jobs]);
  const size_t o_pk = m.take<uint64_t>(n_pk), o_pc = m.take<uint32_t>(n_pk), o_pf = m.take<uint64_t>(n_pf);
  HIPC(c, m.ensure());
  std::vector<uint8_t> up(o_pack - o_refs, 0);  // the uploaded block as the device holds it
  NbRef *href = (NbRef *)up.data();
  NbCtl *hctl = (NbCtl *)(up.data() + (o_ctl - o_refs));
  uint64_t *hstart = (uint64_t *)(up.data() + (o_start - o_refs)), *hseeds = (uint64_t *)(up.data() + (o_seeds - o_refs));
  uint32_t *hsjob = (uint32_t *)(up.data() + (o_sjob - o_refs));
  uint64_t at = 0;
  for (uint32_t j = 0; j < n_jobs; ++j) {
    NbRef &nb = href[j];
    const uint64_t vis_slots = seeds[j].empty() ? 0 : nb_vis_slots(seeds[j].size(), capj[j]);
    nb.vis = m.at<uint64_t>(o_sets) + set_at[j];
    nb.kset = nb.vis + vis_slots;
    nb.vis_mask = vis_slots ? vis_slots - 1 : 0;
    nb.kset_mask = seeds[j].empty() ? 0 : nb_kset_slots(capj[j]) - 1;
    nb.list[0] = m.at<uint64_t>(o_l0) + l_at[j];
    nb.list[1] = m.at<uint64_t>(o_l1) + l_at[j];
    nb.kmers = m.at<uint64_t>(o_km) + k_at[j];
    nb.counts = m.at<uint32_t>(o_ct) + k_at[j];
    nb.cap = capj[j];
    nb.fringe_cap = fcj[j];
    nb.min_count = std::max(min_counts[j], 1u);
    nb.max_levels = max_levels;
    nb.k = (int)k;
    nb.lanes = job_lanes ? job_lanes[j] : 0u;
    hctl[j].cur_n = seeds[j].size();
    hctl[j].status = seeds[j].empty() ? NB_COMPLETE : seeds[j].size() > NB_NARROW ? NB_WIDE : NB_RUN;
    hstart[j] = at;
    for (const uint64_t e : seeds[j]) {
      hseeds[at] = e;
      hsjob[at++] = j;
    }
  }
  hstart[n_jobs] = at;
  NbTableArg tb;
  tb.one = c->tb;
  tb.depths = job_lanes != nullptr;
  if (g) {
    std::copy(shares.begin(), shares.end(), (TableRef *)(up.data() + (o_dir - o_refs)));
    uint32_t owner_bits = 0;
    while ((1u << owner_bits) < n_shares) ++owner_bits;
    tb.shards = NbShards{m.at<TableRef>(o_dir), owner_bits};
  }
  NbRef *drefs = m.at<NbRef>(o_refs);
  NbCtl *dctl = m.at<NbCtl>(o_ctl);
  HIPC(c, hipMemsetAsync(m.at<uint64_t>(o_sets), 0xFF, set_at[n_jobs] * 8, c->stream));  // every set ← EMPTY
  HIPC(c, hipMemcpyAsync(drefs, up.data(), up.size(), hipMemcpyHostToDevice, c->stream));
  {
    ScopedTimer t(c, SHK_K_EXTEND);
    hipLaunchKernelGGL(k_nb_seed_panel, dim3((uint32_t)((n_all_seeds + WG - 1) / WG)), dim3(WG), 0, c->stream,
                       (const NbRef *)drefs, dctl, (const uint64_t *)m.at<uint64_t>(o_seeds),
                       (const uint32_t *)m.at<uint32_t>(o_sjob), (const uint64_t *)m.at<uint64_t>(o_start), n_all_seeds);
  }
  nb_launch(c, tb, drefs, dctl, n_jobs, nullptr, nullptr);
  HIPC(c, hipGetLastError());
  std::vector<NbCtl> h(n_jobs);
  HIPC(c, hipMemcpyAsync(h.data(), dctl, (size_t)n_jobs * sizeof(NbCtl), hipMemcpyDeviceToHost, c->stream));
  HIPC(c, hipStreamSynchronize(c->stream));  // (also: `up` has been read)
  // the exception: a job with a level wider than a workgroup goes on alone
  for (uint32_t j = 0; j < n_jobs; ++j)
    if (h[j].status == NB_WIDE) SHK_TRY(nb_run_levels(c, tb, href[j], drefs + j, dctl + j, h[j]));
  std::vector<NbPack> pk(n_jobs);
  uint64_t tot_k = 0, tot_f = 0;
  for (uint32_t j = 0; j < n_jobs; ++j) {
    pk[j] = NbPack{h[j].k_n, h[j].status == NB_COMPLETE ? 0ull : h[j].cur_n, tot_k, tot_f, h[j].cur_sel, 0};
    if (pk[j].k_n > capj[j] || pk[j].n_f > std::max<uint64_t>(fcj[j], seeds[j].size()))
      return fail(c, SHK_ERR_INVARIANT, "job %u: %llu k-mers / %llu fringe entries beyond its capacities", j, pk[j].k_n, pk[j].n_f);
    tot_k += pk[j].k_n;
    tot_f += pk[j].n_f;
  }
  std::vector<uint64_t> hk(tot_k), hf(tot_f);
  std::vector<uint32_t> hc(tot_k);
  if (tot_k || tot_f) {
    const uint64_t *dk = href[0].kmers, *df = href[0].list[pk[0].sel & 1u];  // one job: its own arrays
    const uint32_t *dc = href[0].counts;
    if (packed) {
      dk = m.at<uint64_t>(o_pk), dc = m.at<uint32_t>(o_pc), df = m.at<uint64_t>(o_pf);
      HIPC(c, hipMemcpyAsync(m.at<NbPack>(o_pack), pk.data(), (size_t)n_jobs * sizeof(NbPack), hipMemcpyHostToDevice, c->stream));
      {
        ScopedTimer t(c, SHK_K_EXTEND);
        hipLaunchKernelGGL(k_nb_pack_panel, dim3(n_jobs), dim3(WG), 0, c->stream, (const NbRef *)drefs,
                           (const NbPack *)m.at<NbPack>(o_pack), m.at<uint64_t>(o_pk), m.at<uint32_t>(o_pc), m.at<uint64_t>(o_pf));
      }
      HIPC(c, hipGetLastError());
    }
    // (one job: the stream is idle here, and plain copies are what the single call always made; a panel's queue behind the pack)
    auto fetch = [&](void *dst, const void *src, size_t bytes) {
      return packed ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream) : hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost);
    };
    if (tot_k) {
      HIPC(c, fetch(hk.data(), dk, tot_k * 8));
      HIPC(c, fetch(hc.data(), dc, tot_k * 4));
    }
    if (tot_f) HIPC(c, fetch(hf.data(), df, tot_f * 8));
    if (packed) HIPC(c, hipStreamSynchronize(c->stream));
  }
  for (uint32_t j = 0; j < n_jobs; ++j) {
    const NbPack &p = pk[j];
    nb_sorted_out(hk.data() + p.pack_k, hc.data() + p.pack_k, p.k_n, hf.data() + p.pack_f, p.n_f, kmers + out_at[j],
                  counts + out_at[j], fringe_nodes + fr_at[j], fringe_dirs + fr_at[j]);
    n_out[j] = p.k_n;
    n_fringe[j] = p.n_f;
    levels_done[j] = h[j].levels_done;
  }
  return SHK_OK;
}

int nb_panel_core(shk_ctx *c, const std::vector<uint64_t> *seeds, uint32_t n_jobs, const uint32_t *min_counts, const uint32_t *job_lanes, uint32_t max_levels,
                  const uint64_t *caps, const uint64_t *fringe_caps, const uint64_t *out_at, const uint64_t *fr_at, uint64_t *kmers,
                  uint32_t *counts, uint64_t *n_out, uint64_t *fringe_nodes, uint8_t *fringe_dirs, uint64_t *n_fringe,
                  uint32_t *levels_done) {
  shk_group *g = c->group;
  uint32_t who = 0;
  const int rc = nb_panel_run(g ? g->ctx[0] : c, g, &who, seeds, n_jobs, min_counts, job_lanes, max_levels, caps, fringe_caps, out_at, fr_at, kmers, counts,
                              n_out, fringe_nodes, fringe_dirs, n_fringe, levels_done);
  return rc == SHK_OK || !g ? rc : group_fail(c, g, rc, who);
}

// How the four graph calls refuse or open on a multi-device context (`name`: the call's) — and refuse an owner share.
int graph_call_begin(shk_ctx *c, const char *name) {
  if (c->group && !(c->cfg.flags & SHK_FLAG_GROUP_GRAPH))
    return fail(c, SHK_ERR_STATE, "%s needs the whole table on one device: this is a multi-device context (n_devices > 1)", name);
  if (c->group) return group_graph_begin(c);
  if (c->n_owners > 1)
    return fail(c, SHK_ERR_STATE, "%s needs the whole table on one device: this context is an owner share (n_owners > 1)", name);
  return SHK_OK;
}

// How the depth calls refuse, before the device is touched: a multi-device context (whatever its flags)
// and an owner share, then a depth that is none — 0 or above the context's lanes; a list: empty, longer than
// SHK_PCR_MAX_DEPTHS or not strictly ascending.
int depth_call_begin(shk_ctx *c, const char *name, const uint32_t *depths, uint32_t n, bool list) {
  if (c->group) return fail(c, SHK_ERR_STATE, "%s: no depths on a multi-device context (n_devices > 1)", name);
  if (c->n_owners > 1) return fail(c, SHK_ERR_STATE, "%s: no depths on an owner share (n_owners > 1)", name);
  if (list && (n == 0 || n > SHK_PCR_MAX_DEPTHS))
    return fail(c, SHK_ERR_BAD_ARG, "%s: n_depths %u is not 1..%u", name, n, (unsigned)SHK_PCR_MAX_DEPTHS);
  if (n && !depths) return SHK_ERR_BAD_ARG;
  for (uint32_t j = 0; j < n; ++j) {
    if (depths[j] == 0 || depths[j] > c->n_lanes)
      return fail(c, SHK_ERR_BAD_ARG, "%s: depth %u is not 1..%u (n_chunks)", name, depths[j], c->n_lanes);
    if (list && j && depths[j] <= depths[j - 1])
      return fail(c, SHK_ERR_BAD_ARG, "%s: depths are not strictly ascending (%u after %u)", name, depths[j], depths[j - 1]);
  }
  return SHK_OK;
}

// The graphs of shk_pcr_extend_panel, and of shk_pcr_extend as a panel of one, into the caller's arrays: gene g's nodes
// from node_offsets[g], its edges from edge_offsets[g] (both filled here, as is found_path, before anything is refused).
// what: "graph" or "panel", as the text of a refusal calls them.
int pcr_graphs_out(shk_ctx *c, const char *what, const std::vector<PcrGraph> &gs, uint64_t *node_sub_kmers, uint8_t *node_flags,
                   uint64_t *node_offsets, uint64_t node_cap, uint32_t *edge_src, uint32_t *edge_tgt, uint32_t *edge_counts,
                   uint64_t *edge_offsets, uint64_t edge_cap, uint32_t *found_path) {
  using ull = unsigned long long;
  const size_t n_genes = gs.size();
  node_offsets[0] = edge_offsets[0] = 0;
  for (size_t g = 0; g < n_genes; ++g) {
    node_offsets[g + 1] = node_offsets[g] + gs[g].sub_kmer.size();
    edge_offsets[g + 1] = edge_offsets[g] + gs[g].esrc.size();
    found_path[g] = gs[g].found_path ? 1u : 0u;
  }
  const uint64_t nn = node_offsets[n_genes], ne = edge_offsets[n_genes];
  if (nn > node_cap || ne > edge_cap)
    return fail(c, SHK_ERR_BAD_ARG, "%s of %llu nodes and %llu edges does not fit node_cap %llu / edge_cap %llu", what, (ull)nn,
                (ull)ne, (ull)node_cap, (ull)edge_cap);
  if ((nn && (!node_sub_kmers || !node_flags)) || (ne && (!edge_src || !edge_tgt || !edge_counts))) return SHK_ERR_BAD_ARG;
  for (size_t g = 0; g < n_genes; ++g) {
    const PcrGraph &gr = gs[g];
    std::copy(gr.sub_kmer.begin(), gr.sub_kmer.end(), node_sub_kmers + node_offsets[g]);
    std::copy(gr.flags.begin(), gr.flags.end(), node_flags + node_offsets[g]);
    std::copy(gr.esrc.begin(), gr.esrc.end(), edge_src + edge_offsets[g]);
    std::copy(gr.etgt.begin(), gr.etgt.end(), edge_tgt + edge_offsets[g]);
    std::copy(gr.ecount.begin(), gr.ecount.end(), edge_counts + edge_offsets[g]);
  }
  return SHK_OK;
}

// One primer scan pass over c's slots (the owned pages of an owner share) for the searched primers dev, per_launch of
// them at a time: launch(grid, s0, s1, the launch's primers on the device, how many, the first one's index, drec, dn,
// dhits) starts k_primer_scan or k_primer_scan_depths.  Back come the n_hits per-(primer, level) hits and, when they fit
// in `room`, the records.  *n_total = records the pass produced (> room: none returned).
template <class Dev, class Launch>
int primer_pass(shk_ctx *c, const std::vector<Dev> &dev, size_t n_hits, uint32_t per_launch, uint64_t room, std::vector<PrimerRec> *recs,
                std::vector<uint64_t> *hits, uint64_t *n_total, Launch launch) {
  SHK_TRY(table_read_begin(c));
  const uint32_t n = (uint32_t)dev.size();
  Scratch m{c->misc};
  const size_t o_n = m.take<unsigned long long>(1), o_hits = m.take<unsigned long long>(n_hits);  // (adjacent)
  const size_t o_prim = m.take<Dev>(n), o_rec = m.take<PrimerRec>(room);
  HIPC(c, m.ensure());
  unsigned long long *dn = m.at<unsigned long long>(o_n), *dhits = m.at<unsigned long long>(o_hits);
  Dev *dprim = m.at<Dev>(o_prim);
  PrimerRec *drec = m.at<PrimerRec>(o_rec);
  HIPC(c, hipMemsetAsync(dn, 0, o_prim - o_n, c->stream));  // the record counter and the hits
  HIPC(c, hipMemcpyAsync(dprim, dev.data(), (size_t)n * sizeof(Dev), hipMemcpyHostToDevice, c->stream));
  const auto [s0, s1] = owned_slots(c);
  for (uint32_t b = 0; b < n; b += per_launch) {
    const uint32_t nb = std::min(per_launch, n - b);
    ScopedTimer t(c, SHK_K_LOOKUP);
    launch(dim3(grid_for(s1 - s0, WG * 8, 2048)), s0, s1, (const Dev *)(dprim + b), nb, b, drec, dn, dhits);
  }
  HIPC(c, hipGetLastError());
  unsigned long long nt = 0;
  hits->assign(n_hits, 0);
  HIPC(c, hipMemcpyAsync(&nt, dn, 8, hipMemcpyDeviceToHost, c->stream));
  HIPC(c, hipMemcpyAsync(hits->data(), dhits, n_hits * 8, hipMemcpyDeviceToHost, c->stream));
  HIPC(c, hipStreamSynchronize(c->stream));  // (also keeps dev alive until its copy ran)
  *n_total = nt;
  recs->clear();
  if (nt <= room && nt) {
    recs->resize(nt);
    HIPC(c, hipMemcpy(recs->data(), drec, nt * sizeof(PrimerRec), hipMemcpyDeviceToHost));
  }
  return SHK_OK;
}

}  // namespace

extern "C" {

int shk_export_table(shk_ctx *c, uint64_t *kmers, uint32_t *counts, uint64_t cap, uint64_t *n_out) {
  SHK_TRY(xs_closed(c));
  if (!c || !n_out) return SHK_ERR_BAD_ARG;
  if (c->group)
    return each_share_appends(c, kmers, counts, cap, n_out, [](shk_ctx *s, uint64_t *k, uint32_t *ct, uint64_t room, uint64_t *n) {
      return shk_export_table(s, k, ct, room, n);
    });
  SHK_TRY(table_read_begin(c));
  Scratch m{c->misc};
  const size_t o_n = m.take<unsigned long long>(1), o_k = m.take<uint64_t>(cap), o_c = m.take<uint32_t>(cap);
  HIPC(c, m.ensure());
  unsigned long long *dn = m.at<unsigned long long>(o_n);
  uint64_t *dk = m.at<uint64_t>(o_k);
  uint32_t *dc = m.at<uint32_t>(o_c);
  HIPC(c, hipMemsetAsync(dn, 0, 8, c->stream));
  const auto [s0, s1] = owned_slots(c);
  {
    ScopedTimer t(c, SHK_K_EXPORT);
    hipLaunchKernelGGL(k_export, dim3(grid_for(s1 - s0, WG * 4, 4096)), dim3(WG), 0, c->stream, c->tb, s0,
                       s1, dk, dc, cap, dn);
  }
  return fetch_appended(c, dn, dk, dc, cap, kmers, counts, n_out);
}

// shk_lookup on one device; lanes != 0: shk_lookup_depth at that depth.
static int lookup_one(shk_ctx *c, const uint64_t *kmers, uint32_t *counts, uint64_t n, int canonical, uint32_t lanes);

int shk_lookup(shk_ctx *c, const uint64_t *kmers, uint32_t *counts, uint64_t n, int canonical) {
  SHK_TRY(xs_closed(c));
  if (c && c->group) {  // exactly one share owns a k-mer; the others answer 0
    std::vector<uint32_t> part(n);
    std::fill(counts, counts + n, 0u);
    for (uint32_t d = 0; d < c->group->D; ++d) {
      const int rc = shk_lookup(c->group->ctx[d], kmers, part.data(), n, canonical);
      if (rc != SHK_OK) return group_fail(c, c->group, rc, d);
      for (uint64_t i = 0; i < n; ++i) counts[i] += part[i];
    }
    return SHK_OK;
  }
  if (!c) return SHK_ERR_BAD_ARG;
  return lookup_one(c, kmers, counts, n, canonical, 0);
}

int shk_lookup_depth(shk_ctx *c, const uint64_t *kmers, uint32_t *counts, uint64_t n, int canonical, uint32_t depth) {
  SHK_TRY(xs_closed(c));
  if (!c) return SHK_ERR_BAD_ARG;
  SHK_TRY(depth_call_begin(c, "shk_lookup_depth", &depth, 1, false));
  return lookup_one(c, kmers, counts, n, canonical, depth);
}

static int lookup_one(shk_ctx *c, const uint64_t *kmers, uint32_t *counts, uint64_t n, int canonical, uint32_t lanes) {
  if (n == 0) return SHK_OK;
  SHK_TRY(table_read_begin(c));
  Scratch m{c->misc};
  const size_t o_k = m.take<uint64_t>(n), o_c = m.take<uint32_t>(n);
  HIPC(c, m.ensure());
  uint64_t *dk = m.at<uint64_t>(o_k);
  uint32_t *dc = m.at<uint32_t>(o_c);
  HIPC(c, hipMemcpyAsync(dk, kmers, n * 8, hipMemcpyHostToDevice, c->stream));
  {
    ScopedTimer t(c, SHK_K_LOOKUP);
    const dim3 grid((uint32_t)((n + WG - 1) / WG));
    if (lanes)
      hipLaunchKernelGGL(k_lookup_depth, grid, dim3(WG), 0, c->stream, c->tb, dk, dc, n, canonical, (int)c->cfg.k, lanes);
    else
      hipLaunchKernelGGL(k_lookup, grid, dim3(WG), 0, c->stream, c->tb, dk, dc, n, canonical, (int)c->cfg.k);
  }
  HIPC(c, hipMemcpyAsync(counts, dc, n * 4, hipMemcpyDeviceToHost, c->stream));
  HIPC(c, hipStreamSynchronize(c->stream));
  return SHK_OK;
}

int shk_neighborhood(shk_ctx *c, const uint64_t *nodes, const uint8_t *dirs, uint64_t n_seeds, uint32_t min_count,
                     uint32_t max_levels, uint64_t *kmers, uint32_t *counts, uint64_t cap, uint64_t *n_out,
                     uint64_t *fringe_nodes, uint8_t *fringe_dirs, uint64_t fringe_cap, uint64_t *n_fringe,
                     uint32_t *levels_done) {
  SHK_TRY(xs_closed(c));
  if (!c || !n_out || !n_fringe || !levels_done || (n_seeds && (!nodes || !dirs))) return SHK_ERR_BAD_ARG;
  SHK_TRY(graph_call_begin(c, "shk_neighborhood"));
  const uint32_t k = c->cfg.k;
  if (k < 2) return fail(c, SHK_ERR_BAD_ARG, "shk_neighborhood needs k >= 2 (a node is a (k-1)-mer), got k=%u", k);
  if ((cap && (!kmers || !counts)) || (fringe_cap && (!fringe_nodes || !fringe_dirs))) return SHK_ERR_BAD_ARG;
  if (cap > (1ull << 32) || fringe_cap > (1ull << 32))
    return fail(c, SHK_ERR_BAD_ARG, "cap %llu / fringe_cap %llu above 2^32", (unsigned long long)cap, (unsigned long long)fringe_cap);
  std::vector<uint64_t> seeds;  // level 0
  SHK_TRY(nb_level0(c, "", nodes, dirs, n_seeds, k, fringe_cap, &seeds));
  // one job of the panel's core: its outputs at the start of the caller's arrays
  const uint64_t at0 = 0;
  return nb_panel_core(c, &seeds, 1, &min_count, nullptr, max_levels, &cap, &fringe_cap, &at0, &at0, kmers, counts, n_out, fringe_nodes,
                       fringe_dirs, n_fringe, levels_done);
}

int shk_pcr_extend(shk_ctx *c, const uint64_t *fwd_kmers, const uint32_t *fwd_counts, uint64_t n_fwd,
                   const uint64_t *rev_kmers, const uint32_t *rev_counts, uint64_t n_rev, const shk_pcr_extend_params *p,
                   uint64_t *node_sub_kmers, uint8_t *node_flags, uint64_t node_cap, uint64_t *n_nodes, uint32_t *edge_src,
                   uint32_t *edge_tgt, uint32_t *edge_counts, uint64_t edge_cap, uint64_t *n_edges, uint32_t *found_path,
                   uint32_t *threshold_used, uint32_t *steps_run) {
  SHK_TRY(xs_closed(c));
  if (!c || !p || !n_nodes || !n_edges || !found_path || !threshold_used || !steps_run) return SHK_ERR_BAD_ARG;
  if ((n_fwd && (!fwd_kmers || !fwd_counts)) || (n_rev && (!rev_kmers || !rev_counts))) return SHK_ERR_BAD_ARG;
  SHK_TRY(graph_call_begin(c, "shk_pcr_extend"));
  const uint32_t k = c->cfg.k;
  if (k < 2) return fail(c, SHK_ERR_BAD_ARG, "shk_pcr_extend needs k >= 2 (a node is a (k-1)-mer), got k=%u", k);
  const uint64_t kmask = ~0ull >> (64 - 2 * k);
  for (uint64_t i = 0; i < n_fwd; ++i)
    if (fwd_kmers[i] > kmask) return fail(c, SHK_ERR_BAD_ARG, "forward primer k-mer %llu is not a %u-mer", (unsigned long long)i, k);
  for (uint64_t i = 0; i < n_rev; ++i)
    if (rev_kmers[i] > kmask) return fail(c, SHK_ERR_BAD_ARG, "reverse primer k-mer %llu is not a %u-mer", (unsigned long long)i, k);
  // a panel of one gene
  const PcrPrimers primers{fwd_kmers, fwd_counts, n_fwd, rev_kmers, rev_counts, n_rev};
  std::vector<PcrGraph> gs;
  std::string msg;
  const int rc = pcr_extend_panel_run(c, k, &primers, 1, p, false, &gs, threshold_used, steps_run, &msg);
  if (rc != SHK_OK) return msg.empty() ? rc : fail(c, rc, "%s", msg.c_str());  // (else the neighbourhood fetch's own text stands)
  uint64_t node_offsets[2], edge_offsets[2];
  const int rc_out = pcr_graphs_out(c, "graph", gs, node_sub_kmers, node_flags, node_offsets, node_cap, edge_src, edge_tgt, edge_counts,
                                    edge_offsets, edge_cap, found_path);
  *n_nodes = node_offsets[1];
  *n_edges = edge_offsets[1];
  return rc_out;
}

// shk_neighborhood_panel, and with job_depths shk_neighborhood_panel_depths (the same call but for the depth check and
// the bounded probe).
static int nb_panel_call(shk_ctx *c, const uint64_t *nodes, const uint8_t *dirs, const uint64_t *seed_offsets, uint32_t n_jobs,
                         const uint32_t *min_counts, const uint32_t *job_depths, uint32_t max_levels, const uint64_t *caps,
                         const uint64_t *fringe_caps, uint64_t *kmers, uint32_t *counts, uint64_t *n_out, uint64_t *fringe_nodes,
                         uint8_t *fringe_dirs, uint64_t *n_fringe, uint32_t *levels_done) {
  SHK_TRY(xs_closed(c));
  using ull = unsigned long long;
  if (!c) return SHK_ERR_BAD_ARG;
  // (at most SHK_PCR_MAX_GENES depths are looked at: a longer list is refused below, by the n_jobs check, whatever its rest holds)
  if (job_depths) SHK_TRY(depth_call_begin(c, "shk_neighborhood_panel_depths", job_depths, std::min<uint32_t>(n_jobs, SHK_PCR_MAX_GENES), false));
  SHK_TRY(graph_call_begin(c, "shk_neighborhood_panel"));
  const uint32_t k = c->cfg.k;
  if (k < 2) return fail(c, SHK_ERR_BAD_ARG, "shk_neighborhood_panel needs k >= 2 (a node is a (k-1)-mer), got k=%u", k);
  if (n_jobs > SHK_PCR_MAX_GENES) return fail(c, SHK_ERR_BAD_ARG, "n_jobs %u above SHK_PCR_MAX_GENES (%u)", n_jobs, (unsigned)SHK_PCR_MAX_GENES);
  if (n_jobs == 0) return SHK_OK;
  if (!seed_offsets || !min_counts || !caps || !fringe_caps || !n_out || !n_fringe || !levels_done) return SHK_ERR_BAD_ARG;
  // every job's arguments before the device is touched
  std::vector<std::vector<uint64_t>> seeds(n_jobs);  // level 0 per job
  std::vector<uint64_t> out_at(n_jobs + 1, 0), fr_at(n_jobs + 1, 0);  // where a job's outputs start in the caller's arrays
  for (uint32_t j = 0; j < n_jobs; ++j) {
    char who[32];
    snprintf(who, sizeof who, "job %u: ", j);
    if (seed_offsets[j + 1] < seed_offsets[j])
      return fail(c, SHK_ERR_BAD_ARG, "%sseed_offsets decrease (%llu after %llu)", who, (ull)seed_offsets[j + 1], (ull)seed_offsets[j]);
    if (caps[j] > (1ull << 32) || fringe_caps[j] > (1ull << 32))
      return fail(c, SHK_ERR_BAD_ARG, "%scap %llu / fringe_cap %llu above 2^32", who, (ull)caps[j], (ull)fringe_caps[j]);
    const uint64_t a = seed_offsets[j], n = seed_offsets[j + 1] - a;
    if (n && (!nodes || !dirs)) return SHK_ERR_BAD_ARG;
    SHK_TRY(nb_level0(c, who, nodes ? nodes + a : nullptr, dirs ? dirs + a : nullptr, n, k, fringe_caps[j], &seeds[j]));
    out_at[j + 1] = out_at[j] + caps[j];
    fr_at[j + 1] = fr_at[j] + fringe_caps[j];
  }
  if ((out_at[n_jobs] && (!kmers || !counts)) || (fr_at[n_jobs] && (!fringe_nodes || !fringe_dirs))) return SHK_ERR_BAD_ARG;
  return nb_panel_core(c, seeds.data(), n_jobs, min_counts, job_depths, max_levels, caps, fringe_caps, out_at.data(), fr_at.data(), kmers,
                       counts, n_out, fringe_nodes, fringe_dirs, n_fringe, levels_done);
}

int shk_neighborhood_panel(shk_ctx *c, const uint64_t *nodes, const uint8_t *dirs, const uint64_t *seed_offsets, uint32_t n_jobs,
                           const uint32_t *min_counts, uint32_t max_levels, const uint64_t *caps, const uint64_t *fringe_caps,
                           uint64_t *kmers, uint32_t *counts, uint64_t *n_out, uint64_t *fringe_nodes, uint8_t *fringe_dirs,
                           uint64_t *n_fringe, uint32_t *levels_done) {
  return nb_panel_call(c, nodes, dirs, seed_offsets, n_jobs, min_counts, nullptr, max_levels, caps, fringe_caps, kmers, counts, n_out,
                       fringe_nodes, fringe_dirs, n_fringe, levels_done);
}

int shk_neighborhood_panel_depths(shk_ctx *c, const uint64_t *nodes, const uint8_t *dirs, const uint64_t *seed_offsets, uint32_t n_jobs,
                                  const uint32_t *min_counts, const uint32_t *job_depths, uint32_t max_levels, const uint64_t *caps,
                                  const uint64_t *fringe_caps, uint64_t *kmers, uint32_t *counts, uint64_t *n_out,
                                  uint64_t *fringe_nodes, uint8_t *fringe_dirs, uint64_t *n_fringe, uint32_t *levels_done) {
  if (c && n_jobs && !job_depths) return SHK_ERR_BAD_ARG;
  static const uint32_t none = 0;  // (n_jobs == 0: the plain call's answer after the depth call's state checks)
  return nb_panel_call(c, nodes, dirs, seed_offsets, n_jobs, min_counts, job_depths ? job_depths : &none, max_levels, caps, fringe_caps,
                       kmers, counts, n_out, fringe_nodes, fringe_dirs, n_fringe, levels_done);
}

// shk_pcr_extend_panel, and with gene_depths shk_pcr_extend_panel_depths.
static int pcr_extend_panel_call(shk_ctx *c, const uint64_t *primer_kmers, const uint32_t *primer_counts, const uint64_t *primer_offsets,
                                 uint32_t n_genes, const shk_pcr_extend_params *params, const uint32_t *gene_depths,
                                 uint64_t *node_sub_kmers, uint8_t *node_flags, uint64_t *node_offsets, uint64_t node_cap,
                                 uint32_t *edge_src, uint32_t *edge_tgt, uint32_t *edge_counts, uint64_t *edge_offsets, uint64_t edge_cap,
                                 uint32_t *found_path, uint32_t *threshold_used, uint32_t *steps_run) {
  SHK_TRY(xs_closed(c));
  using ull = unsigned long long;
  if (!c || !node_offsets || !edge_offsets) return SHK_ERR_BAD_ARG;
  // (as above: the n_genes check below refuses a list longer than SHK_PCR_MAX_GENES)
  if (gene_depths) SHK_TRY(depth_call_begin(c, "shk_pcr_extend_panel_depths", gene_depths, std::min<uint32_t>(n_genes, SHK_PCR_MAX_GENES), false));
  SHK_TRY(graph_call_begin(c, "shk_pcr_extend_panel"));
  const uint32_t k = c->cfg.k;
  if (k < 2) return fail(c, SHK_ERR_BAD_ARG, "shk_pcr_extend_panel needs k >= 2 (a node is a (k-1)-mer), got k=%u", k);
  if (n_genes > SHK_PCR_MAX_GENES) return fail(c, SHK_ERR_BAD_ARG, "n_genes %u above SHK_PCR_MAX_GENES (%u)", n_genes, (unsigned)SHK_PCR_MAX_GENES);
  node_offsets[0] = edge_offsets[0] = 0;
  if (n_genes == 0) return SHK_OK;
  if (!primer_offsets || !params || !found_path || !threshold_used || !steps_run) return SHK_ERR_BAD_ARG;
  const uint64_t kmask = ~0ull >> (64 - 2 * k);
  static const char *const dir_name[2] = {"forward", "reverse"};
  for (uint32_t d = 0; d < 2 * n_genes; ++d) {
    if (primer_offsets[d + 1] < primer_offsets[d])
      return fail(c, SHK_ERR_BAD_ARG, "gene %u, %s set: primer_offsets decrease (%llu after %llu)", d / 2, dir_name[d & 1],
                  (ull)primer_offsets[d + 1], (ull)primer_offsets[d]);
    if (primer_offsets[d + 1] > primer_offsets[d] && (!primer_kmers || !primer_counts)) return SHK_ERR_BAD_ARG;
    for (uint64_t i = primer_offsets[d]; i < primer_offsets[d + 1]; ++i)
      if (primer_kmers[i] > kmask)
        return fail(c, SHK_ERR_BAD_ARG, "gene %u: %s primer k-mer %llu is not a %u-mer", d / 2, dir_name[d & 1],
                    (ull)(i - primer_offsets[d]), k);
  }
  std::vector<PcrPrimers> primers(n_genes);
  for (uint32_t g = 0; g < n_genes; ++g) {
    const uint64_t f0 = primer_offsets[2 * g], r0 = primer_offsets[2 * g + 1], r1 = primer_offsets[2 * g + 2];
    primers[g] = PcrPrimers{primer_kmers + f0, primer_counts + f0, r0 - f0, primer_kmers + r0, primer_counts + r0, r1 - r0};
  }
  std::vector<PcrGraph> gs;
  std::string msg;
  const int rc = pcr_extend_panel_run(c, k, primers.data(), n_genes, params, true, &gs, threshold_used, steps_run, &msg, gene_depths);
  if (rc != SHK_OK) return msg.empty() ? rc : fail(c, rc, "%s", msg.c_str());  // (else shk_neighborhood_panel's own text stands)
  return pcr_graphs_out(c, "panel", gs, node_sub_kmers, node_flags, node_offsets, node_cap, edge_src, edge_tgt, edge_counts, edge_offsets,
                        edge_cap, found_path);
}

int shk_pcr_extend_panel(shk_ctx *c, const uint64_t *primer_kmers, const uint32_t *primer_counts, const uint64_t *primer_offsets,
                         uint32_t n_genes, const shk_pcr_extend_params *params, uint64_t *node_sub_kmers, uint8_t *node_flags,
                         uint64_t *node_offsets, uint64_t node_cap, uint32_t *edge_src, uint32_t *edge_tgt, uint32_t *edge_counts,
                         uint64_t *edge_offsets, uint64_t edge_cap, uint32_t *found_path, uint32_t *threshold_used,
                         uint32_t *steps_run) {
  return pcr_extend_panel_call(c, primer_kmers, primer_counts, primer_offsets, n_genes, params, nullptr, node_sub_kmers, node_flags,
                               node_offsets, node_cap, edge_src, edge_tgt, edge_counts, edge_offsets, edge_cap, found_path, threshold_used,
                               steps_run);
}

int shk_pcr_extend_panel_depths(shk_ctx *c, const uint64_t *primer_kmers, const uint32_t *primer_counts, const uint64_t *primer_offsets,
                                uint32_t n_genes, const shk_pcr_extend_params *params, const uint32_t *gene_depths,
                                uint64_t *node_sub_kmers, uint8_t *node_flags, uint64_t *node_offsets, uint64_t node_cap,
                                uint32_t *edge_src, uint32_t *edge_tgt, uint32_t *edge_counts, uint64_t *edge_offsets, uint64_t edge_cap,
                                uint32_t *found_path, uint32_t *threshold_used, uint32_t *steps_run) {
  if (c && n_genes && !gene_depths) return SHK_ERR_BAD_ARG;
  static const uint32_t none = 0;  // (n_genes == 0: the plain call's answer after the depth call's state checks)
  return pcr_extend_panel_call(c, primer_kmers, primer_counts, primer_offsets, n_genes, params, gene_depths ? gene_depths : &none,
                               node_sub_kmers, node_flags, node_offsets, node_cap, edge_src, edge_tgt, edge_counts, edge_offsets, edge_cap,
                               found_path, threshold_used, steps_run);
}

int shk_find_oligos(shk_ctx *c, const uint64_t *oligos, uint32_t n_oligos, uint32_t oligo_len,
                    uint32_t min_count, uint64_t *kmers, uint32_t *counts, uint64_t cap, uint64_t *n_out) {
  SHK_TRY(xs_closed(c));
  if (c && c->group)
    return each_share_appends(c, kmers, counts, cap, n_out, [&](shk_ctx *s, uint64_t *k, uint32_t *ct, uint64_t room, uint64_t *n) {
      return shk_find_oligos(s, oligos, n_oligos, oligo_len, min_count, k, ct, room, n);
    });
  if (!c || !n_out) return SHK_ERR_BAD_ARG;
  const uint32_t k = c->cfg.k;
  // the reference asserts these (primers.rs:169-186)
  if (n_oligos == 0 || !oligos) return fail(c, SHK_ERR_BAD_ARG, "find_oligos_in_kmers called with no oligos");
  if (!(oligo_len > 0 && oligo_len < k))
    return fail(c, SHK_ERR_BAD_ARG, "oligo length %u out of range for k=%u (must be 1..k-1); trim must be < k",
                oligo_len, k);
  if (n_oligos > 3000) return fail(c, SHK_ERR_BAD_ARG, "too many oligos (%u > 3000)", n_oligos);
  SHK_TRY(table_read_begin(c));
  auto rc_of = [](uint64_t x, int len) {  // reverse complement of a len-base value (host side)
    uint64_t r = 0;
    for (int i = 0; i < len; ++i) {
      r = (r << 2) | (3 - (x & 3));
      x >>= 2;
    }
    return r;
  };
  std::vector<uint64_t> fwd(n_oligos), rc(n_oligos);
  for (uint32_t i = 0; i < n_oligos; ++i) {
    fwd[i] = oligos[i] << (2 * (k - oligo_len));  // primers.rs:189-192
    rc[i] = rc_of(oligos[i], (int)oligo_len);      // primers.rs:206-209
  }
  std::sort(fwd.begin(), fwd.end());
  std::sort(rc.begin(), rc.end());
  Scratch m{c->misc};
  const size_t o_n = m.take<unsigned long long>(1), o_sets = m.take<uint64_t>(2 * (size_t)n_oligos), o_k = m.take<uint64_t>(cap),
               o_c = m.take<uint32_t>(cap);
  HIPC(c, m.ensure());
  unsigned long long *dn = m.at<unsigned long long>(o_n);
  uint64_t *dsets = m.at<uint64_t>(o_sets);  // the forward set, then the reverse-complement set
  uint64_t *dk = m.at<uint64_t>(o_k);
  uint32_t *dc = m.at<uint32_t>(o_c);
  HIPC(c, hipMemsetAsync(dn, 0, 8, c->stream));
  HIPC(c, hipMemcpyAsync(dsets, fwd.data(), (size_t)n_oligos * 8, hipMemcpyHostToDevice, c->stream));
  HIPC(c, hipMemcpyAsync(dsets + n_oligos, rc.data(), (size_t)n_oligos * 8, hipMemcpyHostToDevice, c->stream));
  const auto [s0, s1] = owned_slots(c);
  {
    ScopedTimer t(c, SHK_K_LOOKUP);
    hipLaunchKernelGGL(k_find_oligos, dim3(grid_for(s1 - s0, WG * 8, 2048)), dim3(WG), (size_t)n_oligos * 16,
                       c->stream, c->tb, s0, s1, (int)k, (int)oligo_len, min_count, (const uint64_t *)dsets,
                       (const uint64_t *)(dsets + n_oligos), n_oligos, dk, dc, cap, dn);
  }
  return fetch_appended(c, dn, dk, dc, cap, kmers, counts, n_out);  // (its wait keeps fwd/rc alive until their copies ran)
}

namespace {

// Selection: per primer, level ascending, count descending, k-mer ascending (discover_primer_kmers_by_round's
// sort, primers.rs:407-408, applied round by round), the first max_kmers.  Equal output k-mers are never merged
// here: a table entry x yields x and revcomp(x) (distinct unless x is a palindrome, and then f = r yields it once),
// and two entries never yield the same k-mer because the table holds canonical k-mers only — so the reference's
// "already found at a lower level" filter (primers.rs:398-403) never drops anything.
// all: the records, tagged with the searched primer j; hits: [j][SHK_PRIMER_LEVELS]; searched primer j is result slot
// who[j] (ascending) of n_slots, max_kmers[j] its cap.
void primer_select(const std::vector<PrimerRec> &all, const std::vector<uint64_t> &hits, const std::vector<uint32_t> &who,
                   const std::vector<uint64_t> &max_kmers, uint32_t n_slots, uint64_t *kmers, uint32_t *counts, uint8_t *levels, uint64_t *offsets,
                   uint64_t *level_hits) {
  const uint32_t n = (uint32_t)who.size();
  std::vector<uint64_t> first(n + 1, 0);
  for (const PrimerRec &r : all) ++first[(r.tag >> 8) + 1];
  for (uint32_t j = 0; j < n; ++j) first[j + 1] += first[j];
  std::vector<PrimerRec> by(all.size());
  {
    std::vector<uint64_t> at(first.begin(), first.end() - 1);
    for (const PrimerRec &r : all) by[at[r.tag >> 8]++] = r;
  }
  auto before = [](const PrimerRec &a, const PrimerRec &b) {
    const uint32_t la = a.tag & 0xFF, lb = b.tag & 0xFF;
    if (la != lb) return la < lb;
    if (a.count != b.count) return a.count > b.count;
    return a.kmer < b.kmer;
  };
  uint64_t o = 0;
  uint32_t j = 0;
  for (uint32_t i = 0; i < n_slots; ++i) {
    offsets[i] = o;
    if (j >= n || who[j] != i) continue;
    PrimerRec *b = by.data() + first[j], *e = by.data() + first[j + 1];
    const uint64_t take = std::min<uint64_t>(max_kmers[j], (uint64_t)(e - b));
    std::partial_sort(b, b + take, e, before);
    for (uint64_t t = 0; t < take; ++t, ++o) {
      kmers[o] = b[t].kmer;
      counts[o] = b[t].count;
      levels[o] = (uint8_t)(b[t].tag & 0xFF);
    }
    if (level_hits) std::copy(hits.begin() + (size_t)j * SHK_PRIMER_LEVELS, hits.begin() + (size_t)(j + 1) * SHK_PRIMER_LEVELS,
                              level_hits + (size_t)i * SHK_PRIMER_LEVELS);
    ++j;
  }
  offsets[n_slots] = o;
}

// shk_primer_kmers and shk_primer_kmers_depths: ONE scan over parts × virtual primers j · n_primers + i (primer i in
// block j).  Plain (sweep false): one block, no lane bound, k_primer_scan over the shares of a multi-device context
// (disjoint: the answer is the top of the union) or over the context itself.  Sweep: primer i at depths[j] for D depths
// in one part, the fused k_primer_scan_depths.  Either way: a first pass per part; on an overflow of a part's candidate
// buffer — the counts are complete, so every virtual primer's cut level is known — a rerun of that part, sized exactly.
int primer_scan(shk_ctx *c, const shk_primer *primers, uint32_t n_primers, bool sweep, const uint32_t *depths, uint32_t D, uint64_t *kmers,
                uint32_t *counts, uint8_t *levels, uint64_t cap, uint64_t *offsets, uint64_t *level_hits) {
  using ull = unsigned long long;
  if (!sweep && n_primers >= (1u << 24)) return fail(c, SHK_ERR_BAD_ARG, "too many primers (%u)", n_primers);
  if (sweep && (uint64_t)n_primers * D >= (1u << 24)) return fail(c, SHK_ERR_BAD_ARG, "too many primers (%u at %u depths)", n_primers, D);
  const uint32_t k = c->cfg.k;
  // preprocess_primer_by_mismatch of every direction before any scan (primers.rs:440-450), then the conversion
  // check of the searched ones (their first round, primers.rs:383-393)
  std::vector<PrimerPlan> plans(n_primers);
  std::string msg;
  for (uint32_t i = 0; i < n_primers; ++i) {
    const int rc = primer_plan(&primers[i], k, &plans[i], &msg);
    if (rc != SHK_OK) return fail(c, rc, "%s", msg.c_str());
  }
  for (uint32_t i = 0; i < n_primers; ++i) {
    const int rc = primer_check_chars(plans[i], &msg);
    if (rc != SHK_OK) return fail(c, rc, "%s", msg.c_str());
  }
  uint64_t need = 0;
  for (const PrimerPlan &pl : plans) need += pl.scanned() ? pl.max_kmers : 0;
  need *= D;
  if (cap < need) return fail(c, SHK_ERR_BAD_ARG, sweep ? "cap %llu < n_depths x sum of max_kmers %llu" : "cap %llu < sum of max_kmers %llu", (ull)cap, (ull)need);
  if (need && (!kmers || !counts || !levels)) return SHK_ERR_BAD_ARG;
  const uint32_t n_slots = n_primers * D;
  if (level_hits) std::fill(level_hits, level_hits + (size_t)n_slots * SHK_PRIMER_LEVELS, 0ull);
  std::vector<uint32_t> who1;  // searched primer p = primers[who1[p]]
  std::vector<PrimerDev> dev;
  for (uint32_t i = 0; i < n_primers; ++i)
    if (plans[i].scanned()) {
      const PrimerPlan &pl = plans[i];
      who1.push_back(i);
      // (a sweep: a key whose count at the depth is 0 is not in that depth's table — the floor of 1)
      dev.push_back(PrimerDev{{pl.allow[0], pl.allow[1], pl.allow[2], pl.allow[3]}, pl.L, pl.M, sweep ? std::max(pl.min_count, 1u) : pl.min_count, 0});
    }
  const uint32_t n = (uint32_t)dev.size();
  const size_t nv = (size_t)n * D, n_hits = nv * SHK_PRIMER_LEVELS;
  std::vector<uint32_t> who(nv);  // searched virtual primer j · n + p is result slot j · n_primers + who1[p]
  std::vector<uint64_t> max_kmers(nv);
  for (size_t v = 0; v < nv; ++v) who[v] = (uint32_t)(v / n) * n_primers + who1[v % n], max_kmers[v] = plans[who1[v % n]].max_kmers;
  std::vector<shk_ctx *> parts;
  if (c->group)
    for (uint32_t d = 0; d < c->group->D; ++d) parts.push_back(c->group->ctx[d]);
  else
    parts.push_back(c);
  auto part_fail = [&](int rc, uint32_t d) { return c->group ? group_fail(c, c->group, rc, d) : rc; };
  PrimerDepths dep{};
  for (uint32_t j = 0; sweep && j < D; ++j) dep.d[dep.n++] = depths[j];
  // one pass over a part keeping, of virtual primer v, the levels 0..cut[v]
  auto pass = [&](shk_ctx *part, const std::vector<uint32_t> &cut, uint64_t room, std::vector<PrimerRec> *recs, std::vector<uint64_t> *hits,
                  uint64_t *n_total) {
    uint32_t stride = 1;  // LDS counters per virtual primer: levels 0..max cut
    for (const uint32_t m : cut) stride = std::max(stride, m + 1);
    if (!sweep) {
      std::vector<PrimerDev> pd = dev;
      for (uint32_t p = 0; p < n; ++p) pd[p].M = cut[p];
      // primers per launch: their table and counters in 48 KiB of LDS (three workgroups per CU)
      const uint32_t per_primer = (uint32_t)sizeof(PrimerDev) + 4 * stride;
      return primer_pass(part, pd, n_hits, (48u << 10) / per_primer, room, recs, hits, n_total,
                         [&](dim3 grid, auto s0, auto s1, const PrimerDev *dp, uint32_t nb, uint32_t b, PrimerRec *drec, ull *dn, ull *dhits) {
                           hipLaunchKernelGGL(k_primer_scan, grid, dim3(WG), (size_t)nb * per_primer, part->stream, part->tb, s0, s1, (int)part->cfg.k,
                                              dp, nb, b, stride, drec, room, dn, dhits);
                         });
    }
    std::vector<PrimerDevD> pd(n);
    for (uint32_t p = 0; p < n; ++p) {
      pd[p].p = dev[p];
      pd[p].p.M = 0;
      for (uint32_t j = 0; j < SHK_PCR_MAX_DEPTHS; ++j) {
        const uint32_t m = j < D ? cut[(size_t)j * n + p] : 0u;
        pd[p].cut[j] = (uint8_t)m;
        pd[p].p.M = std::max(pd[p].p.M, m);
      }
    }
    // primers per launch group: their table and D × the counters in 48 KiB of LDS (three workgroups per CU)
    const uint32_t per_primer = (uint32_t)sizeof(PrimerDevD) + 4 * stride * D;
    return primer_pass(part, pd, n_hits, std::max(1u, (48u << 10) / per_primer), room, recs, hits, n_total,
                       [&](dim3 grid, auto s0, auto s1, const PrimerDevD *dp, uint32_t nb, uint32_t b, PrimerRec *drec, ull *dn, ull *dhits) {
                         hipLaunchKernelGGL(k_primer_scan_depths, grid, dim3(WG), (size_t)nb * per_primer, part->stream, part->tb, s0, s1,
                                            (int)part->cfg.k, dp, nb, b, n, stride, dep, drec, room, dn, dhits);
                       });
  };
  std::vector<PrimerRec> all;
  std::vector<uint64_t> hits(n_hits, 0);
  if (n) {
    const uint64_t room = (uint64_t)std::max(env_int("SHK_PRIMER_CANDIDATES", 1 << 18), 1);
    std::vector<std::vector<uint64_t>> part_hits(parts.size());
    std::vector<uint64_t> part_n(parts.size());
    std::vector<PrimerRec> recs;
    std::vector<uint32_t> cut(nv);
    for (size_t v = 0; v < nv; ++v) cut[v] = dev[v % n].M;
    // a pass over part d whose records are appended to `all` (straight into it while it is empty: no copy with one part)
    auto pass_into_all = [&](uint32_t d, uint64_t room_d, std::vector<uint64_t> *hits_d, uint64_t *n_d) {
      if (all.empty()) return pass(parts[d], cut, room_d, &all, hits_d, n_d);
      const int rc = pass(parts[d], cut, room_d, &recs, hits_d, n_d);
      all.insert(all.end(), recs.begin(), recs.end());
      return rc;
    };
    for (uint32_t d = 0; d < parts.size(); ++d) {
      const int rc = pass_into_all(d, room, &part_hits[d], &part_n[d]);
      if (rc != SHK_OK) return part_fail(rc, d);
      for (size_t j = 0; j < n_hits; ++j) hits[j] += part_hits[d][j];
    }
    // A part overflowed.  The cut level of a virtual primer: the first level at which its hits, over all parts, reach
    // max_kmers.  Nothing above it can be selected: the parts that overflowed run again keeping levels ≤ cut, sized exactly.
    const bool overflowed = std::any_of(part_n.begin(), part_n.end(), [&](uint64_t x) { return x > room; });
    for (size_t v = 0; overflowed && v < nv; ++v) {
      uint64_t acc = 0;
      for (uint32_t m = 0; m <= dev[v % n].M; ++m) {
        acc += hits[v * SHK_PRIMER_LEVELS + m];
        if (acc >= max_kmers[v]) {
          cut[v] = m;
          break;
        }
      }
    }
    for (uint32_t d = 0; d < parts.size(); ++d) {
      if (part_n[d] <= room) continue;
      uint64_t exact = 0;
      for (size_t v = 0; v < nv; ++v)
        for (uint32_t m = 0; m <= cut[v]; ++m) exact += part_hits[d][v * SHK_PRIMER_LEVELS + m];
      std::vector<uint64_t> h2;
      uint64_t n2 = 0;
      const int rc = pass_into_all(d, exact, &h2, &n2);
      if (rc != SHK_OK) return part_fail(rc, d);
      if (n2 != exact) return fail(c, SHK_ERR_INVARIANT, "primer scan rerun produced %llu records, expected %llu", (ull)n2, (ull)exact);
    }
  }
  primer_select(all, hits, who, max_kmers, n_slots, kmers, counts, levels, offsets, level_hits);
  return SHK_OK;
}

}  // namespace

int shk_primer_kmers(shk_ctx *c, const shk_primer *primers, uint32_t n_primers, uint64_t *kmers, uint32_t *counts,
                     uint8_t *levels, uint64_t cap, uint64_t *offsets, uint64_t *level_hits) {
  SHK_TRY(xs_closed(c));
  if (!c || (n_primers && !primers) || !offsets) return SHK_ERR_BAD_ARG;
  return primer_scan(c, primers, n_primers, false, nullptr, 1, kmers, counts, levels, cap, offsets, level_hits);
}

int shk_primer_kmers_depths(shk_ctx *c, const shk_primer *primers, uint32_t n_primers, const uint32_t *depths, uint32_t n_depths,
                            uint64_t *kmers, uint32_t *counts, uint8_t *levels, uint64_t cap, uint64_t *offsets, uint64_t *level_hits) {
  SHK_TRY(xs_closed(c));
  if (!c || (n_primers && !primers) || !offsets) return SHK_ERR_BAD_ARG;
  SHK_TRY(depth_call_begin(c, "shk_primer_kmers_depths", depths, n_depths, true));
  return primer_scan(c, primers, n_primers, true, depths, n_depths, kmers, counts, levels, cap, offsets, level_hits);
}

int shk_table_geometry(shk_ctx *c, uint64_t *n_pages, uint32_t *page_slots, uint32_t *n_lanes) {
  SHK_TRY(xs_closed(c));
  SHK_TRY(single_device_only(c));
  HIPC(c, hipSetDevice(c->cfg.device));
  SHK_TRY(settle(c));  // a pending spill may still grow the table
  if (n_pages) *n_pages = 1ull << c->tb.log_pages;
  if (page_slots) *page_slots = PAGE_SLOTS;
  if (n_lanes) *n_lanes = c->n_lanes;
  return SHK_OK;
}

int shk_table_reserve_pages(shk_ctx *c, uint64_t n_pages) {
  SHK_TRY(xs_closed(c));
  SHK_TRY(single_device_only(c));
  HIPC(c, hipSetDevice(c->cfg.device));
  SHK_TRY(settle(c));  // (no tb_fresh: grow_to carries nothing over from a table that was still to be cleared)
  uint32_t lp = 0;
  while ((1ull << lp) < n_pages) lp++;
  c->finalized = c->hist_ready = false;
  return grow_to(c, lp);
}

int shk_table_device_ptrs(shk_ctx *c, void **d_keys, void **d_vals) {
  SHK_TRY(xs_closed(c));
  SHK_TRY(single_device_only(c));
  SHK_TRY(table_read_begin(c));
  HIPC(c, hipStreamSynchronize(c->stream));
  if (d_keys) *d_keys = c->tb.keys;
  if (d_vals) *d_vals = c->tb.vals;
  return SHK_OK;
}

int shk_merge_pages(shk_ctx *c, uint64_t p0, uint64_t p1, const void *d_keys, const void *d_vals,
                    uint64_t vals_lane_stride) {
  SHK_TRY(xs_closed(c));
  SHK_TRY(single_device_only(c));
  if (p1 <= p0) return SHK_OK;
  SHK_TRY(table_read_begin(c));
  c->finalized = c->hist_ready = false;
  c->zero_count_keys = true;  // (a peer's table may hold keys inserted with count 0: keep reading the keys)
  const uint64_t n_slots = (p1 - p0) << PAGE_LOG;
  // worst case every peer key is new here
  HIPC(c, c->spillA.ensure(n_slots * c->n_lanes * 16));
  SpillRef sp = spill_ref(c->spillA, n_slots * c->n_lanes);
  HIPC(c, hipMemsetAsync(&c->d_stats->spill_count, 0, sizeof(unsigned long long), c->stream));
  {
    ScopedTimer t(c, SHK_K_MERGE);
    hipLaunchKernelGGL(k_merge, dim3(grid_for(n_slots, WG, 8192)), dim3(WG), 0, c->stream, c->tb,
                       n_slots, vals_lane_stride, (const uint64_t *)d_keys, (const uint32_t *)d_vals,
                       c->d_stats, sp, 0ull, ~0u);
  }
  SHK_TRY(read_stats(c));
  return drain_spill(c, n_slots * c->n_lanes);
}

int shk_owner_counts(shk_ctx *c, uint32_t n_owners, uint64_t *counts) {
  SHK_TRY(xs_closed(c));
  SHK_TRY(single_device_only(c));
  if (!counts || n_owners == 0) return SHK_ERR_BAD_ARG;
  SHK_TRY(owner_split_check(c, n_owners));
  SHK_TRY(table_read_begin(c));
  Scratch m{c->misc};
  const size_t o_c = m.take<unsigned long long>(n_owners);
  HIPC(c, m.ensure());
  unsigned long long *dc = m.at<unsigned long long>(o_c);
  HIPC(c, hipMemsetAsync(dc, 0, (size_t)n_owners * 8, c->stream));
  const uint32_t bpo = owner_blocks(n_owners);
  hipLaunchKernelGGL(k_owner_counts, dim3(n_owners * bpo), dim3(WG), 0, c->stream, c->tb,
                     c->tb.cap / n_owners, bpo, dc);
  HIPC(c, hipMemcpyAsync(counts, dc, (size_t)n_owners * 8, hipMemcpyDeviceToHost, c->stream));
  HIPC(c, hipStreamSynchronize(c->stream));
  return SHK_OK;
}

// (No settle, unlike table_read_begin: the exact-count protocol calls this behind shk_owner_counts, which settled, with
// nothing launched in between — the segment offsets it is given were worked out from those counts.)
int shk_compact_owners(shk_ctx *c, uint32_t n_owners, const uint64_t *seg_offsets, void *d_keys, void *d_vals,
                       uint64_t vals_lane_stride, int32_t skip_owner) {
  SHK_TRY(xs_closed(c));
  SHK_TRY(single_device_only(c));
  if (!seg_offsets || n_owners == 0) return SHK_ERR_BAD_ARG;
  SHK_TRY(owner_split_check(c, n_owners));
  HIPC(c, hipSetDevice(c->cfg.device));
  SHK_TRY(tb_fresh(c));
  SHK_TRY(compact_owners_launch(c, n_owners, seg_offsets, nullptr, d_keys, d_vals, vals_lane_stride, skip_owner, 0ull, nullptr));
  HIPC(c, hipStreamSynchronize(c->stream));  // the caller hands the buffers to a collective next
  return SHK_OK;
}

// (No settle either, for the same reason: `counts` are shk_owner_counts' answer.)
int shk_compact_owners_packed(shk_ctx *c, uint32_t n_owners, const uint64_t *counts, void *d_buf, int32_t skip_owner) {
  SHK_TRY(xs_closed(c));
  SHK_TRY(single_device_only(c));
  if (!counts || n_owners == 0) return SHK_ERR_BAD_ARG;
  SHK_TRY(owner_split_check(c, n_owners));
  HIPC(c, hipSetDevice(c->cfg.device));
  SHK_TRY(tb_fresh(c));
  HIPC(c, c->h_rebased[0].ensure((size_t)n_owners * 16));  // offsets and counts staged through pinned memory
  uint64_t *h = (uint64_t *)c->h_rebased[0].p;
  uint64_t run = 0;
  for (uint32_t o = 0; o < n_owners; ++o) {
    h[o] = run;
    h[n_owners + o] = counts[o];
    run += counts[o];
  }
  SHK_TRY(compact_owners_launch(c, n_owners, h, h + n_owners, d_buf, nullptr, 0, skip_owner, 0ull, nullptr));
  HIPC(c, hipGetLastError());
  return SHK_OK;  // (asynchronous on the context's stream: run the collective on shk_stream())
}

int shk_compact_owners_fixed(shk_ctx *c, uint32_t n_owners, uint64_t capacity, void *d_buf, int32_t skip_owner) {
  SHK_TRY(xs_closed(c));
  SHK_TRY(single_device_only(c));
  if (n_owners == 0 || capacity == 0 || !d_buf) return SHK_ERR_BAD_ARG;
  SHK_TRY(owner_split_check(c, n_owners));
  HIPC(c, hipSetDevice(c->cfg.device));
  if (c->acc_active) SHK_TRY(settle(c));  // records still waiting for their page pass
  // (Otherwise nothing is waited for: a counting launch nobody has looked at yet may have spilled records, in which
  // case the table read here is incomplete — k_piece_headers sees that on the device and poisons every header, no
  // rank merges anything, and the finalize that follows repairs the table before the exchange is repeated.)
  // (One exception: a table left virtual by the last launch is written here, and that does wait — the launch is looked
  // at, the materialising pass runs and is settled.  Once per context at the most: it writes its tables eagerly after.)
  SHK_TRY(tb_fresh(c));
  HIPC(c, c->h_rebased[0].ensure((size_t)n_owners * 16));
  uint64_t *h = (uint64_t *)c->h_rebased[0].p;
  for (uint32_t o = 0; o < n_owners; ++o) {
    h[o] = (uint64_t)o * capacity;  // every piece at its fixed place
    h[n_owners + o] = capacity;
  }
  const size_t piece_bytes = 8 + capacity * (8 + 4 * (size_t)c->n_lanes);
  // unused places read as EMPTY k-mers, which the merge skips
  HIPC(c, hipMemsetAsync(d_buf, 0xFF, (size_t)n_owners * piece_bytes, c->stream));
  HIPC(c, hipMemsetAsync(&c->d_stats->scratch[1], 0, 16, c->stream));  // [1]: fullest range here, [2]: … anywhere (merge)
  SHK_TRY(compact_owners_launch(c, n_owners, h, h + n_owners, d_buf, nullptr, 0, skip_owner, 8ull, &c->d_stats->scratch[1]));
  hipLaunchKernelGGL(k_piece_headers, dim3((n_owners + 63) / 64), dim3(64), 0, c->stream, (uint32_t *)d_buf, n_owners,
                     (unsigned long long)(piece_bytes / 4), (const DevStats *)c->d_stats);
  HIPC(c, hipGetLastError());
  return SHK_OK;
}

int shk_merge_pieces_max(shk_ctx *c, uint64_t *max_count) {
  SHK_TRY(xs_closed(c));
  if (!c || !max_count) return SHK_ERR_BAD_ARG;
  if (c->group) return fail(c, SHK_ERR_STATE, "not available on a multi-device context");
  HIPC(c, hipSetDevice(c->cfg.device));
  if (!c->finalized && !c->hist_ready) SHK_TRY(read_stats(c));  // (a finalize has just brought the control block back otherwise)
  *max_count = c->h_stats->scratch[2];
  return SHK_OK;
}

static int merge_launch(shk_ctx *c, const void *d_keys, const void *d_vals, uint64_t n, uint64_t vals_lane_stride,
                        uint64_t piece_cap, uint32_t skip_piece);

int shk_merge_entries(shk_ctx *c, const void *d_keys, const void *d_vals, uint64_t n, uint64_t vals_lane_stride) {
  SHK_TRY(xs_closed(c));
  SHK_TRY(single_device_only(c));
  if (n == 0) return SHK_OK;
  return merge_launch(c, d_keys, d_vals, n, vals_lane_stride, 0, ~0u);
}

int shk_merge_pieces(shk_ctx *c, const void *d_buf, uint32_t n_pieces, uint64_t capacity, int32_t skip_piece) {
  SHK_TRY(xs_closed(c));
  SHK_TRY(single_device_only(c));
  if (!d_buf) return SHK_ERR_BAD_ARG;
  if (n_pieces == 0 || capacity == 0) return SHK_OK;
  return merge_launch(c, d_buf, nullptr, (uint64_t)n_pieces * capacity, capacity, capacity, skip_piece < 0 ? ~0u : (uint32_t)skip_piece);
}

static int merge_launch(shk_ctx *c, const void *d_keys, const void *d_vals, uint64_t n, uint64_t vals_lane_stride,
                        uint64_t piece_cap, uint32_t skip_piece) {
  HIPC(c, hipSetDevice(c->cfg.device));
  SHK_TRY(tb_fresh(c));  // (a virtual table is written and settled here: a host round trip, once per context at the most)
  // (Not table_read_begin: the settle depends on ride_on.)
  // Fixed-capacity pieces behind a counting launch nobody has looked at yet: nothing is waited for.  If that
  // launch spilled, the senders' headers are poisoned and k_merge touches nothing; if not, what the merge spills
  // goes on the same list (same capacity, the counter runs on) and the finalize that follows repairs it.
  // (Only when that list could take the merge's own worst case — every entry spilling on every lane, which is what
  // W pieces' worth of new keys do to pages sized for the local shard alone: k_merge drops what does not fit the list,
  // and the settle that follows would fail the job with "spill list overflow" where the exact-count protocol would
  // have finished.  A counting launch's list has a place per k-mer of the launch, so this holds whenever the pieces
  // are no larger than the batch.)
  const bool ride_on = piece_cap && c->unsettled && !c->acc_active && c->unsettled_spill_cap >= n * c->n_lanes &&
                       c->spillA.cap >= c->unsettled_spill_cap * 16;
  if (!ride_on) SHK_TRY(settle(c));
  c->finalized = c->hist_ready = false;
  c->zero_count_keys = true;  // (a peer's table may hold keys inserted with count 0: keep reading the keys)
  const uint64_t spill_cap = ride_on ? c->unsettled_spill_cap : n * c->n_lanes;  // worst case every entry spills on every lane
  if (!ride_on) {
    HIPC(c, c->spillA.ensure(spill_cap * 16));
    HIPC(c, hipMemsetAsync(&c->d_stats->spill_count, 0, sizeof(unsigned long long), c->stream));
  }
  SpillRef sp = spill_ref(c->spillA, spill_cap);
  {
    ScopedTimer t(c, SHK_K_MERGE);
    hipLaunchKernelGGL(k_merge, dim3(grid_for(n, WG, 8192)), dim3(WG), 0, c->stream, c->tb, n, vals_lane_stride,
                       (const uint64_t *)d_keys, (const uint32_t *)d_vals, c->d_stats, sp, piece_cap, skip_piece);
  }
  // (nothing is waited for: the outcome — spilled entries, load factor — is looked at by the next call that
  // needs the table, at the latest finalize)
  c->unsettled = true;
  c->unsettled_spill_cap = spill_cap;
  return SHK_OK;
}

int shk_set_owned_pages(shk_ctx *c, uint64_t p0, uint64_t p1) {
  SHK_TRY(xs_closed(c));
  SHK_TRY(single_device_only(c));
  if (p1 < p0 || p1 > (1ull << c->tb.log_pages)) return fail(c, SHK_ERR_BAD_ARG, "bad page range");
  c->own_p0 = p0;
  c->own_p1 = p1;
  c->own_set = true;
  c->own_share_n = 0;
  c->finalized = c->hist_ready = false;
  return SHK_OK;
}

int shk_set_owner_share(shk_ctx *c, uint32_t n_owners, uint32_t owner) {
  SHK_TRY(xs_closed(c));
  SHK_TRY(single_device_only(c));
  if (n_owners == 0 || (n_owners & (n_owners - 1)) || owner >= n_owners || n_owners > (1ull << c->tb.log_pages))
    return fail(c, SHK_ERR_BAD_ARG, "bad owner share %u of %u", owner, n_owners);
  c->own_share_n = n_owners;  // (no settle: the range is worked out from the page count of the moment a scan is launched)
  c->own_share_id = owner;
  c->own_set = true;
  c->finalized = c->hist_ready = false;
  return SHK_OK;
}

}  // extern "C"
