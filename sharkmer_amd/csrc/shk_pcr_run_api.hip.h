// shk_pcr_run_api.hip.h — shk_pcr_run (included by shk_engine.hip, same translation unit, behind the stage files whose
// calls and cores it runs): do_pcr for every gene of a panel (src/pcr/mod.rs:431-819) as run_pcr drives it
// (src/stats.rs:84-98), the genes side by side — each stage once for the genes still alive.  No kernel
// of its own: the primer scan, the extension's fetches, the panel filter, the prune, the threading and the dedup are the
// stage calls', launched through shk_primer_kmers, shk_pcr_extend_panel, panel_core, shk_pcr_prune_panel,
// thread_panel_core and shk_pcr_products_panel.  The two read-side stages share ONE opened batch.
namespace {

// Slices [off[g], off[g + 1]) of src for the genes of sel, back to back.
template <class T>
void pcr_gather(const T *src, const std::vector<uint64_t> &off, const std::vector<uint32_t> &sel, std::vector<T> *dst) {
  dst->clear();
  for (const uint32_t g : sel) dst->insert(dst->end(), src + off[g], src + off[g + 1]);
}
std::vector<uint64_t> pcr_gather_offsets(const std::vector<uint64_t> &off, const std::vector<uint32_t> &sel) {
  std::vector<uint64_t> o(sel.size() + 1, 0);
  for (size_t i = 0; i < sel.size(); ++i) o[i + 1] = o[i] + (off[sel[i] + 1] - off[sel[i]]);
  return o;
}

// KmerCounts::get_median_count (counting.rs:275-298) of a primer set's counts
uint32_t pcr_median_count(const uint32_t *counts, uint64_t n) {
  if (!n) return 0;
  std::vector<uint32_t> v(counts, counts + n);
  std::sort(v.begin(), v.end());
  const uint64_t mid = n / 2;
  return n % 2 == 0 ? v[mid - 1] / 2 + v[mid] / 2 : v[mid];
}

uint64_t pcr_canonical(uint64_t x, uint32_t k) {
  uint64_t r = 0, y = x;
  for (uint32_t i = 0; i < k; ++i, y >>= 2) r = (r << 2) | (3 - (y & 3));
  return std::min(x, r);
}

template <class T>
void pcr_fill(T *p, uint32_t n, T v) {
  if (p) std::fill(p, p + n, v);
}

int pcr_run_impl(shk_ctx *c, const shk_pcr_gene *genes, uint32_t ng, const shk_pcr_run_params *p, shk_pcr_run_out *out) {
  using ull = unsigned long long;
  const uint32_t k = c->cfg.k;
  shk_pcr_records &R = out->records;
  R.n_records = R.n_seq_bytes = 0;
  std::fill(R.record_offsets, R.record_offsets + ng + 1, 0ull);
  pcr_fill(R.paths_found, ng, (uint64_t)0), pcr_fill(R.generated, ng, (uint64_t)0), pcr_fill(R.states_explored, ng, (uint64_t)0);
  pcr_fill(out->n_fwd_kmers, ng, 0u), pcr_fill(out->n_rev_kmers, ng, 0u), pcr_fill(out->max_fwd_count, ng, 0u), pcr_fill(out->max_rev_count, ng, 0u);
  pcr_fill(out->median_primer_count, ng, 0u), pcr_fill(out->threshold_used, ng, 0u), pcr_fill(out->steps_run, ng, 0u), pcr_fill(out->found_path, ng, 0u);
  pcr_fill(out->n_nodes, ng, (uint64_t)0), pcr_fill(out->n_edges, ng, (uint64_t)0), pcr_fill(out->n_pruned_nodes, ng, (uint64_t)0);
  pcr_fill(out->n_pruned_edges, ng, (uint64_t)0), pcr_fill(out->n_reads_matched, ng, (uint64_t)0), pcr_fill(out->n_paired_links, ng, (uint64_t)0);
  pcr_fill(out->threaded, ng, (uint8_t)0), pcr_fill(out->low_primer_counts, ng, (uint8_t)0);
  pcr_fill(out->status, ng, (uint32_t)SHK_PCR_NO_PATH);

  // ---- everything that is refused, the first in gene order, before the device is touched ----
  if (ng > SHK_PCR_MAX_GENES) return fail(c, SHK_ERR_BAD_ARG, "n_genes %u above SHK_PCR_MAX_GENES (%u)", ng, (unsigned)SHK_PCR_MAX_GENES);
  if (p->reads > SHK_PCR_READS_HOST) return fail(c, SHK_ERR_BAD_ARG, "shk_pcr_run: reads = %u is none of SHK_PCR_READS_*", p->reads);
  // per gene, the first in gene order wins: validate_pcr_params (mod.rs:295-399; the gene's first failure), the name taken
  // by an earlier gene (cli.rs:572-581), then get_primer_kmers' own errors in its order (primers.rs:440-478): too many
  // variants forward, reverse, then an invalid character forward, reverse — one batched shk_primer_kmers call would
  // report every gene's variants before any gene's characters.  Step 1's clamp is here too (cli.rs:556-570).
  const uint32_t floor = std::max(p->min_kmer_count, 1u);
  std::vector<shk_primer> primers(2 * (size_t)ng);
  std::vector<uint32_t> min_count(ng);
  uint64_t primer_cap = 0;
  for (uint32_t g = 0; g < ng; ++g) {
    char text[1024];
    if (shk_pcr_validate_gene(&genes[g], text, sizeof text) != 0) {
      if (char *nl = strchr(text, '\n')) *nl = 0;
      return fail(c, SHK_ERR_BAD_ARG, "gene %u '%s': %s", g, genes[g].gene_name ? genes[g].gene_name : "", text);
    }
    for (uint32_t h = 0; h < g; ++h)
      if (!strcmp(genes[g].gene_name, genes[h].gene_name)) return fail(c, SHK_ERR_BAD_ARG, "Duplicate gene name '%s'", genes[g].gene_name);
    min_count[g] = std::max(genes[g].min_count, floor);
    primers[2 * g] = shk_primer{genes[g].forward_seq, genes[g].trim, genes[g].mismatches, min_count[g], genes[g].max_primer_kmers};
    primers[2 * g + 1] = shk_primer{genes[g].reverse_seq, genes[g].trim, genes[g].mismatches, min_count[g], genes[g].max_primer_kmers};
    primer_cap += 2 * (uint64_t)genes[g].max_primer_kmers;
    char ef[512], er[512];
    uint32_t tl = 0, nl = 0;
    uint64_t nv[SHK_PRIMER_LEVELS];
    const int rf = shk_primer_compile(&primers[2 * g], k, &tl, &nl, nv, ef, sizeof ef);
    const int rr = shk_primer_compile(&primers[2 * g + 1], k, &tl, &nl, nv, er, sizeof er);
    const char *why = rf == SHK_ERR_BAD_ARG ? ef : rr == SHK_ERR_BAD_ARG ? er : rf != SHK_OK ? ef : rr != SHK_OK ? er : nullptr;
    const int code = rf == SHK_ERR_BAD_ARG ? rf : rr == SHK_ERR_BAD_ARG ? rr : rf != SHK_OK ? rf : rr;
    if (why) return fail(c, code, "gene %u '%s': %s", g, genes[g].gene_name, why);
  }
  SHK_TRY(graph_call_begin(c, "shk_pcr_extend_panel"));
  // A multi-device context (SHK_FLAG_GROUP_GRAPH): the calls that take the context take it as it is — the primer scan
  // goes over the shares, the extension through the share directory, prune and products on the first device — and the
  // read-side cores run on the lead share rd, the device the public read calls use; on0: their error text to the context.
  shk_ctx *rd = c->group ? c->group->ctx[0] : c;
  auto on0 = [&](int rc) { return rc == SHK_OK || !c->group ? rc : group_fail(c, c->group, rc, 0); };
  const bool host = p->reads == SHK_PCR_READS_HOST, retained = p->reads == SHK_PCR_READS_RETAINED;
  // … and with SHK_FLAG_GROUP_READS too, over retained reads, every share runs them over its own store
  const bool shared_reads = retained && c->group;
  if (retained && !retain_is_on(c)) return fail(c, SHK_ERR_STATE, "shk_pcr_run: reads are not retained (shk_retain_reads)");
  const uint64_t *read_index = host ? p->read_index : nullptr;
  const uint8_t *mate = host ? p->mate : nullptr;
  if ((read_index == nullptr) != (mate == nullptr))
    return fail(c, SHK_ERR_BAD_ARG, "read_index and mate go together: both (thread_reads_paired) or neither (thread_reads)");
  uint64_t host_max_len = 0;
  if (host && p->n_seqs) {
    if (!p->offsets) return fail(c, SHK_ERR_BAD_ARG, "shk_pcr_run: offsets is missing");
    SHK_TRY(batch_check_offsets(c, p->offsets, p->n_seqs, p->offsets[p->n_seqs], "shk_pcr_run", &host_max_len));
    if (p->offsets[p->n_seqs] && !p->bases) return fail(c, SHK_ERR_BAD_ARG, "shk_pcr_run: bases is missing");
    for (uint64_t i = 0; mate && i < p->n_seqs; ++i)
      if (mate[i] > 2) return fail(c, SHK_ERR_BAD_ARG, "mate[%llu] = %u: 0 unpaired, 1 R1, 2 R2", (ull)i, mate[i]);
  }
  const bool mate_rule = !mate && p->paired && p->reads != SHK_PCR_READS_NONE;
  if (ng == 0) return SHK_OK;

  // ---- step 2: the primer k-mers of the whole panel in one table pass ----
  std::vector<uint64_t> pk(std::max<uint64_t>(primer_cap, 1)), poff(2 * (size_t)ng + 1, 0);
  std::vector<uint32_t> pc(pk.size());
  std::vector<uint8_t> plev(pk.size());
  SHK_TRY(shk_primer_kmers(c, primers.data(), 2 * ng, pk.data(), pc.data(), plev.data(), primer_cap, poff.data(), nullptr));
  uint64_t budget = p->max_num_nodes;
  if (!budget) {  // main.rs:147-165
    shk_counters cn{};
    SHK_TRY(shk_get_counters(c, &cn));
    budget = shk_pcr_node_budget(cn.n_bases_ingested);
  }
  std::vector<uint32_t> status(ng, SHK_PCR_NO_PATH), alive;  // alive: both sets found
  for (uint32_t g = 0; g < ng; ++g) {
    const uint64_t nf = poff[2 * g + 1] - poff[2 * g], nr = poff[2 * g + 2] - poff[2 * g + 1];
    const uint32_t mf = nf ? *std::max_element(pc.begin() + poff[2 * g], pc.begin() + poff[2 * g + 1]) : 0;
    const uint32_t mr = nr ? *std::max_element(pc.begin() + poff[2 * g + 1], pc.begin() + poff[2 * g + 2]) : 0;
    if (out->n_fwd_kmers) out->n_fwd_kmers[g] = (uint32_t)nf;
    if (out->n_rev_kmers) out->n_rev_kmers[g] = (uint32_t)nr;
    if (out->max_fwd_count) out->max_fwd_count[g] = mf;
    if (out->max_rev_count) out->max_rev_count[g] = mr;
    if (!nf || !nr) {  // mod.rs:446-468: nothing more for this gene
      status[g] = !nf && !nr ? SHK_PCR_NO_PRIMERS : !nf ? SHK_PCR_NO_FORWARD : SHK_PCR_NO_REVERSE;
      continue;
    }
    if (out->median_primer_count)
      out->median_primer_count[g] = std::min(pcr_median_count(pc.data() + poff[2 * g], nf), pcr_median_count(pc.data() + poff[2 * g + 1], nr));
    if (out->low_primer_counts) out->low_primer_counts[g] = mf < 5 || mr < 5;  // mod.rs:752-759
    alive.push_back(g);
  }
  const uint32_t na = (uint32_t)alive.size();

  // ---- step 3: the reads, opened once for the filter and the threading; the alive genes' lists ----
  ReadBatch batch{};
  bool have_batch = false;
  std::vector<uint64_t> moff(na + 1, 0);  // per alive gene
  std::unique_ptr<uint64_t[]> mreads;
  if (na && p->reads != SHK_PCR_READS_NONE) {
    if (host && p->n_seqs) {
      SHK_TRY(on0(batch_from_host(rd, p->bases, p->offsets, p->n_seqs, host_max_len, &batch)));  // the one upload of the batch
      have_batch = true;
    } else if (retained) {
      if (shared_reads) {
        SHK_TRY(group_retained_begin(c, "shk_pcr_run"));
        batch.n_seqs = c->group->reads_dir.total();  // (no batch is opened here: the shares open theirs)
        have_batch = batch.n_seqs > 0;
      } else {
        SHK_TRY(retained_begin(c, "shk_pcr_run"));
      }
      if (!shared_reads && c->retain.n_reads) {
        SHK_TRY(batch_from_retained(c, "shk_pcr_run", &batch));
        have_batch = true;
      }
    }
  }
  if (have_batch) {
    std::vector<uint64_t> fk, foff(na + 1, 0);
    for (uint32_t a = 0; a < na; ++a) {  // from_primer_kmers (read_filter.rs:24-41): the canonical forms of both sets
      const uint32_t g = alive[a];
      for (uint64_t j = poff[2 * g]; j < poff[2 * g + 2]; ++j) fk.push_back(pcr_canonical(pk[j], k));
      foff[a + 1] = fk.size();
    }
    HostKeyRuns pl;
    SHK_TRY(on0(panel_plan(rd, fk.data(), foff.data(), na, &pl)));
    uint64_t cap = std::min<uint64_t>(batch.n_seqs * na, 1ull << 22), n_matches = 0;
    for (int attempt = 0; attempt < 2 && !pl.items.empty(); ++attempt) {
      mreads.reset(new uint64_t[std::max<uint64_t>(cap, 1)]);
      std::fill(moff.begin(), moff.end(), 0ull);
      const int rc = shared_reads ? group_filter_retained(c, pl, na, moff.data(), mreads.get(), cap, &n_matches)
                                  : on0(panel_core(rd, pl, na, batch, moff.data(), mreads.get(), cap, &n_matches));
      if (rc == SHK_ERR_BAD_ARG && attempt == 0 && n_matches > cap) {  // (a panel whose lists outgrow 2^22 entries: once more, with room)
        cap = n_matches;
        continue;
      }
      SHK_TRY(rc);
      break;
    }
    for (uint32_t a = 0; a < na && out->n_reads_matched; ++a) out->n_reads_matched[alive[a]] = moff[a + 1] - moff[a];
  }

  // ---- step 4: the extension of the alive genes ----
  std::vector<uint64_t> xsub, xnoff(na + 1, 0), xeoff(na + 1, 0);
  std::vector<uint8_t> xflags;
  std::vector<uint32_t> xes, xet, xec, xfound(std::max(na, 1u), 0), xthr(std::max(na, 1u), 0), xsteps(std::max(na, 1u), 0);
  std::vector<uint32_t> found;  // positions in alive of the genes whose last step found a path
  if (na) {
    std::vector<uint64_t> ak, aoff(2 * (size_t)na + 1, 0);
    std::vector<uint32_t> ac;
    std::vector<shk_pcr_extend_params> xp(na);
    for (uint32_t a = 0; a < na; ++a) {
      const uint32_t g = alive[a];
      ak.insert(ak.end(), pk.begin() + poff[2 * g], pk.begin() + poff[2 * g + 2]);
      ac.insert(ac.end(), pc.begin() + poff[2 * g], pc.begin() + poff[2 * g + 2]);
      aoff[2 * a + 1] = aoff[2 * a] + (poff[2 * g + 1] - poff[2 * g]);
      aoff[2 * a + 2] = aoff[2 * a] + (poff[2 * g + 2] - poff[2 * g]);
      xp[a] = shk_pcr_extend_params{min_count[g], p->min_kmer_count, genes[g].high_coverage_ratio, budget, 1u, 0u};
    }
    uint64_t node_cap = 4096ull * na, edge_cap = 8192ull * na;
    for (int attempt = 0;; ++attempt) {
      xsub.resize(node_cap), xflags.resize(node_cap), xes.resize(edge_cap), xet.resize(edge_cap), xec.resize(edge_cap);
      const int rc = shk_pcr_extend_panel(c, ak.data(), ac.data(), aoff.data(), na, xp.data(), xsub.data(), xflags.data(), xnoff.data(), node_cap,
                                          xes.data(), xet.data(), xec.data(), xeoff.data(), edge_cap, xfound.data(), xthr.data(), xsteps.data());
      if (rc == SHK_ERR_BAD_ARG && attempt == 0 && (xnoff[na] > node_cap || xeoff[na] > edge_cap)) {  // the offsets say what it needs
        node_cap = std::max(node_cap, xnoff[na]), edge_cap = std::max(edge_cap, xeoff[na]);
        continue;
      }
      SHK_TRY(rc);
      break;
    }
    for (uint32_t a = 0; a < na; ++a) {
      const uint32_t g = alive[a];
      const uint64_t nn = xnoff[a + 1] - xnoff[a];
      if (out->threshold_used) out->threshold_used[g] = xthr[a];
      if (out->steps_run) out->steps_run[g] = xsteps[a];
      if (out->found_path) out->found_path[g] = xfound[a];
      if (out->n_nodes) out->n_nodes[g] = nn;
      if (out->n_edges) out->n_edges[g] = xeoff[a + 1] - xeoff[a];
      status[g] = nn >= budget ? SHK_PCR_NODE_BUDGET : SHK_PCR_NO_PATH;  // step 5 (mod.rs:567, 621-623)
      if (xfound[a]) found.push_back(a);
    }
  }
  const uint32_t nf = (uint32_t)found.size();

  // ---- step 6, for the genes with a path: prune, thread, products ----
  int products_rc = SHK_OK;
  if (nf) {
    std::vector<uint64_t> fsub, fnoff = pcr_gather_offsets(xnoff, found), feoff = pcr_gather_offsets(xeoff, found);
    std::vector<uint8_t> fflags;
    std::vector<uint32_t> fes, fet, fec;
    pcr_gather(xsub.data(), xnoff, found, &fsub), pcr_gather(xflags.data(), xnoff, found, &fflags);
    pcr_gather(xes.data(), xeoff, found, &fes), pcr_gather(xet.data(), xeoff, found, &fet), pcr_gather(xec.data(), xeoff, found, &fec);
    std::vector<shk_pcr_prune_params> pp(nf);
    for (uint32_t f = 0; f < nf; ++f) pp[f] = shk_pcr_prune_params{genes[alive[found[f]]].tip_coverage_fraction, 3u, 0u};
    const uint64_t nn = fnoff[nf], ne = feoff[nf];
    std::vector<uint8_t> keep(std::max<uint64_t>(nn, 1)), qflags(std::max<uint64_t>(nn, 1));
    std::vector<uint64_t> qsub(std::max<uint64_t>(nn, 1)), qnoff(nf + 1, 0), qeoff(nf + 1, 0);
    std::vector<uint32_t> qes(std::max<uint64_t>(ne, 1)), qet(qes.size()), qec(qes.size());
    std::vector<double> qratio(qes.size());
    shk_pcr_prune_out po{};
    po.node_keep = keep.data(), po.out_node_offsets = qnoff.data(), po.out_edge_offsets = qeoff.data();
    po.node_sub_kmers = qsub.data(), po.node_flags = qflags.data(), po.node_cap = nn;
    po.edge_src = qes.data(), po.edge_tgt = qet.data(), po.edge_counts = qec.data(), po.coverage_ratio = qratio.data(), po.edge_cap = ne;
    SHK_TRY(shk_pcr_prune_panel(c, fsub.data(), fflags.data(), fnoff.data(), fes.data(), fet.data(), fec.data(), feoff.data(), nf, pp.data(), &po));
    // the threaded genes: reads were given and the gene's list is not empty (mod.rs:664-697)
    std::vector<uint32_t> thr;  // positions in found
    for (uint32_t f = 0; f < nf && have_batch; ++f)
      if (moff[found[f] + 1] > moff[found[f]]) thr.push_back(f);
    const uint32_t nt = (uint32_t)thr.size();
    std::vector<uint8_t> has(nf, 0);
    std::vector<uint32_t> stot(std::max<uint64_t>(qeoff[nf], 1), 0), suna(stot.size(), 0), lin, lout, lcnt;
    std::vector<uint64_t> loff(nf + 1, 0);
    if (nt) {
      std::vector<uint64_t> tsub, tnoff = pcr_gather_offsets(qnoff, thr), teoff = pcr_gather_offsets(qeoff, thr), tloff(nt + 1, 0), tlist;
      std::vector<uint32_t> tes, tet;
      pcr_gather(qsub.data(), qnoff, thr, &tsub), pcr_gather(qes.data(), qeoff, thr, &tes), pcr_gather(qet.data(), qeoff, thr, &tet);
      for (uint32_t t = 0; t < nt; ++t) {
        const uint32_t a = found[thr[t]];
        tlist.insert(tlist.end(), mreads.get() + moff[a], mreads.get() + moff[a + 1]);
        tloff[t + 1] = tlist.size();
      }
      std::vector<uint32_t> ttot(std::max<uint64_t>(teoff[nt], 1), 0), tuna(ttot.size(), 0);
      shk_thread_panel_out shape{};
      shape.support_total = ttot.data(), shape.support_unambiguous = tuna.data();
      ThreadPanelPlan tp;
      SHK_TRY(on0(thread_panel_plan(rd, tsub.data(), tnoff.data(), tes.data(), tet.data(), teoff.data(), nt, batch.n_seqs, tloff.data(), tlist.data(),
                                read_index, mate, &shape, &tp)));
      ThreadPanelResult res{ttot.data(), tuna.data(), nullptr, {}, {}, {}, {}, {}};
      if (shared_reads)
        SHK_TRY(group_thread_retained(c, tp, nt, tloff.data(), tlist.data(), read_index, mate, mate_rule, &res));
      else
        SHK_TRY(on0(thread_panel_core(rd, tp, nt, batch, tloff.data(), tlist.data(), read_index, mate, &res, mate_rule)));
      for (uint32_t t = 0, f = 0; f < nf; ++f) {  // into the layout of the pruned panel
        loff[f + 1] = loff[f];
        if (t == nt || thr[t] != f) continue;
        has[f] = 1;
        std::copy(ttot.begin() + teoff[t], ttot.begin() + teoff[t + 1], stot.begin() + qeoff[f]);
        std::copy(tuna.begin() + teoff[t], tuna.begin() + teoff[t + 1], suna.begin() + qeoff[f]);
        lin.insert(lin.end(), res.link_in.begin() + res.link_off[t], res.link_in.begin() + res.link_off[t + 1]);
        lout.insert(lout.end(), res.link_out.begin() + res.link_off[t], res.link_out.begin() + res.link_off[t + 1]);
        lcnt.insert(lcnt.end(), res.link_counts.begin() + res.link_off[t], res.link_counts.begin() + res.link_off[t + 1]);
        loff[f + 1] = lin.size();
        const uint32_t g = alive[found[f]];
        if (out->threaded) out->threaded[g] = 1;
        if (out->n_paired_links) out->n_paired_links[g] = res.n_paired[t];
        ++t;
      }
    }
    // the products, with annotations exactly for the threaded genes
    shk_pcr_graphs G{};
    G.n_genes = nf;
    G.node_sub_kmers = qsub.data(), G.node_flags = qflags.data(), G.node_offsets = qnoff.data();
    G.edge_src = qes.data(), G.edge_tgt = qet.data(), G.edge_counts = qec.data(), G.coverage_ratio = qratio.data(), G.edge_offsets = qeoff.data();
    lin.resize(std::max<size_t>(lin.size(), 1)), lout.resize(lin.size()), lcnt.resize(lin.size());
    if (nt) {
      G.support_total = stot.data(), G.support_unambiguous = suna.data(), G.link_offsets = loff.data();
      G.link_in = lin.data(), G.link_out = lout.data(), G.link_counts = lcnt.data(), G.has_threading = has.data();
    }
    std::vector<shk_pcr_paths_params> path_p(nf);
    std::vector<uint32_t> dedup_t(nf);
    for (uint32_t f = 0; f < nf; ++f) {
      const shk_pcr_gene &ge = genes[alive[found[f]]];
      path_p[f] = shk_pcr_paths_params{ge.min_length, ge.max_length, ge.max_dfs_states, ge.max_paths_per_pair, ge.max_node_visits};
      dedup_t[f] = ge.dedup_edit_threshold;
    }
    std::vector<uint64_t> roff(nf + 1, 0), paths_found(nf, 0), generated(nf, 0), states(nf, 0);
    shk_pcr_records loc = R;  // the caller's record arrays and capacities; the per-gene arrays are this call's
    loc.record_offsets = roff.data(), loc.paths_found = paths_found.data(), loc.generated = generated.data(), loc.states_explored = states.data();
    products_rc = shk_pcr_products_panel(c, &G, path_p.data(), dedup_t.data(), &loc, nullptr, nullptr);
    if (products_rc != SHK_OK && !(products_rc == SHK_ERR_BAD_ARG && (loc.n_records > R.record_cap || loc.n_seq_bytes > R.seq_cap))) return products_rc;
    R.n_records = loc.n_records, R.n_seq_bytes = loc.n_seq_bytes;
    for (uint32_t f = 0; f < nf; ++f) {
      const uint32_t g = alive[found[f]];
      R.record_offsets[g + 1] = roff[f + 1] - roff[f];  // (lengths; summed below)
      if (R.paths_found) R.paths_found[g] = paths_found[f];
      if (R.generated) R.generated[g] = generated[f];
      if (R.states_explored) R.states_explored[g] = states[f];
      if (out->n_pruned_nodes) out->n_pruned_nodes[g] = qnoff[f + 1] - qnoff[f];
      if (out->n_pruned_edges) out->n_pruned_edges[g] = qeoff[f + 1] - qeoff[f];
      if (generated[f]) status[g] = SHK_PCR_SUCCESS;  // mod.rs:735-743; otherwise the reason of step 5 stays
    }
    for (uint32_t g = 0; g < ng; ++g) R.record_offsets[g + 1] += R.record_offsets[g];
  }
  std::copy(status.begin(), status.end(), out->status);
  if (getenv("SHK_TRACE"))  // (read at each call, like the stages' lines)
    for (uint32_t g = 0; g < ng; ++g)
      fprintf(stderr, "[shk] pcr_run: gene %u '%s': %s, primer k-mers %llu + %llu, threshold %u after %u steps, %llu nodes, %llu edges, %llu reads matched%s, %llu products\n",
              g, genes[g].gene_name, status[g] == SHK_PCR_SUCCESS ? "success" : shk_pcr_failure_reason(status[g]),
              (ull)(poff[2 * g + 1] - poff[2 * g]), (ull)(poff[2 * g + 2] - poff[2 * g + 1]), out->threshold_used ? out->threshold_used[g] : 0u,
              out->steps_run ? out->steps_run[g] : 0u, (ull)(out->n_nodes ? out->n_nodes[g] : 0), (ull)(out->n_edges ? out->n_edges[g] : 0),
              (ull)(out->n_reads_matched ? out->n_reads_matched[g] : 0), out->threaded && out->threaded[g] ? ", threaded" : "",
              (ull)(R.record_offsets[g + 1] - R.record_offsets[g]));
  return products_rc;  // (SHK_OK, or the record capacities' SHK_ERR_BAD_ARG with everything per gene complete)
}

}  // namespace

extern "C" int shk_pcr_run(shk_ctx *c, const shk_pcr_gene *genes, uint32_t n_genes, const shk_pcr_run_params *params, shk_pcr_run_out *out) {
  SHK_TRY(xs_closed(c));
  if (!c || !params || !out || !out->status || !out->records.record_offsets || (n_genes && !genes)) return SHK_ERR_BAD_ARG;
  try {
    return pcr_run_impl(c, genes, n_genes, params, out);
  } catch (...) {  // no exception leaves the C ABI
    return fail(c, SHK_ERR_NOMEM, "shk_pcr_run: out of host memory");
  }
}
