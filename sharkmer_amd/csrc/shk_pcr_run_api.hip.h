// shk_pcr_run_api.hip.h — shk_pcr_run and shk_pcr_run_depths (included by shk_engine.hip, same translation unit, behind
// the stage files whose calls and cores it runs): do_pcr for every gene of a panel (src/pcr/mod.rs:431-819) as run_pcr
// drives it (src/stats.rs:84-98), the genes side by side — each stage once for the genes still alive.
// ONE pipeline (pcr_pipeline) over the virtual genes v = j · ng + g of D output blocks: shk_pcr_run is D = 1 on the table
// as it is, shk_pcr_run_depths gene g at depths[j].  No kernel of its own: the primer scan, the
// extension's fetches, the panel filter, the prune, the threading and the dedup are the stage calls', launched through
// shk_primer_kmers[_depths], shk_pcr_extend_panel[_depths], panel_core, shk_pcr_prune_panel, thread_panel_core and
// shk_pcr_products_panel.  The two read-side stages share ONE opened batch.
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

// A run's outputs before anything is known: no records, every per-gene figure 0, every status NO_PATH.
void pcr_out_clear(shk_pcr_run_out *out, uint32_t ng) {
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
}

// The host checks of a panel, the first gene in gene order that fails one, and what the primer scan takes: gene g's two
// directions at primers[2g], primers[2g + 1] with the clamped min_count[g]; *primer_cap = Σ 2 · max_primer_kmers.
int pcr_genes_check(shk_ctx *c, const shk_pcr_gene *genes, uint32_t ng, const shk_pcr_run_params *p, std::vector<shk_primer> *primers_out,
                    std::vector<uint32_t> *min_count_out, uint64_t *primer_cap_out) {
  // per gene, the first in gene order wins: validate_pcr_params (mod.rs:295-399; the gene's first failure), the name taken
  // by an earlier gene (cli.rs:572-581), then get_primer_kmers' own errors in its order (primers.rs:440-478): too many
  // variants forward, reverse, then an invalid character forward, reverse — one batched shk_primer_kmers call would
  // report every gene's variants before any gene's characters.  Step 1's clamp is here too (cli.rs:556-570).
  const uint32_t k = c->cfg.k, floor = std::max(p->min_kmer_count, 1u);
  std::vector<shk_primer> &primers = *primers_out;
  std::vector<uint32_t> &min_count = *min_count_out;
  primers.resize(2 * (size_t)ng), min_count.resize(ng);
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
  *primer_cap_out = primer_cap;
  return SHK_OK;
}

// ---- the stages of the pipeline: each is handed its virtual genes gathered ----

// Step 4's output: the extended graphs of the alive genes back to back, and per gene what the sweep reports.
struct PcrExtended {
  std::vector<uint64_t> sub, noff, eoff;
  std::vector<uint8_t> flags;
  std::vector<uint32_t> es, et, ec, found, thr, steps;
  explicit PcrExtended(uint32_t na) : noff(na + 1, 0), eoff(na + 1, 0), found(std::max(na, 1u), 0), thr(std::max(na, 1u), 0), steps(std::max(na, 1u), 0) {}
};
// Step 4's call for na genes: shk_pcr_extend_panel, or with gene_depths its depth form, with room that grows once to what
// the offsets say it needs.
int pcr_extend_stage(shk_ctx *c, const std::vector<uint64_t> &ak, const std::vector<uint32_t> &ac, const std::vector<uint64_t> &aoff, uint32_t na,
                     const std::vector<shk_pcr_extend_params> &xp, const uint32_t *gene_depths, PcrExtended *x) {
  uint64_t node_cap = 4096ull * na, edge_cap = 8192ull * na;
  for (int attempt = 0;; ++attempt) {
    x->sub.resize(node_cap), x->flags.resize(node_cap), x->es.resize(edge_cap), x->et.resize(edge_cap), x->ec.resize(edge_cap);
    const int rc =
        gene_depths ? shk_pcr_extend_panel_depths(c, ak.data(), ac.data(), aoff.data(), na, xp.data(), gene_depths, x->sub.data(), x->flags.data(),
                                                  x->noff.data(), node_cap, x->es.data(), x->et.data(), x->ec.data(), x->eoff.data(), edge_cap,
                                                  x->found.data(), x->thr.data(), x->steps.data())
                    : shk_pcr_extend_panel(c, ak.data(), ac.data(), aoff.data(), na, xp.data(), x->sub.data(), x->flags.data(), x->noff.data(), node_cap,
                                           x->es.data(), x->et.data(), x->ec.data(), x->eoff.data(), edge_cap, x->found.data(), x->thr.data(),
                                           x->steps.data());
    if (rc == SHK_ERR_BAD_ARG && attempt == 0 && (x->noff[na] > node_cap || x->eoff[na] > edge_cap)) {  // the offsets say what it needs
      node_cap = std::max(node_cap, x->noff[na]), edge_cap = std::max(edge_cap, x->eoff[na]);
      continue;
    }
    return rc;
  }
}

// Step 6's pruned graphs of the genes with a path, back to back (the layout shk_pcr_products_panel takes).
struct PcrPruned {
  std::vector<uint64_t> sub, noff, eoff;
  std::vector<uint8_t> flags;
  std::vector<uint32_t> es, et, ec;
  std::vector<double> ratio;
};
// The prune of the graphs `found` (positions in x) under tip[f], one shk_pcr_prune_panel call.
int pcr_prune_stage(shk_ctx *c, const PcrExtended &x, const std::vector<uint32_t> &found, const std::vector<double> &tip, PcrPruned *q) {
  const uint32_t nf = (uint32_t)found.size();
  std::vector<uint64_t> fsub, fnoff = pcr_gather_offsets(x.noff, found), feoff = pcr_gather_offsets(x.eoff, found);
  std::vector<uint8_t> fflags;
  std::vector<uint32_t> fes, fet, fec;
  pcr_gather(x.sub.data(), x.noff, found, &fsub), pcr_gather(x.flags.data(), x.noff, found, &fflags);
  pcr_gather(x.es.data(), x.eoff, found, &fes), pcr_gather(x.et.data(), x.eoff, found, &fet), pcr_gather(x.ec.data(), x.eoff, found, &fec);
  std::vector<shk_pcr_prune_params> pp(nf);
  for (uint32_t f = 0; f < nf; ++f) pp[f] = shk_pcr_prune_params{tip[f], 3u, 0u};
  const uint64_t nn = fnoff[nf], ne = feoff[nf];
  std::vector<uint8_t> keep(std::max<uint64_t>(nn, 1));
  q->flags.assign(std::max<uint64_t>(nn, 1), 0), q->sub.assign(std::max<uint64_t>(nn, 1), 0), q->noff.assign(nf + 1, 0), q->eoff.assign(nf + 1, 0);
  q->es.assign(std::max<uint64_t>(ne, 1), 0), q->et.assign(q->es.size(), 0), q->ec.assign(q->es.size(), 0), q->ratio.assign(q->es.size(), 0.0);
  shk_pcr_prune_out po{};
  po.node_keep = keep.data(), po.out_node_offsets = q->noff.data(), po.out_edge_offsets = q->eoff.data();
  po.node_sub_kmers = q->sub.data(), po.node_flags = q->flags.data(), po.node_cap = nn;
  po.edge_src = q->es.data(), po.edge_tgt = q->et.data(), po.edge_counts = q->ec.data(), po.coverage_ratio = q->ratio.data(), po.edge_cap = ne;
  return shk_pcr_prune_panel(c, fsub.data(), fflags.data(), fnoff.data(), fes.data(), fet.data(), fec.data(), feoff.data(), nf, pp.data(), &po);
}

// What shk_pcr_products_panel takes per gene, for the genes fgene (indices into genes).
void pcr_products_params(const shk_pcr_gene *genes, const std::vector<uint32_t> &fgene, std::vector<shk_pcr_paths_params> *path_p,
                         std::vector<uint32_t> *dedup_t) {
  path_p->resize(fgene.size()), dedup_t->resize(fgene.size());
  for (size_t f = 0; f < fgene.size(); ++f) {
    const shk_pcr_gene &ge = genes[fgene[f]];
    (*path_p)[f] = shk_pcr_paths_params{ge.min_length, ge.max_length, ge.max_dfs_states, ge.max_paths_per_pair, ge.max_node_visits};
    (*dedup_t)[f] = ge.dedup_edit_threshold;
  }
}

// The SHK_TRACE line of virtual gene v (gene g of o): shk_pcr_run's, or with a depth shk_pcr_run_depths'.
void pcr_trace_line(const shk_pcr_gene &gene, uint32_t g, uint32_t status, uint64_t n_fwd, uint64_t n_rev, const shk_pcr_run_out &o, uint32_t depth) {
  using ull = unsigned long long;
  const char *what = status == SHK_PCR_SUCCESS ? "success" : shk_pcr_failure_reason(status);
  if (depth) {
    fprintf(stderr, "[shk] pcr_run_depths: depth %u gene %u '%s': %s, primer k-mers %llu + %llu\n", depth, g, gene.gene_name, what, (ull)n_fwd, (ull)n_rev);
    return;
  }
  fprintf(stderr, "[shk] pcr_run: gene %u '%s': %s, primer k-mers %llu + %llu, threshold %u after %u steps, %llu nodes, %llu edges, %llu reads matched%s, %llu products\n",
          g, gene.gene_name, what, (ull)n_fwd, (ull)n_rev, o.threshold_used ? o.threshold_used[g] : 0u, o.steps_run ? o.steps_run[g] : 0u,
          (ull)(o.n_nodes ? o.n_nodes[g] : 0), (ull)(o.n_edges ? o.n_edges[g] : 0), (ull)(o.n_reads_matched ? o.n_reads_matched[g] : 0),
          o.threaded && o.threaded[g] ? ", threaded" : "", (ull)(o.records.record_offsets[g + 1] - o.records.record_offsets[g]));
}

// The pipeline of shk_pcr_run and shk_pcr_run_depths over the virtual genes v = j · ng + g: gene g into
// slot g of outs[j], each stage called once for the virtual genes still alive.
//   plain (sweep false): D = 1 — outs is the caller's one block, the table as it is, any of the three read modes, the
//     records written by the products call straight into the caller's arrays;
//   sweep: gene g at depths[j] for D depths, no reads, the records into arrays of this call's and from there dealt out to
//     every outs[j] under that block's own capacities.
int pcr_pipeline(shk_ctx *c, const shk_pcr_gene *genes, uint32_t ng, const shk_pcr_run_params *p, bool sweep, const uint32_t *depths,
                 uint32_t D, shk_pcr_run_out *outs) {
  using ull = unsigned long long;
  const uint32_t k = c->cfg.k;
  // ---- everything that is refused, the first in gene order, before the device is touched: each entry point in its order ----
  if (sweep) {
    SHK_TRY(depth_call_begin(c, "shk_pcr_run_depths", depths, D, true));
    for (uint32_t j = 0; j < D; ++j)
      if (!outs[j].status || !outs[j].records.record_offsets) return SHK_ERR_BAD_ARG;
    if ((uint64_t)ng * D > SHK_PCR_MAX_GENES)
      return fail(c, SHK_ERR_BAD_ARG, "n_genes %u x n_depths %u above SHK_PCR_MAX_GENES (%u)", ng, D, (unsigned)SHK_PCR_MAX_GENES);
    for (uint32_t j = 0; j < D; ++j) pcr_out_clear(&outs[j], ng);
    if (p->reads != SHK_PCR_READS_NONE) return fail(c, SHK_ERR_BAD_ARG, "shk_pcr_run_depths: a depth sweep takes no reads");
  } else {
    pcr_out_clear(outs, ng);
    if (ng > SHK_PCR_MAX_GENES) return fail(c, SHK_ERR_BAD_ARG, "n_genes %u above SHK_PCR_MAX_GENES (%u)", ng, (unsigned)SHK_PCR_MAX_GENES);
    if (p->reads > SHK_PCR_READS_HOST) return fail(c, SHK_ERR_BAD_ARG, "shk_pcr_run: reads = %u is none of SHK_PCR_READS_*", p->reads);
  }
  std::vector<shk_primer> primers;
  std::vector<uint32_t> min_count;
  uint64_t primer_cap = 0;
  SHK_TRY(pcr_genes_check(c, genes, ng, p, &primers, &min_count, &primer_cap));
  if (!sweep) SHK_TRY(graph_call_begin(c, "shk_pcr_extend_panel"));
  // A multi-device context (SHK_FLAG_GROUP_GRAPH): the calls that take the context take it as it is — the primer scan
  // goes over the shares, the extension through the share directory, prune and products on the first device — and the
  // read-side cores run on the lead share rd, the device the public read calls use; on0: their error text to the context.
  shk_ctx *rd = c->group ? c->group->ctx[0] : c;
  auto on0 = [&](int rc) { return rc == SHK_OK || !c->group ? rc : group_fail(c, c->group, rc, 0); };
  // (a sweep has reads = NONE: none of the checks of the reads below can refuse it)
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
  const uint32_t nv = ng * D;

  // ---- step 2: the primer k-mers of every virtual gene in one table pass (a sweep: the fused one): slot 2v + direction ----
  primer_cap *= D;
  std::vector<uint64_t> pk(std::max<uint64_t>(primer_cap, 1)), poff(2 * (size_t)nv + 1, 0);
  std::vector<uint32_t> pc(pk.size());
  std::vector<uint8_t> plev(pk.size());
  SHK_TRY(sweep ? shk_primer_kmers_depths(c, primers.data(), 2 * ng, depths, D, pk.data(), pc.data(), plev.data(), primer_cap, poff.data(), nullptr)
                : shk_primer_kmers(c, primers.data(), 2 * ng, pk.data(), pc.data(), plev.data(), primer_cap, poff.data(), nullptr));
  std::vector<uint64_t> budget(D, p->max_num_nodes);  // per block
  if (!p->max_num_nodes && sweep) {  // main.rs:147-165 on the bases of the chunks below the depth
    std::vector<uint64_t> cb(c->n_lanes);
    SHK_TRY(shk_chunk_bases(c, cb.data()));
    uint64_t sum = 0;
    for (uint32_t j = 0, l = 0; j < D; ++j) {
      for (; l < depths[j]; ++l) sum += cb[l];
      budget[j] = shk_pcr_node_budget(sum);
    }
  } else if (!p->max_num_nodes) {  // main.rs:147-165
    shk_counters cn{};
    SHK_TRY(shk_get_counters(c, &cn));
    budget[0] = shk_pcr_node_budget(cn.n_bases_ingested);
  }
  std::vector<uint32_t> status(nv, SHK_PCR_NO_PATH), alive;  // alive: both sets found
  for (uint32_t v = 0; v < nv; ++v) {
    shk_pcr_run_out &o = outs[v / ng];
    const uint32_t g = v % ng;
    const uint64_t nf = poff[2 * v + 1] - poff[2 * v], nr = poff[2 * v + 2] - poff[2 * v + 1];
    const uint32_t mf = nf ? *std::max_element(pc.begin() + poff[2 * v], pc.begin() + poff[2 * v + 1]) : 0;
    const uint32_t mr = nr ? *std::max_element(pc.begin() + poff[2 * v + 1], pc.begin() + poff[2 * v + 2]) : 0;
    if (o.n_fwd_kmers) o.n_fwd_kmers[g] = (uint32_t)nf;
    if (o.n_rev_kmers) o.n_rev_kmers[g] = (uint32_t)nr;
    if (o.max_fwd_count) o.max_fwd_count[g] = mf;
    if (o.max_rev_count) o.max_rev_count[g] = mr;
    if (!nf || !nr) {  // mod.rs:446-468: nothing more for this gene
      status[v] = !nf && !nr ? SHK_PCR_NO_PRIMERS : !nf ? SHK_PCR_NO_FORWARD : SHK_PCR_NO_REVERSE;
      continue;
    }
    if (o.median_primer_count)
      o.median_primer_count[g] = std::min(pcr_median_count(pc.data() + poff[2 * v], nf), pcr_median_count(pc.data() + poff[2 * v + 1], nr));
    if (o.low_primer_counts) o.low_primer_counts[g] = mf < 5 || mr < 5;  // mod.rs:752-759
    alive.push_back(v);
  }
  const uint32_t na = (uint32_t)alive.size();

  // ---- step 3 (never in a sweep): the reads, opened once for the filter and the threading; the alive genes' lists ----
  ReadBatch batch{};
  bool have_batch = false;
  std::vector<uint64_t> moff;  // per alive gene, with a batch
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
      const uint32_t v = alive[a];
      for (uint64_t j = poff[2 * v]; j < poff[2 * v + 2]; ++j) fk.push_back(pcr_canonical(pk[j], k));
      foff[a + 1] = fk.size();
    }
    HostKeyRuns pl;
    SHK_TRY(on0(panel_plan(rd, fk.data(), foff.data(), na, &pl)));
    uint64_t cap = std::min<uint64_t>(batch.n_seqs * na, 1ull << 22), n_matches = 0;
    moff.assign(na + 1, 0);
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
    for (uint32_t a = 0; a < na; ++a)
      if (uint64_t *matched = outs[alive[a] / ng].n_reads_matched) matched[alive[a] % ng] = moff[a + 1] - moff[a];
  }

  // ---- step 4: the extension of the alive virtual genes, in a sweep each at its depth ----
  PcrExtended X(na);
  const std::vector<uint64_t> &xnoff = X.noff, &xeoff = X.eoff;
  const std::vector<uint32_t> &xfound = X.found, &xthr = X.thr, &xsteps = X.steps;
  std::vector<uint32_t> found;  // positions in alive of the virtual genes whose last step found a path
  if (na) {
    std::vector<uint64_t> ak, aoff(2 * (size_t)na + 1, 0);
    std::vector<uint32_t> ac, adepth(sweep ? na : 0);
    std::vector<shk_pcr_extend_params> xp(na);
    for (uint32_t a = 0; a < na; ++a) {
      const uint32_t v = alive[a], g = v % ng;
      ak.insert(ak.end(), pk.begin() + poff[2 * v], pk.begin() + poff[2 * v + 2]);
      ac.insert(ac.end(), pc.begin() + poff[2 * v], pc.begin() + poff[2 * v + 2]);
      aoff[2 * a + 1] = aoff[2 * a] + (poff[2 * v + 1] - poff[2 * v]);
      aoff[2 * a + 2] = aoff[2 * a] + (poff[2 * v + 2] - poff[2 * v]);
      xp[a] = shk_pcr_extend_params{min_count[g], p->min_kmer_count, genes[g].high_coverage_ratio, budget[v / ng], 1u, 0u};
      if (sweep) adepth[a] = depths[v / ng];
    }
    SHK_TRY(pcr_extend_stage(c, ak, ac, aoff, na, xp, sweep ? adepth.data() : nullptr, &X));
    for (uint32_t a = 0; a < na; ++a) {
      const uint32_t v = alive[a], g = v % ng;
      shk_pcr_run_out &o = outs[v / ng];
      const uint64_t nn = xnoff[a + 1] - xnoff[a];
      if (o.threshold_used) o.threshold_used[g] = xthr[a];
      if (o.steps_run) o.steps_run[g] = xsteps[a];
      if (o.found_path) o.found_path[g] = xfound[a];
      if (o.n_nodes) o.n_nodes[g] = nn;
      if (o.n_edges) o.n_edges[g] = xeoff[a + 1] - xeoff[a];
      status[v] = nn >= budget[v / ng] ? SHK_PCR_NODE_BUDGET : SHK_PCR_NO_PATH;  // step 5 (mod.rs:567, 621-623)
      if (xfound[a]) found.push_back(a);
    }
  }
  const uint32_t nf = (uint32_t)found.size();

  // ---- step 6, for the virtual genes with a path: one prune, the threading where reads were given, one products call ----
  int short_rc = SHK_OK;
  if (nf) {
    std::vector<uint32_t> fgene(nf);  // the gene of every virtual gene with a path
    std::vector<double> tip(nf);
    for (uint32_t f = 0; f < nf; ++f) fgene[f] = alive[found[f]] % ng, tip[f] = genes[fgene[f]].tip_coverage_fraction;
    PcrPruned Q;
    SHK_TRY(pcr_prune_stage(c, X, found, tip, &Q));
    std::vector<uint64_t> &qsub = Q.sub, &qnoff = Q.noff, &qeoff = Q.eoff;
    std::vector<uint8_t> &qflags = Q.flags;
    std::vector<uint32_t> &qes = Q.es, &qet = Q.et, &qec = Q.ec;
    std::vector<double> &qratio = Q.ratio;
    // the threaded genes: reads were given and the gene's list is not empty (mod.rs:664-697)
    std::vector<uint32_t> thr;  // positions in found
    for (uint32_t f = 0; f < nf && have_batch; ++f)
      if (moff[found[f] + 1] > moff[found[f]]) thr.push_back(f);
    const uint32_t nt = (uint32_t)thr.size();
    std::vector<uint8_t> has;  // the annotations in the layout of the pruned panel: sized only where a gene is threaded
    std::vector<uint32_t> stot, suna, lin, lout, lcnt;
    std::vector<uint64_t> loff;
    if (nt) {
      has.assign(nf, 0), stot.assign(std::max<uint64_t>(qeoff[nf], 1), 0), suna.assign(stot.size(), 0), loff.assign(nf + 1, 0);
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
        shk_pcr_run_out &o = outs[alive[found[f]] / ng];
        if (o.threaded) o.threaded[fgene[f]] = 1;
        if (o.n_paired_links) o.n_paired_links[fgene[f]] = res.n_paired[t];
        ++t;
      }
    }
    // the products, with annotations exactly for the threaded genes
    shk_pcr_graphs G{};
    G.n_genes = nf;
    G.node_sub_kmers = qsub.data(), G.node_flags = qflags.data(), G.node_offsets = qnoff.data();
    G.edge_src = qes.data(), G.edge_tgt = qet.data(), G.edge_counts = qec.data(), G.coverage_ratio = qratio.data(), G.edge_offsets = qeoff.data();
    if (nt) {
      lin.resize(std::max<size_t>(lin.size(), 1)), lout.resize(lin.size()), lcnt.resize(lin.size());
      G.support_total = stot.data(), G.support_unambiguous = suna.data(), G.link_offsets = loff.data();
      G.link_in = lin.data(), G.link_out = lout.data(), G.link_counts = lcnt.data(), G.has_threading = has.data();
    }
    std::vector<shk_pcr_paths_params> path_p;
    std::vector<uint32_t> dedup_t;
    pcr_products_params(genes, fgene, &path_p, &dedup_t);
    // The records: plain, into the caller's arrays under the caller's capacities — short there is this call's outcome, with
    // everything per gene complete; a sweep, into arrays of this call's, sized by a second call when the first guess was
    // short.  The per-gene arrays are this call's either way.
    std::vector<uint64_t> roff(nf + 1, 0), paths_found(nf, 0), generated(nf, 0), states(nf, 0);
    PcrRecordArrays own(64ull * nf, 1ull << 20);
    shk_pcr_records loc{};
    for (int attempt = 0;; ++attempt) {
      loc = sweep ? own.bind(0, PcrRecordArrays::NODES | PcrRecordArrays::SCORE_FIELDS) : outs[0].records;
      loc.record_offsets = roff.data(), loc.paths_found = paths_found.data(), loc.generated = generated.data(), loc.states_explored = states.data();
      short_rc = shk_pcr_products_panel(c, &G, path_p.data(), dedup_t.data(), &loc, nullptr, nullptr);
      if (!(short_rc == SHK_ERR_BAD_ARG && PcrRecordArrays::is_short(loc))) SHK_TRY(short_rc);  // (anything but short room)
      if (short_rc == SHK_OK || !sweep) break;
      if (attempt) return short_rc;
      own.grow(loc);
    }
    // found is ascending in v, so a block's virtual genes are a run [f0, f1) of it and their records a run of the records
    for (uint32_t j = 0, f0 = 0; j < D; ++j) {
      uint32_t f1 = f0;
      while (f1 < nf && alive[found[f1]] / ng == j) ++f1;
      shk_pcr_run_out &o = outs[j];
      shk_pcr_records &R = o.records;
      for (uint32_t f = f0; f < f1; ++f) {
        const uint32_t g = fgene[f];
        R.record_offsets[g + 1] = roff[f + 1] - roff[f];  // (lengths; summed below)
        if (R.paths_found) R.paths_found[g] = paths_found[f];
        if (R.generated) R.generated[g] = generated[f];
        if (R.states_explored) R.states_explored[g] = states[f];
        if (o.n_pruned_nodes) o.n_pruned_nodes[g] = qnoff[f + 1] - qnoff[f];
        if (o.n_pruned_edges) o.n_pruned_edges[g] = qeoff[f + 1] - qeoff[f];
        if (generated[f]) status[alive[found[f]]] = SHK_PCR_SUCCESS;  // mod.rs:735-743; otherwise the reason of step 5 stays
      }
      for (uint32_t g = 0; g < ng; ++g) R.record_offsets[g + 1] += R.record_offsets[g];
      std::string err;
      if (!sweep)
        R.n_records = loc.n_records, R.n_seq_bytes = loc.n_seq_bytes;  // (the records are where the products call wrote them)
      else if (pcr_records_slice(loc, roff[f0], roff[f1] - roff[f0], &R, &err) != SHK_OK && short_rc == SHK_OK)
        short_rc = fail(c, SHK_ERR_BAD_ARG, "%s", err.c_str());  // (the first short block's text; every block is still completed)
      f0 = f1;
    }
  }
  for (uint32_t v = 0; v < nv; ++v) outs[v / ng].status[v % ng] = status[v];
  if (getenv("SHK_TRACE"))  // (read at each call, like the stages' lines)
    for (uint32_t v = 0; v < nv; ++v)
      pcr_trace_line(genes[v % ng], v % ng, status[v], poff[2 * v + 1] - poff[2 * v], poff[2 * v + 2] - poff[2 * v + 1], outs[v / ng],
                     sweep ? depths[v / ng] : 0u);
  return short_rc;  // (SHK_OK, or the record capacities' SHK_ERR_BAD_ARG with every block complete)
}

}  // namespace

extern "C" int shk_pcr_run_depths(shk_ctx *c, const shk_pcr_gene *genes, uint32_t n_genes, const shk_pcr_run_params *params,
                                  const uint32_t *depths, uint32_t n_depths, shk_pcr_run_out *outs) {
  SHK_TRY(xs_closed(c));
  if (!c || !params || !outs || (n_genes && !genes)) return SHK_ERR_BAD_ARG;
  try {
    return pcr_pipeline(c, genes, n_genes, params, true, depths, n_depths, outs);
  } catch (...) {  // no exception leaves the C ABI
    return fail(c, SHK_ERR_NOMEM, "shk_pcr_run_depths: out of host memory");
  }
}

extern "C" int shk_pcr_run(shk_ctx *c, const shk_pcr_gene *genes, uint32_t n_genes, const shk_pcr_run_params *params, shk_pcr_run_out *out) {
  SHK_TRY(xs_closed(c));
  if (!c || !params || !out || !out->status || !out->records.record_offsets || (n_genes && !genes)) return SHK_ERR_BAD_ARG;
  try {
    return pcr_pipeline(c, genes, n_genes, params, false, nullptr, 1, out);
  } catch (...) {  // no exception leaves the C ABI
    return fail(c, SHK_ERR_NOMEM, "shk_pcr_run: out of host memory");
  }
}
