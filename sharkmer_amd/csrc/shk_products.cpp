// shk_products.cpp — sPCR's last stage on the host: resolve_bubbles (src/pcr/bubble.rs:52-275), get_assembly_paths and
// generate_sequences_from_paths (src/pcr/paths.rs:78-356), PathScore::composite (src/pcr/mod.rs:80-113), per gene and
// statement for statement, and shk_edit_within, the host route and yardstick of the dedup.
//
// The search is one dependent chain per start node (a stack, a visit count per node, budgets that end it in the
// middle) and every figure of a record is a double summed in path order: both stay on the host.  A
// panel's genes are independent, so they run on a few threads, striped as the replays of shk_pcr_extend_panel are.
#include "shk_products.h"

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <thread>
#include <unordered_map>

namespace {

constexpr uint32_t MAX_BUBBLE_DEPTH = 50;  // bubble.rs:17
const double NONE = std::numeric_limits<double>::quiet_NaN();

// median_via_select (graph.rs:82-103) of u64 values as f64; 0.0 when there are none (compute_median)
double median_u64(std::vector<uint64_t> v) {
  if (v.empty()) return 0.0;
  const size_t mid = v.size() / 2;
  std::nth_element(v.begin(), v.begin() + mid, v.end());
  if (v.size() % 2 == 0) return ((double)*std::max_element(v.begin(), v.begin() + mid) + (double)v[mid]) / 2.0;
  return (double)v[mid];
}

struct Gene {  // one gene's view of the panel
  uint32_t k = 0, n = 0, e = 0;
  const uint64_t *sub = nullptr;
  const uint8_t *flags = nullptr;
  const uint32_t *src = nullptr, *tgt = nullptr, *counts = nullptr;
  const double *ratio = nullptr;
  bool threaded = false;
  const uint32_t *sup_total = nullptr, *sup_unamb = nullptr, *link_in = nullptr, *link_out = nullptr, *link_counts = nullptr;
  uint64_t n_links = 0;
  shk_pcr_paths_params p{};
};

// One side of the adjacency: node v's edges are list[first[v] .. first[v + 1]) in DESCENDING edge index — the order
// edges_directed yields on a graph that add_edge built and the pruning only removed from.
void adjacency(const uint32_t *at, uint32_t n, uint32_t e, std::vector<uint32_t> &first, std::vector<uint32_t> &list) {
  first.assign((size_t)n + 1, 0u);
  for (uint32_t i = 0; i < e; ++i) first[at[i] + 1] += 1;
  for (uint32_t v = 0; v < n; ++v) first[v + 1] += first[v];
  std::vector<uint32_t> fill(first.begin(), first.end() - 1);
  list.resize(e);
  for (uint32_t i = e; i-- > 0;) list[fill[at[i]]++] = i;
}

// resolve_bubbles: pref[edge], NaN where the map has no entry
void resolve_bubbles(const Gene &g, const std::vector<uint32_t> &out_first, const std::vector<uint32_t> &out_list, std::vector<double> &pref) {
  std::vector<uint32_t> in_first, in_list;
  adjacency(g.tgt, g.n, g.e, in_first, in_list);
  std::unordered_map<uint64_t, uint32_t> links;  // branch_links
  for (uint64_t i = 0; i < g.n_links; ++i) links[(uint64_t)g.link_in[i] << 32 | g.link_out[i]] = g.link_counts[i];
  std::vector<uint32_t> stamp(g.n, 0u);
  uint32_t now = 0;
  struct Sink {
    uint32_t node;
    std::vector<std::vector<uint32_t>> branches;
  };
  struct Ranking {
    const std::vector<uint32_t> *edges;
    uint32_t evidence;
    uint64_t key;
  };
  for (uint32_t source = 0; source < g.n; ++source) {
    const uint32_t o0 = out_first[source], o1 = out_first[source + 1];
    if (o1 - o0 < 2) continue;
    std::vector<Sink> endpoints;  // branch_endpoints in first-seen order (its own order does not reach the result)
    for (uint32_t o = o0; o < o1; ++o) {
      const uint32_t first_edge = out_list[o];
      uint32_t current = g.tgt[first_edge];
      std::vector<uint32_t> branch{first_edge};
      if (++now == 0) std::fill(stamp.begin(), stamp.end(), 0u), now = 1;
      stamp[source] = now;  // visited = {source}
      uint32_t depth = 0;
      bool natural = false;
      for (;;) {
        if (depth >= MAX_BUBBLE_DEPTH) break;
        depth += 1;
        if (stamp[current] == now) break;
        stamp[current] = now;
        if (out_first[current + 1] - out_first[current] == 1) {
          const uint32_t next = out_list[out_first[current]];
          branch.push_back(next);
          current = g.tgt[next];
        } else {
          natural = true;
          break;
        }
      }
      if (!natural) continue;
      auto it = std::find_if(endpoints.begin(), endpoints.end(), [&](const Sink &s) { return s.node == current; });
      if (it == endpoints.end()) {
        endpoints.push_back(Sink{current, {}});
        it = endpoints.end() - 1;
      }
      it->branches.push_back(std::move(branch));
    }
    for (const Sink &s : endpoints) {
      if (s.branches.size() < 2 || s.node == source) continue;
      std::vector<Ranking> rank;
      for (const auto &b : s.branches) {
        uint32_t total = 0, phasing = 0;  // (u32 sums wrap, as the release build's do)
        for (const uint32_t ed : b) total += g.sup_total[ed];
        for (uint32_t i = in_first[source]; i < in_first[source + 1]; ++i) {
          auto l = links.find((uint64_t)in_list[i] << 32 | b[0]);
          if (l != links.end()) phasing += l->second;
        }
        rank.push_back(Ranking{&b, total + phasing, (g.sub[g.src[b[0]]] << 2) | (g.sub[g.tgt[b[0]]] & 3)});
      }
      std::stable_sort(rank.begin(), rank.end(),
                       [](const Ranking &a, const Ranking &b) { return a.evidence != b.evidence ? a.evidence > b.evidence : a.key < b.key; });
      uint32_t max_support = 0;
      for (const Ranking &r : rank) max_support = std::max(max_support, r.evidence);
      for (const Ranking &r : rank) {
        const double preference = max_support > 0 ? (double)r.evidence / (double)max_support : 1.0;
        for (const uint32_t ed : *r.edges) pref[ed] = preference;
      }
    }
  }
}

// PathScore::composite (mod.rs:80-113); zero < 0: no threading data
double composite(double median, double cv, double ratio, int64_t zero, double frac) {
  const double cv_penalty = cv > 1.0 ? 1.0 / cv : 1.0;
  const double repeat_penalty = ratio > 5.0 ? 5.0 / ratio : 1.0;
  double factor = 1.0;
  if (zero >= 0) {
    const double zero_penalty = zero > 0 ? std::ldexp(1.0, -(int)std::min<int64_t>(zero, 10)) : 1.0;  // 0.5f64.powi(..)
    factor = zero_penalty * std::max(frac, 0.1);
  }
  return median * cv_penalty * repeat_penalty * factor;
}

struct Step {
  uint32_t node, edge;
};

// generate_sequences_from_paths for one path
void record(const Gene &g, const std::vector<Step> &path, PcrGeneRecords &r, std::vector<uint64_t> &ec, std::vector<uint64_t> &un) {
  const uint64_t len = (uint64_t)(g.k - 1) + (path.size() - 1);
  if (len < g.p.min_length || path.size() < 2) return;
  static const char B[] = "ACGT";
  const uint64_t s0 = g.sub[path[0].node];
  for (uint32_t i = 0; i + 1 < g.k; ++i) r.seqs.push_back((uint8_t)B[(s0 >> (2 * (g.k - 2 - i))) & 3]);
  ec.clear();
  for (size_t i = 1; i < path.size(); ++i) {
    r.seqs.push_back((uint8_t)B[g.sub[path[i].node] & 3]);
    ec.push_back(g.counts[path[i].edge]);
  }
  r.seq_offsets.push_back(r.seqs.size());
  uint64_t sum = 0, mn = ec[0], mx = ec[0];
  for (const uint64_t c : ec) sum += c, mn = std::min(mn, c), mx = std::max(mx, c);
  const double n = (double)ec.size();
  const double mean = (double)sum / n, median = median_u64(ec);
  double cv = 0.0;
  if (mean > 0.0) {
    double var = 0.0;
    for (const uint64_t c : ec) {
      const double d = (double)c - mean;
      var += d * d;
    }
    cv = std::sqrt(var / n) / mean;
  }
  double ratio = 0.0;
  for (size_t i = 1; i < path.size(); ++i) ratio = std::fmax(ratio, g.ratio ? g.ratio[path[i].edge] : 0.0);
  double zero = NONE, med_un = NONE, frac = NONE;
  int64_t zero_i = -1;
  if (g.threaded) {
    uint32_t supported = 0, zeros = 0;
    un.clear();
    for (size_t i = 1; i < path.size(); ++i) {
      const uint32_t ed = path[i].edge;
      if (g.sup_total[ed] > 0) {
        supported += 1;
        un.push_back(g.sup_unamb ? g.sup_unamb[ed] : 0u);
      } else {
        zeros += 1;
        un.push_back(0);
      }
    }
    frac = (double)supported / (double)(uint32_t)ec.size();
    med_un = median_u64(un);
    zero = (double)zeros, zero_i = zeros;
  }
  r.start_node.push_back(path[0].node);
  r.path_nodes.push_back(path.size());
  r.count_mean.push_back(mean), r.count_median.push_back(median), r.count_min.push_back(mn), r.count_max.push_back(mx);
  r.score.push_back(composite(median, cv, ratio, zero_i, frac));
  const double f[SHK_PCR_SCORE_FIELDS] = {(double)(uint32_t)mn, cv, ratio, zero, med_un, frac};
  r.fields.insert(r.fields.end(), f, f + SHK_PCR_SCORE_FIELDS);
}

void run_gene(const Gene &g, PcrGeneRecords &r) {
  if (!g.n) return;
  std::vector<uint32_t> out_first, out_list;
  adjacency(g.src, g.n, g.e, out_first, out_list);
  std::vector<double> pref;
  if (g.threaded) {
    pref.assign(g.e, NONE);
    resolve_bubbles(g, out_first, out_list, pref);
  }
  // sorted_children once per node: the order the search pops them in — score descending, equal scores by ascending edge
  struct Child {
    uint32_t edge;
    double score;
  };
  std::vector<uint32_t> order(g.e);
  std::vector<Child> ch;
  for (uint32_t v = 0; v < g.n; ++v) {
    ch.clear();
    for (uint32_t o = out_first[v]; o < out_first[v + 1]; ++o) {
      const uint32_t ed = out_list[o];
      const double pf = g.threaded && pref[ed] == pref[ed] ? pref[ed] : 1.0;
      ch.push_back(Child{ed, (double)g.counts[ed] * pf});
    }
    std::stable_sort(ch.begin(), ch.end(), [](const Child &a, const Child &b) { return a.score < b.score; });  // (scores are >= +0.0: total_cmp)
    for (size_t i = 0; i < ch.size(); ++i) order[out_first[v] + i] = ch[ch.size() - 1 - i].edge;
  }
  const uint64_t k = g.k;
  const uint64_t min_path_nodes = g.p.min_length <= k ? 1 : g.p.min_length - k + 2;
  const uint64_t max_path_nodes = g.p.max_length <= k ? 1 : g.p.max_length - k + 2;
  std::vector<uint64_t> visits, ec, un;
  std::vector<Step> path;
  std::vector<uint32_t> cursor;  // child_stack: per frame, the next position of its node's list
  for (uint32_t start = 0; start < g.n; ++start) {
    if (!(g.flags[start] & 1)) continue;
    uint64_t paths_from_start = 0, states = 0;
    visits.assign(g.n, 0);
    visits[start] = 1;
    path.assign(1, Step{start, 0});
    cursor.assign(1, out_first[start]);
    for (;;) {
      if (paths_from_start >= g.p.max_paths_per_pair || states >= g.p.max_dfs_states) break;
      const uint32_t at = path[cursor.size() - 1].node;
      if (cursor.back() < out_first[at + 1]) {
        const uint32_t ed = order[cursor.back()++];
        const uint32_t nb = g.tgt[ed];
        states += 1;
        if (visits[nb] >= g.p.max_node_visits) continue;
        path.push_back(Step{nb, ed});
        visits[nb] += 1;
        const uint64_t path_len = path.size();
        if ((g.flags[nb] & 2) && path_len >= min_path_nodes) {
          r.paths_found += 1;
          record(g, path, r, ec, un);
          paths_from_start += 1;
          visits[nb] -= 1;
          path.pop_back();
          continue;
        }
        if (path_len >= max_path_nodes) {
          visits[nb] -= 1;
          path.pop_back();
          continue;
        }
        cursor.push_back(out_first[nb]);
      } else {
        cursor.pop_back();
        if (cursor.empty()) break;
        visits[path.back().node] -= 1;
        path.pop_back();
      }
    }
    r.states_explored += states;
  }
}

int bad(std::string *err, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
int bad(std::string *err, const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  *err = buf;
  return SHK_ERR_BAD_ARG;
}

}  // namespace

int pcr_paths_panel_run(uint32_t k, const shk_pcr_graphs *gr, const shk_pcr_paths_params *params, std::vector<PcrGeneRecords> *out,
                        std::string *err) {
  using ull = unsigned long long;
  out->clear();
  if (!gr) return bad(err, "shk_pcr_paths_panel: graphs is missing");
  const uint32_t ng = gr->n_genes;
  if (ng > SHK_PCR_MAX_GENES) return bad(err, "n_genes %u above SHK_PCR_MAX_GENES (%u)", ng, (unsigned)SHK_PCR_MAX_GENES);
  if (k < 2 || k > 31) return bad(err, "k %u: the paths take 2 <= k <= 31", k);
  if (ng == 0) return SHK_OK;
  if (!gr->node_offsets || !gr->edge_offsets || !params) return bad(err, "shk_pcr_paths_panel: an offsets array or params is missing");
  const bool ann = gr->support_total != nullptr;
  if (ann && !gr->link_offsets) return bad(err, "shk_pcr_paths_panel: support_total without link_offsets");
  const uint64_t mask = (1ull << (2 * (k - 1))) - 1;
  std::vector<Gene> genes(ng);
  for (uint32_t g = 0; g < ng; ++g) {
    const uint64_t va = gr->node_offsets[g], vb = gr->node_offsets[g + 1], ea = gr->edge_offsets[g], eb = gr->edge_offsets[g + 1];
    if (vb < va) return bad(err, "gene %u: node_offsets decrease (%llu after %llu)", g, (ull)vb, (ull)va);
    if (eb < ea) return bad(err, "gene %u: edge_offsets decrease (%llu after %llu)", g, (ull)eb, (ull)ea);
    if (vb - va >= (1ull << 32) || eb - ea >= (1ull << 32)) return bad(err, "gene %u: 2^32 nodes or edges or more", g);
    if ((vb > va && (!gr->node_sub_kmers || !gr->node_flags)) || (eb > ea && (!gr->edge_src || !gr->edge_tgt || !gr->edge_counts)))
      return bad(err, "gene %u: a graph array is missing", g);
    Gene &G = genes[g];
    G.k = k, G.n = (uint32_t)(vb - va), G.e = (uint32_t)(eb - ea), G.p = params[g];
    G.sub = gr->node_sub_kmers + va, G.flags = gr->node_flags + va;
    G.src = gr->edge_src + ea, G.tgt = gr->edge_tgt + ea, G.counts = gr->edge_counts + ea;
    G.ratio = gr->coverage_ratio ? gr->coverage_ratio + ea : nullptr;
    for (uint32_t v = 0; v < G.n; ++v) {
      if (G.flags[v] > 3) return bad(err, "gene %u: node %u has flags %u (1 is_start, 2 is_end)", g, v, G.flags[v]);
      if (G.sub[v] > mask) return bad(err, "gene %u: node %u: sub-k-mer %llu does not fit %u bases", g, v, (ull)G.sub[v], k - 1);
    }
    for (uint32_t i = 0; i < G.e; ++i)
      if (G.src[i] >= G.n || G.tgt[i] >= G.n)
        return bad(err, "gene %u: edge %u: endpoint (%u, %u) outside the gene's %u nodes", g, i, G.src[i], G.tgt[i], G.n);
    if (ann) {
      const uint64_t la = gr->link_offsets[g], lb = gr->link_offsets[g + 1];
      if (lb < la) return bad(err, "gene %u: link_offsets decrease (%llu after %llu)", g, (ull)lb, (ull)la);
      if (lb > la && (!gr->link_in || !gr->link_out || !gr->link_counts)) return bad(err, "gene %u: a link array is missing", g);
      for (uint64_t i = la; i < lb; ++i)
        if (gr->link_in[i] >= G.e || gr->link_out[i] >= G.e)
          return bad(err, "gene %u: link %llu: edge (%u, %u) outside the gene's %u edges", g, (ull)(i - la), gr->link_in[i], gr->link_out[i], G.e);
      G.threaded = !gr->has_threading || gr->has_threading[g];
      G.sup_total = gr->support_total + ea, G.sup_unamb = gr->support_unambiguous ? gr->support_unambiguous + ea : nullptr;
      G.link_in = gr->link_in + la, G.link_out = gr->link_out + la, G.link_counts = gr->link_counts + la, G.n_links = lb - la;
    }
  }
  const char *env_threads = getenv("SHK_PCR_PANEL_THREADS");  // default 8; whatever is given is clamped to 1..16
  const uint32_t T = std::min<uint32_t>((uint32_t)std::min<long long>(std::max<long long>(env_threads ? atoll(env_threads) : 8, 1), 16), ng);
  std::vector<uint8_t> failed(T, 0);
  try {
    out->resize(ng);
  } catch (...) {
    *err = "shk_pcr_paths_panel: out of host memory";
    return SHK_ERR_NOMEM;
  }
  auto work = [&](uint32_t t) {
    try {
      for (uint32_t g = t; g < ng; g += T) run_gene(genes[g], (*out)[g]);
    } catch (...) {  // out of memory in a gene: no exception leaves a thread or the C ABI
      failed[t] = 1;
    }
  };
  {
    std::vector<std::thread> pool;
    uint32_t started = 1;
    try {
      pool.reserve(T);
      for (; started < T; ++started) pool.emplace_back(work, started);
    } catch (...) {  // no more threads to be had: the calling thread takes the stripes that got none
    }
    work(0);
    for (uint32_t t = started; t < T; ++t) work(t);
    for (std::thread &th : pool) th.join();
  }
  if (std::find(failed.begin(), failed.end(), 1) != failed.end()) {
    *err = "shk_pcr_paths_panel: out of host memory in a gene's search";
    return SHK_ERR_NOMEM;
  }
  return SHK_OK;
}

int pcr_records_fit(const shk_pcr_records &out, std::string *err) {
  using ull = unsigned long long;
  if (out.n_records <= out.record_cap && (!out.seqs || out.n_seq_bytes <= out.seq_cap)) return SHK_OK;
  char buf[256];
  snprintf(buf, sizeof buf, "%llu records of %llu bases do not fit record_cap %llu / seq_cap %llu", (ull)out.n_records, (ull)out.n_seq_bytes,
           (ull)out.record_cap, (ull)out.seq_cap);
  *err = buf;
  return SHK_ERR_BAD_ARG;
}

int pcr_records_slice(const shk_pcr_records &src, uint64_t r0, uint64_t nr, shk_pcr_records *out, std::string *err) {
  const uint64_t b0 = src.seq_offsets[r0], nb = src.seq_offsets[r0 + nr] - b0;
  out->n_records = nr, out->n_seq_bytes = nb;
  if (const int rc = pcr_records_fit(*out, err)) return rc;
  if (out->seq_offsets) out->seq_offsets[0] = 0;
  if (out->seqs && nb) memcpy(out->seqs, src.seqs + b0, nb);
  for (uint64_t i = 0, r = r0; i < nr; ++i, ++r) {
    if (out->seq_offsets) out->seq_offsets[i + 1] = src.seq_offsets[r + 1] - b0;
    if (out->start_node) out->start_node[i] = src.start_node[r];
    if (out->path_nodes) out->path_nodes[i] = src.path_nodes[r];
    if (out->count_mean) out->count_mean[i] = src.count_mean[r];
    if (out->count_median) out->count_median[i] = src.count_median[r];
    if (out->count_min) out->count_min[i] = src.count_min[r];
    if (out->count_max) out->count_max[i] = src.count_max[r];
    if (out->score) out->score[i] = src.score[r];
    if (out->score_fields)
      std::copy(src.score_fields + SHK_PCR_SCORE_FIELDS * r, src.score_fields + SHK_PCR_SCORE_FIELDS * (r + 1),
                out->score_fields + SHK_PCR_SCORE_FIELDS * i);
  }
  return SHK_OK;
}

int pcr_records_store(const std::vector<PcrGeneRecords> &records, const std::vector<std::vector<uint32_t>> *pick, shk_pcr_records *out,
                      std::string *err) {
  const size_t ng = records.size();
  uint64_t nr = 0, nb = 0;
  out->record_offsets[0] = 0;
  for (size_t g = 0; g < ng; ++g) {
    const PcrGeneRecords &r = records[g];
    const size_t m = pick ? (*pick)[g].size() : r.size();
    for (size_t i = 0; i < m; ++i) {
      const uint32_t j = pick ? (*pick)[g][i] : (uint32_t)i;
      nb += r.seq_offsets[j + 1] - r.seq_offsets[j];
    }
    nr += m;
    out->record_offsets[g + 1] = nr;
    if (out->paths_found) out->paths_found[g] = r.paths_found;
    if (out->generated) out->generated[g] = r.size();
    if (out->states_explored) out->states_explored[g] = r.states_explored;
  }
  out->n_records = nr, out->n_seq_bytes = nb;
  if (const int rc = pcr_records_fit(*out, err)) return rc;
  uint64_t at = 0, sb = 0;
  if (out->seq_offsets) out->seq_offsets[0] = 0;
  for (size_t g = 0; g < ng; ++g) {
    const PcrGeneRecords &r = records[g];
    const size_t m = pick ? (*pick)[g].size() : r.size();
    for (size_t i = 0; i < m; ++i, ++at) {
      const uint32_t j = pick ? (*pick)[g][i] : (uint32_t)i;
      const uint64_t a = r.seq_offsets[j], len = r.seq_offsets[j + 1] - a;
      if (out->seqs && len) memcpy(out->seqs + sb, r.seqs.data() + a, len);
      sb += len;
      if (out->seq_offsets) out->seq_offsets[at + 1] = sb;
      if (out->start_node) out->start_node[at] = r.start_node[j];
      if (out->path_nodes) out->path_nodes[at] = r.path_nodes[j];
      if (out->count_mean) out->count_mean[at] = r.count_mean[j];
      if (out->count_median) out->count_median[at] = r.count_median[j];
      if (out->count_min) out->count_min[at] = r.count_min[j];
      if (out->count_max) out->count_max[at] = r.count_max[j];
      if (out->score) out->score[at] = r.score[j];
      if (out->score_fields)
        std::copy(r.fields.begin() + SHK_PCR_SCORE_FIELDS * j, r.fields.begin() + SHK_PCR_SCORE_FIELDS * (j + 1),
                  out->score_fields + SHK_PCR_SCORE_FIELDS * at);
    }
  }
  return SHK_OK;
}

extern "C" int shk_pcr_paths_panel(uint32_t k, const shk_pcr_graphs *graphs, const shk_pcr_paths_params *params, shk_pcr_records *out, char *err,
                                   size_t err_cap) {
  std::string msg;
  int rc = SHK_ERR_BAD_ARG;
  if (!out || !out->record_offsets) {
    msg = "shk_pcr_paths_panel: out or its record_offsets is missing";
  } else {
    try {
      std::vector<PcrGeneRecords> records;
      out->n_records = out->n_seq_bytes = 0;
      out->record_offsets[0] = 0;
      rc = pcr_paths_panel_run(k, graphs, params, &records, &msg);
      if (rc == SHK_OK) rc = pcr_records_store(records, nullptr, out, &msg);
    } catch (...) {
      msg = "shk_pcr_paths_panel: out of host memory", rc = SHK_ERR_NOMEM;
    }
  }
  if (err && err_cap) snprintf(err, err_cap, "%s", msg.c_str());
  return rc;
}

extern "C" int shk_edit_within(const uint8_t *a, uint64_t la, const uint8_t *b, uint64_t lb, uint32_t t) {
  if (la > lb) std::swap(a, b), std::swap(la, lb);  // (the distance is symmetric) la <= lb
  if (lb - la > t) return 0;
  if (t >= lb) return 1;
  // rows over a, columns over b, the band |j - i| <= t; INF stands for "above t"
  const uint64_t T = t, INF = T + 1;
  std::vector<uint64_t> prev(lb + 2, INF), cur(lb + 2, INF);
  for (uint64_t j = 0; j <= std::min(lb, T); ++j) prev[j] = j;
  for (uint64_t i = 1; i <= la; ++i) {
    const uint64_t j0 = i > T ? i - T : 0, j1 = std::min(lb, i + T);
    uint64_t best = INF;
    if (j0 > 0) cur[j0 - 1] = INF;
    for (uint64_t j = j0; j <= j1; ++j) {
      uint64_t v;
      if (j == 0) {
        v = i;
      } else {
        v = prev[j - 1] + (a[i - 1] != b[j - 1]);
        v = std::min(v, prev[j] + 1);
        v = std::min(v, cur[j - 1] + 1);
      }
      cur[j] = v = std::min(v, INF);
      best = std::min(best, v);
    }
    if (j1 < lb) cur[j1 + 1] = INF;
    if (best > T) return 0;
    prev.swap(cur);
  }
  return prev[lb] <= T;
}
