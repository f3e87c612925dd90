// shk_pcr.cpp — sPCR's graph extension replayed on the host over counts fetched in bulk (shk_neighborhood).
//
// extend_graph (src/pcr/graph.rs:321-528) asks the table for four k-mer counts per node and decides in FIFO order:
// the decisions depend on the order, the counts do not.  So the counts are fetched ahead — the neighbourhood of
// everything now in the queue, many levels in one call — into a host map, and the reference's loop runs over the map.
// A node enters the reference's graph only over an accepted k-mer, so everything it can look at lies inside the
// neighbourhood at the step's threshold; a k-mer outside it has a count below the threshold, which the reference
// treats like absence.  When the loop reaches an entry whose expansion it does not hold yet (the fetch was cut by its
// capacities, or a cap was small), it fetches again from what is in the queue then.
#include "shk_pcr.h"

#include <algorithm>
#include <cstdlib>
#include <deque>
#include <unordered_map>
#include <unordered_set>

namespace {

constexpr uint64_t EVALUATION_FREQUENCY = 1000;  // EXTENSION_EVALUATION_FREQUENCY, graph.rs:16
constexpr uint32_t COVERAGE_MULTIPLIER = 2, COVERAGE_STEPS = 4;  // mod.rs:46-49

uint64_t revcomp_kmer(uint64_t x, uint32_t k) {
  uint64_t r = 0;
  for (uint32_t i = 0; i < k; ++i) {
    r = (r << 2) | (3 - (x & 3));
    x >>= 2;
  }
  return r;
}

// The counts the replay reads: accepted canonical k-mers (merged count ≥ accept) fetched so far at this threshold,
// and the (node << 1 | dir) entries whose four candidates they settle.
struct Counts {
  shk_ctx *ctx;
  uint32_t k, accept;
  uint64_t mask;
  int shift;
  uint64_t fetch_cap;  // SHK_PCR_FETCH_CAP, 0: sized by the caller's room
  std::unordered_map<uint64_t, uint32_t> known;
  std::unordered_set<uint64_t> expanded;

  uint64_t candidate(uint64_t sub, uint32_t dir, uint64_t b) const {
    return dir ? (b << shift) | sub : (sub << 2) | b;  // graph.rs:419-423
  }
  uint64_t successor(uint64_t kmer, uint32_t dir) const { return dir ? kmer >> 2 : kmer & mask; }  // graph.rs:441-444
  uint32_t count(uint64_t kmer) const {  // 0: not accepted
    const uint64_t rc = revcomp_kmer(kmer, k);
    auto it = known.find(kmer < rc ? kmer : rc);
    return it == known.end() ? 0u : it->second;
  }

  int fetch(std::vector<uint64_t> seeds, uint64_t room, std::string *err) {
    std::sort(seeds.begin(), seeds.end());
    seeds.erase(std::unique(seeds.begin(), seeds.end()), seeds.end());
    const uint64_t n = seeds.size();
    // level 0 always fits 4 k-mers and 4 successors per entry: every fetch gets at least one level further
    const uint64_t cap = std::max<uint64_t>(fetch_cap ? fetch_cap : room, 4 * n);
    std::vector<uint64_t> nodes(n), kmers(cap), fnodes(cap);
    std::vector<uint8_t> dirs(n), fdirs(cap);
    std::vector<uint32_t> counts(cap);
    for (uint64_t i = 0; i < n; ++i) {
      nodes[i] = seeds[i] >> 1;
      dirs[i] = (uint8_t)(1u << (seeds[i] & 1));
    }
    uint64_t n_out = 0, n_fringe = 0;
    uint32_t levels = 0;
    const int rc = shk_neighborhood(ctx, nodes.data(), dirs.data(), n, accept, 0, kmers.data(), counts.data(), cap, &n_out,
                                    fnodes.data(), fdirs.data(), cap, &n_fringe, &levels);
    if (rc != SHK_OK) return rc;
    if (levels == 0) {
      *err = "shk_pcr_extend: a neighbourhood fetch made no progress";
      return SHK_ERR_INVARIANT;
    }
    for (uint64_t i = 0; i < n_out; ++i) known[kmers[i]] = counts[i];
    // which entries the fetch expanded: its levels below `levels`, walked from the seeds over the merged map (every
    // accepted candidate of such an entry is in the map, and the map holds accepted k-mers only)
    std::unordered_set<uint64_t> seen(seeds.begin(), seeds.end());
    std::vector<uint64_t> level = seeds, next;
    for (uint32_t l = 0; l < levels && !level.empty(); ++l) {
      next.clear();
      for (const uint64_t e : level) {
        expanded.insert(e);
        const uint32_t dir = (uint32_t)(e & 1);
        for (uint64_t b = 0; b < 4; ++b) {
          const uint64_t x = candidate(e >> 1, dir, b);
          if (!count(x)) continue;
          const uint64_t s = successor(x, dir) << 1 | dir;
          if (seen.insert(s).second) next.push_back(s);
        }
      }
      level.swap(next);
    }
    return SHK_OK;
  }
};

// create_seed_graph (graph.rs:196-278)
PcrGraph seed_graph(uint32_t k, const uint64_t *fwd, uint64_t n_fwd, const uint64_t *rev, uint64_t n_rev) {
  PcrGraph g;
  std::unordered_map<uint64_t, uint32_t> lookup;
  const uint64_t mask = (1ull << (2 * (k - 1))) - 1ull;
  std::vector<uint64_t> f(fwd, fwd + n_fwd), r(rev, rev + n_rev);
  std::sort(f.begin(), f.end());
  std::sort(r.begin(), r.end());
  auto seed = [&](uint64_t sub, uint8_t flag) {
    auto it = lookup.find(sub);
    if (it != lookup.end()) {
      g.flags[it->second] |= flag;
    } else {
      lookup.emplace(sub, (uint32_t)g.sub_kmer.size());
      g.sub_kmer.push_back(sub);
      g.flags.push_back(flag);
    }
  };
  for (const uint64_t kmer : f) seed(kmer >> 2, 1);
  for (const uint64_t kmer : r) seed(revcomp_kmer(kmer, k) & mask, 2);  // strand-normalised, graph.rs:254-255
  return g;
}

// extend_graph (graph.rs:321-528) at one threshold, from a fresh copy of the seed graph
int extend(Counts &cn, PcrGraph &g, uint32_t min_count, double high_coverage_ratio, uint64_t max_num_nodes,
           std::string *err) {
  std::unordered_map<uint64_t, uint32_t> lookup;
  for (uint32_t i = 0; i < g.sub_kmer.size(); ++i) lookup.emplace(g.sub_kmer[i], i);
  std::unordered_set<uint64_t> edges;  // find_edge: source << 32 | target
  bool found_path = false;
  double median = pcr_median_u32(g.ecount, (double)min_count);
  uint64_t last_median_check = 0;
  std::deque<std::pair<uint32_t, uint32_t>> frontier;  // (node, dir: 0 Forward, 1 Reverse)
  std::vector<uint8_t> processed(g.sub_kmer.size(), 0), added_by(g.sub_kmer.size(), 0);  // bit 0 fwd, bit 1 rev
  for (uint32_t i = 0; i < g.sub_kmer.size(); ++i) {
    if (g.flags[i] & 1) frontier.emplace_back(i, 0u);
    if (g.flags[i] & 2) frontier.emplace_back(i, 1u);
    added_by[i] = g.flags[i] & 3;
  }
  while (!frontier.empty()) {
    const uint32_t node = frontier.front().first, dir = frontier.front().second;
    frontier.pop_front();
    if (processed[node] >> dir & 1) continue;
    processed[node] |= (uint8_t)(1u << dir);
    const uint64_t n_nodes = g.sub_kmer.size();
    if (n_nodes > max_num_nodes) break;  // graph.rs:389
    if (n_nodes > last_median_check && n_nodes - last_median_check > EVALUATION_FREQUENCY) {  // graph.rs:400-405
      median = pcr_median_u32(g.ecount, (double)min_count);
      last_median_check = n_nodes - n_nodes % EVALUATION_FREQUENCY;
    }
    const uint64_t sub = g.sub_kmer[node];
    if (!cn.expanded.count(sub << 1 | dir)) {
      std::vector<uint64_t> seeds{sub << 1 | dir};
      for (const auto &e : frontier) {
        const uint64_t s = g.sub_kmer[e.first] << 1 | e.second;
        if (!(processed[e.first] >> e.second & 1) && !cn.expanded.count(s)) seeds.push_back(s);
      }
      // what the node budget still allows, with some room for k-mers that lead to no node
      const uint64_t room = std::max<uint64_t>(2 * std::min<uint64_t>(max_num_nodes - n_nodes + 1, 1ull << 19), 4096);
      const int rc = cn.fetch(std::move(seeds), room, err);
      if (rc != SHK_OK) return rc;
    }
    uint64_t cand[4];
    uint32_t cand_count[4], n_cand = 0;
    for (uint64_t b = 0; b < 4; ++b) {
      const uint64_t kmer = cn.candidate(sub, dir, b);
      const uint32_t c = cn.count(kmer);
      if (c) {
        cand[n_cand] = kmer;
        cand_count[n_cand++] = c;
      }
    }
    for (uint32_t i = 0; i < n_cand; ++i) {
      const uint64_t new_sub = cn.successor(cand[i], dir);
      if (new_sub == sub) continue;  // self-loop
      auto it = lookup.find(new_sub);
      if (it != lookup.end()) {
        const uint32_t existing = it->second;
        const uint32_t src = dir ? existing : node, tgt = dir ? node : existing;
        if (edges.insert((uint64_t)src << 32 | tgt).second) {
          g.esrc.push_back(src);
          g.etgt.push_back(tgt);
          g.ecount.push_back(cand_count[i]);
          if (added_by[existing] >> (dir ^ 1u) & 1) found_path = true;  // graph.rs:464, 478
        }
      } else {
        if ((double)cand_count[i] > median * high_coverage_ratio) continue;  // graph.rs:495
        const uint32_t nn = (uint32_t)g.sub_kmer.size();
        g.sub_kmer.push_back(new_sub);
        g.flags.push_back(0);
        processed.push_back(0);
        added_by.push_back((uint8_t)(1u << dir));
        lookup.emplace(new_sub, nn);
        const uint32_t src = dir ? nn : node, tgt = dir ? node : nn;
        edges.insert((uint64_t)src << 32 | tgt);
        g.esrc.push_back(src);
        g.etgt.push_back(tgt);
        g.ecount.push_back(cand_count[i]);
        frontier.emplace_back(nn, dir);
      }
    }
  }
  g.found_path = found_path;
  return SHK_OK;
}

}  // namespace

double pcr_median_u32(std::vector<uint32_t> counts, double dflt) {
  if (counts.empty()) return dflt;
  const size_t mid = counts.size() / 2;
  std::nth_element(counts.begin(), counts.begin() + mid, counts.end());
  if (counts.size() % 2 == 0) {
    const double upper_min = (double)counts[mid];
    const double lower_max = (double)*std::max_element(counts.begin(), counts.begin() + mid);
    return (lower_max + upper_min) / 2.0;
  }
  return (double)counts[mid];
}

std::vector<uint32_t> pcr_coverage_thresholds(uint32_t primer_count, uint32_t min_count) {
  const uint32_t high = primer_count / COVERAGE_MULTIPLIER;
  std::vector<uint32_t> t;
  if (high <= min_count) {
    t.push_back(min_count);
  } else {
    const uint32_t step = (high - min_count) / (COVERAGE_STEPS - 1);
    for (uint32_t i = 0; i < COVERAGE_STEPS; ++i) t.push_back(high >= i * step ? high - i * step : 0u);
    t.back() = min_count;
  }
  t.erase(std::unique(t.begin(), t.end()), t.end());
  return t;
}

int pcr_extend_run(shk_ctx *ctx, uint32_t k, const uint64_t *fwd_kmers, const uint32_t *fwd_counts, uint64_t n_fwd,
                   const uint64_t *rev_kmers, const uint32_t *rev_counts, uint64_t n_rev,
                   const shk_pcr_extend_params &p, PcrGraph *out, uint32_t *threshold_used, uint32_t *steps_run,
                   std::string *err) {
  const PcrGraph seed = seed_graph(k, fwd_kmers, n_fwd, rev_kmers, n_rev);
  // get_max_count of either set (0 when empty), mod.rs:542-544
  uint32_t max_f = 0, max_r = 0;
  for (uint64_t i = 0; i < n_fwd; ++i) max_f = std::max(max_f, fwd_counts[i]);
  for (uint64_t i = 0; i < n_rev; ++i) max_r = std::max(max_r, rev_counts[i]);
  std::vector<uint32_t> thresholds{p.min_count};
  if (p.sweep) thresholds = pcr_coverage_thresholds(std::min(max_f, max_r), p.min_count);
  const char *env = getenv("SHK_PCR_FETCH_CAP");
  const long long fetch_cap = env ? atoll(env) : 0;
  *out = seed;
  *steps_run = 0;
  *threshold_used = thresholds[0];
  for (const uint32_t t : thresholds) {  // mod.rs:585-619: every step starts from the seed graph
    Counts cn{};
    cn.ctx = ctx;
    cn.k = k;
    cn.accept = std::max(std::max(t, p.table_min_count), 1u);
    cn.shift = 2 * (int)(k - 1);
    cn.mask = (1ull << cn.shift) - 1ull;
    cn.fetch_cap = fetch_cap > 0 ? (uint64_t)fetch_cap : 0;
    PcrGraph g = seed;
    const int rc = extend(cn, g, t, p.high_coverage_ratio, p.max_num_nodes, err);
    if (rc != SHK_OK) return rc;
    *out = std::move(g);
    *steps_run += 1;
    *threshold_used = t;
    if (out->found_path) break;
  }
  return SHK_OK;
}

extern "C" uint64_t shk_pcr_node_budget(uint64_t n_bases_ingested) {  // graph.rs:40-52
  const uint64_t low_bp = 150000000ull, high_bp = 750000000ull, min_budget = 100000, max_budget = 500000;
  if (n_bases_ingested <= low_bp) return min_budget;
  if (n_bases_ingested >= high_bp) return max_budget;
  const double fraction = (double)(n_bases_ingested - low_bp) / (double)(high_bp - low_bp);
  return (uint64_t)((double)min_budget + fraction * (double)(max_budget - min_budget));
}
