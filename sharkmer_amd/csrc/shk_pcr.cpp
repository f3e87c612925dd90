// shk_pcr.cpp — sPCR's graph extension replayed on the host over counts fetched in bulk (shk_neighborhood_panel).
//
// extend_graph (src/pcr/graph.rs:321-528) asks the table for four k-mer counts per node and decides in FIFO order:
// the decisions depend on the order, the counts do not.  So the counts are fetched ahead — the neighbourhood of
// everything now in the queue, many levels in one call — into a host map, and the reference's loop runs over the map.
// A node enters the reference's graph only over an accepted k-mer, so everything it can look at lies inside the
// neighbourhood at the step's threshold; a k-mer outside it has a count below the threshold, which the reference
// treats like absence.  When the loop reaches an entry whose expansion it does not hold yet (the fetch was cut by its
// capacities, or a cap was small), it fetches again from what is in the queue then.
//
// The loop is a state object (Extension) that stops where it needs a fetch and is taken up again after it: a panel's
// genes run side by side, and what they need goes to the device in one shk_neighborhood_panel call per round.  One gene
// (shk_pcr_extend) is a panel of one, replayed on the calling thread.
#include "shk_pcr.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <deque>
#include <exception>
#include <memory>
#include <thread>
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
  uint32_t k = 0, accept = 0;
  uint64_t mask = 0;
  int shift = 0;
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

  // The answer of a fetch from `seeds` (distinct entries) that expanded `levels` levels.
  void merge(const std::vector<uint64_t> &seeds, const uint64_t *kmers, const uint32_t *counts, uint64_t n_out, uint32_t levels) {
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

// extend_graph (graph.rs:321-528) at one threshold, from a fresh copy of the seed graph, as a state that run() carries
// forward: until the step ends, or until it has popped an entry whose expansion the counts do not hold — then `seeds`
// and `room` say what to fetch, and the next run() takes that entry up where it left it (its `processed` mark and the
// budget check are not repeated).
struct Extension {
  Counts cn;
  PcrGraph g;
  uint32_t min_count = 0;
  double high_coverage_ratio = 0;
  uint64_t max_num_nodes = 0;
  std::unordered_map<uint64_t, uint32_t> lookup;
  std::unordered_set<uint64_t> edges;  // find_edge: source << 32 | target
  bool found_path = false, resume = false;
  double median = 0;
  uint64_t last_median_check = 0;
  std::deque<std::pair<uint32_t, uint32_t>> frontier;  // (node, dir: 0 Forward, 1 Reverse)
  std::vector<uint8_t> processed, added_by;            // bit 0 fwd, bit 1 rev
  uint32_t node = 0, dir = 0;                          // the entry in hand
  std::vector<uint64_t> seeds;                         // the fetch asked for: distinct entries, ascending
  uint64_t room = 0;

  void start(const PcrGraph &seed, uint32_t k, uint32_t threshold, const shk_pcr_extend_params &p) {
    *this = Extension();
    cn.k = k;
    cn.accept = std::max(std::max(threshold, p.table_min_count), 1u);
    cn.shift = 2 * (int)(k - 1);
    cn.mask = (1ull << cn.shift) - 1ull;
    g = seed;
    min_count = threshold;
    high_coverage_ratio = p.high_coverage_ratio;
    max_num_nodes = p.max_num_nodes;
    for (uint32_t i = 0; i < g.sub_kmer.size(); ++i) lookup.emplace(g.sub_kmer[i], i);
    median = pcr_median_u32(g.ecount, (double)min_count);
    processed.assign(g.sub_kmer.size(), 0);
    added_by.assign(g.sub_kmer.size(), 0);
    for (uint32_t i = 0; i < g.sub_kmer.size(); ++i) {
      if (g.flags[i] & 1) frontier.emplace_back(i, 0u);
      if (g.flags[i] & 2) frontier.emplace_back(i, 1u);
      added_by[i] = g.flags[i] & 3;
    }
  }

  // true: the step is over (g is its graph); false: fetch `seeds` with `room`, merge, and call again
  bool run() {
    while (resume || !frontier.empty()) {
      if (!resume) {
        node = frontier.front().first, dir = frontier.front().second;
        frontier.pop_front();
        if (processed[node] >> dir & 1) continue;
        processed[node] |= (uint8_t)(1u << dir);
        const uint64_t n_nodes = g.sub_kmer.size();
        if (n_nodes > max_num_nodes) break;  // graph.rs:389
        if (n_nodes > last_median_check && n_nodes - last_median_check > EVALUATION_FREQUENCY) {  // graph.rs:400-405
          median = pcr_median_u32(g.ecount, (double)min_count);
          last_median_check = n_nodes - n_nodes % EVALUATION_FREQUENCY;
        }
        if (!cn.expanded.count(g.sub_kmer[node] << 1 | dir)) {
          seeds.assign(1, g.sub_kmer[node] << 1 | dir);
          for (const auto &e : frontier) {
            const uint64_t s = g.sub_kmer[e.first] << 1 | e.second;
            if (!(processed[e.first] >> e.second & 1) && !cn.expanded.count(s)) seeds.push_back(s);
          }
          std::sort(seeds.begin(), seeds.end());
          seeds.erase(std::unique(seeds.begin(), seeds.end()), seeds.end());
          // what the node budget still allows, with some room for k-mers that lead to no node
          room = std::max<uint64_t>(2 * std::min<uint64_t>(max_num_nodes - n_nodes + 1, 1ull << 19), 4096);
          resume = true;
          return false;
        }
      }
      resume = false;
      const uint64_t sub = g.sub_kmer[node];
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
    return true;
  }
};

// One gene under the threshold sweep of do_pcr (mod.rs:559-619): every step starts from the seed graph, the first step
// that finds a path is the last.
struct GeneSweep {
  uint32_t k = 0;
  shk_pcr_extend_params p{};
  PcrGraph seed, out;
  std::vector<uint32_t> thresholds;
  uint32_t step = 0, steps_run = 0, threshold_used = 0;
  bool done = false;
  Extension ex;
  // the answer of the fetch ex asked for, merged at the start of the next advance()
  const uint64_t *ans_kmers = nullptr;
  const uint32_t *ans_counts = nullptr;
  uint64_t ans_n = 0;
  uint32_t ans_levels = 0;
  bool ans_pending = false;

  void init(uint32_t k_, const uint64_t *fwd_kmers, const uint32_t *fwd_counts, uint64_t n_fwd, const uint64_t *rev_kmers,
            const uint32_t *rev_counts, uint64_t n_rev, const shk_pcr_extend_params &p_) {
    k = k_;
    p = p_;
    seed = seed_graph(k, fwd_kmers, n_fwd, rev_kmers, n_rev);
    // get_max_count of either set (0 when empty), mod.rs:542-544
    uint32_t max_f = 0, max_r = 0;
    for (uint64_t i = 0; i < n_fwd; ++i) max_f = std::max(max_f, fwd_counts[i]);
    for (uint64_t i = 0; i < n_rev; ++i) max_r = std::max(max_r, rev_counts[i]);
    thresholds.assign(1, p.min_count);
    if (p.sweep) thresholds = pcr_coverage_thresholds(std::min(max_f, max_r), p.min_count);
    out = seed;
    threshold_used = thresholds[0];
    ex.start(seed, k, thresholds[0], p);
  }
  void answer(const uint64_t *kmers, const uint32_t *counts, uint64_t n, uint32_t levels) {
    ans_kmers = kmers, ans_counts = counts, ans_n = n, ans_levels = levels, ans_pending = true;
  }
  // Until the gene needs a fetch (ex.seeds / ex.room say which) or its sweep is over (done).
  void advance() {
    if (ans_pending) {
      ex.cn.merge(ex.seeds, ans_kmers, ans_counts, ans_n, ans_levels);
      ans_pending = false;
    }
    while (!done) {
      if (!ex.run()) return;
      out = std::move(ex.g);
      steps_run += 1;
      threshold_used = thresholds[step];
      if (out.found_path || ++step == thresholds.size())
        done = true;
      else
        ex.start(seed, k, thresholds[step], p);
    }
  }
};

uint64_t env_u64(const char *name, uint64_t dflt) {
  const char *env = getenv(name);
  const long long v = env ? atoll(env) : 0;
  return v > 0 ? (uint64_t)v : dflt;
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

namespace {

// A grow-only array that is never value-initialised (the panel's output arrays are as large as its capacities).
template <typename T>
struct Raw {
  std::unique_ptr<T[]> p;
  size_t cap = 0;
  T *need(size_t n) {
    if (n > cap) {
      p.reset(new T[n]);
      cap = n;
    }
    return p.get();
  }
};

// who: the public call, for its error texts.  The panel-only knobs (SHK_PCR_PANEL_*) are the panel's: the single call
// has no launch budget to share, one thread, and no trace line.
int panel_run(shk_ctx *ctx, uint32_t k, const PcrPrimers *primers, uint32_t n_genes, const shk_pcr_extend_params *params, bool panel,
              const char *who, std::vector<PcrGraph> *out, uint32_t *threshold_used, uint32_t *steps_run, std::string *err,
              const uint32_t *gene_depths) {
  const uint64_t fetch_cap = env_u64("SHK_PCR_FETCH_CAP", 0);  // 0: sized by the replay's room
  const uint64_t budget = panel ? env_u64("SHK_PCR_PANEL_FETCH_CAP", 1ull << 22) : ~0ull;
  const char *env_threads = panel ? getenv("SHK_PCR_PANEL_THREADS") : "1";  // default 8; whatever is given is clamped to 1..16
  const uint32_t n_threads = (uint32_t)std::min<long long>(std::max<long long>(env_threads ? atoll(env_threads) : 8, 1), 16);
  std::vector<GeneSweep> genes(n_genes);
  for (uint32_t g = 0; g < n_genes; ++g) {
    const PcrPrimers &pr = primers[g];
    genes[g].init(k, pr.fwd_kmers, pr.fwd_counts, pr.n_fwd, pr.rev_kmers, pr.rev_counts, pr.n_rev, params[g]);
  }
  std::vector<uint32_t> active(n_genes);
  for (uint32_t g = 0; g < n_genes; ++g) active[g] = g;
  // one launch's arrays (a gene's answer is read from them at the start of the next round)
  // (kept from round to round, and the four output arrays — as large as the capacities — never value-initialised)
  struct Launch {
    std::vector<uint64_t> nodes, seed_offsets, caps, n_out, n_fringe;
    std::vector<uint8_t> dirs;
    std::vector<uint32_t> min_counts, levels, depths;
    Raw<uint64_t> kmers, fnodes;
    Raw<uint32_t> counts;
    Raw<uint8_t> fdirs;
  };
  std::vector<Launch> launches;
  size_t launches_used = 0;
  uint64_t n_rounds = 0, n_launches = 0;  // (SHK_PCR_PANEL_TRACE: what tools/pcr_extend_panel_bench.py reports)
  while (!active.empty()) {
    // 1. every unfinished gene until it needs a fetch or its sweep is over: gene i of the round on thread i mod T
    const uint32_t T = (uint32_t)std::min<size_t>(n_threads, active.size());
    std::vector<uint8_t> failed(T, 0);  // (a slot per thread: nothing shared)
    auto work = [&](uint32_t t) {
      try {
        for (size_t i = t; i < active.size(); i += T) genes[active[i]].advance();
      } catch (...) {  // out of memory in a replay: no exception leaves a thread or the C ABI
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
      *err = std::string(who) + ": out of host memory in a gene's replay";
      return SHK_ERR_NOMEM;
    }
    launches_used = 0;
    n_rounds += 1;
    active.erase(std::remove_if(active.begin(), active.end(), [&](uint32_t g) { return genes[g].done; }), active.end());
    // 2. the pending fetches, as many per launch as the budget takes at 4 k-mers per seed (what level 0 needs)
    for (size_t a = 0; a < active.size();) {
      size_t b = a;
      uint64_t least = 0;
      while (b < active.size() && (b == a || least + 4 * genes[active[b]].ex.seeds.size() <= budget))
        least += 4 * genes[active[b++]].ex.seeds.size();
      const uint32_t n_jobs = (uint32_t)(b - a);
      const uint64_t share = budget / n_jobs;
      if (launches_used == launches.size()) launches.emplace_back();
      Launch &L = launches[launches_used++];
      L.nodes.clear(), L.dirs.clear(), L.min_counts.clear(), L.caps.clear(), L.depths.clear();
      L.seed_offsets.assign(1, 0);
      uint64_t total = 0;
      for (size_t i = a; i < b; ++i) {
        const Extension &ex = genes[active[i]].ex;
        for (const uint64_t s : ex.seeds) {
          L.nodes.push_back(s >> 1);
          L.dirs.push_back((uint8_t)(1u << (s & 1)));
        }
        L.seed_offsets.push_back(L.nodes.size());
        L.min_counts.push_back(ex.cn.accept);
        if (gene_depths) L.depths.push_back(gene_depths[active[i]]);
        // level 0 always fits 4 k-mers and 4 successors per entry: every fetch gets at least one level further
        L.caps.push_back(std::max<uint64_t>(fetch_cap ? fetch_cap : std::min(share, ex.room), 4 * ex.seeds.size()));
        total += L.caps.back();
      }
      L.n_out.resize(n_jobs), L.n_fringe.resize(n_jobs), L.levels.resize(n_jobs);
      uint64_t *const lk = L.kmers.need(total), *const lfn = L.fnodes.need(total);
      uint32_t *const lc = L.counts.need(total);
      uint8_t *const lfd = L.fdirs.need(total);
      const int rc = gene_depths ? shk_neighborhood_panel_depths(ctx, L.nodes.data(), L.dirs.data(), L.seed_offsets.data(), n_jobs,
                                                                 L.min_counts.data(), L.depths.data(), 0, L.caps.data(), L.caps.data(), lk,
                                                                 lc, L.n_out.data(), lfn, lfd, L.n_fringe.data(), L.levels.data())
                                 : shk_neighborhood_panel(ctx, L.nodes.data(), L.dirs.data(), L.seed_offsets.data(), n_jobs,
                                                          L.min_counts.data(), 0, L.caps.data(), L.caps.data(), lk, lc, L.n_out.data(), lfn,
                                                          lfd, L.n_fringe.data(), L.levels.data());
      if (rc != SHK_OK) return rc;
      n_launches += 1;
      // 3. each job's answer to its gene (merged by the gene's thread of the next round)
      uint64_t at = 0;
      for (uint32_t j = 0; j < n_jobs; ++j) {
        if (L.levels[j] == 0) {
          *err = std::string(who) + (panel ? ": gene " + std::to_string(active[a + j]) : "") + ": a neighbourhood fetch made no progress";
          return SHK_ERR_INVARIANT;
        }
        genes[active[a + j]].answer(L.kmers.p.get() + at, L.counts.p.get() + at, L.n_out[j], L.levels[j]);
        at += L.caps[j];
      }
      a = b;
    }
  }
  if (panel && getenv("SHK_PCR_PANEL_TRACE"))
    fprintf(stderr, "shk_pcr_extend_panel: genes %u rounds %llu launches %llu threads %u\n", n_genes, (unsigned long long)n_rounds,
            (unsigned long long)n_launches, n_threads);
  out->resize(n_genes);
  for (uint32_t g = 0; g < n_genes; ++g) {
    (*out)[g] = std::move(genes[g].out);
    threshold_used[g] = genes[g].threshold_used;
    steps_run[g] = genes[g].steps_run;
  }
  return SHK_OK;
}

}  // namespace

int pcr_extend_panel_run(shk_ctx *ctx, uint32_t k, const PcrPrimers *primers, uint32_t n_genes, const shk_pcr_extend_params *params,
                         bool panel, std::vector<PcrGraph> *out, uint32_t *threshold_used, uint32_t *steps_run, std::string *err,
                         const uint32_t *gene_depths) {
  const char *who = panel ? "shk_pcr_extend_panel" : "shk_pcr_extend";
  try {
    return panel_run(ctx, k, primers, n_genes, params, panel, who, out, threshold_used, steps_run, err, gene_depths);
  } catch (const std::exception &e) {  // bad_alloc on the calling thread: an error code, not an exception across the C ABI
    *err = std::string(who) + ": " + e.what();
    return SHK_ERR_NOMEM;
  }
}

extern "C" uint64_t shk_pcr_node_budget(uint64_t n_bases_ingested) {  // graph.rs:40-52
  const uint64_t low_bp = 150000000ull, high_bp = 750000000ull, min_budget = 100000, max_budget = 500000;
  if (n_bases_ingested <= low_bp) return min_budget;
  if (n_bases_ingested >= high_bp) return max_budget;
  const double fraction = (double)(n_bases_ingested - low_bp) / (double)(high_bp - low_bp);
  return (uint64_t)((double)min_budget + fraction * (double)(max_budget - min_budget));
}
