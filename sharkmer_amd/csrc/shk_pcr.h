// shk_pcr.h — host side of sPCR's graph extension (create_seed_graph + extend_graph, src/pcr/graph.rs:196-528, under
// the threshold sweep of do_pcr, src/pcr/mod.rs:559-619): the reference's order-dependent logic replayed statement for
// statement over counts fetched in bulk by shk_neighborhood_panel (plain C++: no HIP; the device is reached through
// that entry point only).
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "../../include/shk.h"

struct PcrGraph {                       // StableDiGraph<DBNode, DBEdge> as arrays in index order
  std::vector<uint64_t> sub_kmer;       // DBNode.sub_kmer, NodeIndex order
  std::vector<uint8_t> flags;           // 1 is_start, 2 is_end
  std::vector<uint32_t> esrc, etgt, ecount;  // EdgeIndex order
  bool found_path = false;
};

// median_via_select (graph.rs:82-103) of edge counts; `dflt` when there are none (compute_median_edge_count)
double pcr_median_u32(std::vector<uint32_t> counts, double dflt);
// compute_coverage_thresholds (mod.rs:403-428)
std::vector<uint32_t> pcr_coverage_thresholds(uint32_t primer_count, uint32_t min_count);

struct PcrPrimers {  // one gene's two primer sets
  const uint64_t *fwd_kmers;
  const uint32_t *fwd_counts;
  uint64_t n_fwd;
  const uint64_t *rev_kmers;
  const uint32_t *rev_counts;
  uint64_t n_rev;
};

// The sweep of every gene of a panel over a context of k-mer length k: gene g from primers[g] under params[g].  Per
// gene, threshold_used / steps_run describe the last step run, whose graph is (*out)[g].  The genes' replays run in
// rounds on a few host threads (SHK_PCR_PANEL_THREADS); what they need from the table goes into one
// shk_neighborhood_panel call per round, made by the calling thread.  panel: shk_pcr_extend_panel's call; else
// shk_pcr_extend's, one gene on the calling thread, which the SHK_PCR_PANEL_* knobs do not govern.  Returns SHK_OK or
// the code of a failed shk_neighborhood_panel (its text is the context's last error); *err is set for failures of its
// own, a failed host allocation among them (SHK_ERR_NOMEM).  gene_depths (or nullptr): gene g reads the table at depth
// gene_depths[g] — its fetches go through shk_neighborhood_panel_depths, all else is the same.
int pcr_extend_panel_run(shk_ctx *ctx, uint32_t k, const PcrPrimers *primers, uint32_t n_genes, const shk_pcr_extend_params *params,
                         bool panel, std::vector<PcrGraph> *out, uint32_t *threshold_used, uint32_t *steps_run, std::string *err,
                         const uint32_t *gene_depths = nullptr);
