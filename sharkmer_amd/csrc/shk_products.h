// shk_products.h — host side of sPCR's last stage (src/pcr/mod.rs:699-813): bubble preferences, the budgeted path
// search, sequences and scores per gene, statement for statement as the reference (plain C++: no HIP), and the pieces
// the dedup shares between its host route and its device route.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "../../include/shk.h"

struct PcrGeneRecords {  // generate_sequences_from_paths' records of one gene, enumeration order
  std::vector<uint8_t> seqs;
  std::vector<uint64_t> seq_offsets{0};
  std::vector<uint32_t> start_node;
  std::vector<uint64_t> path_nodes, count_min, count_max;
  std::vector<double> count_mean, count_median, score, fields;  // fields: SHK_PCR_SCORE_FIELDS per record
  uint64_t paths_found = 0, states_explored = 0;
  size_t size() const { return start_node.size(); }
};

// Checks the panel (the errors of shk_pcr_paths_panel) and runs every gene.  SHK_OK, or a code with *err set.
int pcr_paths_panel_run(uint32_t k, const shk_pcr_graphs *graphs, const shk_pcr_paths_params *params, std::vector<PcrGeneRecords> *out,
                        std::string *err);
// Copies records[g][pick[g][..]] (pick == nullptr: all, in order) into out under the capacity rule of shk_pcr_records.
int pcr_records_store(const std::vector<PcrGeneRecords> &records, const std::vector<std::vector<uint32_t>> *pick, shk_pcr_records *out,
                      std::string *err);
