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
// The capacity rule itself, for out's n_records and n_seq_bytes: SHK_OK, or SHK_ERR_BAD_ARG with the text in *err (seq_cap
// binds only where seqs is given).
int pcr_records_fit(const shk_pcr_records &out, std::string *err);
// Copies records [r0, r0 + nr) of src (which carries every record array) into out from record 0 on, under the same rule
// and out's optional pointers: n_records and n_seq_bytes always, the records when they fit.  The per-gene arrays of out
// (record_offsets, paths_found, generated, states_explored) are the caller's to fill.
int pcr_records_slice(const shk_pcr_records &src, uint64_t r0, uint64_t nr, shk_pcr_records *out, std::string *err);

// The arrays a shk_pcr_records points to, owned: bind() hands them out at the capacities held, a call fills them, and where
// that call came back is_short(), grow() takes what it reported for the next bind().
struct PcrRecordArrays {
  enum : uint32_t { NODES = 1, SCORE_FIELDS = 2, PER_GENE = 4, ALL = 7 };  // the optional arrays bind() carries
  uint64_t record_cap = 0, seq_cap = 0;
  std::vector<uint64_t> record_offsets, seq_offsets, path_nodes, count_min, count_max, paths_found, generated, states_explored;
  std::vector<uint8_t> seqs;
  std::vector<uint32_t> start_node;
  std::vector<double> count_mean, count_median, score, score_fields;

  PcrRecordArrays(uint64_t record_cap_, uint64_t seq_cap_) : record_cap(record_cap_), seq_cap(seq_cap_) {}
  // Every array zeroed at the capacities held; always: record_offsets, seq_offsets, seqs, the four counts and score; with
  // NODES start_node and path_nodes, with SCORE_FIELDS score_fields, with PER_GENE paths_found, generated, states_explored.
  shk_pcr_records bind(uint32_t n_genes, uint32_t carry) {
    const uint64_t n = record_cap ? record_cap : 1, ng = n_genes ? n_genes : 1;
    shk_pcr_records r{};
    record_offsets.assign((size_t)n_genes + 1, 0), seq_offsets.assign(record_cap + 1, 0), seqs.assign(seq_cap ? seq_cap : 1, 0);
    count_mean.assign(n, 0), count_median.assign(n, 0), count_min.assign(n, 0), count_max.assign(n, 0), score.assign(n, 0);
    r.record_offsets = record_offsets.data(), r.seq_offsets = seq_offsets.data(), r.seqs = seqs.data();
    r.record_cap = record_cap, r.seq_cap = seq_cap;
    r.count_mean = count_mean.data(), r.count_median = count_median.data(), r.count_min = count_min.data(), r.count_max = count_max.data();
    r.score = score.data();
    if (carry & NODES) start_node.assign(n, 0), path_nodes.assign(n, 0), r.start_node = start_node.data(), r.path_nodes = path_nodes.data();
    if (carry & SCORE_FIELDS) score_fields.assign(n * SHK_PCR_SCORE_FIELDS, 0), r.score_fields = score_fields.data();
    if (carry & PER_GENE) {
      paths_found.assign(ng, 0), generated.assign(ng, 0), states_explored.assign(ng, 0);
      r.paths_found = paths_found.data(), r.generated = generated.data(), r.states_explored = states_explored.data();
    }
    return r;
  }
  // What a finished call left in r: more than r had room for.
  static bool is_short(const shk_pcr_records &r) { return r.n_records > r.record_cap || r.n_seq_bytes > r.seq_cap; }
  void grow(const shk_pcr_records &r) {
    if (r.n_records > record_cap) record_cap = r.n_records;
    if (r.n_seq_bytes > seq_cap) seq_cap = r.n_seq_bytes;
  }
};
