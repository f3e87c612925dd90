// pcr_records_driver — a native caller of the record arrays' owner (PcrRecordArrays) and the record slice copy
// (pcr_records_slice) of csrc/shk_products.h, which the sPCR pipeline deals a sweep's records out with.  Built with
// AddressSanitizer and UBSan, the runtimes linked statically (make -C sharkmer_amd/csrc pcr_records_driver &&
// ./pcr_records_driver): slices at the start, in the middle, at the end and empty ones into exactly-sized heap arrays,
// every optional destination pointer absent, capacities short by one, grow-then-fits — each against pcr_records_store
// on the same records and the same destination capacities (code, text and every array).  CPU only; exit status 0 and
// "ok N" (N checks) when everything held.
#include "../../sharkmer_amd/csrc/shk_products.h"

#include <cstdio>
#include <cstring>
#include <memory>
#include <random>
#include <string>
#include <vector>

static long checks = 0;
static int failures = 0;
#define CHECK(cond)                                                    \
  do {                                                                 \
    ++checks;                                                          \
    if (!(cond)) {                                                     \
      fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
      ++failures;                                                      \
    }                                                                  \
  } while (0)

static const uint32_t F = SHK_PCR_SCORE_FIELDS;

// A destination whose arrays are exactly as long as its capacities say, so that a write past either end is seen;
// `present` bit i: optional array i is there (0 seq_offsets, 1 seqs, 2 start_node, 3 path_nodes, 4 count_mean,
// 5 count_median, 6 count_min, 7 count_max, 8 score, 9 score_fields).
struct Dest {
  std::vector<uint64_t> record_offsets{0, 0}, seq_offsets, path_nodes, count_min, count_max;
  std::unique_ptr<uint8_t[]> seqs;  // (an array of no bytes is still an array: seqs is there, with no room)
  std::vector<uint32_t> start_node;
  std::vector<double> count_mean, count_median, score, score_fields;
  shk_pcr_records r{};
  Dest(uint64_t record_cap, uint64_t seq_cap, uint32_t present) {
    seq_offsets.assign(record_cap + 1, 7), seqs.reset(new uint8_t[seq_cap]), memset(seqs.get(), 7, seq_cap), start_node.assign(record_cap, 7), path_nodes.assign(record_cap, 7);
    count_mean.assign(record_cap, 7), count_median.assign(record_cap, 7), count_min.assign(record_cap, 7), count_max.assign(record_cap, 7);
    score.assign(record_cap, 7), score_fields.assign(record_cap * F, 7);
    r.record_offsets = record_offsets.data(), r.record_cap = record_cap, r.seq_cap = seq_cap;
    if (present & 1) r.seq_offsets = seq_offsets.data();
    if (present & 2) r.seqs = seqs.get();
    if (present & 4) r.start_node = start_node.data();
    if (present & 8) r.path_nodes = path_nodes.data();
    if (present & 16) r.count_mean = count_mean.data();
    if (present & 32) r.count_median = count_median.data();
    if (present & 64) r.count_min = count_min.data();
    if (present & 128) r.count_max = count_max.data();
    if (present & 256) r.score = score.data();
    if (present & 512) r.score_fields = score_fields.data();
  }
  bool same_records(const Dest &o) const {
    return seq_offsets == o.seq_offsets && !memcmp(seqs.get(), o.seqs.get(), r.seq_cap) && start_node == o.start_node && path_nodes == o.path_nodes &&
           count_mean == o.count_mean && count_median == o.count_median && count_min == o.count_min && count_max == o.count_max &&
           score == o.score && score_fields == o.score_fields;
  }
};

// n records of lengths 0..40 in arrays a PcrRecordArrays owns (src) and as one gene's PcrGeneRecords (gene)
struct Source {
  PcrRecordArrays own{0, 0};
  shk_pcr_records src{};
  PcrGeneRecords gene;
  Source(uint32_t n, std::mt19937 &rng) {
    for (uint32_t i = 0; i < n; ++i) {
      const uint32_t len = i % 5 == 3 ? 0 : rng() % 41;
      for (uint32_t b = 0; b < len; ++b) gene.seqs.push_back("ACGT"[rng() % 4]);
      gene.seq_offsets.push_back(gene.seqs.size());
      gene.start_node.push_back(rng()), gene.path_nodes.push_back(rng()), gene.count_min.push_back(rng()), gene.count_max.push_back(rng());
      gene.count_mean.push_back(rng() / 7.0), gene.count_median.push_back(rng() / 3.0), gene.score.push_back(rng() / 11.0);
      for (uint32_t f = 0; f < F; ++f) gene.fields.push_back(rng() / 13.0);
    }
    own = PcrRecordArrays(n, gene.seqs.size());
    src = own.bind(1, PcrRecordArrays::ALL);
    src.n_records = n, src.n_seq_bytes = gene.seqs.size();
    own.record_offsets[1] = n;
    std::copy(gene.seq_offsets.begin(), gene.seq_offsets.end(), own.seq_offsets.begin());
    std::copy(gene.seqs.begin(), gene.seqs.end(), own.seqs.begin());
    std::copy(gene.start_node.begin(), gene.start_node.end(), own.start_node.begin());
    std::copy(gene.path_nodes.begin(), gene.path_nodes.end(), own.path_nodes.begin());
    std::copy(gene.count_min.begin(), gene.count_min.end(), own.count_min.begin());
    std::copy(gene.count_max.begin(), gene.count_max.end(), own.count_max.begin());
    std::copy(gene.count_mean.begin(), gene.count_mean.end(), own.count_mean.begin());
    std::copy(gene.count_median.begin(), gene.count_median.end(), own.count_median.begin());
    std::copy(gene.score.begin(), gene.score.end(), own.score.begin());
    std::copy(gene.fields.begin(), gene.fields.end(), own.score_fields.begin());
  }
  uint64_t bases(uint64_t r0, uint64_t nr) const { return gene.seq_offsets[r0 + nr] - gene.seq_offsets[r0]; }
};

// The slice [r0, r0 + nr) into a destination of these capacities and arrays, and pcr_records_store of the same records
// (picked out of the one gene) into another of the same: code, text, needs and every array agree.  Returns the code.
static int slice_case(const Source &s, uint64_t r0, uint64_t nr, uint64_t record_cap, uint64_t seq_cap, uint32_t present, std::string *text = nullptr) {
  Dest a(record_cap, seq_cap, present), b(record_cap, seq_cap, present);
  std::string ea, eb;
  const int ra = pcr_records_slice(s.src, r0, nr, &a.r, &ea);
  std::vector<std::vector<uint32_t>> pick(1);
  for (uint64_t i = 0; i < nr; ++i) pick[0].push_back((uint32_t)(r0 + i));
  const int rb = pcr_records_store({s.gene}, &pick, &b.r, &eb);
  CHECK(ra == rb && ea == eb);
  CHECK(a.r.n_records == nr && a.r.n_seq_bytes == s.bases(r0, nr));
  CHECK(a.r.n_records == b.r.n_records && a.r.n_seq_bytes == b.r.n_seq_bytes);
  CHECK(a.same_records(b));  // (a refused copy wrote nothing: both still hold the fill)
  const bool fits = nr <= record_cap && (!(present & 2) || s.bases(r0, nr) <= seq_cap);
  CHECK((ra == SHK_OK) == fits && (ra == SHK_OK || ra == SHK_ERR_BAD_ARG) && (ra == SHK_OK) == ea.empty());
  if (ra == SHK_OK && (present & 1)) CHECK(a.seq_offsets[0] == 0 && a.seq_offsets[nr] == s.bases(r0, nr));
  if (ra == SHK_OK && (present & 2)) CHECK(!memcmp(a.seqs.get(), s.gene.seqs.data() + s.gene.seq_offsets[r0], s.bases(r0, nr)));
  if (text) *text = ea;
  return ra;
}

static void slices() {
  std::mt19937 rng(24);
  const Source s(23, rng);
  const uint32_t all = 1023;
  for (const uint32_t present : {all, 0u, 1u, 2u, 3u, all & ~2u, all & ~1u, 512u, 4u | 256u}) {
    for (const auto &[r0, nr] : std::vector<std::pair<uint64_t, uint64_t>>{{0, 5}, {9, 7}, {18, 5}, {0, 23}, {0, 0}, {11, 0}, {23, 0}, {3, 1}, {22, 1}}) {
      const uint64_t nb = s.bases(r0, nr);
      CHECK(slice_case(s, r0, nr, nr, nb, present) == SHK_OK);  // exactly sized
      CHECK(slice_case(s, r0, nr, nr + 3, nb + 9, present) == SHK_OK);
      std::string text;
      if (nr) {  // record_cap short by one
        CHECK(slice_case(s, r0, nr, nr - 1, nb, present, &text) == SHK_ERR_BAD_ARG);
        CHECK(text == std::to_string(nr) + " records of " + std::to_string(nb) + " bases do not fit record_cap " + std::to_string(nr - 1) +
                          " / seq_cap " + std::to_string(nb));
      }
      if (nb)  // seq_cap short by one: short with seqs, not short without (nothing is written there)
        CHECK(slice_case(s, r0, nr, nr, nb - 1, present, &text) == ((present & 2) ? SHK_ERR_BAD_ARG : SHK_OK));
    }
  }
  for (int it = 0; it < 2000; ++it) {  // random slices, capacities around what they need, random optional arrays
    const uint64_t r0 = rng() % 24, nr = rng() % (24 - r0), nb = s.bases(r0, nr);
    slice_case(s, r0, nr, nr + rng() % 3 - (nr ? rng() % 2 : 0), nb + rng() % 3 - (nb ? rng() % 2 : 0), rng() % 1024);
  }
}

static void owner() {
  std::mt19937 rng(25);
  const Source s(12, rng);
  PcrRecordArrays own(1, 1);  // a first guess that is short of both
  shk_pcr_records r = own.bind(3, PcrRecordArrays::ALL);
  CHECK(r.record_cap == 1 && r.seq_cap == 1 && r.start_node && r.path_nodes && r.score_fields && r.paths_found && r.generated && r.states_explored);
  CHECK(own.record_offsets.size() == 4 && own.seq_offsets.size() == 2 && own.paths_found.size() == 3);
  std::string err;
  CHECK(pcr_records_slice(s.src, 2, 9, &r, &err) == SHK_ERR_BAD_ARG && PcrRecordArrays::is_short(r));
  own.grow(r);
  CHECK(own.record_cap == 9 && own.seq_cap == s.bases(2, 9));
  r = own.bind(3, PcrRecordArrays::ALL);  // exactly what the call reported: it fits, to the last element
  err.clear();
  CHECK(pcr_records_slice(s.src, 2, 9, &r, &err) == SHK_OK && err.empty() && !PcrRecordArrays::is_short(r));
  CHECK(own.seq_offsets.size() == 10 && own.seq_offsets[9] == s.bases(2, 9) && own.start_node[8] == s.gene.start_node[10]);
  CHECK(own.score_fields.size() == 9 * F && own.score_fields[9 * F - 1] == s.gene.fields[11 * F - 1]);
  own.grow(r);  // (what fitted grows nothing)
  CHECK(own.record_cap == 9 && own.seq_cap == s.bases(2, 9));
  // the choice of optional arrays; no genes, no room: still arrays to point to
  PcrRecordArrays few(0, 0);
  r = few.bind(0, 0);
  CHECK(r.record_offsets && r.seq_offsets && r.seqs && r.count_mean && r.count_median && r.count_min && r.count_max && r.score);
  CHECK(!r.start_node && !r.path_nodes && !r.score_fields && !r.paths_found && !r.generated && !r.states_explored);
  CHECK(pcr_records_slice(s.src, 5, 0, &r, &err) == SHK_OK && r.n_records == 0 && !PcrRecordArrays::is_short(r));
  r = few.bind(2, PcrRecordArrays::NODES);
  CHECK(r.start_node && r.path_nodes && !r.score_fields && !r.paths_found);
  r = few.bind(2, PcrRecordArrays::SCORE_FIELDS | PcrRecordArrays::PER_GENE);
  CHECK(!r.start_node && r.score_fields && r.paths_found && r.generated && r.states_explored && few.generated.size() == 2);
}

int main() {
  slices();
  owner();
  if (failures) {
    fprintf(stderr, "pcr_records_driver: %d failures\n", failures);
    return 1;
  }
  printf("ok %ld\n", checks);
  return 0;
}
