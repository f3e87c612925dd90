// pcr_depths_driver — a native caller of the depth sweep's host helpers in csrc/shk_front.cpp: the
// --pcr-depths value's parser, the depth-list check and the {sample}.pcr_depths.tsv writer.  Built with AddressSanitizer
// and UBSan, the runtimes linked statically (make -C sharkmer_amd/csrc pcr_depths_driver && ./pcr_depths_driver [tmpdir]):
// the cases of the command line, exactly-sized buffers, and random lists against a plain model.  CPU only; exit status 0
// and "ok N" (N checks) when everything held.
#include "../../include/shk.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
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

static std::string slurp(const std::string &path) {
  std::string out;
  if (FILE *f = fopen(path.c_str(), "rb")) {
    char buf[4096];
    for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;) out.append(buf, n);
    fclose(f);
  }
  return out;
}

// the parse into exactly-sized heap buffers, so that a write past either end is seen
static int parse(const std::string &spec, uint32_t chunks, size_t cap, std::vector<uint32_t> *out, uint64_t *n, std::string *err, size_t err_cap = 200) {
  std::vector<uint32_t> d(cap, 0xABABABABu);
  std::vector<char> e(err_cap, 'x');
  const int rc = shk_pcr_parse_depths(spec.c_str(), chunks, cap ? d.data() : nullptr, cap, n, e.data(), e.size());
  CHECK(memchr(e.data(), 0, e.size()) != nullptr);
  *err = e.data();
  *out = d;
  return rc;
}

// the model: what a list must be
static bool model_ok(const std::vector<uint32_t> &d, uint32_t chunks) {
  if (chunks == 0 || d.empty()) return false;
  for (size_t j = 0; j < d.size(); ++j)
    if (d[j] == 0 || d[j] > chunks || (j && d[j] <= d[j - 1])) return false;
  return true;
}

static void parser_cases() {
  std::vector<uint32_t> d;
  uint64_t n = 0;
  std::string err;
  CHECK(parse("all", 3, 3, &d, &n, &err) == SHK_OK && n == 3 && d == std::vector<uint32_t>({1, 2, 3}) && err.empty());
  CHECK(parse("all", 1, 1, &d, &n, &err) == SHK_OK && n == 1 && d[0] == 1);
  CHECK(parse("2", 3, 1, &d, &n, &err) == SHK_OK && n == 1 && d[0] == 2);
  CHECK(parse("1,3", 3, 2, &d, &n, &err) == SHK_OK && n == 2 && d[0] == 1 && d[1] == 3);
  CHECK(parse("+1,3", 3, 2, &d, &n, &err) == SHK_OK && n == 2);
  CHECK(parse("all", 0, 4, &d, &n, &err) == SHK_ERR_BAD_ARG && err.find("--chunks of at least 1") != std::string::npos);
  CHECK(parse("1", 0, 4, &d, &n, &err) == SHK_ERR_BAD_ARG && err.find("--chunks of at least 1") != std::string::npos);
  CHECK(parse("4", 3, 4, &d, &n, &err) == SHK_ERR_BAD_ARG && err.find("depth 4 is not in 1..3") != std::string::npos);
  CHECK(parse("0,1", 3, 4, &d, &n, &err) == SHK_ERR_BAD_ARG && err.find("depth 0 is not in 1..3") != std::string::npos);
  CHECK(parse("2,2", 3, 4, &d, &n, &err) == SHK_ERR_BAD_ARG && err.find("strictly ascending (2 after 2)") != std::string::npos);
  CHECK(parse("3,1", 3, 4, &d, &n, &err) == SHK_ERR_BAD_ARG && err.find("strictly ascending (1 after 3)") != std::string::npos);
  for (const char *bad : {"", ",", "1,", ",1", "1,,2", "ALL", "all,1", "1 ,2", "-1", "1.5", "99999999999", "x"})
    CHECK(parse(bad, 3, 4, &d, &n, &err) == SHK_ERR_BAD_ARG && err.find("neither 'all' nor a list") != std::string::npos);
  // too little room: the count is reported, nothing is written
  CHECK(parse("all", 5, 2, &d, &n, &err) == SHK_ERR_BAD_ARG && n == 5 && d[0] == 0xABABABABu && d[1] == 0xABABABABu);
  CHECK(parse("all", 5, 0, &d, &n, &err) == SHK_ERR_BAD_ARG && n == 5);
  // an error text longer than its buffer is cut, with its NUL
  CHECK(parse("3,1", 3, 4, &d, &n, &err, 8) == SHK_ERR_BAD_ARG && err.size() == 7);
  CHECK(shk_pcr_parse_depths(nullptr, 3, nullptr, 0, &n, nullptr, 0) == SHK_ERR_BAD_ARG);
  CHECK(shk_pcr_parse_depths("1", 3, nullptr, 0, nullptr, nullptr, 0) == SHK_ERR_BAD_ARG);
  CHECK(shk_pcr_check_depths(nullptr, 0, 3, nullptr, 0) == SHK_ERR_BAD_ARG);
  const uint32_t one = 1;
  CHECK(shk_pcr_check_depths(&one, 1, 1, nullptr, 0) == SHK_OK);
}

static void random_lists() {
  std::mt19937 rng(23);
  for (int it = 0; it < 20000; ++it) {
    const uint32_t chunks = rng() % 6;
    std::vector<uint32_t> want(rng() % 5);
    for (uint32_t &x : want) x = rng() % 7;
    if (rng() % 2) {  // often a valid one
      want.clear();
      for (uint32_t c = 1; c <= chunks; ++c)
        if (rng() % 2) want.push_back(c);
    }
    std::string spec;
    for (size_t j = 0; j < want.size(); ++j) spec += (j ? "," : "") + std::to_string(want[j]);
    std::vector<uint32_t> got;
    uint64_t n = 0;
    std::string err;
    const int rc = parse(spec, chunks, want.size(), &got, &n, &err);
    const bool ok = model_ok(want, chunks);
    CHECK((rc == SHK_OK) == ok);
    CHECK(ok ? (n == want.size() && got == want && err.empty()) : !err.empty());
    std::vector<char> e(64, 'x');
    CHECK((shk_pcr_check_depths(want.empty() ? nullptr : want.data(), want.size(), chunks, e.data(), e.size()) == SHK_OK) == ok);
    CHECK(memchr(e.data(), 0, e.size()) != nullptr);
  }
}

static void tsv(const std::string &tmp) {
  const std::string path = tmp + "/s.pcr_depths.tsv";
  const std::vector<uint64_t> lengths = {1731, 250, 99};  // exactly sized: a read past a row's lengths is seen
  std::vector<shk_pcr_depth_row> rows = {
      {1, 0, 3804, {"18s", SHK_PCR_NO_PRIMERS, 0, nullptr}},
      {1, 0, 3804, {"co1", SHK_PCR_NODE_BUDGET, 0, nullptr}},
      {2, 0, 7608, {"18s", SHK_PCR_SUCCESS, 1, lengths.data()}},
      {2, 0, 7608, {"co1", SHK_PCR_SUCCESS, 2, lengths.data() + 1}},
      {3, 0, 18446744073709551615ull, {"odd", 77, 0, nullptr}},
  };
  CHECK(shk_write_pcr_depths_tsv(path.c_str(), rows.data(), rows.size()) == SHK_OK);
  CHECK(slurp(path) ==
        "depth\tn_bases_ingested\tgene\tstatus\tfailure_reason\tn_products\tproduct_lengths\n"
        "1\t3804\t18s\tfail\tforward and reverse primers not found\t0\t\n"
        "1\t3804\tco1\tfail\tnode budget exceeded\t0\t\n"
        "2\t7608\t18s\tsuccess\t\t1\t1731\n"
        "2\t7608\tco1\tsuccess\t\t2\t250,99\n"
        "3\t18446744073709551615\todd\tfail\tunknown (no reason reported by PCR pipeline)\t0\t\n");
  CHECK(shk_write_pcr_depths_tsv(path.c_str(), nullptr, 0) == SHK_OK);
  CHECK(slurp(path) == "depth\tn_bases_ingested\tgene\tstatus\tfailure_reason\tn_products\tproduct_lengths\n");
  CHECK(shk_write_pcr_depths_tsv(nullptr, rows.data(), 1) == SHK_ERR_BAD_ARG);
  CHECK(shk_write_pcr_depths_tsv(path.c_str(), nullptr, 1) == SHK_ERR_BAD_ARG);
  shk_pcr_depth_row bad = rows[2];
  bad.gene.product_lengths = nullptr;
  CHECK(shk_write_pcr_depths_tsv(path.c_str(), &bad, 1) == SHK_ERR_BAD_ARG);
  bad = rows[0];
  bad.gene.gene_name = nullptr;
  CHECK(shk_write_pcr_depths_tsv(path.c_str(), &bad, 1) == SHK_ERR_BAD_ARG);
  CHECK(shk_write_pcr_depths_tsv((tmp + "/no/such/dir/x.tsv").c_str(), rows.data(), 1) == SHK_ERR_IO);
}

int main(int argc, char **argv) {
  const std::string tmp = argc > 1 ? argv[1] : "/tmp";
  parser_cases();
  random_lists();
  tsv(tmp);
  if (failures) {
    fprintf(stderr, "pcr_depths_driver: %d failures\n", failures);
    return 1;
  }
  printf("ok %ld\n", checks);
  return 0;
}
