// pcr_run_driver — a native caller of sPCR's host helpers in csrc/shk_front.cpp: the primer specification's parser
// (parse_pcr_primers_string, cli.rs:12-140), the validator and its report (pcr/mod.rs:295-399, cli.rs:528-554), the
// FASTA writer (io.rs:144-158) and the stats writer with pcr_results (stats.rs:11-45).  Built with AddressSanitizer and
// UBSan, the runtimes linked statically (make -C sharkmer_amd/csrc pcr_run_driver && ./pcr_run_driver [tmpdir]): the
// cases of tests/test_pcr_run_ref_cpu.py, tight buffers, and 10^4 random specifications.  CPU only; exit status 0 and
// "pcr_run_driver ok" when everything held.
#include "../../include/shk.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

static int failures = 0;
#define CHECK(cond)                                                    \
  do {                                                                 \
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

// the parse into exactly-sized heap buffers, so that a byte written past either end is seen
static int parse(const std::string &spec, shk_pcr_gene *g, std::vector<char> *strings, std::string *err, size_t err_cap = 256) {
  strings->assign(spec.size() + 3, 'x');
  std::vector<char> e(err_cap, 'x');
  const int rc = shk_pcr_parse_primers(spec.c_str(), g, strings->data(), strings->size(), e.data(), e.size());
  CHECK(memchr(e.data(), 0, e.size()) != nullptr);
  *err = e.data();
  return rc;
}

static void parser_cases() {
  shk_pcr_gene g;
  std::vector<char> s;
  std::string err;
  CHECK(parse("forward=grctgtttaccaaaaacata,reverse=AATTCAACATMGAGG,name=16s", &g, &s, &err) == SHK_OK && err.empty());
  CHECK(!strcmp(g.gene_name, "16s") && !strcmp(g.forward_seq, "GRCTGTTTACCAAAAACATA") && !strcmp(g.reverse_seq, "AATTCAACATMGAGG"));
  CHECK(g.min_length == 0 && g.max_length == 10000 && g.min_count == 2 && g.mismatches == 2 && g.trim == 15 && g.dedup_edit_threshold == 10);
  CHECK(g.max_dfs_states == 100000 && g.max_paths_per_pair == 20 && g.max_node_visits == 2 && g.max_primer_kmers == 40);
  CHECK(g.high_coverage_ratio == 10.0 && g.tip_coverage_fraction == 0.1);
  CHECK(parse("NAME=x,Forward=ac,REVERSE=gt,max-length=700,min-length=500,min-count=3,mismatches=1,trim=12,dedup-edit-threshold=4,"
              "citation=doi:10.1/x?a=b,notes=a=b=c", &g, &s, &err) == SHK_OK);
  CHECK(g.max_length == 700 && g.min_length == 500 && g.min_count == 3 && g.mismatches == 1 && g.trim == 12 && g.dedup_edit_threshold == 4);
  CHECK(parse("name=a=b,forward=AC,reverse=GT", &g, &s, &err) == SHK_OK && !strcmp(g.gene_name, "a=b"));
  CHECK(parse("max-length=18446744073709551615,name=n", &g, &s, &err) == SHK_OK && g.max_length == ~0ull);
  const struct { const char *spec, *text; } bad[] = {
      {"", "Invalid empty primer specification"},
      {"forward=AC,reverse", "Invalid parameter (should be key=value): 'reverse'\nCommas are not allowed in field values. Use --pcr-panel-file with a YAML panel for complex metadata."},
      {"name=x,Name=y", "Duplicate parameter 'name' in primer specification 'name=x,Name=y'. Each key may appear at most once."},
      {"name=x,colour=red", "Unexpected parameter: colour"},
      {"name=x,max-length=7k", "Invalid value for max-length: 7k"},
      {"name=x,max-length=18446744073709551616", "Invalid value for max-length: 18446744073709551616"},
      {"name=x,min-count=-1", "Invalid value for min-count: -1"},
      {"name=x,trim=", "Invalid value for trim: "},
      {"name=x,mismatches=4294967296", "Invalid value for mismatches: 4294967296"},
  };
  for (const auto &b : bad) {
    CHECK(parse(b.spec, &g, &s, &err, 512) == SHK_ERR_BAD_ARG);
    CHECK(err == b.text);
  }
  // a text longer than the buffer is cut, never overrun
  CHECK(parse("name=x,Name=y", &g, &s, &err, 8) == SHK_ERR_BAD_ARG && err == "Duplica");
  CHECK(parse("name=x,Name=y", &g, &s, &err, 1) == SHK_ERR_BAD_ARG && err.empty());
  // strings_cap too small is refused, not overrun
  std::vector<char> tight(5, 'x'), e(128);
  CHECK(shk_pcr_parse_primers("name=abc,forward=ACGT,reverse=TT", &g, tight.data(), tight.size(), e.data(), e.size()) == SHK_ERR_BAD_ARG);
}

static shk_pcr_gene gene(const char *name, const char *f, const char *r) {
  shk_pcr_gene g{};
  shk_pcr_gene_defaults(&g);
  g.gene_name = name, g.forward_seq = f, g.reverse_seq = r;
  return g;
}

static void validator_cases() {
  std::vector<char> buf(4096);
  shk_pcr_gene ok = gene("g", "ACGTAC", "TTGCA");
  CHECK(shk_pcr_validate_gene(&ok, buf.data(), buf.size()) == 0 && buf[0] == 0);
  shk_pcr_gene bad = gene("", "A", "A");
  bad.min_length = 5, bad.max_length = 0, bad.min_count = 0;
  CHECK(shk_pcr_validate_gene(&bad, buf.data(), buf.size()) == 6);
  CHECK(std::string(buf.data()) ==
        "Forward primer sequence is too short: 'A'\nPrimer sequences must be at least 2 bases\n"
        "Reverse primer sequence is too short: 'A'\nPrimer sequences must be at least 2 bases\n"
        "min-length (5) is greater than max-length (0)\nSwap the values or adjust the range\n"
        "min-count is 0, must be at least 2\nSet min-count to at least 2\n"
        "max-length is 0\nSet max-length to a positive value\n"
        "Gene name is empty\nProvide a unique name for the primer pair via the 'name' field\n");
  shk_pcr_gene chars = gene("c", "ACXGTZ", "ACXGTZ");
  CHECK(shk_pcr_validate_gene(&chars, buf.data(), buf.size()) == 3);
  CHECK(strstr(buf.data(), "Invalid nucleotide(s) X, Z in forward primer ACXGTZ\n") && strstr(buf.data(), "Forward and reverse primers are identical: ACXGTZ\n"));
  shk_pcr_gene high = gene("h", "AC\xC3\xA9GT", "TT\xFFGG");  // a two-byte character, and a byte that is none
  CHECK(shk_pcr_validate_gene(&high, buf.data(), buf.size()) == 2 && strstr(buf.data(), "Invalid nucleotide(s) \xC3\xA9 in forward primer"));
  CHECK(shk_pcr_validate_gene(&bad, nullptr, 0) == 6);
  std::vector<char> tiny(10, 'x');
  CHECK(shk_pcr_validate_gene(&bad, tiny.data(), tiny.size()) == 6 && strlen(tiny.data()) == 9);
  shk_pcr_gene nulls{};
  shk_pcr_gene_defaults(&nulls);
  CHECK(shk_pcr_validate_gene(&nulls, buf.data(), buf.size()) == 3);  // both primers too short, no name
  const shk_pcr_gene panel[3] = {gene("g", "ACGTAC", "TTGCA"), bad, chars};
  const char *sources[3] = {nullptr, "panel file 'p.yaml'", nullptr};
  CHECK(shk_pcr_validation_report(panel, 1, nullptr, buf.data(), buf.size()) == 0 && buf[0] == 0);
  CHECK(shk_pcr_validation_report(panel, 3, sources, buf.data(), buf.size()) == 9);
  const std::string rep = buf.data();
  CHECK(rep.rfind("Primer validation failed (9 errors):\n\n   (panel file 'p.yaml'):\n    - Forward primer sequence is too short: 'A'\n      Suggestion: ", 0) == 0);
  CHECK(rep.find("\n  c (--pcr-primers):\n    - Invalid nucleotide(s) X, Z in forward primer ACXGTZ\n") != std::string::npos);
  for (uint32_t s = 0; s < 8; ++s) CHECK((shk_pcr_failure_reason(s) == nullptr) == (s == 0 || s > 5));
}

static void writer_cases(const std::string &dir) {
  // records of 79, 80, 81, 160, 161 and 0 bases
  const uint64_t lens[6] = {79, 80, 81, 160, 161, 0};
  std::vector<uint64_t> soff(7, 0), cmin(6, 3), cmax(6, 30), roff = {0, 6};
  std::vector<double> mean(6, 12.345), median = {12.0, 12.5, 7.0, 0.5, 100.0, 3.0}, score(6, 0.125);
  for (int i = 0; i < 6; ++i) soff[i + 1] = soff[i] + lens[i];
  std::vector<uint8_t> seqs(soff[6]);  // (exactly as long as the records: a read past the last base is seen)
  for (size_t i = 0; i < seqs.size(); ++i) seqs[i] = "ACGT"[i % 4];
  shk_pcr_records R{};
  R.record_offsets = roff.data(), R.seq_offsets = soff.data(), R.seqs = seqs.data(), R.record_cap = 6, R.seq_cap = seqs.size();
  R.count_mean = mean.data(), R.count_median = median.data(), R.count_min = cmin.data(), R.count_max = cmax.data(), R.score = score.data();
  const shk_pcr_gene g = gene("18s", "AC", "GT");
  const std::string path = dir + "/pcr_run_driver.fasta";
  CHECK(shk_write_fasta(path.c_str(), "s1", &g, &R, 0, 6) == SHK_OK);
  const std::string text = slurp(path);
  CHECK(text.rfind(">s1_18s_0 sample=s1 gene=18s product=0 length=79 kmer_count_mean=12.35 kmer_count_median=12 kmer_count_min=3 kmer_count_max=30 score=0.12\n", 0) == 0);
  CHECK(text.find(" product=1 length=80 kmer_count_mean=12.35 kmer_count_median=12.5 ") != std::string::npos);
  CHECK(text.find(" product=3 length=160 kmer_count_mean=12.35 kmer_count_median=0.5 ") != std::string::npos);
  std::vector<size_t> widths;
  size_t headers = 0;
  for (size_t at = 0; at < text.size();) {
    const size_t nl = text.find('\n', at);
    CHECK(nl != std::string::npos);
    if (nl == std::string::npos) break;
    if (text[at] == '>') ++headers;
    else widths.push_back(nl - at);
    at = nl + 1;
  }
  CHECK(headers == 6 && (widths == std::vector<size_t>{79, 80, 80, 1, 80, 80, 80, 80, 1}));
  CHECK(shk_write_fasta(path.c_str(), "s1", &g, &R, 2, 1) == SHK_OK);  // a slice: record 2 as product 0
  CHECK(slurp(path).rfind(">s1_18s_0 sample=s1 gene=18s product=0 length=81 ", 0) == 0);
  CHECK(shk_write_fasta(path.c_str(), "s1", &g, &R, 0, 0) == SHK_OK && slurp(path).empty());
  CHECK(shk_write_fasta((dir + "/no/such/dir/x.fasta").c_str(), "s1", &g, &R, 0, 1) == SHK_ERR_IO);
  remove(path.c_str());

  shk_run_stats st{};
  st.sharkmer_version = "3.1.0", st.command = "shk_count -k 21 -s x", st.sample = "x";
  st.kmer_length = 21, st.chunks = 2, st.n_reads_read = 10, st.n_bases_read = 1500, st.n_subreads_ingested = 10, st.n_bases_ingested = 1490;
  st.n_kmers = 1300, st.n_multi_kmers = 900, st.n_singleton_kmers = 400, st.peak_memory_bytes = 7, st.has_histogram = 1;
  const std::string a = dir + "/pcr_run_driver_a.yaml", b = dir + "/pcr_run_driver_b.yaml";
  CHECK(shk_write_stats_yaml(a.c_str(), &st) == SHK_OK && shk_write_stats_yaml_pcr(b.c_str(), &st, nullptr, 0) == SHK_OK);
  const std::string head = slurp(a);
  CHECK(!head.empty() && head == slurp(b));
  const std::vector<uint64_t> two = {1780, 1779};
  const shk_pcr_gene_stat results[4] = {{"18s", SHK_PCR_SUCCESS, 2, two.data()}, {"co1", SHK_PCR_NO_FORWARD, 0, nullptr},
                                        {"16s: v2", SHK_PCR_NODE_BUDGET, 0, nullptr}, {"123", SHK_PCR_NO_PATH, 0, nullptr}};
  CHECK(shk_write_stats_yaml_pcr(b.c_str(), &st, results, 4) == SHK_OK);
  CHECK(slurp(b) == head + "pcr_results:\n"
                           "- gene_name: 18s\n  status: success\n  n_products: 2\n  product_lengths:\n  - 1780\n  - 1779\n"
                           "- gene_name: co1\n  status: fail\n  n_products: 0\n  failure_reason: forward primer not found\n"
                           "- gene_name: '16s: v2'\n  status: fail\n  n_products: 0\n  failure_reason: node budget exceeded\n"
                           "- gene_name: '123'\n  status: fail\n  n_products: 0\n  failure_reason: no path found\n");
  const shk_pcr_gene_stat no_lengths = {"x", SHK_PCR_SUCCESS, 2, nullptr};
  CHECK(shk_write_stats_yaml_pcr(b.c_str(), &st, &no_lengths, 1) == SHK_ERR_BAD_ARG);
  remove(a.c_str());
  remove(b.c_str());
}

// 10^4 specifications drawn from the pieces a user can type: whatever comes out, the parse either succeeds with
// strings inside the caller's buffer or fails with a text, and the validator takes what was parsed
static void random_specs() {
  std::mt19937_64 rng(20240611);
  const char *keys[] = {"name", "forward", "reverse", "max-length", "min-length", "min-count", "mismatches", "trim", "dedup-edit-threshold",
                        "citation", "notes", "Name", "FORWARD", "colour", "", "max-length "};
  const char *values[] = {"", "x", "18s", "ACGT", "acgtn", "GRCTGTTTACCAAAAACATA", "0", "1", "15", "700", "-1", "+5", "4294967295", "4294967296",
                          "18446744073709551615", "99999999999999999999999", "7k", " 5", "a=b", "=", "\xC3\xA9", "\xFF", "N N"};
  uint64_t ok = 0, refused = 0;
  std::vector<char> buf(8192);
  for (int it = 0; it < 10000; ++it) {
    std::string spec;
    const int n = (int)(rng() % 7);
    for (int i = 0; i < n; ++i) {
      if (i) spec += ',';
      const uint64_t shape = rng() % 16;
      if (shape == 0) {
        spec += values[rng() % (sizeof values / sizeof *values)];  // no '='
        continue;
      }
      spec += keys[rng() % (sizeof keys / sizeof *keys)];
      spec += '=';
      spec += values[rng() % (sizeof values / sizeof *values)];
    }
    shk_pcr_gene g;
    std::vector<char> s;
    std::string err;
    const int rc = parse(spec, &g, &s, &err, 64 + rng() % 512);
    CHECK(rc == SHK_OK || rc == SHK_ERR_BAD_ARG);
    CHECK((rc == SHK_OK) == err.empty());
    if (rc != SHK_OK) {
      ++refused;
      continue;
    }
    ++ok;
    for (const char *p : {g.gene_name, g.forward_seq, g.reverse_seq}) CHECK(p >= s.data() && p + strlen(p) < s.data() + s.size());
    const int ne = shk_pcr_validate_gene(&g, buf.data(), buf.size());
    CHECK(ne >= 0 && ne <= 9);
    CHECK(shk_pcr_validation_report(&g, 1, nullptr, buf.data(), buf.size()) == ne);
  }
  CHECK(ok > 500 && refused > 500);
}

int main(int argc, char **argv) {
  const std::string dir = argc > 1 ? argv[1] : (getenv("TMPDIR") ? getenv("TMPDIR") : "/tmp");
  parser_cases();
  validator_cases();
  writer_cases(dir);
  random_specs();
  if (failures) {
    fprintf(stderr, "pcr_run_driver: %d checks failed\n", failures);
    return 1;
  }
  printf("pcr_run_driver ok\n");
  return 0;
}
