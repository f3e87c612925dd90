// shk_count — sharkmer's counting-related command line over libshk:
//   shk_count -k 21 --chunks 10 --histo-max 10000 -m 1000000 -s sample -o outdir/ reads.fastq.gz …
// Flags mirror the reference's clap definitions (src/cli.rs:165-232): -k (default 19), --chunks
// (0), --histo-max (10000), -m/--max-reads, -s/--sample, -o/--outdir ("./"), -t/--threads
// (accepted; counting was single-threaded in the reference and is on the GPU here),
// --validate-every (0).  sPCR (cli.rs:12-140, 234-330; main.rs:33-56, 133-199): --pcr-primers SPEC (repeatable),
// --min-kmer-count (2), --read-threading, --node-budget-global, and the six global tuning flags that overwrite every
// gene's values as the reference does: --max-dfs-states, --max-paths-per-pair, --max-node-visits, --max-primer-kmers,
// --high-coverage-ratio, --tip-coverage-fraction; --pcr-depths all|d1,d2,… (not a reference flag: with --pcr-primers and
// --chunks >= 1, the panel at every listed cumulative chunk from the one count — {sample}_{gene}.depth{d}.fasta and
// {sample}.pcr_depths.tsv; refused with --read-threading and with more than one device).  With a gene, {sample}_{gene}.fasta is written for every gene with
// products and the stats file carries pcr_results.  Exit status and "Error: …" on stderr follow anyhow's main().
#include "../../include/shk.h"

#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

static bool parse_u64(const char *s, unsigned long long *out) {
  if (!s || !*s) return false;
  char *end = nullptr;
  *out = strtoull(s, &end, 10);
  return end && *end == 0;
}

int main(int argc, char **argv) {
  bool gzip_all = false;
  uint32_t bgzf_flags = 0;  // --bgzf-batch / --bgzf-device
  unsigned long long k = 19, chunks = 0, histo_max = 10000, max_reads = 0, validate_every = 0, threads = 1,
                     device = 0, hint = 0;
  const char *sample = nullptr, *outdir = "./";
  std::vector<int32_t> devices;  // --devices 0,1,2,3: one multi-device context (not a reference flag)
  std::vector<const char *> inputs;
  std::vector<const char *> specs;  // --pcr-primers, in order
  bool read_threading = false;
  const char *pcr_depths = nullptr;  // --pcr-depths
  bool group_graph = false;  // --group-graph: sPCR over --devices (SHK_FLAG_GROUP_GRAPH; not a reference flag)
  bool group_reads = false;  // --group-reads: --read-threading over --devices (SHK_FLAG_GROUP_READS; not a reference flag)
  unsigned long long min_kmer_count = 2, node_budget = 0, max_dfs_states = 100000, max_paths_per_pair = 20, max_node_visits = 2,
                     max_primer_kmers = 40;
  double high_coverage_ratio = 10.0, tip_coverage_fraction = 0.1;
  std::string command;
  for (int i = 0; i < argc; ++i) {
    if (i) command += ' ';
    command += argv[i];
  }
  auto need = [&](int &i, const char *flag) -> const char * {
    if (i + 1 >= argc) {
      fprintf(stderr, "error: a value is required for '%s' but none was supplied\n", flag);
      exit(2);
    }
    return argv[++i];
  };
  for (int i = 1; i < argc; ++i) {
    std::string a = argv[i];
    const char *val = nullptr;
    auto eq = a.find('=');
    std::string key = a, inl;
    if (a.rfind("--", 0) == 0 && eq != std::string::npos) {
      key = a.substr(0, eq);
      inl = a.substr(eq + 1);
      val = inl.c_str();
    }
    auto num = [&](unsigned long long *dst) {
      const char *v = val ? val : need(i, key.c_str());
      if (!parse_u64(v, dst)) {
        fprintf(stderr, "error: invalid value '%s' for '%s'\n", v, key.c_str());
        exit(2);
      }
    };
    auto real = [&](double *dst) {
      const char *v = val ? val : need(i, key.c_str());
      char *end = nullptr;
      *dst = strtod(v, &end);
      if (!*v || !end || *end) {
        fprintf(stderr, "error: invalid value '%s' for '%s'\n", v, key.c_str());
        exit(2);
      }
    };
    if (key == "-k") num(&k);
    else if (key == "--pcr-primers") specs.push_back(val ? argv[i] + eq + 1 : need(i, key.c_str()));
    else if (key == "--min-kmer-count") num(&min_kmer_count);
    else if (key == "--read-threading") read_threading = true;
    else if (key == "--pcr-depths") pcr_depths = val ? argv[i] + eq + 1 : need(i, key.c_str());
    else if (key == "--group-graph") group_graph = true;
    else if (key == "--group-reads") group_reads = true;
    else if (key == "--node-budget-global") num(&node_budget);
    else if (key == "--max-dfs-states") num(&max_dfs_states);
    else if (key == "--max-paths-per-pair") num(&max_paths_per_pair);
    else if (key == "--max-node-visits") num(&max_node_visits);
    else if (key == "--max-primer-kmers") num(&max_primer_kmers);
    else if (key == "--high-coverage-ratio") real(&high_coverage_ratio);
    else if (key == "--tip-coverage-fraction") real(&tip_coverage_fraction);
    else if (key == "--chunks") num(&chunks);
    else if (key == "--histo-max") num(&histo_max);
    else if (key == "-m" || key == "--max-reads") num(&max_reads);
    else if (key == "--validate-every") num(&validate_every);
    else if (key == "--gzip-all-members") gzip_all = true;  // (not a sharkmer flag: sharkmer reads a gzip file's first member)
    else if (key == "--bgzf-batch") bgzf_flags |= SHK_FASTQ_BGZF_BATCH;    // (nor these: every member, BGZF members in batches on host threads …
    else if (key == "--bgzf-device") bgzf_flags |= SHK_FASTQ_BGZF_DEVICE;  //  … or on the device)
    else if (key == "--device-parse") bgzf_flags |= SHK_FASTQ_DEVICE_PARSE;  // (with --bgzf-device: the text stays on the device and is framed there)
    else if (key == "-t" || key == "--threads") num(&threads);
    else if (key == "--device") num(&device);
    else if (key == "--capacity-hint") num(&hint);
    else if (key == "--devices") {
      const char *v = val ? val : need(i, key.c_str());
      for (const char *p = v; *p;) {
        char *end = nullptr;
        devices.push_back((int32_t)strtol(p, &end, 10));
        if (end == p) {
          fprintf(stderr, "error: invalid value '%s' for '--devices'\n", v);
          return 2;
        }
        p = *end == ',' ? end + 1 : end;
      }
    }
    else if (key == "-s" || key == "--sample") sample = val ? argv[i] + eq + 1 : need(i, key.c_str());
    else if (key == "-o" || key == "--outdir") outdir = val ? argv[i] + eq + 1 : need(i, key.c_str());
    else if (key == "-h" || key == "--help") {
      printf("Usage: shk_count [-k K] [--chunks N] [--histo-max M] [-m READS] -s SAMPLE [-o OUTDIR] "
             "[--validate-every N] [--gzip-all-members] [--bgzf-batch | --bgzf-device [--device-parse]] [--pcr-primers \"forward=...,reverse=...,name=...\"]... "
             "[--min-kmer-count N] [--read-threading] [--pcr-depths all|D1,D2,...] [--node-budget-global N] [--devices 0,1,... [--group-graph] [--group-reads]] [FASTQ[.gz] ...]\n");
      return 0;
    } else if (a.size() > 1 && a[0] == '-' && a != "-") {
      fprintf(stderr, "error: unexpected argument '%s' found\n", a.c_str());
      return 2;
    } else {
      inputs.push_back(argv[i]);
    }
  }
  // collect_pcr_params (cli.rs:521-554) and the global tuning flags (main.rs:49-56)
  std::vector<shk_pcr_gene> genes(specs.size());
  std::vector<std::vector<char>> strings(specs.size());
  for (size_t g = 0; g < specs.size(); ++g) {
    char err[1024];
    strings[g].resize(strlen(specs[g]) + 3);
    if (shk_pcr_parse_primers(specs[g], &genes[g], strings[g].data(), strings[g].size(), err, sizeof err) != SHK_OK) {
      fprintf(stderr, "Error: Could not parse primer specification: \"%s\"\n\nCaused by:\n    %s\n", specs[g], err);
      return 1;
    }
    genes[g].max_dfs_states = max_dfs_states, genes[g].max_paths_per_pair = max_paths_per_pair, genes[g].max_node_visits = max_node_visits;
    genes[g].max_primer_kmers = (uint32_t)max_primer_kmers;
    genes[g].high_coverage_ratio = high_coverage_ratio, genes[g].tip_coverage_fraction = tip_coverage_fraction;
  }
  if (min_kmer_count < 1) {  // cli.rs validate_args
    fprintf(stderr, "Error: min-kmer-count must be at least 1\n");
    return 1;
  }
  std::vector<uint32_t> depths;
  if (pcr_depths) {  // refused before a read is read
    if (genes.empty()) {
      fprintf(stderr, "Error: --pcr-depths needs --pcr-primers\n");
      return 1;
    }
    if (read_threading) {
      fprintf(stderr, "Error: --pcr-depths takes no --read-threading: a depth sweep takes no reads\n");
      return 1;
    }
    if (devices.size() > 1) {
      fprintf(stderr, "Error: --pcr-depths needs one device: no depths on a multi-device context\n");
      return 1;
    }
    char err[256];
    uint64_t n = 0;
    depths.resize(std::max<size_t>(chunks < (1ull << 32) ? (size_t)chunks : 0, strlen(pcr_depths)) + 1);
    if (shk_pcr_parse_depths(pcr_depths, (uint32_t)std::min<unsigned long long>(chunks, 0xFFFFFFFFull), depths.data(), depths.size(), &n, err,
                             sizeof err) != SHK_OK) {
      fprintf(stderr, "Error: %s\n", err);
      return 1;
    }
    depths.resize(n);
  }
  shk_pcr_file_config pcr{};
  pcr.depths = depths.empty() ? nullptr : depths.data();
  pcr.n_depths = depths.size();
  pcr.genes = genes.data();
  pcr.n_genes = (uint32_t)genes.size();
  pcr.min_kmer_count = (uint32_t)min_kmer_count;
  pcr.read_threading = read_threading;
  pcr.context_flags = (group_graph ? SHK_FLAG_GROUP_GRAPH : 0) | (group_reads ? SHK_FLAG_GROUP_READS : 0);
  pcr.node_budget_global = node_budget;
  shk_run_config rc{};
  rc.inputs = inputs.data();
  rc.n_inputs = (uint32_t)inputs.size();
  rc.k = (uint32_t)k;
  rc.chunks = (uint32_t)chunks;
  rc.device = (int32_t)device;
  rc.histo_max = histo_max;
  rc.max_reads = max_reads;
  rc.validate_every = validate_every;
  rc.fastq_flags = (gzip_all ? SHK_FASTQ_GZIP_ALL_MEMBERS : 0) | bgzf_flags;
  rc.sample = sample;
  rc.outdir = outdir;
  rc.command = command.c_str();
  rc.table_capacity_hint = hint;
  rc.n_devices = (uint32_t)devices.size();
  rc.device_ids = devices.empty() ? nullptr : devices.data();
  shk_run_stats st{};
  int rcode = genes.empty() ? shk_run_files(&rc, &st) : shk_run_files_pcr(&rc, &pcr, &st, nullptr);
  if (rcode != SHK_OK) {
    fprintf(stderr, "Error: %s\n", shk_run_error());
    return 1;
  }
  fprintf(stderr, "%llu reads, %llu kmers\n", (unsigned long long)st.n_reads_read, (unsigned long long)st.n_kmers);
  return 0;
}
