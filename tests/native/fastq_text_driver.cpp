// fastq_text_driver.cpp — the host shim (one lane in the wave's place) of shk_fastq_text_core.h, the bodies of the
// K_FASTQ kernels, under AddressSanitizer and UBSan (make -C sharkmer_amd/csrc fastq_text_driver;
// tests/test_fastq_text_core_cpu.py).
//
//   fastq_text_driver parse FILE    every case of FILE (tests/fastq_text_cases.py: write_case_file) framed by the core's
//                                   passes must give exactly what the file says: result words, offsets, bases
//   fastq_text_driver crc SEED N    N random extents of 0..70000 bytes (and the lengths round the shares' borders) at
//                                   random alignments: the 64 shares' parts, combined and conditioned, against
//                                   crc32_update
//   fastq_text_driver plan FILE BUDGET...   bgzf_plan_batch over FILE, batch after batch to the file's end or to the first
//                                   member it does not take, once per budget (bytes): per batch the member count,
//                                   out_bytes, where it begins and ends in the file, the first and the last job
//   fastq_text_driver inside        bgzf_jobs_inside on jobs at the batch's edges and near UINT64_MAX
//   fastq_text_driver budget DEFAULT   bgzf_batch_budget(DEFAULT) under the environment it is started in
// The text lies at the case's alignment in an allocation that ends with its last byte, the line table has exactly
// the text's lines, and bases and offsets have exactly the expected sizes between guard bytes: a read or a write
// outside any of them is the sanitizer's, or a guard's, to report.
#include "../../sharkmer_amd/csrc/shk_fastq_text_core.h"
#include "../../sharkmer_amd/csrc/shk_inflate.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace shk;

static const size_t GUARD = 64;

static std::vector<uint8_t> slurp(const char *path) {
  std::vector<uint8_t> v;
  FILE *f = fopen(path, "rb");
  if (!f) {
    fprintf(stderr, "cannot open %s\n", path);
    exit(2);
  }
  uint8_t buf[65536];
  size_t n;
  while ((n = fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + n);
  fclose(f);
  return v;
}
struct Cursor {
  const std::vector<uint8_t> &v;
  size_t at = 0;
  const uint8_t *take(size_t n) {
    if (at + n > v.size()) {
      fprintf(stderr, "the case file ends early\n");
      exit(2);
    }
    const uint8_t *p = v.data() + at;
    at += n;
    return p;
  }
  uint64_t u64() {
    uint64_t x;
    memcpy(&x, take(8), 8);
    return x;
  }
  uint32_t u32() {
    uint32_t x;
    memcpy(&x, take(4), 4);
    return x;
  }
};
static bool guards_ok(const uint8_t *block, size_t payload) {
  for (size_t i = 0; i < GUARD; ++i)
    if (block[i] != 0xC3 || block[GUARD + payload + i] != 0xC3) return false;
  return true;
}

static int run_parse(const char *path) {
  const std::vector<uint8_t> file = slurp(path);
  Cursor in{file};
  const uint32_t n_cases = in.u32();
  uint64_t n_records = 0;
  for (uint32_t k = 0; k < n_cases; ++k) {
    const uint32_t name_len = in.u32();
    const std::string name((const char *)in.take(name_len), name_len);
    FqSerialParams p;
    p.first_record = in.u64();
    p.validate_every = in.u64();
    p.max_records = in.u64();
    p.last = in.u64() != 0;
    const uint64_t align = in.u64(), n = in.u64();
    FqResultWords want;
    want.n_records = in.u64();
    want.n_bases = in.u64();
    want.bytes_consumed = in.u64();
    want.anomaly_record = in.u64();
    want.anomaly_kind = (uint32_t)in.u64();
    const uint8_t *text_src = in.take(n), *want_offsets = in.take((want.n_records + 1) * 8), *want_bases = in.take(want.n_bases);
    // the text: `align` bytes into an allocation (16-byte aligned) that ends with the text's last byte
    uint8_t *tb = (uint8_t *)malloc(align + n ? (size_t)(align + n) : 1);
    uint8_t *text = tb + align;
    memcpy(text, text_src, n);
    uint64_t n_nl = 0;
    for (uint64_t i = 0; i < n; ++i) n_nl += text_src[i] == '\n';
    uint64_t n_look = fq_n_lines(n, n_nl, p.last, n && text_src[n - 1] == '\n') / 4;
    if (p.max_records && n_look > p.max_records) n_look = p.max_records;
    uint32_t *line_end = (uint32_t *)malloc(n_nl * 4 + 4);
    // bases: the looked-at records' sequences may be more than the emitted ones'; their room is the sum of those
    // lengths, which no expected value states — the text's size bounds it
    const size_t bases_cap = (size_t)n, offs_n = (size_t)n_look + 1;
    uint8_t *bb = (uint8_t *)malloc(bases_cap + 2 * GUARD), *ob = (uint8_t *)malloc(offs_n * 8 + 2 * GUARD);
    memset(bb, 0xC3, bases_cap + 2 * GUARD);
    memset(ob, 0xC3, offs_n * 8 + 2 * GUARD);
    FqResultWords got;
    const bool fits = fq_parse_serial(text, n, p, line_end, n_nl, bb + GUARD, bases_cap, (uint64_t *)(ob + GUARD), offs_n, &got);
    bool ok = fits && guards_ok(bb, bases_cap) && guards_ok(ob, offs_n * 8);
    ok = ok && got.n_records == want.n_records && got.n_bases == want.n_bases && got.bytes_consumed == want.bytes_consumed &&
         got.anomaly_record == want.anomaly_record && got.anomaly_kind == want.anomaly_kind;
    ok = ok && !memcmp(ob + GUARD, want_offsets, (want.n_records + 1) * 8) && (want.n_bases == 0 || !memcmp(bb + GUARD, want_bases, want.n_bases));
    if (!ok) {
      fprintf(stderr, "%s: fits %d; records %llu (want %llu), bases %llu (%llu), consumed %llu (%llu), anomaly %llu kind %u (%llu kind %u), or guards / offsets / bases\n",
              name.c_str(), (int)fits, (unsigned long long)got.n_records, (unsigned long long)want.n_records, (unsigned long long)got.n_bases,
              (unsigned long long)want.n_bases, (unsigned long long)got.bytes_consumed, (unsigned long long)want.bytes_consumed,
              (unsigned long long)got.anomaly_record, got.anomaly_kind, (unsigned long long)want.anomaly_record, want.anomaly_kind);
      return 1;
    }
    // capacities one short: nothing beyond them is written, and the call says so
    if (n_look && n < 65536) {  // (the small texts: the large ones differ from each other by a padding only)
      memset(ob, 0xC3, offs_n * 8 + 2 * GUARD);
      if (fq_parse_serial(text, n, p, line_end, n_nl, bb + GUARD, bases_cap, (uint64_t *)(ob + GUARD + 8), offs_n - 1, &got) || got.n_records != n_look ||
          !guards_ok(ob, offs_n * 8)) {
        fprintf(stderr, "%s: offsets one short were not refused\n", name.c_str());
        return 1;
      }
    }
    if (want.n_bases && n < 65536) {
      uint8_t *sb = (uint8_t *)malloc((size_t)want.n_bases - 1 + 2 * GUARD);
      memset(sb, 0xC3, (size_t)want.n_bases - 1 + 2 * GUARD);
      if (fq_parse_serial(text, n, p, line_end, n_nl, sb + GUARD, want.n_bases - 1, (uint64_t *)(ob + GUARD), offs_n, &got) || got.n_bases != want.n_bases ||
          !guards_ok(sb, (size_t)want.n_bases - 1)) {
        fprintf(stderr, "%s: bases one short were not refused\n", name.c_str());
        return 1;
      }
      free(sb);
    }
    n_records += want.n_records;
    free(tb);
    free(line_end);
    free(bb);
    free(ob);
  }
  printf("parse ok: %u cases, %llu records\n", n_cases, (unsigned long long)n_records);
  return 0;
}

static uint64_t rng_state;
static uint64_t rng() {  // splitmix64
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
static int run_crc(uint64_t seed, size_t n_random) {
  rng_state = seed;
  uint32_t tab[256];
  for (uint32_t i = 0; i < 256; ++i) tab[i] = fq_crc_table_entry(i);
  std::vector<uint32_t> lens = {0, 1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 255, 256, 4095, 4096, 65279, 65280, 65535, 65536, 70000};
  for (size_t i = 0; i < n_random; ++i) lens.push_back((uint32_t)(rng() % 70001));
  for (uint32_t len : lens) {
    const uint32_t align = (uint32_t)(rng() & 7);
    uint8_t *block = (uint8_t *)malloc((size_t)align + len ? (size_t)align + len : 1);  // (the extent ends where the allocation ends)
    uint8_t *p = block + align;
    for (uint32_t i = 0; i < len; ++i) p[i] = (uint8_t)rng();
    uint32_t raw = 0;
    for (uint32_t share = 0; share < (uint32_t)FQ_CRC_SHARES; ++share) raw ^= fq_crc_share(tab, p, len, share);
    const uint32_t got = fq_crc_condition(raw, len), want = crc32_update(0, p, len);
    if (got != want) {
      fprintf(stderr, "crc of %u bytes at alignment %u: %08x, crc32_update says %08x\n", len, align, got, want);
      return 1;
    }
    free(block);
  }
  printf("crc ok: %zu extents\n", lens.size());
  return 0;
}

static int run_plan(const char *path, int n_budgets, char **budgets) {
  const std::vector<uint8_t> file = slurp(path);
  const uint8_t *const p0 = file.data(), *const pe = p0 + file.size();
  for (int k = 0; k < n_budgets; ++k) {
    const uint64_t budget = strtoull(budgets[k], nullptr, 10);
    printf("budget %llu\n", (unsigned long long)budget);
    BgzfBatch b;
    const uint8_t *p = p0;
    while (p < pe && bgzf_plan_batch(p, pe, budget, &b)) {
      if (b.begin != p || b.end <= p || b.jobs.size() != b.ms.size() || !bgzf_jobs_inside(b.jobs.data(), (uint32_t)b.jobs.size(), (size_t)(b.end - b.begin), b.out_bytes)) {
        fprintf(stderr, "a batch at %zu that is not one\n", (size_t)(p - p0));
        return 1;
      }
      const MemberJob &f = b.jobs.front(), &l = b.jobs.back();
      printf("batch %zu %llu %zu %zu %llu %llu %u %u %llu %llu %u %u\n", b.ms.size(), (unsigned long long)b.out_bytes, (size_t)(b.begin - p0), (size_t)(b.end - p0),
             (unsigned long long)f.in_offset, (unsigned long long)f.out_offset, f.in_len, f.out_len, (unsigned long long)l.in_offset,
             (unsigned long long)l.out_offset, l.in_len, l.out_len);
      p = b.end;
    }
    if (p < pe)
      printf("stop %zu\n", (size_t)(p - p0));
    else
      printf("end\n");
  }
  return 0;
}

static int run_inside() {
  const uint64_t M = ~0ull;
  struct {
    MemberJob j;
    size_t comp_len;
    uint64_t out_bytes;
    bool want;
  } cases[] = {
      {{0, 0, 0, 0}, 0, 0, true},
      {{10, 20, 90, 80}, 100, 100, true},
      {{10, 20, 91, 80}, 100, 100, false},
      {{10, 20, 90, 81}, 100, 100, false},
      {{101, 0, 0, 0}, 100, 100, false},
      {{0, 101, 0, 0}, 100, 100, false},
      {{0, 0, 65536, 65536}, 65536, 65536, true},
      {{0, 0, 65537, 1}, 1 << 20, 1 << 20, false},
      {{0, 0, 1, 65537}, 1 << 20, 1 << 20, false},
      {{M, 0, 1, 0}, 100, 100, false},       // (in_offset + in_len wraps to 0)
      {{M - 5, 0, 10, 0}, 100, 100, false},  // (… to 4)
      {{0, M, 0, 1}, 100, 100, false},
      {{0, M - 5, 0, 10}, 100, 100, false},
      {{M, M, 65536, 65536}, (size_t)M, M, false},
      {{M - 65536, M - 65536, 65536, 65536}, (size_t)M, M, true},
  };
  for (const auto &c : cases)
    if (bgzf_jobs_inside(&c.j, 1, c.comp_len, c.out_bytes) != c.want) {
      fprintf(stderr, "bgzf_jobs_inside({%llu, %llu, %u, %u}, %zu, %llu) is not %d\n", (unsigned long long)c.j.in_offset, (unsigned long long)c.j.out_offset, c.j.in_len,
              c.j.out_len, c.comp_len, (unsigned long long)c.out_bytes, (int)c.want);
      return 1;
    }
  // one job outside among good ones
  const MemberJob three[3] = {{0, 0, 10, 10}, {M - 1, 10, 10, 10}, {20, 20, 10, 10}};
  if (bgzf_jobs_inside(three, 3, 100, 100) || !bgzf_jobs_inside(three, 1, 100, 100) || !bgzf_jobs_inside(three, 0, 0, 0)) return 1;
  printf("inside ok: %zu jobs\n", sizeof cases / sizeof cases[0]);
  return 0;
}

int main(int argc, char **argv) {
  if (argc >= 4 && !strcmp(argv[1], "plan")) return run_plan(argv[2], argc - 3, argv + 3);
  if (argc == 2 && !strcmp(argv[1], "inside")) return run_inside();
  if (argc == 3 && !strcmp(argv[1], "budget")) return printf("%llu\n", (unsigned long long)bgzf_batch_budget(strtoull(argv[2], nullptr, 10))) < 0;
  if (argc == 3 && !strcmp(argv[1], "parse")) return run_parse(argv[2]);
  if (argc == 4 && !strcmp(argv[1], "crc")) return run_crc(strtoull(argv[2], nullptr, 10), strtoull(argv[3], nullptr, 10));
  fprintf(stderr, "usage: %s parse FILE | crc SEED N | plan FILE BUDGET... | inside | budget DEFAULT\n", argv[0]);
  return 2;
}
