// inflate_core_driver.cpp — the host shim (one lane) of shk_inflate_core.h over the members of BGZF files, under
// AddressSanitizer and UBSan (make -C sharkmer_amd/csrc inflate_core_driver; tests/test_inflate_core_cpu.py).
//
//   inflate_core_driver clean FILE...        every member of FILE decodes "ok" to the bytes of FILE.raw (what zlib gave)
//   inflate_core_driver damage SEED N FILE   every truncation length of the first, a middle and the last non-empty
//                                            member, then N single-bit flips and N random-byte overwrites of members
//                                            drawn with SEED: each must return a status
//   inflate_core_driver expect LIST          LIST: lines "path member_index status"; that member, at each of the four
//                                            alignments, must return exactly that status (all are printed)
// Every decode runs with the compressed bytes in an allocation that ends where the stated slack ends, the output slot
// between guard bytes, and a step count held against STEP_FACTOR · (in_len + out_len) + STEP_FLOOR.  Damage may decode
// "ok" to wrong bytes (a member's CRC-32 catches that, not the decoder): asserted are memory safety, termination, and
// that "ok" always comes with exactly ISIZE bytes.
#define SHK_INFC_COUNT_STEPS 1
#include "../../sharkmer_amd/csrc/shk_inflate_core.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace shk;

// A block costs at least 10 bits and at most ~3000 steps of table set-up (320 lengths read, counted and sorted, 1280
// table entries), a symbol at least one bit and at most 16 steps: 4096 steps per byte covers both with room.
static const uint64_t STEP_FACTOR = 4096, STEP_FLOOR = 8192;
static const size_t GUARD = 64;

struct Member {
  size_t body, body_len;  // the DEFLATE stream within the file
  uint32_t isize;
};
static std::vector<uint8_t> slurp(const std::string &path) {
  std::vector<uint8_t> v;
  FILE *f = fopen(path.c_str(), "rb");
  if (!f) {
    fprintf(stderr, "cannot open %s\n", path.c_str());
    exit(2);
  }
  uint8_t buf[65536];
  size_t n;
  while ((n = fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + n);
  fclose(f);
  return v;
}
static std::vector<Member> members_of(const std::vector<uint8_t> &f) {  // (the files are the test's own: well-formed BGZF)
  std::vector<Member> m;
  size_t p = 0;
  while (p + 18 <= f.size()) {
    const size_t xlen = f[p + 10] | f[p + 11] << 8, bsize = (size_t)(f[p + 16] | f[p + 17] << 8) + 1;
    if (xlen != 6 || p + bsize > f.size()) {
      fprintf(stderr, "not the test's BGZF framing at %zu\n", p);
      exit(2);
    }
    Member x;
    x.body = p + 18;
    x.body_len = bsize - 26;
    memcpy(&x.isize, &f[p + bsize - 4], 4);
    m.push_back(x);
    p += bsize;
  }
  return m;
}

struct Result {
  uint32_t status, opos;
  std::vector<uint8_t> out;
};
static uint64_t n_decodes = 0, max_steps_per_byte_x100 = 0;
static Result decode(const uint8_t *body, size_t in_len, uint32_t out_len, uint32_t align) {
  // the compressed bytes at offset 4 + align of an allocation that ends with the dword holding their last byte
  const size_t in_off = 4 + align, alloc = (in_off + in_len + 3) & ~(size_t)3;
  uint8_t *in = (uint8_t *)malloc(alloc ? alloc : 4);
  memset(in, 0xA5, alloc);
  memcpy(in + in_off, body, in_len);
  uint8_t *ob = (uint8_t *)malloc(out_len + 2 * GUARD);
  memset(ob, 0xC3, out_len + 2 * GUARD);
  InfCoreScratch S;
  memset((void *)&S, 0x5A, sizeof S);
  S.steps = 0;
  // (lane 0 of 1; `in + 4` is 4-byte aligned: malloc's alignment)
  InfCore<1> c(S, 0, in + 4, align, (uint32_t)in_len, ob + GUARD, out_len);
  Result r;
  r.status = c.run();
  r.opos = c.opos;
  for (size_t i = 0; i < GUARD; ++i)
    if (ob[i] != 0xC3 || ob[GUARD + out_len + i] != 0xC3) {
      fprintf(stderr, "guard byte overwritten (in_len %zu, out_len %u)\n", in_len, out_len);
      exit(1);
    }
  if (r.status == INFC_OK && r.opos != out_len) {
    fprintf(stderr, "ok with %u of %u bytes\n", r.opos, out_len);
    exit(1);
  }
  if (r.status > INFC_INPUT_LEFT || r.opos > out_len) {
    fprintf(stderr, "status %u, %u bytes of %u\n", r.status, r.opos, out_len);
    exit(1);
  }
  const uint64_t bound = STEP_FACTOR * (in_len + out_len) + STEP_FLOOR;
  if (S.steps > bound) {
    fprintf(stderr, "%llu steps for %zu bytes in, %u out (bound %llu)\n", (unsigned long long)S.steps, in_len, out_len, (unsigned long long)bound);
    exit(1);
  }
  if (in_len + out_len) max_steps_per_byte_x100 = std::max<uint64_t>(max_steps_per_byte_x100, S.steps * 100 / (in_len + out_len));
  ++n_decodes;
  r.out.assign(ob + GUARD, ob + GUARD + out_len);
  free(in);
  free(ob);
  return r;
}

static uint64_t rng_state;
static uint64_t rng() {  // splitmix64
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

int main(int argc, char **argv) {
  if (argc >= 3 && !strcmp(argv[1], "clean")) {
    size_t n_members = 0;
    for (int a = 2; a < argc; ++a) {
      const std::vector<uint8_t> f = slurp(argv[a]), raw = slurp(std::string(argv[a]) + ".raw");
      size_t at = 0;
      uint32_t k = 0;
      for (const Member &m : members_of(f)) {
        const Result r = decode(f.data() + m.body, m.body_len, m.isize, k++ & 3);
        if (r.status != INFC_OK || at + m.isize > raw.size() || (m.isize && memcmp(r.out.data(), raw.data() + at, m.isize))) {
          fprintf(stderr, "%s: member %u: status %u, or not zlib's bytes\n", argv[a], k - 1, r.status);
          return 1;
        }
        at += m.isize;
        ++n_members;
      }
      if (at != raw.size()) {
        fprintf(stderr, "%s: %zu bytes decoded, %zu expected\n", argv[a], at, raw.size());
        return 1;
      }
    }
    printf("clean ok: %zu members, at most %.2f steps per byte\n", n_members, max_steps_per_byte_x100 / 100.0);
    return 0;
  }
  if (argc == 5 && !strcmp(argv[1], "damage")) {
    rng_state = strtoull(argv[2], nullptr, 10);
    const size_t n = strtoull(argv[3], nullptr, 10);
    const std::vector<uint8_t> f = slurp(argv[4]);
    std::vector<Member> ms;
    for (const Member &m : members_of(f))
      if (m.isize) ms.push_back(m);
    if (ms.empty()) return 2;
    size_t n_ok = 0;
    const size_t pick[3] = {0, ms.size() / 2, ms.size() - 1};
    for (size_t p = 0; p < 3; ++p) {
      const Member &m = ms[pick[p]];
      for (size_t len = 0; len < m.body_len; ++len) {
        const Result r = decode(f.data() + m.body, len, m.isize, (uint32_t)(len & 3));
        if (r.status == INFC_OK) {  // (cannot be: the final block's end is the stream's last bits)
          fprintf(stderr, "a truncated member decoded ok (%zu of %zu bytes)\n", len, m.body_len);
          return 1;
        }
      }
    }
    std::vector<uint8_t> body;
    for (size_t i = 0; i < 2 * n; ++i) {
      const Member &m = ms[rng() % ms.size()];
      body.assign(f.begin() + (long)m.body, f.begin() + (long)(m.body + m.body_len));
      if (i < n) {
        const uint64_t bit = rng() % (body.size() * 8);
        body[bit >> 3] ^= (uint8_t)(1u << (bit & 7));
      } else {
        const size_t at = rng() % body.size(), cnt = 1 + rng() % 8;
        for (size_t j = at; j < body.size() && j < at + cnt; ++j) body[j] = (uint8_t)rng();
      }
      // ISIZE as the trailer has it, and now and then off by one (what a damaged trailer claims)
      uint32_t isize = m.isize;
      if ((rng() & 7) == 0) isize += (rng() & 1) ? 1 : (uint32_t)-1;
      n_ok += decode(body.data(), body.size(), isize, (uint32_t)(rng() & 3)).status == INFC_OK;
    }
    printf("damage ok: %llu decodes (%zu of the damaged ones decoded \"ok\"), at most %.2f steps per byte\n", (unsigned long long)n_decodes, n_ok,
           max_steps_per_byte_x100 / 100.0);
    return 0;
  }
  if (argc == 3 && !strcmp(argv[1], "expect")) {
    FILE *lf = fopen(argv[2], "r");
    if (!lf) return 2;
    char path[4096];
    unsigned index, want;
    size_t n_lines = 0, n_bad = 0;
    while (fscanf(lf, "%4095s %u %u", path, &index, &want) == 3) {
      const std::vector<uint8_t> f = slurp(path);
      const std::vector<Member> ms = members_of(f);
      if (index >= ms.size()) {
        fprintf(stderr, "%s has no member %u\n", path, index);
        return 2;
      }
      const Member &m = ms[index];
      printf("%s %u want %u got", path, index, want);
      for (uint32_t align = 0; align < 4; ++align) {
        const Result r = decode(f.data() + m.body, m.body_len, m.isize, align);
        printf(" %u", r.status);
        n_bad += r.status != want;
      }
      printf("\n");
      ++n_lines;
    }
    fclose(lf);
    if (n_bad) {
      fprintf(stderr, "%zu statuses are not the expected ones\n", n_bad);
      return 1;
    }
    printf("expect ok: %zu members at 4 alignments, at most %.2f steps per byte\n", n_lines, max_steps_per_byte_x100 / 100.0);
    return 0;
  }
  fprintf(stderr, "usage: %s clean FILE... | damage SEED N FILE | expect LIST\n", argv[0]);
  return 2;
}
