// shk_primer.cpp — primer preprocessing of sPCR (src/pcr/primers.rs:60-99, 234-313) without listing a variant.
//
// preprocess_primer_by_mismatch builds level m as the strings whose Hamming distance to resolve_primer(P) is m.
// resolve_primer(P) is the product of the per-position sets allowed(P[i]), so that distance is the number of positions
// i where the base is not in allowed(P[i]): one bit mask per base and position describes every level at once
// (tests/test_primer_kmers_cpu.py pins this against literal enumeration).
#include "shk_primer.h"
#include "shk_mix.h"

#include <cstdio>
#include <cstring>

namespace {

// allowed(c) as a 4-bit set over A C G T (bit b = base b), resolve_primer's table (primers.rs:63-77); 0: not a code
uint32_t iupac_bits(char c) {
  switch (c) {
    case 'A': return 1;
    case 'C': return 2;
    case 'G': return 4;
    case 'T': return 8;
    case 'R': return 1 | 4;
    case 'Y': return 2 | 8;
    case 'S': return 4 | 2;
    case 'W': return 1 | 8;
    case 'K': return 4 | 8;
    case 'M': return 1 | 2;
    case 'B': return 2 | 4 | 8;
    case 'D': return 1 | 4 | 8;
    case 'H': return 1 | 2 | 8;
    case 'V': return 1 | 2 | 4;
    case 'N': return 15;
    default: return 0;
  }
}

}  // namespace

int primer_plan(const shk_primer *p, uint32_t k, PrimerPlan *out, std::string *err) {
  *out = PrimerPlan();
  if (!p || k < 1 || k > 31) {
    *err = "primer or k out of range (need 1 <= k <= 31)";
    return SHK_ERR_BAD_ARG;
  }
  const std::string seq = p->seq ? p->seq : "";
  size_t trim = p->trim;
  if (trim >= k) trim = k - 1;  // primers.rs:250-259
  out->trimmed = seq.size() > trim ? seq.substr(seq.size() - trim) : seq;  // primers.rs:262-271
  out->L = (uint32_t)out->trimmed.size();
  out->M = p->mismatches < out->L ? p->mismatches : out->L;  // primers.rs:286-287
  out->min_count = p->min_count;
  out->max_kmers = p->max_kmers;
  // ∏ (a_i + (4 − a_i) x): a character outside the codes stays as itself in resolve_primer (a_i = 1) and each of the
  // four bases permute_sequences writes over it is a new string (4 − a_i = 4 there, not 3)
  unsigned __int128 poly[PRIMER_LEVELS + 1] = {};
  poly[0] = 1;
  unsigned __int128 n = 1;
  for (uint32_t i = 0; i < out->L; ++i) {
    const char c = out->trimmed[i];
    const uint32_t bits = iupac_bits(c);
    const uint32_t a = bits ? (uint32_t)__builtin_popcount(bits) : 1u;
    const uint32_t miss = bits ? 4u - a : 4u;
    if (!bits && out->bad_pos < 0) out->bad_pos = (int)i;
    if (bits && a > 1) out->ambiguous = true;
    n *= a;
    for (int m = (int)PRIMER_LEVELS; m >= 0; --m) poly[m] = poly[m] * a + (m ? poly[m - 1] * miss : 0);
    for (uint32_t b = 0; b < 4; ++b)
      if (bits >> b & 1u) out->allow[b] |= 1ull << (2 * (k - 1 - i));
  }
  out->n_resolved = out->L ? (uint64_t)n : 0;  // resolve_primer("") is the empty set
  for (uint32_t m = 0; out->L && m <= out->M; ++m)
    out->level_size[m] = poly[m] > (unsigned __int128)UINT64_MAX ? UINT64_MAX : (uint64_t)poly[m];
  if (out->n_resolved > PRIMER_MAX_VARIANTS) {  // primers.rs:273-284
    char buf[256];
    snprintf(buf, sizeof buf, "%llu", (unsigned long long)out->n_resolved);
    *err = "Primer " + out->trimmed + " has too many ambiguous bases: " + buf +
           " resolved variants exceeds limit of 10000. Reduce ambiguity or use a more specific primer.";
    return SHK_ERR_BAD_ARG;
  }
  return SHK_OK;
}

int primer_check_chars(const PrimerPlan &pl, std::string *err) {
  if (!pl.scanned() || pl.bad_pos < 0) return SHK_OK;
  // string_to_oligo names the first character that is not A C G T, in the variant being converted.  Without an
  // ambiguity code that variant is P itself; with one it is whichever variant the reference's hash set yields first:
  // here every code resolved to its first base (only "Invalid nucleotide {c} in " is the reference's for sure).
  std::string variant = pl.trimmed;
  for (char &c : variant) {
    const uint32_t bits = iupac_bits(c);
    if (bits) c = "ACGT"[__builtin_ctz(bits)];
  }
  *err = std::string("Invalid nucleotide ") + pl.trimmed[pl.bad_pos] + " in " + variant;
  return SHK_ERR_INVALID_CHAR;
}

extern "C" int shk_primer_compile(const shk_primer *p, uint32_t k, uint32_t *trimmed_len, uint32_t *n_levels,
                                  uint64_t *n_variants, char *err, size_t err_len) {
  PrimerPlan pl;
  std::string msg;
  int rc = primer_plan(p, k, &pl, &msg);
  if (rc == SHK_OK) rc = primer_check_chars(pl, &msg);
  if (trimmed_len) *trimmed_len = pl.L;
  if (n_levels) *n_levels = pl.L ? pl.M + 1 : 0;
  if (n_variants) memcpy(n_variants, pl.level_size, sizeof pl.level_size);
  if (err && err_len) snprintf(err, err_len, "%s", rc == SHK_OK ? "" : msg.c_str());
  return rc;
}

// The owner share of a canonical k-mer: the top log2(n_owners) bits of its mixed key, which is what home_of reads off
// hash64 on the device (shk_device.hip.h).
extern "C" uint32_t shk_key_owner(uint32_t k, uint32_t n_owners, uint64_t canonical_kmer) {
  if (k == 0 || k >= 32 || n_owners == 0 || n_owners > 64 || (n_owners & (n_owners - 1))) return ~0u;
  uint32_t owner_bits = 0;
  while ((1u << owner_bits) < n_owners) ++owner_bits;
  if (!owner_bits) return 0;
  const uint32_t bits = 2 * k;
  const uint64_t kmer = canonical_kmer & (~0ull >> (64 - bits));
  if (owner_bits > bits) return ~0u;  // (k = 1, 2 with more owners than keys have bits: the engine makes no such context)
  return (uint32_t)(shk::mix_key(kmer, bits) >> (bits - owner_bits));
}
