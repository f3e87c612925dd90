// shk_primer.h — host side of sPCR's primer seed discovery (get_primer_kmers, src/pcr/primers.rs:234-480): the
// trim, the ambiguity-code check and the mismatch levels of one primer direction, as the per-position allow masks
// k_primer_scan matches against (plain C++: no HIP, no device).
#pragma once

#include <cstdint>
#include <string>

#include "../../include/shk.h"

constexpr uint32_t PRIMER_MAX_VARIANTS = 10000;  // MAX_RESOLVED_VARIANTS, primers.rs:275
constexpr uint32_t PRIMER_LEVELS = SHK_PRIMER_LEVELS;

struct PrimerPlan {
  std::string trimmed;            // P: the primer's last `trim` bases (primers.rs:244-271)
  uint32_t L = 0;                 // |P|
  uint32_t M = 0;                 // min(mismatches, L) (primers.rs:286-287)
  uint32_t min_count = 0, max_kmers = 0;
  uint64_t n_resolved = 0;        // ∏ |allowed(P[i])| = |resolve_primer(P)|
  uint64_t level_size[PRIMER_LEVELS] = {};  // |level m| = [x^m] ∏ (a_i + (4 − a_i) x), saturating
  // allow[b]: bit 2(k−1−i) set when base b (A C G T = 0 1 2 3) is in allowed(P[i]): the masks sit on the FIRST L
  // bases of a k-mer, where find_oligos_in_kmers puts the oligo (primers.rs:188-199)
  uint64_t allow[4] = {};
  int bad_pos = -1;               // first character of P outside ACGTRYWSKMBDHVN, or −1
  bool ambiguous = false;         // P holds an ambiguity code
  bool scanned() const { return L > 0 && max_kmers > 0; }
};

// Trim, resolve and level one primer direction for a table of k-mers of length k (1 ≤ k ≤ 31).  Fails (SHK_ERR_BAD_ARG,
// *err = the reference's text) when the resolved variants exceed PRIMER_MAX_VARIANTS (primers.rs:273-284).
int primer_plan(const shk_primer *p, uint32_t k, PrimerPlan *out, std::string *err);
// The conversion check of get_kmers_from_primers (string_to_oligo, primers.rs:33-55, 342-352): a scanned primer with a
// character outside the IUPAC codes fails (SHK_ERR_INVALID_CHAR) in its first non-empty round.
int primer_check_chars(const PrimerPlan &pl, std::string *err);
