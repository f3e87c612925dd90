// shk_mix.h — the engine's key mix, for the device code (shk_device.hip.h) and the plain C++ host side (shk_key_owner in
// shk_primer.cpp) alike: the two multipliers, their inverses and mix_key / unmix_key in one place.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define SHK_MIX_FN __host__ __device__ __forceinline__
#else
#define SHK_MIX_FN inline
#endif

namespace shk {

// mix_key: a BIJECTION of the 2k-bit key space — ONE multiplication by an odd constant mod 2^2k — so the
// position of a key in the table (page = top log_pages bits of the product, home bucket = the next 11
// bits) together with the remaining low bits identifies the key.  The 4-byte-record path of the paged
// counter ships only those low bits and rebuilds a key with unmix_key (the inverse multiplication) when
// it has to.  Everything the engine reads off the mixed key it reads off its TOP bits (owner, partition,
// page, bucket), and the top bits of a product depend on every bit of the key; the low bits, which depend
// on the key's low bits only, are just carried along as the fingerprint.  Up to 42 key bits (k ≤ 21: the
// 4-byte-record path, k_scatter32, which is bound by VALU issue) the multiplier is a 32-bit constant — a
// 64-bit product by it is one v_mad_u64_u32 + one v_mul_lo_u32 — beyond that a 64-bit one (longer keys need
// the wider constant for keys that differ in their low bits only to reach the top).  tools/hash_eval.py:
// page occupancy and bucket overflow match a Poisson process on random, AT-rich, tandem-repeat and
// sequential keys for k = 9…31 (round 1 used multiply–fold–multiply; one multiply measures the same
// spread and takes five instructions fewer per k-mer in the scatter's walk).
#ifndef SHK_MIX_M32
#define SHK_MIX_M32 0xC2B2AE35ull
#define SHK_MIX_M32_INV 0xD16E308E7ED1B41Dull
#endif
constexpr uint64_t MIX_M32 = SHK_MIX_M32, MIX_M64 = 0x9E3779B97F4A7C15ull;
constexpr uint64_t MIX_M32_INV = SHK_MIX_M32_INV, MIX_M64_INV = 0xF1DE83E19937733Dull;  // mod 2^64
static_assert((MIX_M32 * MIX_M32_INV) == 1ull && (MIX_M64 * MIX_M64_INV) == 1ull, "inverses mod 2^64");
#ifndef SHK_MIX_NARROW_BITS
#define SHK_MIX_NARROW_BITS 42
#endif
constexpr uint32_t MIX_NARROW_BITS = SHK_MIX_NARROW_BITS;
SHK_MIX_FN uint64_t mix_key(uint64_t x, uint32_t bits) {
  const uint64_t mask = ~0ull >> (64 - bits);
  return (x * (bits <= MIX_NARROW_BITS ? MIX_M32 : MIX_M64)) & mask;
}
SHK_MIX_FN uint64_t unmix_key(uint64_t y, uint32_t bits) {
  const uint64_t mask = ~0ull >> (64 - bits);
  return (y * (bits <= MIX_NARROW_BITS ? MIX_M32_INV : MIX_M64_INV)) & mask;
}

}  // namespace shk
