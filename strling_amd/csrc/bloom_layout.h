// bloom_layout.h -- where the bits of a key lie in the Bloom bitmap of the hot qname groups (pair.hip).  The one definition:
// the marks (bloom_set, device_util.h), the probe (pair_probe_kernel) and the CPU test (tests/emu/bloom_emu.cpp, plain g++
// under STRL_EMU) all compile these functions.
//
// A key is the mixed 64-bit qname hash m = fmix64(hash).  All BLOOM_K bits of a key lie in ONE aligned 64-bit word of the
// bitmap: the word's index comes from the low bits of m, the bit positions from BLOOM_K disjoint 6-bit fields of m's high
// half (bits 32..55).  A mark is one 64-bit atomic OR, a test is one 8-byte load and (w & pattern) == pattern in registers.
// Fields may coincide: a pattern has between 1 and BLOOM_K bits set.
// Against two bits anywhere in the bitmap (the layout before) the blocked form loses some of a Bloom filter's spread and
// wins it back with k = 4: at 1.2e6 keys in 2^24 bits 0.77 % of unmarked keys pass instead of 1.77 % (tests/test_bloom_layout.py
// measures both on the CPU).
#pragma once
#include <stdint.h>

#if defined(STRL_EMU) || !defined(__HIPCC__)
#define STRL_BLOOM_HD inline
#else
#define STRL_BLOOM_HD __host__ __device__ __forceinline__
#endif

namespace strl {

constexpr int BLOOM_K = 4;            // bits per key
constexpr int BLOOM_WORD_SHIFT = 6;   // log2 of the word's width in bits

// index of the key's 64-bit word; mask = bits of the bitmap - 1 (a power of two, at least 2^16 bits)
STRL_BLOOM_HD uint32_t bloom_word(uint64_t m, uint32_t mask) { return (uint32_t)m & (mask >> BLOOM_WORD_SHIFT); }
// the key's bits inside its word
STRL_BLOOM_HD uint64_t bloom_pattern(uint64_t m) {
  const uint32_t h = (uint32_t)(m >> 32);
  uint64_t pat = 0;
  for (int f = 0; f < BLOOM_K; ++f) pat |= 1ull << ((h >> (6 * f)) & 63u);
  return pat;
}

}  // namespace strl
