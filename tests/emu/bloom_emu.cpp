// bloom_emu.cpp -- TEST-ONLY host build of the Bloom bitmap's index arithmetic (strling_amd/csrc/bloom_layout.h under STRL_EMU):
// the very functions bloom_set and pair_probe_kernel compile, over arrays of mixed hashes, for tests/test_bloom_layout.py.
// The product never links this file.
#define STRL_EMU 1
#include "../../strling_amd/csrc/bloom_layout.h"
#include <stddef.h>

extern "C" {
int bloom_emu_k() { return strl::BLOOM_K; }
int bloom_emu_word_bits() { return 1 << strl::BLOOM_WORD_SHIFT; }
void bloom_emu_words(const uint64_t *m, size_t n, uint32_t mask, uint32_t *out) {
  for (size_t i = 0; i < n; ++i) out[i] = strl::bloom_word(m[i], mask);
}
void bloom_emu_patterns(const uint64_t *m, size_t n, uint64_t *out) {
  for (size_t i = 0; i < n; ++i) out[i] = strl::bloom_pattern(m[i]);
}
}
