// The compressor's core (strling_amd/csrc/deflate_core.h) compiled for the host with g++, for tests/test_deflate_cases.py:
// the code-length routine on its own, and the whole rule as a team of one.
#define STRL_EMU 1
#include "../../strling_amd/csrc/deflate_core.h"

using namespace strl;

// len[0, nsym) from freq[0, nsym) with no code longer than `limit`
extern "C" int emu_code_lengths(const uint32_t *freq, uint32_t nsym, uint32_t limit, uint8_t *len) {
  if (nsym > 288u || limit < 1u || limit > 15u) return -1;
  std::unique_ptr<DflWork> W(new DflWork);
  memset(W.get(), 0, sizeof(DflWork));
  uint32_t hist[288] = {0};
  uint8_t out[288] = {0};
  for (uint32_t s = 0; s < nsym; ++s) hist[s] = freq[s];
  dfl_code_lengths(DflSerial(), *W, hist, nsym, limit, out);
  for (uint32_t s = 0; s < nsym; ++s) len[s] = out[s];
  return 0;
}

extern "C" int emu_deflate_host(const uint8_t *in, uint64_t in_bytes, uint32_t block_bytes, uint8_t *out, uint64_t out_cap, uint64_t *out_bytes, uint32_t *csize,
                                uint32_t *n_stored) {
  return dfl_deflate_host(in, in_bytes, block_bytes, out, out_cap, out_bytes, csize, n_stored);
}
