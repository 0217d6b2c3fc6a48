// classify_emu.cpp -- TEST-ONLY host build of the turn arithmetic of classify_kernel (strling_amd/csrc/classify_turn.h): the very
// functions the kernel compiles, and a walk over every wave's loop that takes the kernel's decisions in the kernel's order (range,
// early return, first load, full or general turn, prefetch, the two register sets that swap roles), for tests/test_classify_cases.py.
// Nothing of the predicate is here.  The product never links this file.
#include "../../strling_amd/csrc/classify_turn.h"
#include <stddef.h>

using namespace strl;

extern "C" {
uint32_t classify_emu_turn() { return CT_TURN; }
uint32_t classify_emu_ilp() { return CT_ILP; }
void classify_emu_range(uint64_t n, uint64_t per, uint64_t gw, uint64_t *out) {
  const ClassifyRange R = classify_range(n, per, gw);
  out[0] = R.r0; out[1] = R.r1; out[2] = classify_owns(R) ? 1 : 0; out[3] = classify_owns(R) ? classify_len(R) : 0;
}
int classify_emu_full(uint32_t off, uint32_t len) { return classify_full(off, len) ? 1 : 0; }
// the reads of one vector-variant turn in the order (j, lane): offsets from r0
void classify_emu_read_offs(uint32_t off, uint32_t *out) {
  for (uint32_t j = 0; j < CT_ILP; ++j)
    for (uint32_t lane = 0; lane < CT_LANES; ++lane) out[j * CT_LANES + lane] = classify_read_off(off, lane, j);
}

// Every wave's loop.  turns: rows {wave, base, end, full} (at most cap rows are written; the count is returned).
// handled[r] += 1 for every read a turn handles.  acc: {exclusive upper bound of the reads a full turn (or an unmasked first load)
// LOADS, its prefetch included; the same for its STORES; number of full turns; unmasked accesses outside the wave's own range;
// turns that found another turn's vectors in the register set they consume; waves that returned before their first load}.
long classify_emu_walk(uint64_t n, uint64_t per, uint64_t n_waves, int vec, uint64_t *turns, long cap, uint32_t *handled, uint64_t *acc) {
  long nt = 0;
  for (int k = 0; k < 6; ++k) acc[k] = 0;
  for (uint64_t gw = 0; gw < n_waves; ++gw) {
    const ClassifyRange R = classify_range(n, per, gw);
    if (!classify_owns(R)) { ++acc[5]; continue; }
    const uint64_t r0 = R.r0, r1 = R.r1;
    const uint32_t len = classify_len(R);
    auto touch = [&](uint32_t off, bool store) {           // the 16-byte groups of a whole turn, unmasked
      for (uint32_t gq = 0; gq < CT_GROUPS; ++gq)
        for (uint32_t lane = 0; lane < CT_LANES; ++lane) {
          const uint64_t last = (r0 + off) + classify_group_off(0u, lane, gq) + 3;      // the kernel's split: scalar base + lane's part
          if (last >= r1) ++acc[3];
          if (last + 1 > acc[store ? 1 : 0]) acc[store ? 1 : 0] = last + 1;
        }
    };
    uint64_t held[2] = {~0ull, ~0ull};                     // the turn (its base) whose vectors a register set holds
    if (vec && classify_full(0u, len)) touch(0u, false);
    held[0] = r0;
    int cur = 0;
    for (uint64_t base = r0; base < r1; base += CT_TURN, cur ^= 1) {
      const uint32_t off = (uint32_t)(base - r0);
      const bool full = vec && classify_full(off, len);
      if (held[cur] != base) ++acc[4];
      held[cur ^ 1] = base + CT_TURN;
      uint64_t end = base;
      if (full) {
        ++acc[2];
        touch(off + CT_TURN, false);
        touch(off, true);
        for (uint32_t j = 0; j < CT_ILP; ++j)
          for (uint32_t lane = 0; lane < CT_LANES; ++lane) {
            const uint64_t r = r0 + classify_read_off(off, lane, j);
            if (r < n) ++handled[r]; else ++acc[3];
          }
        end = base + CT_TURN;
      } else {
        for (uint32_t j = 0; j < CT_ILP; ++j)
          for (uint32_t lane = 0; lane < CT_LANES; ++lane) {
            const uint64_t r = vec ? r0 + classify_read_off(off, lane, j) : base + (uint64_t)CT_LANES * j + lane;
            if (r < r1) { ++handled[r]; if (r + 1 > end) end = r + 1; }
          }
      }
      if (nt < cap) { turns[4 * nt] = gw; turns[4 * nt + 1] = base; turns[4 * nt + 2] = end; turns[4 * nt + 3] = full ? 1 : 0; }
      ++nt;
    }
  }
  return nt;
}
}
