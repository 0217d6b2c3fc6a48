// classify_turn.h -- the index arithmetic of classify_kernel's turns (score.hip), for the kernel and for a CPU emulation of it
// (tests/emu/classify_emu.cpp, plain g++): both compile these very functions.
//
// A wave owns one contiguous range [r0, r1) of reads and walks it in turns of CT_TURN reads.  A turn is FULL when it and the
// turn behind it lie wholly inside the range: then every lane has eight reads, the next turn's vectors exist, and the kernel
// loads, tests and stores without a bounds test or an exec mask.  Every other turn (the last two of a range, a ragged end) is
// GENERAL and keeps its tests.  Inside a range everything is a 32-bit offset from r0: queue ids are 32 bits already.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define STRL_CT_FN __host__ __device__ __forceinline__
#else
#define STRL_CT_FN inline
#endif

namespace strl {

constexpr uint32_t CT_LANES = 64;
constexpr uint32_t CT_ILP = 8;                        // reads per lane and turn (score.hip asserts CL_ILP against it)
constexpr uint32_t CT_TURN = CT_LANES * CT_ILP;       // reads per wave and turn
constexpr uint32_t CT_GROUPS = CT_ILP / 4;            // 16-byte groups of four consecutive reads per lane and turn

struct ClassifyRange { uint64_t r0, r1; };

// the reads of wave `gw` when every wave's share is `per` reads (the kernel's own line computes `per`)
STRL_CT_FN ClassifyRange classify_range(uint64_t n, uint64_t per, uint64_t gw) {
  ClassifyRange R;
  R.r0 = gw * per;
  R.r1 = R.r0 + per < n ? R.r0 + per : n;
  return R;
}
// a wave that owns no read has r0 >= r1 (r0 may lie beyond n): it must not load anything
STRL_CT_FN bool classify_owns(const ClassifyRange &R) { return R.r0 < R.r1; }
STRL_CT_FN uint32_t classify_len(const ClassifyRange &R) { return (uint32_t)(R.r1 - R.r0); }

// the turn at offset `off` of a range of `len` reads is full: it and the next turn are whole (wave-uniform)
STRL_CT_FN bool classify_full(uint32_t off, uint32_t len) { return off + 2u * CT_TURN <= len; }

// vector variant: offset (from r0) of the first read of the lane's group gq in the turn at `off`; the group is reads +0 .. +3,
// its 16-byte vector is element (offset >> 2) of a column that starts at r0
STRL_CT_FN uint32_t classify_group_off(uint32_t off, uint32_t lane, uint32_t gq) { return off + 4u * CT_LANES * gq + 4u * lane; }
// vector variant: offset of the read the lane handles as sub-item j
STRL_CT_FN uint32_t classify_read_off(uint32_t off, uint32_t lane, uint32_t j) { return classify_group_off(off, lane, j >> 2) + (j & 3u); }

}  // namespace strl
