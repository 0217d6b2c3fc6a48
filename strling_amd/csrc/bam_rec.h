// bam_rec.h -- the one statement of a BAM record's end on the reference that the device kernels share (evidence.hip step 2,
// bamindex.hip bai_read, bamindex_core.h bai_read_bounded, sweep_core.h sweep_keys_body).  Compiles for the host too (the host index
// builder; STRL_EMU: tests/emu/sweep_emu.cpp).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) && !defined(STRL_EMU)
#define STRL_REC_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define STRL_REC_FN inline
#endif

namespace strl {

STRL_REC_FN uint32_t rec_ld32(const uint8_t *p) { uint32_t v; __builtin_memcpy(&v, p, 4); return v; }
STRL_REC_FN uint32_t rec_ld16(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }

// bam_endpos of the record whose block_size word sits at R, with Rec::stop's rule: an unmapped record (flag 0x4) and one whose
// CIGAR consumes no reference base end one base behind pos.  The CIGAR lies inside the record (the record scan has checked it).
STRL_REC_FN int64_t bam_rec_end(const uint8_t *R) {
  const uint32_t l_name = R[12], n_cig = rec_ld16(R + 16), flag = rec_ld16(R + 18);
  int64_t rl = 0;
  if (!(flag & 4u)) {
    const uint8_t *cg = R + 36 + l_name;
    for (uint32_t j = 0; j < n_cig; ++j) {
      const uint32_t c = rec_ld32(cg + 4u * j), op = c & 15u;
      if (op == 0u || op == 2u || op == 3u || op == 7u || op == 8u) rl += c >> 4;
    }
  }
  return (int64_t)(int32_t)rec_ld32(R + 8) + (rl ? rl : 1);
}

}  // namespace strl
