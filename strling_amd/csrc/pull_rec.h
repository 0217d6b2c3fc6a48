// pull_rec.h -- the one reading of a BAM record `strling pull` has, for the device (pull.hip) and the host (pull_logic.cpp):
// the core fields, the plausibility check of bam_reader.cpp's append_record, bam_endpos with EvRec::stop's rule, the row.
#pragma once
#include <stdint.h>
#include "../../include/strling_amd.h"
#include "nim_tables.h"

namespace strl {

NIM_HD uint32_t pl_ld32(const uint8_t *p) { uint32_t v; __builtin_memcpy(&v, p, 4); return v; }
NIM_HD uint32_t pl_ld16(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }

// Do the 36 bytes at h start a record that lies inside `left` bytes?  (block_size in range, the fixed part, the name, the CIGAR
// and the 4-bit SEQ inside block_size: append_record's check)
NIM_HD bool pl_plausible(const uint8_t *h, uint64_t left) {
  if (left < 36) return false;
  const uint32_t bs = pl_ld32(h);
  if (bs < 32u || bs > (1u << 28) || 4ull + bs > left) return false;
  const uint64_t l_name = h[12], n_cig = pl_ld16(h + 16);
  const int32_t l_seq = (int32_t)pl_ld32(h + 20);
  return l_seq >= 0 && 32ull + l_name + 4ull * n_cig + (uint64_t)(((int64_t)l_seq + 1) / 2) <= bs;
}

struct PlRec {            // the core fields of the record whose block_size word sits at p (pl_plausible has held for it)
  const uint8_t *p;
  int32_t tid, pos, mtid, mpos;
  uint32_t bs, l_name, n_cig, flag;
  NIM_HD void load(const uint8_t *at) {
    p = at;
    bs = pl_ld32(p);
    tid = (int32_t)pl_ld32(p + 4); pos = (int32_t)pl_ld32(p + 8);
    l_name = p[12];
    n_cig = pl_ld16(p + 16); flag = pl_ld16(p + 18);
    mtid = (int32_t)pl_ld32(p + 24); mpos = (int32_t)pl_ld32(p + 28);
  }
  NIM_HD uint32_t name_len() const { return l_name ? l_name - 1u : 0u; }
  NIM_HD const uint8_t *name() const { return p + 36; }
  NIM_HD uint32_t hash() const { return (uint32_t)nim::hash_bytes(p + 36, (int)name_len()); }   // Nim's murmur of the qname
  NIM_HD int64_t stop() const {   // bam_endpos: pos + 1 for an unmapped record or a CIGAR of reference length 0 (EvRec::stop)
    int64_t rl = 0;
    if (!(flag & 0x4u))
      for (uint32_t j = 0; j < n_cig; ++j) {
        const uint32_t c = pl_ld32(p + 36 + l_name + 4u * j), op = c & 0xfu;
        if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) rl += c >> 4;
      }
    return (int64_t)pos + (rl ? rl : 1);
  }
  // extract_region.nim:46-47 behind htslib's iterator filter, and the tile's ownership rule
  NIM_HD bool kept_by(const strl_pull_tile &T) const {
    return tid == T.tid && pos < T.end && !(flag & 0x900u) && pos >= T.own_beg && pos < T.own_end && stop() > (int64_t)T.beg;
  }
  NIM_HD strl_pull_row row(uint64_t off, uint32_t h) const {
    strl_pull_row r;
    r.off = off; r.tid = tid; r.pos = pos; r.mtid = mtid; r.mpos = mpos; r.size = 4u + bs; r.hash = h;
    r.flag = (uint16_t)flag; r.l_name = (uint8_t)l_name; r.found = 1; r.count = 0;
    return r;
  }
};

}  // namespace strl
