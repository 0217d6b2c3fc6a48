// evidence_core.h -- the per-record rule of evidence_kernel (evidence.hip): what spanners() (collect.nim:130-182, with
// spanning.nim:22-49) decides about ONE record against ONE bound, free of anything that belongs to a workgroup.
//   ev_header_ok                       step 1: does the record at this place of the region's bytes parse
//   ev_keep                            step 2: htslib's iterator filter, the flag / mapq filter, the two depth slots
//   ev_row                             step 3: the row of a kept record -- expected_spanning_probability, overlapping_read with
//                                      find_read_position and the greedy unit count, the wrapping cigar_ins / cigar_del sums,
//                                      pair eligibility, Nim's murmur hash of the qname
//   ev_bound_make                      (host) a strl_bounds and the window as the kernel needs them, with the capacity rule
// The window walk, the ballots and ranks, the row reservation, the depth scan with its histogram and the LDS hash table stay in
// evidence.hip.  The same source compiles for the host (STRL_EMU: tests/emu/evidence_emu.cpp, a stand-alone program under
// AddressSanitizer and UBSan) so that the CPU suite runs the rule itself.  No wave intrinsics for that reason.
#pragma once
#include <stdint.h>
#include <string.h>
#include "../../include/strling_amd.h"
#include "bam_rec.h"
#include "nim_tables.h"

#if defined(__HIPCC__) && !defined(STRL_EMU)
#define EV_FN __device__ __forceinline__
#else
#define EV_FN inline
#endif

namespace strl {

constexpr uint32_t EV_MAX_RECORDS = 4096;   // records in a region's byte range the device path takes
constexpr int64_t EV_MAX_SPAN = 9190;       // right - left + 2 * window it takes: 1000 (callclusters.nim:52-66) + 2 * 4095 (the fragment histogram's bins)
constexpr uint8_t EV_OVERLAP = 1, EV_PAIR = 2;
constexpr uint16_t EVF_REVERSE = 0x10, EVF_SECONDARY = 0x100, EVF_DUP = 0x400, EVF_SUPPL = 0x800;
// What the device returns of a record that passes spanners()' filters (collect.nim:138-141), in record order.
struct EvRow {
  uint32_t ord;        // ordinal of the record in the region's bytes
  uint32_t name_id;    // row (of this region) of the first kept record with the same qname bytes
  uint32_t hash;       // Nim's murmur hash of the qname
  float prob;          // expected_spanning_probability (spanning.nim:22-49): 1.0f - cd[dist], or 0
  int32_t start, isize;
  int64_t stop;        // bam_endpos
  uint8_t flags;       // EV_OVERLAP: overlapping_read() holds, the four fields below are its Support; EV_PAIR: tid == mtid and |isize| <= 5000
  uint8_t type, repeat_count, cigar_ins, cigar_del;
  uint8_t pad[2];
};
static_assert(sizeof(EvRow) == 40, "EvRow layout");

struct EvBound {          // a bound as the kernel needs it, made on the host
  int64_t left, right, wl;   // wl = left - window
  int32_t tid, beg, end;     // the query: [max(0, left - window), right + window)
  int32_t depth_n;           // right - left + 2 * window
  int32_t k, slop;           // unit length, bound_slop (collect.nim:97-104)
  uint32_t status;           // != 0: not for the device (1: the walk's verdict; 2: beyond the capacity rule)
  uint64_t unit;             // its bytes, the first in the low byte (a register: a char array indexed by a loop counter would be spilled to LDS)
};

EV_FN bool ev_cons_query(int op) { return op == 0 || op == 1 || op == 4 || op == 7 || op == 8; }
EV_FN bool ev_cons_ref(int op) { return op == 0 || op == 2 || op == 3 || op == 7 || op == 8; }

// step 1's test of the record whose 36 header bytes sit at h, `left` bytes in front of the range's end (left >= 36): the
// block_size word, and append_record's check that name, CIGAR and SEQ lie inside the block
EV_FN bool ev_header_ok(const uint8_t *h, uint64_t left, uint32_t *block_size) {
  const uint32_t bs = rec_ld32(h);
  if (bs < 32u || bs > (1u << 28) || 4ull + bs > left) return false;
  const uint64_t l_name = h[12], n_cig = rec_ld16(h + 16);
  const int32_t l_seq = (int32_t)rec_ld32(h + 20);
  if (l_seq < 0 || 32ull + l_name + 4ull * n_cig + (uint64_t)(((int64_t)l_seq + 1) / 2) > bs) return false;
  *block_size = bs;
  return true;
}

struct EvRec {            // the core fields of the record whose block_size word sits at p (the walk has checked that it parses)
  const uint8_t *p;
  int32_t tid, pos, l_seq, mtid, isize;
  uint32_t l_name, n_cig, flag, mapq;
  EV_FN void load(const uint8_t *at) {
    p = at;
    tid = (int32_t)rec_ld32(p + 4); pos = (int32_t)rec_ld32(p + 8);
    l_name = p[12]; mapq = p[13];
    n_cig = rec_ld16(p + 16); flag = rec_ld16(p + 18);
    l_seq = (int32_t)rec_ld32(p + 20); mtid = (int32_t)rec_ld32(p + 24); isize = (int32_t)rec_ld32(p + 32);
  }
  EV_FN uint32_t cig(uint32_t j) const { return rec_ld32(p + 36 + l_name + 4u * j); }
  EV_FN const uint8_t *qname() const { return p + 36; }
  EV_FN uint32_t qname_len() const { return l_name ? l_name - 1u : 0u; }
  EV_FN int base(int64_t j) const { return (p[36 + l_name + 4u * n_cig + (uint32_t)(j >> 1)] >> ((~j & 1) << 2)) & 0xf; }
  EV_FN int64_t stop() const { return bam_rec_end(p); }   // bam_endpos, with Rec::stop's rule for unmapped / zero-length
};

// spanning.nim:22-49
EV_FN float ev_expected_spanning_probability(const float *cd, int64_t start, int64_t stop, bool reverse, int64_t ev_start, int64_t ev_stop) {
  const int64_t msb = 20;
  int64_t dist;
  if (start < ev_stop - msb) {
    if (reverse) return 0.f;
    dist = ev_start - start;
  } else {
    if (!reverse) return 0.f;
    dist = stop - ev_stop;
  }
  if (dist < 0) return 0.f;
  if (dist + (ev_stop - ev_start) < msb) return 0.f;
  dist += msb + (ev_stop - ev_start);
  if (dist < 0 || dist > 4095) return 0.f;
  return 1.0f - cd[dist];
}
// collect.nim:50-72
EV_FN int64_t ev_find_read_position(const EvRec &R, int64_t position) {
  int64_t r_off = R.pos, q_off = 0;
  for (uint32_t j = 0; j < R.n_cig; ++j) {
    if (r_off > position) return -1;
    const uint32_t c = R.cig(j);
    const int op = (int)(c & 0xf);
    const int64_t len = c >> 4;
    if (ev_cons_query(op)) q_off += len;
    if (ev_cons_ref(op)) r_off += len;
    if (r_off < position) continue;
    const int64_t over = r_off - position;
    if (over > q_off) return -1;
    if (!ev_cons_query(op)) return -1;
    return q_off - over;
  }
  return -1;
}
// collect.nim:75-93; *bad: the CIGAR names bases the record's SEQ does not hold (the host's reader has the word on that one)
EV_FN int ev_count_in_bounds(const EvRec &R, const EvBound &B, bool *bad) {
  const int64_t dlen = R.l_seq;
  int64_t rl = ev_find_read_position(R, B.left), rr = ev_find_read_position(R, B.right);
  if (rl >= 0 && rr < 0) rr = dlen;
  if (rl < 0 && rr < 0) return 0;
  if (rl < 0) rl = 0;
  const int64_t slen = rr - rl > 0 ? rr - rl : 0;
  if (slen > 0 && rl + slen > dlen) { *bad = true; return 0; }
  const int k = B.k;
  const char *nt = "=ACMGRSVTWYHKDBN";
  int result = 0;
  for (int64_t p = rl; p + k <= rl + slen;) {
    bool eq = true;
    for (int j = 0; j < k && eq; ++j) eq = nt[R.base(p + j)] == (char)(B.unit >> (8 * j));
    if (eq) { ++result; p += k; } else ++p;
  }
  if (result < (int)((double)slen * 0.7 / (double)k)) result = 0;
  return result;
}

// step 2 (collect.nim:138-141,154-155): is the record one of those spanners() works on, and if so, the slots of the depth
// difference array that take its +1 (*a) and its -1 (*b), both inside [0, depth_n)
EV_FN bool ev_keep(const EvRec &R, int64_t stop, const EvBound &B, uint32_t min_mapq, int32_t *slot_a, int32_t *slot_b) {
  const int64_t start = R.pos;
  if (!(R.tid == B.tid && start < (int64_t)B.end && stop > (int64_t)B.beg && !(R.flag & (EVF_SECONDARY | EVF_SUPPL | EVF_DUP)) && R.mapq >= min_mapq)) return false;
  const int64_t D = B.depth_n;
  int64_t a = start - B.wl - 1, b = stop - B.wl - 1;
  if (a < 0) a = 0;
  if (a > D - 1) a = D - 1;                              // (cannot happen: start < end = wl + D; keeps the store inside the array whatever comes)
  if (b > D - 1) b = D - 1;
  if (b < 0) b = 0;
  *slot_a = (int32_t)a; *slot_b = (int32_t)b;
  return true;
}

// step 3: the row of the kept record R, the ord-th of the region and the k-th kept one (name_id starts as the row's own number)
EV_FN EvRow ev_row(const EvRec &R, int64_t stop, const EvBound &B, const float *cd, uint32_t ord, uint32_t k, bool *bad) {
  const int64_t start = R.pos;
  EvRow row;
  row.ord = ord; row.name_id = k;
  row.hash = (uint32_t)nim::hash_bytes(R.qname(), (int)R.qname_len());
  row.prob = ev_expected_spanning_probability(cd, start, stop, (R.flag & EVF_REVERSE) != 0, B.left, B.right);
  row.start = R.pos; row.isize = R.isize; row.stop = stop;
  row.flags = 0; row.type = 0; row.repeat_count = 0; row.cigar_ins = 0; row.cigar_del = 0; row.pad[0] = 0; row.pad[1] = 0;
  if ((start > B.left ? start : B.left) <= (stop < B.right ? stop : B.right)) {   // collect.nim:97-119 (the record's tid is the bound's)
    row.flags |= EV_OVERLAP;
    row.type = STRL_OVERLAPPING_READ;
    row.repeat_count = (uint8_t)ev_count_in_bounds(R, B, bad);
    if (start < B.left - B.slop && stop > B.right + B.slop) {
      row.type = STRL_SPANNING_READ;
      for (uint32_t j = 0; j < R.n_cig; ++j) {
        const uint32_t c = R.cig(j);
        if ((c & 0xf) == 1u) row.cigar_ins = (uint8_t)(row.cigar_ins + (uint8_t)(c >> 4));
        if ((c & 0xf) == 2u) row.cigar_del = (uint8_t)(row.cigar_del + (uint8_t)(c >> 4));
      }
    }
  }
  const int64_t tl = R.isize < 0 ? -(int64_t)R.isize : (int64_t)R.isize;
  if (R.tid == R.mtid && tl <= 5000) row.flags |= EV_PAIR;
  return row;
}

// ---- host only: the bound as the kernel takes it
inline int64_t ev_slop(const strl_bounds &b, int k) {   // bound_slop, collect.nim:97-104
  const int64_t width = (int64_t)b.right - (int64_t)b.left;
  int64_t slop = (int64_t)k - 1;
  if (width < 5) slop += 5 - width;
  return slop;
}
// status: what the caller knows of the region already (0: for the device).  The capacity rule: a depth array of
// 1 .. EV_MAX_SPAN entries in LDS (and a query that is one: window >= 0, a unit to count); beyond it the status is 2
inline EvBound ev_bound_make(const strl_bounds &b, int32_t window, uint32_t status) {
  EvBound E;
  memset(&E, 0, sizeof E);
  E.left = b.left; E.right = b.right; E.wl = (int64_t)b.left - window;
  const int64_t wr = (int64_t)b.right + window, span = wr - E.wl;
  E.tid = b.tid;
  E.beg = (int32_t)(E.wl > 0 ? E.wl : 0);
  E.end = (int32_t)(wr < INT32_MAX ? wr : INT32_MAX);
  E.k = (int)strnlen(b.repeat, 6);
  memcpy(&E.unit, b.repeat, 6);
  E.slop = (int32_t)ev_slop(b, E.k);
  E.status = status;
  if (!E.status && (window < 0 || span < 1 || span > EV_MAX_SPAN || wr > INT32_MAX || E.k < 1)) E.status = 2;
  E.depth_n = E.status ? 0 : (int32_t)span;
  return E;
}

}  // namespace strl
