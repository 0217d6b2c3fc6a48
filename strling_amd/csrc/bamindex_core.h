// bamindex_core.h -- the rules of a BAM index (.bai, SAM spec 5.2; CSIv1) that do not depend on where the records come from, one
// source for the device builder (bamindex.hip: behind the record scan, behind extract's parse, over a sort's records), the host
// builder (bamindex_host.cpp: `strling sort --write-index` without a device) and the stand-alone test program
// (tests/emu/bamindex_host_main.cpp): the binning scheme, reg2bin, what a record is refused for and in which words, the linear
// index's window tables, and the bytes of the file from the merged chunks.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <algorithm>
#include <string>
#include <vector>
#include "../../include/strling_amd.h"
#include "bam_rec.h"
#if defined(__HIPCC__)
#define BAI_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define BAI_FN inline
#endif

namespace strl {

constexpr uint32_t BAI_ERR_KINDS = 5;
constexpr uint32_t BAI_E_UNSORTED = 0, BAI_E_RANGE = 1, BAI_E_TID = 2, BAI_E_LREF = 3, BAI_E_NEGPOS = 4;
constexpr uint64_t BAI_KEY_NONE = ~0ull;
constexpr int32_t BAI_MAX_POS = 1 << 29;       // what the five-level binning scheme of a .bai addresses
constexpr int64_t BAI_LREF_SLACK = 1 << 20;    // bases of the linear index kept behind l_ref: max(1, 2^20 >> min_shift) windows (64 of a .bai)
constexpr int32_t CSI_MIN_SHIFT_LO = 8, CSI_MIN_SHIFT_HI = 24, CSI_DEPTH_HI = 8;      // schemes strl_*_begin_csi accepts
constexpr int32_t CSI_MAX_END = 0x7ffffffe;    // bai_read clamps an end to 2^31 - 1: an end of that value may be a clamped one and is refused

// The binning scheme (CSIv1): windows of 2^min_shift bases, `depth` levels of bins below bin 0.  A .bai is (14, 5).  A bin number is
// below 2^(3 depth + 1), so the bin field of a run's key has key_shift = 3 depth + 1 bits (16 for a .bai).
struct BaiScheme { int32_t min_shift, depth, key_shift, max_end; };   // max_end: the largest end of a record the scheme (and a BAM position) holds
struct BaiChunk { uint64_t key, beg_v, end_v; };                      // key = tid << key_shift | bin

struct BaiRec { int32_t tid, pos, end; uint32_t flag, bs; };

// the five numbers of a record of `len` bytes (block_size word included) that no scan has walked: false when the fixed fields or the
// CIGAR do not lie inside len -- nothing behind R + len is read
BAI_FN bool bai_read_bounded(const uint8_t *R, uint32_t len, BaiRec &r) {
  if (len < 36u) return false;
  const uint32_t l_name = R[12], n_cig = rec_ld16(R + 16);
  if (36u + l_name + 4u * n_cig > len) return false;
  r.bs = rec_ld32(R);
  r.tid = (int32_t)rec_ld32(R + 4); r.pos = (int32_t)rec_ld32(R + 8);
  r.flag = rec_ld16(R + 18);
  const int64_t e = bam_rec_end(R);
  r.end = e > 0x7fffffffll ? 0x7fffffff : (int32_t)e;
  return true;
}

BAI_FN uint32_t bai_reg2bin(int32_t beg, int32_t end) {      // SAM spec 5.3
  --end;
  if (beg >> 14 == end >> 14) return 4681u + (uint32_t)(beg >> 14);
  if (beg >> 17 == end >> 17) return 585u + (uint32_t)(beg >> 17);
  if (beg >> 20 == end >> 20) return 73u + (uint32_t)(beg >> 20);
  if (beg >> 23 == end >> 23) return 9u + (uint32_t)(beg >> 23);
  if (beg >> 26 == end >> 26) return 1u + (uint32_t)(beg >> 26);
  return 0u;
}
// the CSI specification's reg2bin for (min_shift, depth); every lane makes all `depth` trips (at most 8), shifts in 64 bits
// (min_shift + 3 (depth - 1) reaches 45).  depth 0: no trip, bin 0
BAI_FN uint32_t csi_reg2bin(int32_t beg, int32_t end, int32_t min_shift, int32_t depth) {
  const uint64_t b = (uint64_t)(uint32_t)beg, e = (uint64_t)(uint32_t)(end - 1);
  uint32_t t = (uint32_t)(((1ull << (3 * depth)) - 1ull) / 7ull), bin = 0;
  int32_t s = min_shift;
  bool found = false;
  for (int32_t l = depth; l > 0; --l) {
    const bool hit = !found && (b >> s) == (e >> s);
    bin = hit ? t + (uint32_t)(b >> s) : bin;
    found = found || hit;
    s += 3;
    t -= 1u << (3 * (l - 1));
  }
  return bin;
}
// a record the index can hold: a reference of the header, 0 <= pos, end <= what the scheme addresses (2^29 for a .bai), its last
// window one of the reference's n_win (l_ref and 1 Mbase behind it: aligners do leave reads that hang over the end of a contig).
// else the kind of refusal.  n_win is read only for a placed record inside the scheme: pass a callable that loads it
template <class NWin> BAI_FN int bai_refusal_rule(int32_t tid, int32_t pos, int32_t end, int32_t n_ref, int32_t max_end, int32_t min_shift, NWin n_win) {
  if (tid < -1 || tid >= n_ref) return (int)BAI_E_TID;
  if (tid < 0) return -1;
  if (pos < 0) return (int)BAI_E_NEGPOS;
  if (pos >= max_end || end > max_end) return (int)BAI_E_RANGE;
  if ((uint64_t)((end - 1) >> min_shift) >= n_win(tid)) return (int)BAI_E_LREF;
  return -1;
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
// the schemes the builders take: window tables and bin numbers stay small
inline bool csi_scheme_ok(int32_t m, int32_t d, std::string &err) {
  if (m >= CSI_MIN_SHIFT_LO && m <= CSI_MIN_SHIFT_HI && d <= CSI_DEPTH_HI) return true;
  char b[200];
  snprintf(b, sizeof b, "CSI scheme: min_shift must be in [%d, %d] and depth at most %d (got min_shift %d, depth %d)", CSI_MIN_SHIFT_LO, CSI_MIN_SHIFT_HI, CSI_DEPTH_HI, m, d);
  err = b;
  return false;
}
// csi: null = a .bai; else {min_shift, depth}, depth < 0 = samtools' rule (the smallest depth whose scheme reaches max(l_ref) + 256)
inline bool bai_scheme_make(const int32_t *csi, int32_t n_ref, const int32_t *l_ref, BaiScheme &sch, std::string &err) {
  sch = BaiScheme{14, 5, 16, BAI_MAX_POS};
  if (!csi) return true;
  int32_t m = csi[0], d = csi[1];
  if (!csi_scheme_ok(m, d, err)) return false;
  if (d < 0) {
    int64_t max_len = 0;
    for (int32_t t = 0; t < n_ref; ++t) max_len = std::max<int64_t>(max_len, l_ref[t]);
    max_len += 256;
    for (d = 0; d < CSI_DEPTH_HI && (1ll << (m + 3 * d)) < max_len; ++d) {}
  }
  sch = BaiScheme{m, d, 3 * d + 1, (int32_t)std::min<int64_t>(1ll << (m + 3 * d), CSI_MAX_END)};
  return true;
}
// win_off[n_ref + 1]: first window of each reference in the linear index.  windows of 2^min_shift bases up to l_ref and 1 Mbase
// behind it, never more than the scheme addresses ((14, 5): 64 behind l_ref, at most 2^15)
inline void bai_windows(const BaiScheme &sch, int32_t n_ref, const int32_t *l_ref, std::vector<uint64_t> &win_off) {
  win_off.assign((size_t)n_ref + 1, 0);
  const int64_t win = 1ll << sch.min_shift, slack = std::max<int64_t>(1, BAI_LREF_SLACK >> sch.min_shift);
  for (int32_t t = 0; t < n_ref; ++t) {
    const int64_t len = std::min<int64_t>(std::max<int64_t>(l_ref[t], 0), sch.max_end);
    win_off[(size_t)t + 1] = win_off[(size_t)t] + (uint64_t)std::min<int64_t>(((len + win - 1) >> sch.min_shift) + slack, ((int64_t)sch.max_end + win - 1) >> sch.min_shift);
  }
}
// the words of a refusal of `kind` at the record of ordinal `at`, and the status that goes with it
inline int bai_refusal_text(uint32_t kind, uint64_t at_, bool csi, bool auto_depth, const BaiScheme &sch, int32_t n_ref, std::string &msg) {
  const unsigned long long at = (unsigned long long)at_;
  char b[600];
  int rc = STRL_ERR_FORMAT;
  switch (kind) {
    case BAI_E_UNSORTED: snprintf(b, sizeof b, "the BAM is not coordinate sorted: record %llu comes behind a record of a later position (or behind an unplaced one); sort it first", at); break;
    case BAI_E_RANGE:
      if (!csi) snprintf(b, sizeof b, "record %llu lies at or reaches past position 2^29 = 536870912, which a .bai cannot address; a CSI index can: `strling bamindex --csi` (strl_bamindex_begin_csi)", at);
      else if (sch.max_end == CSI_MAX_END) snprintf(b, sizeof b, "record %llu reaches position 2^31 - 1 = 2147483647 or past it, which a BAM position cannot hold; not indexed", at);
      else if (auto_depth)
        snprintf(b, sizeof b, "record %llu lies at or reaches past position 2^%d = %lld, which the CSI scheme (min_shift %d, depth %d: chosen for the longest reference of the header) cannot "
                 "address: the record lies past the end of its reference", at, sch.min_shift + 3 * sch.depth, (long long)sch.max_end, sch.min_shift, sch.depth);
      else snprintf(b, sizeof b, "record %llu lies at or reaches past position 2^%d = %lld, which the CSI scheme (min_shift %d, depth %d) cannot address; a greater depth can", at,
                    sch.min_shift + 3 * sch.depth, (long long)sch.max_end, sch.min_shift, sch.depth);
      rc = STRL_ERR_LIMIT;
      break;
    case BAI_E_TID: snprintf(b, sizeof b, "malformed BAM record %llu: its refID is not one of the header's %d references", at, n_ref); break;
    case BAI_E_LREF: snprintf(b, sizeof b, "record %llu reaches more than %lld bases past the end of its reference as the header gives it (l_ref); not indexed", at, (long long)std::max<int64_t>(BAI_LREF_SLACK, 1ll << sch.min_shift)); break;
    default: snprintf(b, sizeof b, "record %llu has a reference but a negative position; not indexed", at); break;
  }
  msg = b;
  return rc;
}
// the first refusal of err_ord[BAI_ERR_KINDS] (~0 = none): its kind, BAI_ERR_KINDS when there is none
inline uint32_t bai_first_refusal(const uint64_t *err_ord) {
  uint32_t kind = BAI_ERR_KINDS;
  for (uint32_t k = 0; k < BAI_ERR_KINDS; ++k)
    if (err_ord[k] != ~0ull && (kind == BAI_ERR_KINDS || err_ord[k] < err_ord[kind])) kind = k;
  return kind;
}

inline void bai_put32(std::vector<uint8_t> &o, uint32_t v) { for (int k = 0; k < 4; ++k) o.push_back((uint8_t)(v >> (8 * k))); }
inline void bai_put64(std::vector<uint8_t> &o, uint64_t v) { for (int k = 0; k < 8; ++k) o.push_back((uint8_t)(v >> (8 * k))); }

// The bytes: per reference the bins ascending with their chunks, the pseudo-bin last, n_no_coor at the end.  .bai (SAM spec
// 5.2): the linear index up to the last window touched behind the bins (empty windows 0).  CSI (CSIv1): no linear index, every
// bin carries loffset = the linear index at the bin's first window, after empty windows have taken the next filled window's
// value from the end towards the start (htslib's update_loff); 0 behind the last window touched.  Done on the caller's copy of
// lin[] (~0 = no record reached the window), which is changed: one pass over words that are copied anyway, and a gather per bin
// beside the bytes being written.  ch: the chunks sorted by key, in file order inside a key.  rb / re: per reference the virtual
// offsets of its first record and behind its last; cnt[2 t], cnt[2 t + 1]: mapped / placed-unmapped records.  -> chunks written
inline uint64_t bai_pack(const BaiScheme &sch, bool csi, int32_t n_ref, const std::vector<uint64_t> &win_off, const std::vector<BaiChunk> &ch, std::vector<uint64_t> &lin,
                         const std::vector<uint64_t> &rb, const std::vector<uint64_t> &re, const std::vector<uint64_t> &cnt, uint64_t n_no_coor, std::vector<uint8_t> &o) {
  const size_t nr = (size_t)n_ref, nw = (size_t)win_off[nr];
  const int ks = sch.key_shift, m = sch.min_shift, d = sch.depth;
  const uint64_t bin_mask = (1ull << ks) - 1ull;
  const uint32_t meta_bin = (uint32_t)(((1ull << (3 * (d + 1))) - 1ull) / 7ull + 1ull);      // 37450 for depth 5
  o.clear();
  o.reserve(16 + ch.size() * 36 + (csi ? 0 : nw * 8) + nr * 64 + 8);
  if (csi) { o.insert(o.end(), {'C', 'S', 'I', 1}); bai_put32(o, (uint32_t)m); bai_put32(o, (uint32_t)d); bai_put32(o, 0); }
  else o.insert(o.end(), {'B', 'A', 'I', 1});
  bai_put32(o, (uint32_t)n_ref);
  size_t at = 0;
  uint64_t n_chunks = 0;
  for (size_t t = 0; t < nr; ++t) {
    size_t e = at, n_bin = 0;
    while (e < ch.size() && (ch[e].key >> ks) == t) { if (e == at || ch[e].key != ch[e - 1].key) ++n_bin; ++e; }
    const bool meta = cnt[2 * t] + cnt[2 * t + 1] != 0;
    const uint64_t w0 = win_off[t], w1 = win_off[t + 1];
    uint64_t n_intv = 0;
    for (uint64_t w = w1; w > w0; --w) if (lin[(size_t)w - 1] != ~0ull) { n_intv = w - w0; break; }
    if (csi)
      for (uint64_t w = n_intv; w > 1; --w) if (lin[(size_t)(w0 + w - 2)] == ~0ull) lin[(size_t)(w0 + w - 2)] = lin[(size_t)(w0 + w - 1)];
    bai_put32(o, (uint32_t)(n_bin + (meta ? 1 : 0)));
    for (size_t a = at; a < e;) {
      size_t b = a;
      while (b < e && ch[b].key == ch[a].key) ++b;
      const uint32_t bin = (uint32_t)(ch[a].key & bin_mask);
      bai_put32(o, bin);
      if (csi) {
        // the bin's level: the first bin of level l is (8^l - 1) / 7; its bins cover 2^(m + 3 (d - l)) bases = 8^(d - l) windows each
        int l = 0;
        while (l < d && bin >= (uint32_t)(((1ull << (3 * (l + 1))) - 1ull) / 7ull)) ++l;
        const uint64_t w = (uint64_t)(bin - (uint32_t)(((1ull << (3 * l)) - 1ull) / 7ull)) << (3 * (d - l));
        bai_put64(o, w < n_intv ? lin[(size_t)(w0 + w)] : 0);
      }
      bai_put32(o, (uint32_t)(b - a));
      for (size_t k = a; k < b; ++k) { bai_put64(o, ch[k].beg_v); bai_put64(o, ch[k].end_v); }
      n_chunks += b - a;
      a = b;
    }
    if (meta) { bai_put32(o, meta_bin); if (csi) bai_put64(o, 0); bai_put32(o, 2); bai_put64(o, rb[t]); bai_put64(o, re[t]); bai_put64(o, cnt[2 * t]); bai_put64(o, cnt[2 * t + 1]); }
    if (!csi) {
      bai_put32(o, (uint32_t)n_intv);
      for (uint64_t w = 0; w < n_intv; ++w) { const uint64_t v = lin[(size_t)(w0 + w)]; bai_put64(o, v == ~0ull ? 0 : v); }
    }
    at = e;
  }
  bai_put64(o, n_no_coor);
  return n_chunks;
}

}  // namespace strl
