// view_core.h -- the rule of `strling view` (a BAM's records as SAM text), one source for the device path (view.hip), the host path
// and the library's host entry (view_host.cpp: strl_view_host) and the stand-alone test program (tests/emu/view_core_main.cpp).
// DESIGN section 24.5.  What `samtools view` is used for; agreement with htslib is unverified (no machine of the project has it).
//
// One record becomes one line:
//   QNAME \t FLAG \t RNAME \t POS \t MAPQ \t CIGAR \t RNEXT \t PNEXT \t TLEN \t SEQ \t QUAL [\t TAG:TYPE:VALUE]... \n
//
//   kept        (flag & require) == require, (flag & exclude) == 0, not (exclude_all != 0 and (flag & exclude_all) == exclude_all),
//               mapq >= min_mapq (-f, -F, -G, -q).  With a region (opts.tid != -2) also tid == region.tid && pos < end && endpos > beg,
//               endpos = pos + the CIGAR's reference length (over M, D, N, =, X), pos + 1 where that length is 0 or flag 4 is set
//               (bam_rec.h's rule, which bamindex_core.h applies).  A record that is not kept owns 0 bytes and is counted as dropped.
//   refused     every record, kept or not: its name, CIGAR, bases and qualities do not fit its block_size (mdup_fields' check), or it holds more
//               than 2^28 bytes.
//               A kept record also for what is marked "refused" below.  The first refused record ends the command; the message names
//               its ordinal and the field.  Where one record earns several refusals the first in the order size, RNAME, RNEXT, CIGAR,
//               tags is named.
//   QNAME       the l_read_name - 1 name bytes as they are, or * when there are none.
//   FLAG, MAPQ  unsigned decimals.
//   POS, PNEXT  pos + 1 and mpos + 1 as signed decimals, so -1 prints 0.
//   TLEN        a signed decimal.
//   RNAME       * for tid < 0, else the reference's name: names[name_off[tid], name_off[tid + 1]).  tid >= n_ref is refused.
//   RNEXT       * for mtid < 0, = for mtid == tid, else the name.  mtid >= n_ref is refused.
//   CIGAR       * for 0 operations, else <len><op> an operation, op from "MIDNSHP=X".  An op code above 8 is refused, as sam_core.h
//               refuses it on the way in.  The CG:B:I convention of long CIGARs is not interpreted.
//   SEQ         * for l_seq == 0, else the 4-bit codes through "=ACMGRSVTWYHKDBN".  The padding nibble of an odd l_seq is never read.
//   QUAL        * for l_seq == 0 and where the first quality byte is 0xFF (htslib's test); else min(q, 93) + 33 a byte.  The clamp is
//               a deliberate difference from htslib, which adds 33 to whatever the byte holds and can so write a newline or a byte
//               above 126 into the line; a 0xFF behind a valid first byte is a value like any other here (clamped to '~').
//   tags        A prints A:c.  c C s S i I print i: and the decimal.  f prints f: and the bytes of snprintf("%g", (double)value); d
//               prints d: and the bytes of snprintf("%g", value).  Z and H print the bytes up to the NUL.  B prints B:<t> and ,value
//               an element (a count of 0 is allowed: B:<t> alone), t in cCsSiIf.  Refused: an unknown type (or B subtype), a Z or H
//               without a NUL inside the record, a B whose elements leave the record, tag bytes that do not end exactly at the
//               record's end.
//   floats      view_float_g gives the exact bytes of %g (precision 6, round-half-even on the exact value, as glibc prints it) in
//               integer arithmetic for +-0 and for every float with 2^-17 <= |v| < 2^63 (biased exponent in [110, 189]); for all
//               others -- inf, nan, subnormals, smaller and larger magnitudes -- it says "not mine" (returns 0).  A double is the
//               float of the same value where there is one in that range, else "not mine".  The device marks a record with such a
//               value "hard" and its chunk is formatted by view_host below, which asks snprintf for those; the bytes are the same.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>
#include "markdup_core.h"

namespace strl {

constexpr int32_t VIEW_NO_REGION = -2;
constexpr uint32_t VIEW_QUAL_MAX = 93;
constexpr uint64_t VIEW_REC_MAX = 1ull << 28;                  // bytes of a record: its line (at most 5 a byte) then fits 32 bits
constexpr uint32_t VIEW_G_EXP_LO = 110, VIEW_G_EXP_HI = 189;      // biased exponents view_float_g answers: 2^-17 <= |v| < 2^63
// the field codes of a refusal, in the order they are named
enum : uint32_t { VIEW_E_NONE = 0, VIEW_E_SIZE, VIEW_E_RNAME, VIEW_E_RNEXT, VIEW_E_CIGAR, VIEW_E_TAG_TYPE, VIEW_E_TAG_Z, VIEW_E_TAG_B, VIEW_E_TAG_END, VIEW_E_KINDS };
inline const char *view_refusal_text(uint32_t code) {
  static const char *const t[VIEW_E_KINDS] = {
      "", "its name, CIGAR, bases and qualities do not fit its block_size", "RNAME: its refID is not one of the header's references",
      "RNEXT: its next refID is not one of the header's references", "CIGAR: an operation code above 8", "tags: an unknown type",
      "tags: a Z or H value without its NUL inside the record", "tags: a B array whose elements leave the record",
      "tags: they do not end exactly at the record's end"};
  return code < VIEW_E_KINDS ? t[code] : "";
}

struct ViewOpts { uint32_t require, exclude, exclude_all, min_mapq; int32_t tid, beg, end; };
struct ViewRefs { const uint8_t *names; const uint32_t *name_off; int32_t n_ref; };      // name_off[n_ref + 1]
struct ViewCounts { uint64_t records, written, dropped, text_bytes; };

// where the parts of a record lie (from its block_size word) and its fixed fields
struct ViewRec {
  MdupFields f;
  int32_t mtid, mpos, tlen;
  uint32_t mapq, n_name, seq_at, tags_at, n_tags;
};
// false: the parts do not fit `len` = 4 + block_size (or len is above VIEW_REC_MAX)
MDUP_HD inline bool view_rec(const uint8_t *rec, uint64_t len, ViewRec *R) {
  if (len > VIEW_REC_MAX || !mdup_fields(rec, len, &R->f)) return false;
  R->mapq = rec[13];
  R->mtid = (int32_t)mdup_ld32(rec + 24); R->mpos = (int32_t)mdup_ld32(rec + 28); R->tlen = (int32_t)mdup_ld32(rec + 32);
  R->n_name = R->f.l_name ? R->f.l_name - 1u : 0u;
  R->seq_at = R->f.qual_at - (R->f.l_seq + 1u) / 2u;
  R->tags_at = R->f.qual_at + R->f.l_seq;
  R->n_tags = (uint32_t)len - R->tags_at;
  return true;
}
MDUP_HD inline bool view_cigar_on_ref(uint32_t op) { return op == 0u || op == 2u || op == 3u || op == 7u || op == 8u; }
// `reflen`: the sum of the lengths of the CIGAR's operations that consume the reference
MDUP_HD inline bool view_kept(const ViewRec &R, const ViewOpts &o, uint64_t reflen) {
  const uint32_t flag = R.f.flag;
  if ((flag & o.require) != o.require || (flag & o.exclude) || (o.exclude_all && (flag & o.exclude_all) == o.exclude_all) || R.mapq < o.min_mapq) return false;
  if (o.tid == VIEW_NO_REGION) return true;
  const int64_t endpos = (int64_t)R.f.pos + (reflen && !(flag & 4u) ? (int64_t)reflen : 1);
  return R.f.tid == o.tid && R.f.pos < o.end && endpos > o.beg;
}

MDUP_HD inline uint32_t view_udigits(uint64_t v) { uint32_t d = 1; while (v >= 10u) { v /= 10u; ++d; } return d; }
MDUP_HD inline uint64_t view_pow10(uint32_t k) { uint64_t p = 1; while (k--) p *= 10u; return p; }
MDUP_HD inline uint8_t view_cigar_letter(uint32_t op) {      // "MIDNSHP=X", no table in memory
  constexpr uint64_t lo = (uint64_t)'M' | (uint64_t)'I' << 8 | (uint64_t)'D' << 16 | (uint64_t)'N' << 24 | (uint64_t)'S' << 32 | (uint64_t)'H' << 40 | (uint64_t)'P' << 48 | (uint64_t)'=' << 56;
  return op < 8u ? (uint8_t)(lo >> (op * 8u)) : (uint8_t)'X';
}
MDUP_HD inline uint8_t view_base(uint32_t code) {            // "=ACMGRSVTWYHKDBN"
  constexpr uint64_t lo = (uint64_t)'=' | (uint64_t)'A' << 8 | (uint64_t)'C' << 16 | (uint64_t)'M' << 24 | (uint64_t)'G' << 32 | (uint64_t)'R' << 40 | (uint64_t)'S' << 48 | (uint64_t)'V' << 56;
  constexpr uint64_t hi = (uint64_t)'T' | (uint64_t)'W' << 8 | (uint64_t)'Y' << 16 | (uint64_t)'H' << 24 | (uint64_t)'K' << 32 | (uint64_t)'D' << 40 | (uint64_t)'B' << 48 | (uint64_t)'N' << 56;
  return (uint8_t)((code & 8u ? hi : lo) >> ((code & 7u) * 8u));
}
MDUP_HD inline uint8_t view_qual(uint32_t q) { return (uint8_t)((q < VIEW_QUAL_MAX ? q : VIEW_QUAL_MAX) + 33u); }
// the lengths of SEQ and QUAL in the line
MDUP_HD inline uint32_t view_seq_len(const ViewRec &R) { return R.f.l_seq ? R.f.l_seq : 1u; }
MDUP_HD inline uint32_t view_qual_len(const uint8_t *rec, const ViewRec &R) { return R.f.l_seq && rec[R.f.qual_at] != 0xffu ? R.f.l_seq : 1u; }

// The exact bytes of snprintf("%g", (double)v) for +-0 and 2^-17 <= |v| < 2^63, in integer arithmetic; 0 = "not mine".
//   v = m 2^e (m < 2^24) is the fraction num / den of two 64-bit integers scaled so that its integer part has six digits: k =
//   floor(log10 v) from the digits of v's integer part, or from the first power of ten that lifts m over 2^-e; num / den =
//   v / 10^(k - 5); the quotient is rounded half to even on the remainder, and 10^6 carries into the exponent.  The largest
//   intermediate is m 10^11 < 2^61.  Then %g's choice: the exponent X = k in [-4, 6) prints fixed, else d.ddddde+-XX; trailing zeros
//   and a bare point go.
template <typename S> MDUP_HD inline bool view_float_g_emit(S &s, float v) {
  uint32_t u;
  memcpy(&u, &v, 4);
  const uint32_t E = u >> 23 & 255u, frac = u & 0x7fffffu;
  if ((E || frac) && (E < VIEW_G_EXP_LO || E > VIEW_G_EXP_HI)) return false;
  if (u >> 31) s.put('-');
  if (!E && !frac) { s.put('0'); return true; }
  const uint64_t m = frac | 0x800000u;
  const int e = (int)E - 150;                               // in [-40, 39]
  const uint32_t sh = e < 0 ? (uint32_t)-e : 0u;
  const uint64_t whole = e >= 0 ? m << e : m >> sh, num0 = e >= 0 ? m << e : m;      // v = num0 / 2^sh
  int k;
  if (whole) k = (int)view_udigits(whole) - 1;
  else { k = -1; for (uint64_t t = m * 10u; t < (1ull << sh); t *= 10u) --k; }      // (k >= -6: t <= m 10^6)
  uint64_t num, den;
  if (k <= 5) { num = num0 * view_pow10((uint32_t)(5 - k)); den = 1ull << sh; }
  else { num = num0; den = view_pow10((uint32_t)(k - 5)) << sh; }                 // (v >= 10^6 with e < 0: sh <= 4)
  uint64_t q64 = num / den;
  const uint64_t r = num % den;
  if (2u * r > den || (2u * r == den && (q64 & 1u))) ++q64;
  if (q64 == 1000000u) { q64 = 100000u; ++k; }
  const uint32_t q = (uint32_t)q64;
  // the six digits as nibbles, the first in the lowest (no array: the kernels keep them in a register)
  const uint32_t dg = q / 100000u | q / 10000u % 10u << 4 | q / 1000u % 10u << 8 | q / 100u % 10u << 12 | q / 10u % 10u << 16 | q % 10u << 20;
  int nd = 6;
  while (nd > 1 && !(dg >> (4 * (nd - 1)) & 15u)) --nd;
  auto digit = [dg](int i) { return (uint8_t)('0' + (dg >> (4 * i) & 15u)); };
  if (k < -4 || k >= 6) {
    s.put(digit(0));
    if (nd > 1) { s.put('.'); for (int i = 1; i < nd; ++i) s.put(digit(i)); }
    s.put('e'); s.put(k < 0 ? '-' : '+');
    const uint32_t a = (uint32_t)(k < 0 ? -k : k);          // (at most 18)
    s.put((uint8_t)('0' + a / 10u)); s.put((uint8_t)('0' + a % 10u));
  } else if (k >= 0) {
    for (int i = 0; i <= k; ++i) s.put(digit(i));
    if (nd > k + 1) { s.put('.'); for (int i = k + 1; i < nd; ++i) s.put(digit(i)); }
  } else {
    s.put('0'); s.put('.');
    for (int i = -1; i > k; --i) s.put('0');
    for (int i = 0; i < nd; ++i) s.put(digit(i));
  }
  return true;
}
// ... of a double: the float of the same value, where there is one
template <typename S> MDUP_HD inline bool view_double_g_emit(S &s, double v) {
  const float f = (float)v;
  return (double)f == v && view_float_g_emit(s, f);
}
// ... into out[16] -> the count of bytes, 0 = "not mine" (the host's and the test program's form)
inline uint32_t view_float_g(float v, char out[16]) {
  struct Arr { char *o; uint32_t n; void put(uint8_t b) { o[n++] = (char)b; } } a{out, 0};
  return view_float_g_emit(a, v) ? a.n : 0u;
}

// ---- where the text goes: a sink counts it or stores it, the text itself is written once -------------------------------------------
struct ViewCount {                                           // the size of the text
  uint64_t n = 0;
  MDUP_HD void put(uint8_t) { ++n; }
  MDUP_HD void bytes(const uint8_t *, uint32_t k) { n += k; }
  MDUP_HD void num(uint64_t v) { n += view_udigits(v); }
};
struct ViewStore {                                           // the text into [p, end): nothing behind `end` is written
  uint8_t *p, *end;
  MDUP_HD void put(uint8_t b) { if (p < end) *p = b; ++p; }
  MDUP_HD void bytes(const uint8_t *s, uint32_t k) { for (uint32_t i = 0; i < k; ++i) put(s[i]); }
  MDUP_HD void num(uint64_t v) {                            // backwards from the last digit's place: no array
    uint8_t *q = p + view_udigits(v);
    p = q;
    do { --q; if (q < end) *q = (uint8_t)('0' + v % 10u); v /= 10u; } while (v);
  }
};
template <typename S> MDUP_HD inline void view_inum(S &s, int64_t v) {
  if (v < 0) { s.put('-'); s.num((uint64_t)0 - (uint64_t)v); } else s.num((uint64_t)v);
}
template <typename S> MDUP_HD inline void view_ref_name(S &s, const ViewRefs &F, int32_t tid) {
  if (tid < 0 || tid >= F.n_ref) { s.put('*'); return; }      // (a tid >= n_ref has been refused)
  s.bytes(F.names + F.name_off[tid], F.name_off[tid + 1] - F.name_off[tid]);
}
// QNAME \t FLAG \t RNAME \t POS \t MAPQ \t
template <typename S> MDUP_HD inline void view_head_emit(S &s, const uint8_t *rec, const ViewRec &R, const ViewRefs &F) {
  if (R.n_name) s.bytes(rec + MDUP_FIXED, R.n_name); else s.put('*');
  s.put('\t'); s.num(R.f.flag);
  s.put('\t'); view_ref_name(s, F, R.f.tid);
  s.put('\t'); view_inum(s, (int64_t)R.f.pos + 1);
  s.put('\t'); s.num(R.mapq);
  s.put('\t');
}
// \t RNEXT \t PNEXT \t TLEN \t
template <typename S> MDUP_HD inline void view_mid_emit(S &s, const ViewRec &R, const ViewRefs &F) {
  s.put('\t');
  if (R.mtid >= 0 && R.mtid == R.f.tid) s.put('='); else view_ref_name(s, F, R.mtid);
  s.put('\t'); view_inum(s, (int64_t)R.mpos + 1);
  s.put('\t'); view_inum(s, (int64_t)R.tlen);
  s.put('\t');
}
template <typename S> MDUP_HD inline void view_cigar_op_emit(S &s, uint32_t w) { s.num(w >> 4); s.put(view_cigar_letter(w & 15u)); }
template <typename S> MDUP_HD inline void view_cigar_emit(S &s, const uint8_t *rec, const ViewRec &R) {
  if (!R.f.n_cigar) { s.put('*'); return; }
  for (uint32_t k = 0; k < R.f.n_cigar; ++k) view_cigar_op_emit(s, mdup_ld32(rec + R.f.cigar_at + 4u * k));
}
template <typename S> MDUP_HD inline void view_g_emit(S &s, bool is_double, const uint8_t *p, uint32_t *hard) {
  float f = 0.f;
  double d = 0.0;
  if (is_double) memcpy(&d, p, 8); else memcpy(&f, p, 4);
  if (is_double ? view_double_g_emit(s, d) : view_float_g_emit(s, f)) return;
#if defined(__HIP_DEVICE_COMPILE__)
  *hard = 1u;
#else
  char b[32];
  const int n = snprintf(b, sizeof b, "%g", is_double ? d : (double)f);
  s.bytes(reinterpret_cast<const uint8_t *>(b), (uint32_t)n);
  *hard = 1u;
#endif
}
MDUP_HD inline uint32_t view_tag_size(uint8_t t) {           // bytes of a number of type t; 0: no such type
  return t == 'c' || t == 'C' ? 1u : t == 's' || t == 'S' ? 2u : t == 'i' || t == 'I' || t == 'f' ? 4u : 0u;
}
template <typename S> MDUP_HD inline void view_tag_num(S &s, uint8_t t, const uint8_t *p, uint32_t *hard) {
  switch (t) {
    case 'c': view_inum(s, (int64_t)(int8_t)p[0]); break;
    case 'C': s.num(p[0]); break;
    case 's': view_inum(s, (int64_t)(int16_t)mdup_ld16(p)); break;
    case 'S': s.num(mdup_ld16(p)); break;
    case 'i': view_inum(s, (int64_t)(int32_t)mdup_ld32(p)); break;
    case 'I': s.num(mdup_ld32(p)); break;
    default: view_g_emit(s, false, p, hard); break;           // 'f'
  }
}
// [\t TAG:TYPE:VALUE]... of the tag bytes t[0, n) -> VIEW_E_NONE or the refusal; *hard = 1 where a float is "not mine" (its bytes are
// then left out: the caller formats the record again where snprintf is)
template <typename S> MDUP_HD inline uint32_t view_tags_emit(S &s, const uint8_t *t, uint32_t n, uint32_t *hard) {
  uint32_t p = 0;
  while (p < n) {
    if (n - p < 3u) return VIEW_E_TAG_END;
    const uint8_t type = t[p + 2];
    s.put('\t'); s.put(t[p]); s.put(t[p + 1]); s.put(':');
    p += 3u;
    if (type == 'A') {
      if (n - p < 1u) return VIEW_E_TAG_END;
      s.put('A'); s.put(':'); s.put(t[p]); p += 1u;
    } else if (type == 'd') {
      if (n - p < 8u) return VIEW_E_TAG_END;
      s.put('d'); s.put(':'); view_g_emit(s, true, t + p, hard); p += 8u;
    } else if (type == 'Z' || type == 'H') {
      uint32_t e = p;
      while (e < n && t[e]) ++e;
      if (e == n) return VIEW_E_TAG_Z;
      s.put(type); s.put(':'); s.bytes(t + p, e - p); p = e + 1u;
    } else if (type == 'B') {
      if (n - p < 5u) return VIEW_E_TAG_B;
      const uint8_t sub = t[p];
      const uint32_t size = view_tag_size(sub), count = mdup_ld32(t + p + 1);
      if (!size) return VIEW_E_TAG_TYPE;
      p += 5u;
      if ((uint64_t)count * size > n - p) return VIEW_E_TAG_B;
      s.put('B'); s.put(':'); s.put(sub);
      for (uint32_t k = 0; k < count; ++k) { s.put(','); view_tag_num(s, sub, t + p + k * size, hard); }
      p += count * size;
    } else {
      const uint32_t size = view_tag_size(type);
      if (!size) return VIEW_E_TAG_TYPE;
      if (n - p < size) return VIEW_E_TAG_END;
      s.put(type == 'f' ? 'f' : 'i'); s.put(':'); view_tag_num(s, type, t + p, hard); p += size;
    }
  }
  return VIEW_E_NONE;
}

// what the size kernel leaves of a kept record for the writer: where the line's variable parts start inside the line.  The head is
// [0, cigar_at), the CIGAR [cigar_at, mid_at), RNEXT PNEXT TLEN with their tabs [mid_at, seq_at), SEQ from seq_at, a tab, QUAL, the
// tags [tags_at, len - 1), the newline.
struct ViewParts { uint32_t cigar_at, mid_at, seq_at, tags_at; };

// ---- the host path ----------------------------------------------------------------------------------------------------------------
// One record (len = 4 + block_size bytes at rec) appended to `out` as its line when it is kept.  -> VIEW_E_NONE or the refusal
inline uint32_t view_line(const uint8_t *rec, uint64_t len, const ViewRefs &F, const ViewOpts &o, std::vector<uint8_t> &out, bool *kept) {
  struct Append {
    std::vector<uint8_t> &v;
    void put(uint8_t b) { v.push_back(b); }
    void bytes(const uint8_t *s, uint32_t k) { v.insert(v.end(), s, s + k); }
    void num(uint64_t x) { char b[24]; const int k = snprintf(b, sizeof b, "%llu", (unsigned long long)x); v.insert(v.end(), b, b + k); }
  };
  ViewRec R;
  *kept = false;
  if (!view_rec(rec, len, &R)) return VIEW_E_SIZE;
  uint64_t reflen = 0;
  for (uint32_t k = 0; k < R.f.n_cigar; ++k) { const uint32_t w = mdup_ld32(rec + R.f.cigar_at + 4u * k); if (view_cigar_on_ref(w & 15u)) reflen += w >> 4; }
  if (!view_kept(R, o, reflen)) return VIEW_E_NONE;
  if (R.f.tid >= F.n_ref) return VIEW_E_RNAME;
  if (R.mtid >= F.n_ref) return VIEW_E_RNEXT;
  for (uint32_t k = 0; k < R.f.n_cigar; ++k) if ((mdup_ld32(rec + R.f.cigar_at + 4u * k) & 15u) > 8u) return VIEW_E_CIGAR;
  const size_t at = out.size();
  Append s{out};
  view_head_emit(s, rec, R, F);
  view_cigar_emit(s, rec, R);
  view_mid_emit(s, R, F);
  if (!R.f.l_seq) s.put('*');
  for (uint32_t j = 0; j < R.f.l_seq; ++j) s.put(view_base((uint32_t)(rec[R.seq_at + (j >> 1)] >> ((~j & 1u) << 2)) & 15u));
  s.put('\t');
  if (view_qual_len(rec, R) != R.f.l_seq || !R.f.l_seq) s.put('*');
  else for (uint32_t j = 0; j < R.f.l_seq; ++j) s.put(view_qual(rec[R.f.qual_at + j]));
  uint32_t hard = 0;
  const uint32_t bad = view_tags_emit(s, rec + R.tags_at, R.n_tags, &hard);
  if (bad) { out.resize(at); return bad; }
  s.put('\n');
  *kept = true;
  return VIEW_E_NONE;
}
// The rule over records back to back (each with its block_size word); the lines are appended to `out`.  ord0: the ordinal of the
// first.  -> -1, or the ordinal of the first record refused (*code says for what)
inline int64_t view_host(const uint8_t *raw, uint64_t bytes, const ViewRefs &F, const ViewOpts &o, std::vector<uint8_t> &out, ViewCounts *counts, uint64_t ord0, uint32_t *code) {
  ViewCounts C{0, 0, 0, 0};
  const size_t at0 = out.size();
  for (uint64_t q = 0; q < bytes;) {
    const int64_t ord = (int64_t)(ord0 + C.records);
    if (bytes - q < 4 || (uint64_t)mdup_ld32(raw + q) + 4u > bytes - q) { *code = VIEW_E_SIZE; out.resize(at0); return ord; }
    const uint64_t len = (uint64_t)mdup_ld32(raw + q) + 4u;
    bool kept = false;
    if ((*code = view_line(raw + q, len, F, o, out, &kept))) { out.resize(at0); return ord; }
    ++C.records;
    if (kept) ++C.written; else ++C.dropped;
    q += len;
  }
  C.text_bytes = out.size() - at0;
  if (counts) *counts = C;
  return -1;
}

}  // namespace strl
