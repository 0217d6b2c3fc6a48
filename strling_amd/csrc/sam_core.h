// sam_core.h -- the rule of `strling sort`'s SAM input: one SAM alignment line encoded as one BAM record, block_size word included
// (SAM spec 1.4, 1.5, 4.2, 4.2.4), and the SAM header as a BAM header.  One source for the kernels (samparse.hip), the host path
// (cli/sort_cli.cpp), the library's host entries (strl_sam_encode / strl_sam_header) and the stand-alone test program
// (tests/emu/sam_core_main.cpp).  DESIGN section 24.2.
//
// The field functions below are what both sides call: the host walks a line with them one field after the other
// (sam_encode_line), the kernels hand a field to a lane each and produce SEQ and QUAL with the whole group.  A refusal is a
// SamErr; the codes ascend in field order, and the host's words for one come from sam_err_words alone -- the device names only the
// line, and the host encodes that line again to say why.
#pragma once
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "bamindex_core.h"
#if defined(__HIPCC__)
#define SAM_HD __host__ __device__ inline
#else
#define SAM_HD inline
#endif

namespace strl {

constexpr uint32_t SAM_LINE_MAX = 8u << 20;      // a longer line is refused before it is parsed
constexpr uint32_t SAM_REC_MAX = 1u << 20;       // FRONT_CARRY_MAX (front.h): the largest record the rest of the sort takes
constexpr uint32_t SAM_MIN_LINE = 21;            // eleven fields of a byte each and ten tabs

enum SamErr : uint32_t {
  SAM_OK = 0, SAM_E_LONG_LINE, SAM_E_EMPTY, SAM_E_FIELDS, SAM_E_QNAME, SAM_E_FLAG, SAM_E_RNAME_FORM, SAM_E_RNAME, SAM_E_POS, SAM_E_MAPQ, SAM_E_CIGAR_OP, SAM_E_CIGAR_LEN,
  SAM_E_CIGAR_N, SAM_E_RNEXT_FORM, SAM_E_RNEXT, SAM_E_PNEXT, SAM_E_TLEN, SAM_E_SEQ, SAM_E_QUAL_NOSEQ, SAM_E_QUAL_LEN, SAM_E_QUAL_BYTE, SAM_E_TAG_FORM, SAM_E_TAG_TYPE,
  SAM_E_TAG_A, SAM_E_TAG_I, SAM_E_TAG_H, SAM_E_TAG_B, SAM_E_TAG_F, SAM_E_RECORD_BIG, SAM_E_OVERRUN, SAM_E_NONE = 0xffu
};

inline const char *sam_err_words(uint32_t e) {
  switch (e) {
    case SAM_E_LONG_LINE: return "line: more than 8388608 bytes";
    case SAM_E_EMPTY: return "line: an empty line";
    case SAM_E_FIELDS: return "line: fewer than the 11 mandatory fields";
    case SAM_E_QNAME: return "QNAME: not 1 to 254 bytes";
    case SAM_E_FLAG: return "FLAG: not a decimal number in [0, 65535]";
    case SAM_E_RNAME_FORM: return "RNAME: an empty field";
    case SAM_E_RNAME: return "RNAME: not one of the header's @SQ names";
    case SAM_E_POS: return "POS: not a decimal number in [0, 2147483647]";
    case SAM_E_MAPQ: return "MAPQ: not a decimal number in [0, 255]";
    case SAM_E_CIGAR_OP: return "CIGAR: not * or <length><operation> with an operation of MIDNSHP=X";
    case SAM_E_CIGAR_LEN: return "CIGAR: an operation's length is not below 2^28 = 268435456";
    case SAM_E_CIGAR_N: return "CIGAR: more than 65535 operations (the CG tag's convention for long CIGARs is not written)";
    case SAM_E_RNEXT_FORM: return "RNEXT: an empty field";
    case SAM_E_RNEXT: return "RNEXT: not one of the header's @SQ names";
    case SAM_E_PNEXT: return "PNEXT: not a decimal number in [0, 2147483647]";
    case SAM_E_TLEN: return "TLEN: not a signed decimal number that fits 32 bits";
    case SAM_E_SEQ: return "SEQ: an empty field";
    case SAM_E_QUAL_NOSEQ: return "QUAL: given although SEQ is *";
    case SAM_E_QUAL_LEN: return "QUAL: not as long as SEQ";
    case SAM_E_QUAL_BYTE: return "QUAL: a byte below 33";
    case SAM_E_TAG_FORM: return "tag: not TAG:TYPE:VALUE";
    case SAM_E_TAG_TYPE: return "tag: a type that is not one of AifZHB";
    case SAM_E_TAG_A: return "tag: an A value that is not one printable character";
    case SAM_E_TAG_I: return "tag: an i value that is not a decimal number in [-2147483648, 4294967295]";
    case SAM_E_TAG_H: return "tag: an H value that is not an even count of hex digits";
    case SAM_E_TAG_B: return "tag: a B array whose type is not one of cCsSiIf or with a value outside its type";
    case SAM_E_TAG_F: return "tag: an f value that is not a number";
    case SAM_E_RECORD_BIG: return "BAM record of more than 1048576 bytes";
    case SAM_E_OVERRUN: return "line: internal error: the record is longer than its computed length";
  }
  return "line: internal error";
}

// ---- the @SQ names: an open-addressing table the host builds (SamRefTable) and both sides probe -----------------------------------
struct SamRefs {
  const uint8_t *names;      // the names back to back, without NULs
  const uint32_t *off;       // [n_ref + 1]
  const int32_t *slot;       // [mask + 1]: a reference's id, -1 = empty; at least one slot is empty
  uint32_t mask;
  int32_t n_ref;
};
SAM_HD uint32_t sam_hash(const uint8_t *p, uint32_t n) {                    // FNV-1a
  uint32_t h = 2166136261u;
  for (uint32_t i = 0; i < n; ++i) h = (h ^ p[i]) * 16777619u;
  return h;
}
SAM_HD uint32_t sam_table_size(int32_t n_ref) { uint32_t s = 2; while (s < 2u * (uint32_t)n_ref) s <<= 1; return s; }
// the id of the name p[0, n), -2 = not in the header.  Bytes are compared on a hit
SAM_HD int32_t sam_ref_find(const SamRefs &R, const uint8_t *p, uint32_t n) {
  if (R.n_ref <= 0) return -2;
  uint32_t h = sam_hash(p, n) & R.mask;
  for (uint32_t trip = 0; trip <= R.mask; ++trip, h = (h + 1u) & R.mask) {
    const int32_t id = R.slot[h];
    if (id < 0 || id >= R.n_ref) return -2;
    const uint32_t a = R.off[id], l = R.off[id + 1] - a;
    if (l != n) continue;
    bool same = true;
    for (uint32_t i = 0; i < n && same; ++i) same = R.names[a + i] == p[i];
    if (same) return id;
  }
  return -2;
}
// RNAME / RNEXT -> the refID: `*` gives -1, `=` (RNEXT only) RNAME's id
SAM_HD uint32_t sam_ref_field(const SamRefs &R, const uint8_t *p, uint32_t n, bool next, int32_t rname_id, int32_t *id) {
  *id = -1;
  if (!n) return next ? SAM_E_RNEXT_FORM : SAM_E_RNAME_FORM;
  if (n == 1 && p[0] == '*') return SAM_OK;
  if (next && n == 1 && p[0] == '=') { *id = rname_id; return SAM_OK; }
  const int32_t f = sam_ref_find(R, p, n);
  if (f < 0) return next ? SAM_E_RNEXT : SAM_E_RNAME;
  *id = f;
  return SAM_OK;
}

// ---- numbers ------------------------------------------------------------------------------------------------------------------------
// decimal digits only, at least one, value <= max (max < 2^60)
SAM_HD bool sam_udec(const uint8_t *p, uint32_t n, uint64_t max, uint64_t *v) {
  if (!n) return false;
  uint64_t x = 0;
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t c = (uint32_t)p[i] - '0';
    if (c > 9u) return false;
    x = x * 10u + c;
    if (x > max) return false;
  }
  *v = x;
  return true;
}
// an optional sign and decimal digits, lo <= value <= hi (|lo|, hi < 2^60)
SAM_HD bool sam_sdec(const uint8_t *p, uint32_t n, int64_t lo, int64_t hi, int64_t *v) {
  bool neg = false;
  if (n && (p[0] == '-' || p[0] == '+')) { neg = p[0] == '-'; ++p; --n; }
  uint64_t m = 0;
  if (!sam_udec(p, n, neg ? (uint64_t)(-lo) : (uint64_t)hi, &m)) return false;
  *v = neg ? -(int64_t)m : (int64_t)m;
  return *v >= lo && *v <= hi;
}

// The exact fast path of a float: at most 15 significant digits as an integer in a double (exact: below 2^53), one multiplication or
// division by a power of ten up to 10^22 (exact in a double), so the result is the correctly rounded double -- strtod's -- and the cast
// to float follows.  false: another spelling (more digits, a larger exponent, inf, nan, anything strtod may or may not take), which
// is the host's to convert.
SAM_HD bool sam_float_fast(const uint8_t *p, uint32_t n, float *out) {
  const double p10[23] = {1e0, 1e1, 1e2, 1e3, 1e4, 1e5, 1e6, 1e7, 1e8, 1e9, 1e10, 1e11, 1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};
  uint32_t i = 0;
  bool neg = false, any = false;
  if (i < n && (p[i] == '-' || p[i] == '+')) { neg = p[i] == '-'; ++i; }
  uint64_t w = 0;
  int nd = 0, dexp = 0;
  for (; i < n && (uint32_t)p[i] - '0' <= 9u; ++i) {
    const uint32_t c = (uint32_t)p[i] - '0';
    any = true;
    if (w || c) { if (nd >= 15) return false; w = w * 10u + c; ++nd; }
  }
  if (i < n && p[i] == '.') {
    for (++i; i < n && (uint32_t)p[i] - '0' <= 9u; ++i) {
      const uint32_t c = (uint32_t)p[i] - '0';
      any = true;
      if (w || c) { if (nd >= 15) return false; w = w * 10u + c; ++nd; }
      --dexp;
      if (dexp < -4000) return false;
    }
  }
  if (!any) return false;
  if (i < n && (p[i] == 'e' || p[i] == 'E')) {
    ++i;
    bool eneg = false;
    if (i < n && (p[i] == '-' || p[i] == '+')) { eneg = p[i] == '-'; ++i; }
    if (i >= n) return false;
    int ex = 0;
    for (; i < n; ++i) {
      const uint32_t c = (uint32_t)p[i] - '0';
      if (c > 9u) return false;
      ex = ex * 10 + (int)c;
      if (ex > 4000) return false;
    }
    dexp += eneg ? -ex : ex;
  }
  if (i != n) return false;
  double d = (double)w;
  if (w) {
    if (dexp < -22 || dexp > 22) return false;
    d = dexp < 0 ? d / p10[-dexp] : d * p10[dexp];
  }
  *out = (float)(neg ? -d : d);
  return true;
}
// the rule itself: (float)strtod(text), the whole field consumed
inline bool sam_float_host(const uint8_t *p, uint32_t n, float *out) {
  if (!n || p[0] == ' ' || (p[0] >= '\t' && p[0] <= '\r')) return false;
  const std::string s(reinterpret_cast<const char *>(p), n);
  if (s.find('\0') != std::string::npos) return false;
  char *end = nullptr;
  const double d = strtod(s.c_str(), &end);
  if (end != s.c_str() + n) return false;
  *out = (float)d;
  return true;
}

// ---- CIGAR --------------------------------------------------------------------------------------------------------------------------
SAM_HD int sam_cigar_op(uint8_t c) {
  switch (c) { case 'M': return 0; case 'I': return 1; case 'D': return 2; case 'N': return 3; case 'S': return 4; case 'H': return 5; case 'P': return 6; case '=': return 7; case 'X': return 8; }
  return -1;
}
// out (null: count only): 4 bytes an operation, at most cap_ops of them written
SAM_HD uint32_t sam_cigar(const uint8_t *p, uint32_t n, uint8_t *out, uint32_t cap_ops, uint32_t *n_ops, uint64_t *reflen) {
  *n_ops = 0; *reflen = 0;
  if (n == 1 && p[0] == '*') return SAM_OK;
  if (!n) return SAM_E_CIGAR_OP;
  uint32_t k = 0;
  uint64_t ref = 0;
  for (uint32_t i = 0; i < n;) {
    uint32_t len = 0, nd = 0;
    for (; i < n && (uint32_t)p[i] - '0' <= 9u; ++i, ++nd) {
      if (len >= (1u << 28)) return SAM_E_CIGAR_LEN;
      len = len * 10u + ((uint32_t)p[i] - '0');
    }
    if (!nd || i >= n) return SAM_E_CIGAR_OP;
    const int op = sam_cigar_op(p[i++]);
    if (op < 0) return SAM_E_CIGAR_OP;
    if (len >= (1u << 28)) return SAM_E_CIGAR_LEN;
    if (k >= 65535u) return SAM_E_CIGAR_N;
    if (out && k < cap_ops) {
      const uint32_t v = len << 4 | (uint32_t)op;
      out[4 * k] = (uint8_t)v; out[4 * k + 1] = (uint8_t)(v >> 8); out[4 * k + 2] = (uint8_t)(v >> 16); out[4 * k + 3] = (uint8_t)(v >> 24);
    }
    if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) ref += len;
    ++k;
  }
  *n_ops = k; *reflen = ref;
  return SAM_OK;
}
// bin of the record at 0-based pos: end = pos + the CIGAR's reference length, pos + 1 when that is 0 or the read is unmapped
SAM_HD uint32_t sam_bin(int32_t pos, uint64_t reflen, uint32_t flag) {
  int64_t end = (int64_t)pos + ((flag & 4u) || !reflen ? 1 : (int64_t)reflen);
  if (end > 0x7fffffffll) end = 0x7fffffffll;
  return bai_reg2bin(pos, (int32_t)end) & 0xffffu;
}

// ---- SEQ and QUAL -------------------------------------------------------------------------------------------------------------------
SAM_HD uint32_t sam_seq_code(uint8_t c) {
  switch (c & 0xdfu) {        // (letters fold to upper case; '=' is 0x3d, which the fold takes to 0x1d)
    case 'A': return 1; case 'C': return 2; case 'M': return 3; case 'G': return 4; case 'R': return 5; case 'S': return 6; case 'V': return 7; case 'T': return 8;
    case 'W': return 9; case 'Y': return 10; case 'H': return 11; case 'K': return 12; case 'D': return 13; case 'B': return 14; case 0x1d: return c == '=' ? 0u : 15u;
  }
  return 15;
}

// ---- optional fields -------------------------------------------------------------------------------------------------------------------
// a writer that counts always and stores only inside [0, cap)
struct SamW {
  uint8_t *o; uint32_t cap, at; bool over;
  SAM_HD void b(uint32_t x) { if (o) { if (at < cap) o[at] = (uint8_t)x; else over = true; } ++at; }
  SAM_HD void w16(uint32_t x) { b(x); b(x >> 8); }
  SAM_HD void w32(uint32_t x) { b(x); b(x >> 8); b(x >> 16); b(x >> 24); }
};
SAM_HD bool sam_is_hex(uint8_t c) { return (uint32_t)c - '0' <= 9u || (uint32_t)(c | 0x20u) - 'a' <= 5u; }

// one float value: the fast path; where that declines, the host's strtod (HOST) or four zero bytes and *needs_host (the device)
template <bool HOST> SAM_HD uint32_t sam_put_float(const uint8_t *p, uint32_t n, SamW &W, uint32_t *needs_host) {
  float f = 0.f;
  if constexpr (HOST) {
#if !defined(__HIP_DEVICE_COMPILE__)
    if (!sam_float_host(p, n, &f)) return SAM_E_TAG_F;
#endif
  } else if (!sam_float_fast(p, n, &f)) { f = 0.f; ++*needs_host; }
  uint32_t u;
  memcpy(&u, &f, 4);
  W.w32(u);
  return SAM_OK;
}

// the optional fields p[0, n) (tab-separated, behind the eleventh tab) as BAM aux data: out null = size only.  *bytes = what they take
// (whatever cap is); SAM_E_OVERRUN when out is given and they do not fit cap.  HOST: floats by strtod, nothing left to finish.
template <bool HOST> SAM_HD uint32_t sam_tags(const uint8_t *p, uint32_t n, uint8_t *out, uint32_t cap, uint32_t *bytes, uint32_t *needs_host) {
  SamW W{out, cap, 0, false};
  *needs_host = 0;
  uint32_t i = 0;
  while (i <= n) {
    uint32_t e = i;
    while (e < n && p[e] != '\t') ++e;
    const uint8_t *f = p + i;
    const uint32_t l = e - i;
    if (l < 5 || f[2] != ':' || f[4] != ':') return SAM_E_TAG_FORM;
    const uint8_t ty = f[3];
    const uint8_t *v = f + 5;
    const uint32_t vl = l - 5;
    W.b(f[0]); W.b(f[1]);
    if (ty == 'A') {
      if (vl != 1 || v[0] < 33 || v[0] > 126) return SAM_E_TAG_A;
      W.b('A'); W.b(v[0]);
    } else if (ty == 'i') {
      int64_t x;
      if (!sam_sdec(v, vl, -2147483648ll, 4294967295ll, &x)) return SAM_E_TAG_I;
      if (x < 0) {
        if (x >= -128) { W.b('c'); W.b((uint32_t)x); }
        else if (x >= -32768) { W.b('s'); W.w16((uint32_t)x); }
        else { W.b('i'); W.w32((uint32_t)x); }
      } else {
        if (x <= 255) { W.b('C'); W.b((uint32_t)x); }
        else if (x <= 65535) { W.b('S'); W.w16((uint32_t)x); }
        else { W.b('I'); W.w32((uint32_t)x); }
      }
    } else if (ty == 'f') {
      W.b('f');
      const uint32_t er = sam_put_float<HOST>(v, vl, W, needs_host);
      if (er) return er;
    } else if (ty == 'Z') {
      W.b('Z');
      for (uint32_t k = 0; k < vl; ++k) W.b(v[k]);
      W.b(0);
    } else if (ty == 'H') {
      if (vl & 1u) return SAM_E_TAG_H;
      for (uint32_t k = 0; k < vl; ++k) if (!sam_is_hex(v[k])) return SAM_E_TAG_H;
      W.b('H');
      for (uint32_t k = 0; k < vl; ++k) W.b(v[k]);
      W.b(0);
    } else if (ty == 'B') {
      if (!vl) return SAM_E_TAG_B;
      const uint8_t st = v[0];
      int64_t lo = 0, hi = 0;
      uint32_t sz = 0;
      switch (st) {
        case 'c': lo = -128; hi = 127; sz = 1; break;
        case 'C': lo = 0; hi = 255; sz = 1; break;
        case 's': lo = -32768; hi = 32767; sz = 2; break;
        case 'S': lo = 0; hi = 65535; sz = 2; break;
        case 'i': lo = -2147483648ll; hi = 2147483647ll; sz = 4; break;
        case 'I': lo = 0; hi = 4294967295ll; sz = 4; break;
        case 'f': sz = 4; break;
        default: return SAM_E_TAG_B;
      }
      uint32_t count = 0;
      for (uint32_t k = 1; k < vl; ++k) count += v[k] == ',';
      if (vl > 1 && v[1] != ',') return SAM_E_TAG_B;
      W.b('B'); W.b(st); W.w32(count);
      for (uint32_t k = 1; k < vl;) {         // v[k] == ','
        uint32_t q = k + 1;
        while (q < vl && v[q] != ',') ++q;
        if (st == 'f') {
          const uint32_t er = sam_put_float<HOST>(v + k + 1, q - k - 1, W, needs_host);
          if (er) return er;
        } else {
          int64_t x;
          if (!sam_sdec(v + k + 1, q - k - 1, lo, hi, &x)) return SAM_E_TAG_B;
          if (sz == 1) W.b((uint32_t)x); else if (sz == 2) W.w16((uint32_t)x); else W.w32((uint32_t)x);
        }
        k = q;
      }
    } else return SAM_E_TAG_TYPE;
    i = e + 1;
    if (e >= n) break;
  }
  *bytes = W.at;
  return W.over ? (uint32_t)SAM_E_OVERRUN : (uint32_t)SAM_OK;
}

// ---- a line's plan: where its fields lie and what its record holds ------------------------------------------------------------------------
// field k = [k ? tab[k - 1] + 1 : 0, tab[k]) for k < 11; tab[10] = the eleventh tab, or the line's end when it has no optional field
struct SamPlan {
  uint32_t tab[11];
  int32_t tid, pos, mtid, mpos, tlen;
  uint32_t flag, mapq, l_qname, n_cig, l_seq, tag_bytes, needs_host, bin;
  uint32_t rec_len;        // block_size word included
};
SAM_HD uint32_t sam_field_beg(const uint32_t *tab, int k) { return k ? tab[k - 1] + 1u : 0u; }
// the record's length from its parts; 0 = more than SAM_REC_MAX
SAM_HD uint32_t sam_rec_len(uint32_t l_qname, uint32_t n_cig, uint32_t l_seq, uint32_t tag_bytes) {
  const uint64_t v = 36ull + l_qname + 1u + 4ull * n_cig + (l_seq + 1u) / 2u + l_seq + tag_bytes;
  return v > SAM_REC_MAX ? 0u : (uint32_t)v;
}
// the line's length without a \r directly before its end
SAM_HD uint32_t sam_strip_cr(const uint8_t *line, uint32_t len) { return len && line[len - 1] == '\r' ? len - 1 : len; }

// one line walked field by field (len: without \n and \r).  HOST as sam_tags
template <bool HOST> SAM_HD uint32_t sam_plan_line(const uint8_t *line, uint32_t len, const SamRefs &R, SamPlan &P) {
  if (len > SAM_LINE_MAX) return SAM_E_LONG_LINE;
  if (!len) return SAM_E_EMPTY;
  uint32_t nt = 0;
  for (uint32_t i = 0; i < len && nt < 11; ++i) if (line[i] == '\t') P.tab[nt++] = i;
  if (nt < 10) return SAM_E_FIELDS;
  if (nt == 10) P.tab[10] = len;
  const uint32_t *t = P.tab;
  uint64_t u;
  int64_t s;
  uint32_t er;
  P.l_qname = t[0];
  if (P.l_qname < 1 || P.l_qname > 254) return SAM_E_QNAME;
  if (!sam_udec(line + t[0] + 1, t[1] - t[0] - 1, 65535, &u)) return SAM_E_FLAG;
  P.flag = (uint32_t)u;
  if ((er = sam_ref_field(R, line + t[1] + 1, t[2] - t[1] - 1, false, -1, &P.tid))) return er;
  if (!sam_udec(line + t[2] + 1, t[3] - t[2] - 1, 2147483647, &u)) return SAM_E_POS;
  P.pos = (int32_t)u - 1;
  if (!sam_udec(line + t[3] + 1, t[4] - t[3] - 1, 255, &u)) return SAM_E_MAPQ;
  P.mapq = (uint32_t)u;
  uint64_t reflen;
  if ((er = sam_cigar(line + t[4] + 1, t[5] - t[4] - 1, nullptr, 0, &P.n_cig, &reflen))) return er;
  if ((er = sam_ref_field(R, line + t[5] + 1, t[6] - t[5] - 1, true, P.tid, &P.mtid))) return er;
  if (!sam_udec(line + t[6] + 1, t[7] - t[6] - 1, 2147483647, &u)) return SAM_E_PNEXT;
  P.mpos = (int32_t)u - 1;
  if (!sam_sdec(line + t[7] + 1, t[8] - t[7] - 1, -2147483648ll, 2147483647ll, &s)) return SAM_E_TLEN;
  P.tlen = (int32_t)s;
  const uint8_t *seq = line + t[8] + 1, *qual = line + t[9] + 1;
  const uint32_t ls = t[9] - t[8] - 1, lq = t[10] - t[9] - 1;
  if (!ls) return SAM_E_SEQ;
  P.l_seq = ls == 1 && seq[0] == '*' ? 0u : ls;
  if (!(lq == 1 && qual[0] == '*')) {
    if (!P.l_seq) return SAM_E_QUAL_NOSEQ;
    if (lq != P.l_seq) return SAM_E_QUAL_LEN;
    for (uint32_t i = 0; i < lq; ++i) if (qual[i] < 33) return SAM_E_QUAL_BYTE;
  }
  P.tag_bytes = 0; P.needs_host = 0;
  if (t[10] < len && (er = sam_tags<HOST>(line + t[10] + 1, len - t[10] - 1, nullptr, 0, &P.tag_bytes, &P.needs_host))) return er;
  P.bin = sam_bin(P.pos, reflen, P.flag);
  P.rec_len = sam_rec_len(P.l_qname, P.n_cig, P.l_seq, P.tag_bytes);
  return P.rec_len ? (uint32_t)SAM_OK : (uint32_t)SAM_E_RECORD_BIG;
}

// the 36 fixed bytes of the record
SAM_HD void sam_put_fixed(uint8_t *o, const SamPlan &P) {
  const uint32_t w[9] = {P.rec_len - 4u, (uint32_t)P.tid, (uint32_t)P.pos, (P.l_qname + 1u) | P.mapq << 8 | P.bin << 16, P.n_cig | P.flag << 16, P.l_seq, (uint32_t)P.mtid,
                         (uint32_t)P.mpos, (uint32_t)P.tlen};
  for (int k = 0; k < 9; ++k) { o[4 * k] = (uint8_t)w[k]; o[4 * k + 1] = (uint8_t)(w[k] >> 8); o[4 * k + 2] = (uint8_t)(w[k] >> 16); o[4 * k + 3] = (uint8_t)(w[k] >> 24); }
}

// ---- the host's encoder: the rule in one walk -------------------------------------------------------------------------------------------
// the record of line[0, len) (no \n; a trailing \r is dropped) appended to `out`.  A refusal leaves `out` as it was and says why:
// "FIELD: words", the name looked for added where one is missing from the header
inline uint32_t sam_encode_line(const uint8_t *line, uint32_t len, const SamRefs &R, std::vector<uint8_t> &out, std::string &why) {
  len = sam_strip_cr(line, len);
  SamPlan P;
  uint32_t er = sam_plan_line<true>(line, len, R, P);
  const size_t base = out.size();
  if (!er) {
    out.resize(base + P.rec_len);
    uint8_t *o = out.data() + base;
    const uint32_t *t = P.tab;
    sam_put_fixed(o, P);
    uint32_t at = 36;
    memcpy(o + at, line, P.l_qname); o[at + P.l_qname] = 0;
    at += P.l_qname + 1;
    uint32_t nc; uint64_t rl;
    sam_cigar(line + t[4] + 1, t[5] - t[4] - 1, o + at, P.n_cig, &nc, &rl);
    at += 4 * P.n_cig;
    const uint8_t *seq = line + t[8] + 1, *qual = line + t[9] + 1;
    for (uint32_t i = 0; i < P.l_seq; i += 2) o[at + i / 2] = (uint8_t)(sam_seq_code(seq[i]) << 4 | (i + 1 < P.l_seq ? sam_seq_code(seq[i + 1]) : 0u));
    at += (P.l_seq + 1) / 2;
    if (t[10] - t[9] - 1 == 1 && qual[0] == '*') memset(o + at, 0xff, P.l_seq);
    else for (uint32_t i = 0; i < P.l_seq; ++i) o[at + i] = (uint8_t)(qual[i] - 33);
    at += P.l_seq;
    if (t[10] < len) {
      uint32_t nb = 0, nh = 0;
      er = sam_tags<true>(line + t[10] + 1, len - t[10] - 1, o + at, P.rec_len - at, &nb, &nh);
      at += nb;
    }
    if (!er && at != P.rec_len) er = SAM_E_OVERRUN;
    if (er) out.resize(base);
  }
  if (er) {
    why = sam_err_words(er);
    if (er == SAM_E_RNAME || er == SAM_E_RNEXT) {
      const int k = er == SAM_E_RNAME ? 2 : 6;
      const uint32_t b = sam_field_beg(P.tab, k);
      why += ": " + std::string(reinterpret_cast<const char *>(line + b), std::min<uint32_t>(P.tab[k] - b, 200));
    }
  }
  return er;
}
inline std::string sam_refusal(uint64_t line_number, const std::string &why) { return "SAM line " + std::to_string(line_number) + ": " + why; }

// the table over the @SQ names, and the view both sides probe
struct SamRefTable {
  std::vector<uint8_t> names;
  std::vector<uint32_t> off{0};
  std::vector<int32_t> slot;
  int32_t n_ref = 0;
  // false: a name occurs twice (*dup = the second one's id)
  bool build(const uint8_t *nm, const uint32_t *name_off, int32_t n, int32_t *dup) {
    n_ref = n;
    names.assign(nm, nm + (n ? name_off[n] - name_off[0] : 0));
    off.resize((size_t)n + 1);
    for (int32_t t = 0; t <= n; ++t) off[t] = name_off[t] - name_off[0];
    const uint32_t size = sam_table_size(n);
    slot.assign(size, -1);
    for (int32_t t = 0; t < n; ++t) {
      const uint32_t l = off[t + 1] - off[t];
      uint32_t h = sam_hash(names.data() + off[t], l) & (size - 1);
      for (; slot[h] >= 0; h = (h + 1) & (size - 1)) {
        const int32_t o = slot[h];
        if (off[o + 1] - off[o] == l && !memcmp(names.data() + off[o], names.data() + off[t], l)) { if (dup) *dup = t; return false; }
      }
      slot[h] = t;
    }
    return true;
  }
  SamRefs view() const { return SamRefs{names.data(), off.data(), slot.data(), (uint32_t)slot.size() - 1u, n_ref}; }
};

// ---- the header ---------------------------------------------------------------------------------------------------------------------
// The leading @ lines of text[0, len) are the BAM header's text, byte for byte; the @SQ lines give the reference list in order.
// -> the BAM header (magic, l_text, text, n_ref, the list) in `out`, *used = bytes of the @ lines.  The text must hold the whole
// header: its end is the first line that does not begin with @, or the end of the text.
struct SamHeader {
  std::vector<uint8_t> bam;        // the BAM header as the input's would be: bsort_header makes the output's from it
  std::vector<uint8_t> names;
  std::vector<uint32_t> name_off{0};
  std::vector<int32_t> l_ref;
  size_t used = 0;
};
inline bool sam_header(const uint8_t *text, size_t len, SamHeader &H, std::string &err) {
  H = SamHeader{};
  size_t at = 0;
  while (at < len && text[at] == '@') {
    const uint8_t *nl = static_cast<const uint8_t *>(memchr(text + at, '\n', len - at));
    const size_t end = nl ? (size_t)(nl - text) : len;
    size_t e = end;
    if (e > at && text[e - 1] == '\r') --e;
    if (e - at >= 4 && !memcmp(text + at, "@SQ\t", 4)) {
      const uint8_t *sn = nullptr, *ln = nullptr;
      size_t sn_l = 0, ln_l = 0;
      for (size_t f = at + 4; f <= e;) {
        size_t g = f;
        while (g < e && text[g] != '\t') ++g;
        if (g - f >= 3 && !memcmp(text + f, "SN:", 3) && !sn) { sn = text + f + 3; sn_l = g - f - 3; }
        if (g - f >= 3 && !memcmp(text + f, "LN:", 3) && !ln) { ln = text + f + 3; ln_l = g - f - 3; }
        f = g + 1;
      }
      const std::string nth = "@SQ line " + std::to_string(H.l_ref.size() + 1);
      uint64_t l = 0;
      if (!sn || !sn_l) { err = "SAM header: " + nth + " has no SN"; return false; }
      if (!ln || !sam_udec(ln, (uint32_t)std::min<size_t>(ln_l, 32), 2147483647, &l) || !l) { err = "SAM header: " + nth + ": LN is missing or not in [1, 2147483647]"; return false; }
      H.names.insert(H.names.end(), sn, sn + sn_l);
      H.name_off.push_back((uint32_t)H.names.size());
      H.l_ref.push_back((int32_t)l);
    }
    at = nl ? end + 1 : len;
  }
  H.used = at;
  const int32_t n = (int32_t)H.l_ref.size();
  SamRefTable T;
  int32_t dup = 0;
  if (!T.build(H.names.data(), H.name_off.data(), n, &dup)) {
    err = "SAM header: the SN " + std::string(reinterpret_cast<const char *>(H.names.data() + H.name_off[dup]), H.name_off[dup + 1] - H.name_off[dup]) + " occurs twice";
    return false;
  }
  if (at > 0x7fffffffu) { err = "SAM header: text of more than 2^31 bytes"; return false; }
  auto w32 = [&](uint32_t v) { for (int k = 0; k < 4; ++k) H.bam.push_back((uint8_t)(v >> (8 * k))); };
  H.bam.insert(H.bam.end(), {'B', 'A', 'M', 1});
  w32((uint32_t)at);
  H.bam.insert(H.bam.end(), text, text + at);
  w32((uint32_t)n);
  for (int32_t t = 0; t < n; ++t) {
    const uint32_t a = H.name_off[t], l = H.name_off[t + 1] - a;
    w32(l + 1);
    H.bam.insert(H.bam.end(), H.names.begin() + a, H.names.begin() + a + l);
    H.bam.push_back(0);
    w32((uint32_t)H.l_ref[t]);
  }
  return true;
}

}  // namespace strl
