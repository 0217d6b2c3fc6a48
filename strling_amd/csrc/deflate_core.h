// deflate_core.h -- the per-block rule of the BGZF compressor (deflate.hip): up to 0xFF00 input bytes in, ONE complete BGZF
// member out -- the 18-byte header with BSIZE, one final DEFLATE block (RFC 1951), CRC-32, ISIZE.  Every block stands alone: no
// match reaches into another block's bytes and no table survives from one block to the next.
//   dfl_block          the whole rule, written once for a TEAM of threads: on the device the team is a workgroup of 256
//                      (deflate.hip: DflWork in LDS), on the host it is one thread (DflSerial) whose loops take the lanes' places
//   dfl_code_lengths   code lengths from a histogram, limited to 15 / 7 bits, with the one tie-breaking rule
//   dfl_deflate_host   (host) the members of a whole buffer back to back: strl_bgzf_deflate_host
// Why host and device write the same bytes, whatever the order lanes and workgroups run in:
//   - positions are taken in batches of 256.  Every position of a batch looks its 4-byte hash up BEFORE any position of the
//     batch is inserted (a team barrier lies between), so a position only ever sees candidates of earlier batches;
//   - an insert is an integer max (the largest position wins): the table after a batch does not depend on the order;
//   - the greedy parse, the histograms, the code lengths and the header are made by ONE lane, in position order;
//   - a token's bits are OR-ed into a zeroed buffer at an offset that follows from a prefix sum: OR commutes;
//   - the CRC-32 is linear over GF(2) (bgzf.hip has the argument): slices may be dealt to the lanes in any way.
// The DEFLATE block is dynamic Huffman (BTYPE=10) with the run-length symbols 16 to 18 in its header; when that form would be no
// smaller than the stored one (BTYPE=00: 5 + n bytes) the block is stored.  Either way a member is at most n + 31 bytes.
// Two match rules share everything behind the tokens: DflFast (the text above: one candidate, a batch old, greedy) and DflDense
// (chains of depth 16 in a window of 16128 with a one-step lazy parse; DESIGN.md 23.1, stated at the struct below).
// The same source compiles for the host without HIP (tests/emu/deflate_emu.cpp, tests/emu/deflate_cases_main.cpp: a
// stand-alone program under AddressSanitizer and UBSan).  No wave intrinsics for that reason.
#pragma once
#include <stdint.h>
#include <string.h>
#include <memory>
#include <vector>
#include "../../include/strling_amd.h"

#if defined(__HIPCC__) && !defined(STRL_EMU)
#define DFL_FN __host__ __device__ inline
#else
#define DFL_FN inline
#endif

namespace strl {

constexpr uint32_t DFL_MAX_BLOCK = 0xFF00;       // input bytes of a member
constexpr uint32_t DFL_MEMBER_EXTRA = 18 + 5 + 8;   // header, the stored form's 5 bytes, CRC-32 and ISIZE: a member is <= n + 31 bytes
constexpr uint32_t DFL_BATCH = 256;              // positions that look up before any of them inserts
constexpr uint32_t DFL_HASH_BITS = 13;
constexpr uint32_t DFL_MIN_MATCH = 4, DFL_MAX_MATCH = 258, DFL_MAX_DIST = 32768;
constexpr uint32_t DFL_NLIT = 286, DFL_NDIST = 30, DFL_NCL = 19;
constexpr uint32_t DFL_BUF_WORDS = 65536 / 4;

// tables of the CRC-32 (zlib's polynomial, reflected): the byte table, and the operator of 2^k zero bytes, one column per state bit
struct DflCrc {
  uint32_t tab[256];
  uint32_t zop[17][32];
};
inline void dfl_crc_make(DflCrc &T) {
  for (uint32_t i = 0; i < 256; ++i) {
    uint32_t c = i;
    for (int k = 0; k < 8; ++k) c = (c & 1u) ? 0xedb88320u ^ (c >> 1) : c >> 1;
    T.tab[i] = c;
  }
  for (int b = 0; b < 32; ++b) { const uint32_t v = 1u << b; T.zop[0][b] = T.tab[v & 0xffu] ^ (v >> 8); }
  for (int k = 1; k < 17; ++k)
    for (int b = 0; b < 32; ++b) {
      const uint32_t v = T.zop[k - 1][b];
      uint32_t r = 0;
      for (int j = 0; j < 32; ++j) if ((v >> j) & 1u) r ^= T.zop[k - 1][j];
      T.zop[k][b] = r;
    }
}

// Everything a team needs for one block (the device keeps it in LDS: ~107 KB of the CU's 160 KB with DflFast's tables, ~125 KB
// with DflDense's)
template <class Rule>
struct DflWorkT {
  uint32_t buf[DFL_BUF_WORDS];          // the block's bytes; after the parse, the bits of the dynamic form
  typename Rule::Search s;              // the match rule's tables
  uint32_t part[DFL_BATCH];             // per-lane sums of the emit pass
  uint32_t lit_hist[288], dist_hist[32], cl_hist[20];
  uint16_t lit_code[288], dist_code[32], cl_code[20];      // bit-reversed: ready to be OR-ed in
  uint8_t lit_len[288], dist_len[32], cl_len[20];
  uint16_t cl_sym[DFL_NLIT + DFL_NDIST + 4];               // the header's code-length symbols: symbol | extra value << 8
  // dfl_code_lengths: used symbols by ascending (count, symbol); weights of the inner nodes; parents; depths
  uint16_t order[288], hpl[288], hpi[288], hdep[288];
  uint32_t hw[288], cnt[16];
  DflCrc crc;
  uint32_t ntok, n_cl, hlit, hdist, hclen, header_bits, total_bits, crc_acc, dynamic;
};
struct DflFast;
struct DflDense;
using DflWork = DflWorkT<DflFast>;

// a team of one: the host twin.  (deflate.hip has the workgroup.)
struct DflSerial {
  static constexpr uint32_t N = 1;
  static constexpr bool IN_ORDER = true;       // its loops visit a batch's positions in ascending order
  DFL_FN uint32_t tid() const { return 0; }
  DFL_FN void sync() const {}
  DFL_FN void max_u32(uint32_t *p, uint32_t v) const { if (*p < v) *p = v; }
  DFL_FN void or_u32(uint32_t *p, uint32_t v) const { *p |= v; }
  DFL_FN void xor_u32(uint32_t *p, uint32_t v) const { *p ^= v; }
};

DFL_FN uint32_t dfl_ld32(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
DFL_FN uint32_t dfl_hash(const uint8_t *p) { return (dfl_ld32(p) * 2654435761u) >> (32 - DFL_HASH_BITS); }
DFL_FN uint32_t dfl_log2(uint32_t v) { return 31u - (uint32_t)__builtin_clz(v); }   // v != 0
// RFC 1951 3.2.5: symbol, number of extra bits and their value of a match length (l = length - 3) and of a distance (d = distance - 1)
DFL_FN void dfl_len_sym(uint32_t l, uint32_t &sym, uint32_t &eb, uint32_t &ev) {
  if (l < 8u) { sym = 257u + l; eb = 0; ev = 0; return; }
  if (l >= 255u) { sym = 285u; eb = 0; ev = 0; return; }
  eb = dfl_log2(l) - 2u;
  sym = 261u + 4u * eb + ((l >> eb) & 3u);
  ev = l & ((1u << eb) - 1u);
}
DFL_FN void dfl_dist_sym(uint32_t d, uint32_t &sym, uint32_t &eb, uint32_t &ev) {
  if (d < 4u) { sym = d; eb = 0; ev = 0; return; }
  const uint32_t k = dfl_log2(d);
  eb = k - 1u;
  sym = 2u * k + ((d >> eb) & 1u);
  ev = d & ((1u << eb) - 1u);
}
DFL_FN uint32_t dfl_len_extra(uint32_t sym) { return sym < 265u || sym >= 285u ? 0u : (sym - 261u) >> 2; }
DFL_FN uint32_t dfl_dist_extra(uint32_t sym) { return sym < 4u ? 0u : (sym >> 1) - 1u; }
DFL_FN uint32_t dfl_rev(uint32_t code, uint32_t len) {
  uint32_t r = 0;
  for (uint32_t i = 0; i < len; ++i) r |= ((code >> i) & 1u) << (len - 1u - i);
  return r;
}
DFL_FN uint32_t dfl_crc_zeros(const DflCrc &C, uint32_t v, uint32_t n_bytes) {
  for (int k = 0; k < 17 && v; ++k) {
    if (n_bytes & (1u << k)) {
      uint32_t r = 0;
      for (int b = 0; b < 32; ++b) r ^= (v >> b) & 1u ? C.zop[k][b] : 0u;
      v = r;
    }
  }
  return v;
}
// nbits <= 32 bits of v at bit `at` of the zeroed buffer (DEFLATE fills bytes from the least significant bit: a little-endian word does the same)
template <class Team>
DFL_FN void dfl_put(const Team &T, uint32_t *buf, uint32_t at, uint32_t v, uint32_t nbits) {
  if (!nbits) return;
  const uint32_t w = at >> 5, sh = at & 31u;
  const uint64_t x = (uint64_t)v << sh;
  if (w < DFL_BUF_WORDS) T.or_u32(buf + w, (uint32_t)x);
  if ((x >> 32) && w + 1u < DFL_BUF_WORDS) T.or_u32(buf + w + 1u, (uint32_t)(x >> 32));
}

// Code lengths of the symbols with hist[s] != 0, none longer than `limit`; len[s] = 0 for the others.
//   no symbol: all zero.  one symbol: one code of one bit (RFC 1951 3.2.7).  otherwise a complete code (Kraft sum 1).
// The rule, and its ties: the used symbols are ordered by ascending (count, symbol).  A Huffman tree is made from two queues,
// the leaves in that order and the inner nodes in the order they are made; of a leaf and an inner node of equal weight the LEAF
// is taken.  Depths beyond the limit are set to the limit, then, while the code is over-subscribed, one code of the limit's
// length is taken away and the longest shorter code is made one bit longer with a sibling beside it (the Kraft sum falls by
// 2^-limit each time, the number of codes stays).  The lengths, longest first, go to the symbols in the order above.
// The team must have made hist[] visible (a sync) before the call; len[] is visible to all after it.
template <class Team, class Work>
DFL_FN void dfl_code_lengths(const Team &T, Work &W, const uint32_t *hist, uint32_t nsym, uint32_t limit, uint8_t *len) {
  const uint32_t tid = T.tid();
  if (nsym > 288u) nsym = 288u;
  for (uint32_t s = tid; s < nsym; s += Team::N) {
    len[s] = 0;
    const uint32_t f = hist[s];
    if (!f) continue;
    uint32_t r = 0;
    for (uint32_t j = 0; j < nsym; ++j) {
      const uint32_t g = hist[j];
      r += (g != 0u && (g < f || (g == f && j < s))) ? 1u : 0u;
    }
    W.order[r] = (uint16_t)s;          // r < the number of used symbols <= nsym
  }
  T.sync();
  if (tid == 0) {
    uint32_t m = 0;
    for (uint32_t s = 0; s < nsym; ++s) m += hist[s] != 0u;
    if (m == 1u) len[W.order[0]] = 1;
    if (m >= 2u) {
      uint32_t li = 0, ii = 0;
      for (uint32_t k = 0; k + 1u < m; ++k) {
        uint32_t sum = 0;
        for (int pick = 0; pick < 2; ++pick) {
          const bool leaf = li < m && (ii >= k || hist[W.order[li]] <= W.hw[ii]);
          if (leaf) { sum += hist[W.order[li]]; W.hpl[li++] = (uint16_t)k; }
          else { sum += W.hw[ii]; W.hpi[ii++] = (uint16_t)k; }
        }
        W.hw[k] = sum;
      }
      W.hdep[m - 2u] = 0;
      for (uint32_t k = m - 2u; k-- > 0u;) W.hdep[k] = (uint16_t)(W.hdep[W.hpi[k]] + 1u);
      for (uint32_t l = 0; l < 16u; ++l) W.cnt[l] = 0;
      for (uint32_t i = 0; i < m; ++i) {
        const uint32_t d = W.hdep[W.hpl[i]] + 1u;
        W.cnt[d < limit ? d : limit]++;
      }
      uint32_t total = 0;
      for (uint32_t l = 1; l <= limit; ++l) total += W.cnt[l] << (limit - l);
      for (uint32_t guard = 0; total > (1u << limit) && guard < 65536u; ++guard) {
        W.cnt[limit]--;
        for (uint32_t l = limit - 1u; l >= 1u; --l)
          if (W.cnt[l]) { W.cnt[l]--; W.cnt[l + 1u] += 2u; break; }
        total--;
      }
      uint32_t idx = 0;
      for (uint32_t l = limit; l >= 1u; --l)
        for (uint32_t c = 0; c < W.cnt[l] && idx < m; ++c) len[W.order[idx++]] = (uint8_t)l;
    }
  }
  T.sync();
}

// canonical codes (RFC 1951 3.2.2) of len[0, nsym), bit-reversed; one lane
DFL_FN void dfl_codes(const uint8_t *len, uint32_t nsym, uint16_t *code) {
  uint32_t next[17], cnt[17];
  for (int l = 0; l < 17; ++l) cnt[l] = 0;
  for (uint32_t s = 0; s < nsym; ++s) cnt[len[s] & 15u]++;
  cnt[0] = 0;
  uint32_t c = 0;
  next[0] = 0;
  for (int l = 1; l <= 15; ++l) { c = (c + cnt[l - 1]) << 1; next[l] = c; }
  for (uint32_t s = 0; s < nsym; ++s) {
    const uint32_t l = len[s] & 15u;
    code[s] = l ? (uint16_t)dfl_rev(next[l]++, l) : (uint16_t)0;
  }
}

DFL_FN uint32_t dfl_cl_order(uint32_t i) {
  const uint8_t o[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
  return o[i < 19u ? i : 18u];
}

// One token of lane 0's parse at `pos`, c = length << 16 | distance of the match taken there or 0 for the literal b[pos]:
// counted in the histograms, written to tok[nt] (nt < n); returns the input bytes it covers.
template <class Work>
DFL_FN uint32_t dfl_token(Work &W, const uint8_t *b, uint32_t pos, uint32_t c, uint32_t *tok, uint32_t nt, uint32_t n) {
  uint32_t t, step;
  if (c) {
    const uint32_t l = (c >> 16) - 3u, d = (c & 0xffffu) - 1u;
    uint32_t sym, eb, ev;
    dfl_len_sym(l, sym, eb, ev);
    W.lit_hist[sym < 288u ? sym : 287u]++;
    dfl_dist_sym(d, sym, eb, ev);
    W.dist_hist[sym & 31u]++;
    t = 0x80000000u | l << 16 | d;
    step = c >> 16;
  } else {
    t = b[pos];
    W.lit_hist[t]++;
    step = 1u;
  }
  if (nt < n) tok[nt] = t;
  return step;
}

// The fast rule: the tokens of b[0, n) from one candidate per position, at least a batch old, parsed greedily (the text at the
// top of this file).  tokens() leaves them in tok[0, W.ntok) and their counts in the histograms; every lane makes the call.
struct DflFast {
  struct Search {
    uint32_t tab[1u << DFL_HASH_BITS];    // hash of 4 bytes -> 1 + the largest inserted position with it (0: none)
    uint32_t cand[DFL_BATCH];             // the batch's candidates: length << 16 | distance, 0 = no match
  };
  template <class Team>
  static DFL_FN void reset(const Team &T, Search &S) {
    for (uint32_t i = T.tid(); i < (1u << DFL_HASH_BITS); i += Team::N) S.tab[i] = 0;
  }
  template <class Team, class Work>
  static DFL_FN void tokens(const Team &T, Work &W, const uint8_t *b, uint32_t n, uint32_t *tok) {
    const uint32_t tid = T.tid();
    Search &S = W.s;
    uint32_t pos = 0, nt = 0;             // lane 0's: where the last token ends, tokens so far
    for (uint32_t base = 0; base < n; base += DFL_BATCH) {
      for (uint32_t t = tid; t < DFL_BATCH; t += Team::N) {
        const uint32_t p = base + t;
        uint32_t c = 0;
        if (p + DFL_MIN_MATCH <= n) {
          const uint32_t e = S.tab[dfl_hash(b + p)];
          if (e && e <= base && p - (e - 1u) <= DFL_MAX_DIST) {     // (e - 1 < base: only earlier batches have been inserted)
            const uint32_t q = e - 1u, maxl = n - p < DFL_MAX_MATCH ? n - p : DFL_MAX_MATCH;
            uint32_t l = 0;
            while (l < maxl && b[q + l] == b[p + l]) ++l;
            if (l >= DFL_MIN_MATCH) c = l << 16 | (p - q);
          }
        }
        S.cand[t] = c;
      }
      T.sync();
      for (uint32_t t = tid; t < DFL_BATCH; t += Team::N) {
        const uint32_t p = base + t;
        if (p + DFL_MIN_MATCH <= n) T.max_u32(&S.tab[dfl_hash(b + p)], p + 1u);
      }
      if (tid == 0) {
        const uint32_t end = base + DFL_BATCH < n ? base + DFL_BATCH : n;
        while (pos < end) {
          pos += dfl_token(W, b, pos, S.cand[pos - base], tok, nt, n);
          ++nt;
        }
      }
      T.sync();
    }
    if (tid == 0) W.ntok = nt < n ? nt : n;
  }
};

// The dense rule, a function of the block's bytes alone:
//   chain(p)  the positions q < p with hash4(q) == hash4(p) and p - q <= WINDOW, nearest first; its first DEPTH entries are
//             looked at, those whose bytes differ (the hash is 12 bits of four bytes) among them;
//   match(p)  the longest common prefix with one of them, at most 258 bytes and the block's end, the nearest of equal lengths;
//             below 4 bytes, and where fewer than four bytes are left, none.  Source and copy may overlap;
//   parse     in position order: where match(pos + 1) is strictly longer than match(pos), the literal b[pos]; else the match.
// How it is kept: head[h] is 1 + the largest inserted position with hash h, ring[q % RING] is 1 + the nearest position before q
// with q's hash: q's link, written when q is inserted.  A batch of 256 positions is inserted at a time, so the slot of q is
// written again by q + RING at the earliest when the batch of q + RING is inserted: no position of that batch is within
// WINDOW = RING - 256 of q.  Every slot a walk may follow is therefore the link of the position it is followed from.
// A walk takes at most DEPTH steps, each to a strictly smaller position within WINDOW, else it ends: whatever a slot holds.
struct DflDense {
  static constexpr uint32_t HASH_BITS = 12, DEPTH = 16, RING = 16384, WINDOW = RING - DFL_BATCH;
  struct Search {
    uint32_t head[1u << HASH_BITS];
    uint16_t ring[RING];
    uint32_t cand[2u * DFL_BATCH];        // match(p) at p % 512, length << 16 | distance, 0 = none: this batch's and the one before
    uint16_t hb[DFL_BATCH];               // the batch's hashes; NO_HASH where fewer than four bytes are left
  };
  static constexpr uint32_t NO_HASH = 0xffffu;
  static DFL_FN uint32_t hash(const uint8_t *p) { return (dfl_ld32(p) * 2654435761u) >> (32 - HASH_BITS); }
  static DFL_FN uint32_t ld32u(const uint8_t *p) { uint32_t v; memcpy(&v, p, 4); return v; }      // (both sides little-endian)
  // the common prefix of b + q and b + p, at most maxl bytes; four bytes at a time (reads stay below p + maxl + 3 < 65536)
  static DFL_FN uint32_t prefix(const uint8_t *b, uint32_t q, uint32_t p, uint32_t maxl) {
    uint32_t l = 0;
    while (l + 4u <= maxl) {
      const uint32_t x = ld32u(b + q + l) ^ ld32u(b + p + l);
      if (x) return l + ((uint32_t)__builtin_ctz(x) >> 3);
      l += 4u;
    }
    while (l < maxl && b[q + l] == b[p + l]) ++l;
    return l;
  }
  // match(p) from p's link e (1 + the nearest earlier position with p's hash, 0: none); p + 4 <= n
  static DFL_FN uint32_t match(const Search &S, const uint8_t *b, uint32_t n, uint32_t p, uint32_t e) {
    const uint32_t maxl = n - p < DFL_MAX_MATCH ? n - p : DFL_MAX_MATCH;
    uint32_t best = DFL_MIN_MATCH - 1u, dist = 0, last = p;
    for (uint32_t step = 0; step < DEPTH && e; ++step) {
      const uint32_t q = e - 1u;
      if (q >= last || p - q > WINDOW) break;
      last = q;
      if (b[q + best] == b[p + best]) {            // (best < maxl: q + best < p + best < n) only then can q be longer than the best
        const uint32_t l = prefix(b, q, p, maxl);
        if (l > best) { best = l; dist = p - q; }
        if (best >= maxl) break;
      }
      e = S.ring[q & (RING - 1u)];
    }
    return dist ? best << 16 | dist : 0u;
  }
  template <class Team>
  static DFL_FN void reset(const Team &T, Search &S) {
    for (uint32_t i = T.tid(); i < (1u << HASH_BITS); i += Team::N) S.head[i] = 0;
  }
  template <class Team, class Work>
  static DFL_FN void tokens(const Team &T, Work &W, const uint8_t *b, uint32_t n, uint32_t *tok) {
    const uint32_t tid = T.tid();
    Search &S = W.s;
    uint32_t pos = 0, nt = 0;             // lane 0's: the position to parse next, tokens so far
    for (uint32_t base = 0; base < n; base += DFL_BATCH) {
      for (uint32_t t = tid; t < DFL_BATCH; t += Team::N) S.hb[t] = (uint16_t)(base + t + DFL_MIN_MATCH <= n ? hash(b + base + t) : NO_HASH);
      T.sync();
      // every position's link.  A team that visits the positions in order inserts as it goes; lanes side by side look for the
      // nearest predecessor among the batch's own hashes first, then in the table, which holds earlier batches only
      for (uint32_t t = tid; t < DFL_BATCH; t += Team::N) {
        const uint32_t p = base + t, h = S.hb[t];
        if (h == NO_HASH) continue;
        uint32_t e = 0;
        if (Team::IN_ORDER) {
          e = S.head[h];
          S.head[h] = p + 1u;
        } else {
          for (uint32_t u = t; u-- > 0u;)
            if (S.hb[u] == h) { e = base + u + 1u; break; }
          if (!e) e = S.head[h];
        }
        S.ring[p & (RING - 1u)] = (uint16_t)e;                        // (e <= 0xFF00)
      }
      T.sync();
      for (uint32_t t = tid; t < DFL_BATCH; t += Team::N) {
        const uint32_t p = base + t, h = S.hb[t];
        S.cand[p & (2u * DFL_BATCH - 1u)] = h == NO_HASH ? 0u : match(S, b, n, p, S.ring[p & (RING - 1u)]);
        if (!Team::IN_ORDER && h != NO_HASH) T.max_u32(&S.head[h], p + 1u);
      }
      T.sync();
      // lane 0 parses what has its look-ahead: all but the batch's last position, which waits for the next batch
      if (tid == 0) {
        const uint32_t end = base + DFL_BATCH < n ? base + DFL_BATCH : n, lim = end == n ? n : end - 1u;
        while (pos < lim) {
          uint32_t c = S.cand[pos & (2u * DFL_BATCH - 1u)];
          if (c && pos + 1u < n && (S.cand[(pos + 1u) & (2u * DFL_BATCH - 1u)] >> 16) > (c >> 16)) c = 0;
          pos += dfl_token(W, b, pos, c, tok, nt, n);
          ++nt;
        }
      }
    }
    if (tid == 0) W.ntok = nt < n ? nt : n;
  }
};
static_assert(DflDense::RING >= DflDense::WINDOW + DFL_BATCH && (DflDense::RING & (DflDense::RING - 1u)) == 0 && DflDense::WINDOW <= DFL_MAX_DIST, "the ring holds a window and a batch");

// One block.  in[0, n), 1 <= n <= 0xFF00; tok[0, n) is scratch (the tokens); out has room for n + 31 bytes.
// Returns the member's size; *stored = 1 when the block went out stored.  Every lane of the team makes the call, with the
// same arguments, and every lane returns the same values.  The work area's type names the match rule.
template <class Team, class Rule>
DFL_FN uint32_t dfl_block(const Team &T, DflWorkT<Rule> &W, const DflCrc &crc, const uint8_t *in, uint32_t n, uint32_t *tok, uint8_t *out, uint32_t *stored) {
  const uint32_t tid = T.tid();
  uint8_t *b = reinterpret_cast<uint8_t *>(W.buf);
  if (n > DFL_MAX_BLOCK) n = DFL_MAX_BLOCK;
  // ---- the block's bytes, empty tables
  for (uint32_t i = tid; i < n; i += Team::N) b[i] = in[i];
  Rule::reset(T, W.s);
  for (uint32_t i = tid; i < 288u; i += Team::N) W.lit_hist[i] = 0;
  for (uint32_t i = tid; i < 32u; i += Team::N) W.dist_hist[i] = 0;
  for (uint32_t i = tid; i < 20u; i += Team::N) W.cl_hist[i] = 0;
  for (uint32_t i = tid; i < 256u; i += Team::N) W.crc.tab[i] = crc.tab[i];
  for (uint32_t i = tid; i < 17u * 32u; i += Team::N) (&W.crc.zop[0][0])[i] = (&crc.zop[0][0])[i];
  if (tid == 0) W.crc_acc = 0;
  T.sync();
  // ---- CRC-32: a contiguous slice per lane, each advanced through the bytes behind it, XOR-ed together
  {
    const uint32_t per = (n + Team::N - 1u) / Team::N;
    for (uint32_t t = tid; t < Team::N; t += Team::N) {
      const uint32_t s = t * per < n ? t * per : n, e = s + per < n ? s + per : n;
      uint32_t c = 0;
      for (uint32_t i = s; i < e; ++i) c = W.crc.tab[(c ^ b[i]) & 0xffu] ^ (c >> 8);
      c = dfl_crc_zeros(W.crc, c, n - e);
      if (t == 0) c ^= dfl_crc_zeros(W.crc, 0xffffffffu, n);       // the all-ones start value, run through the whole block
      if (c) T.xor_u32(&W.crc_acc, c);
    }
  }
  // ---- the tokens: the rule's match search and parse
  Rule::tokens(T, W, b, n, tok);
  if (tid == 0) W.lit_hist[256] = 1;
  T.sync();
  const uint32_t ntok = W.ntok, crc32 = ~W.crc_acc;
  // ---- code lengths and codes
  dfl_code_lengths(T, W, W.lit_hist, DFL_NLIT, 15, W.lit_len);
  dfl_code_lengths(T, W, W.dist_hist, DFL_NDIST, 15, W.dist_len);
  if (tid == 0) {
    dfl_codes(W.lit_len, DFL_NLIT, W.lit_code);
    dfl_codes(W.dist_len, DFL_NDIST, W.dist_code);
    uint32_t hlit = DFL_NLIT, hdist = DFL_NDIST;
    while (hlit > 257u && !W.lit_len[hlit - 1u]) --hlit;
    while (hdist > 1u && !W.dist_len[hdist - 1u]) --hdist;
    W.hlit = hlit; W.hdist = hdist;
    // the two length tables as one sequence, run-length coded (RFC 1951 3.2.7: a run may cross from one table into the other)
    const uint32_t total = hlit + hdist;
    uint32_t k = 0, i = 0;
    auto at = [&](uint32_t j) -> uint32_t { return j < hlit ? W.lit_len[j] : W.dist_len[(j - hlit) & 31u]; };
    auto emit = [&](uint32_t sym, uint32_t extra) {
      if (k < DFL_NLIT + DFL_NDIST + 4u) W.cl_sym[k] = (uint16_t)(sym | extra << 8);
      ++k;
      W.cl_hist[sym]++;
    };
    while (i < total) {
      const uint32_t v = at(i);
      uint32_t run = 1;
      while (i + run < total && at(i + run) == v) ++run;
      i += run;
      if (v == 0u) {
        while (run >= 11u) { const uint32_t r = run < 138u ? run : 138u; emit(18, r - 11u); run -= r; }
        if (run >= 3u) { emit(17, run - 3u); run = 0; }
        while (run--) emit(0, 0);
      } else {
        emit(v, 0); --run;
        while (run >= 3u) { const uint32_t r = run < 6u ? run : 6u; emit(16, r - 3u); run -= r; }
        while (run--) emit(v, 0);
      }
    }
    W.n_cl = k < DFL_NLIT + DFL_NDIST + 4u ? k : DFL_NLIT + DFL_NDIST + 4u;
    // zlib refuses an incomplete code-length code: were there one symbol only, a second one is counted (it is never sent)
    uint32_t used = 0, one = 0;
    for (uint32_t s = 0; s < DFL_NCL; ++s) if (W.cl_hist[s]) { ++used; one = s; }
    if (used == 1u) W.cl_hist[one ? 0u : 1u] = 1;
  }
  T.sync();
  dfl_code_lengths(T, W, W.cl_hist, DFL_NCL, 7, W.cl_len);
  if (tid == 0) {
    dfl_codes(W.cl_len, DFL_NCL, W.cl_code);
    uint32_t hclen = DFL_NCL;
    while (hclen > 4u && !W.cl_len[dfl_cl_order(hclen - 1u)]) --hclen;
    W.hclen = hclen;
    uint32_t bits = 3u + 5u + 5u + 4u + 3u * hclen;
    for (uint32_t j = 0; j < W.n_cl; ++j) {
      const uint32_t sym = W.cl_sym[j] & 0xffu;
      bits += W.cl_len[sym < 20u ? sym : 19u] + (sym == 16u ? 2u : sym == 17u ? 3u : sym == 18u ? 7u : 0u);
    }
    W.header_bits = bits;
    for (uint32_t s = 0; s < DFL_NLIT; ++s) bits += W.lit_hist[s] * (W.lit_len[s] + dfl_len_extra(s));
    for (uint32_t s = 0; s < DFL_NDIST; ++s) bits += W.dist_hist[s] * (W.dist_len[s] + dfl_dist_extra(s));
    W.total_bits = bits;                                            // (<= 65281 tokens of <= 48 bits: no overflow)
    W.dynamic = (bits + 7u) / 8u < 5u + n ? 1u : 0u;
  }
  T.sync();
  const uint32_t dynamic = W.dynamic, body = dynamic ? (W.total_bits + 7u) / 8u : 5u + n, size = 18u + body + 8u;
  // ---- the member: header and trailer
  if (tid == 0) {
    const uint8_t hdr[16] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0};
    for (int i = 0; i < 16; ++i) out[i] = hdr[i];
    out[16] = (uint8_t)((size - 1u) & 0xffu); out[17] = (uint8_t)((size - 1u) >> 8);
    uint8_t *tr = out + 18u + body;
    for (int i = 0; i < 4; ++i) { tr[i] = (uint8_t)(crc32 >> (8 * i)); tr[4 + i] = (uint8_t)(n >> (8 * i)); }
  }
  if (!dynamic) {
    if (tid == 0) {
      out[18] = 1;                                                  // BFINAL = 1, BTYPE = 00, padding
      out[19] = (uint8_t)(n & 0xffu); out[20] = (uint8_t)(n >> 8);
      out[21] = (uint8_t)(~n & 0xffu); out[22] = (uint8_t)((~n >> 8) & 0xffu);
    }
    for (uint32_t i = tid; i < n; i += Team::N) out[23u + i] = b[i];
    T.sync();
    *stored = 1;
    return size;
  }
  // ---- the dynamic form's bits, in place of the block's bytes (which the tokens have replaced)
  const uint32_t words = (body + 3u) / 4u;                          // body < 5 + n: inside buf
  for (uint32_t i = tid; i < words && i < DFL_BUF_WORDS; i += Team::N) W.buf[i] = 0;
  const uint32_t per = (ntok + Team::N - 1u) / Team::N;
  auto tok_bits = [&](uint32_t t) -> uint32_t {
    if (!(t & 0x80000000u)) return W.lit_len[t & 0xffu];
    uint32_t sym, eb, ev, r;
    dfl_len_sym((t >> 16) & 0xffu, sym, eb, ev);
    r = W.lit_len[sym < 288u ? sym : 287u] + eb;
    dfl_dist_sym(t & 0x7fffu, sym, eb, ev);
    return r + W.dist_len[sym & 31u] + eb;
  };
  for (uint32_t t = tid; t < DFL_BATCH; t += Team::N) {
    const uint32_t s = t * per < ntok ? t * per : ntok, e = s + per < ntok ? s + per : ntok;
    uint32_t sum = 0;
    for (uint32_t i = s; i < e; ++i) sum += tok_bits(tok[i]);
    W.part[t] = sum;
  }
  T.sync();
  if (tid == 0) {
    uint32_t at = 0;
    dfl_put(T, W.buf, at, 1u | 2u << 1, 3); at += 3;                // BFINAL = 1, BTYPE = 10
    dfl_put(T, W.buf, at, W.hlit - 257u, 5); at += 5;
    dfl_put(T, W.buf, at, W.hdist - 1u, 5); at += 5;
    dfl_put(T, W.buf, at, W.hclen - 4u, 4); at += 4;
    for (uint32_t j = 0; j < W.hclen; ++j) { dfl_put(T, W.buf, at, W.cl_len[dfl_cl_order(j)], 3); at += 3; }
    for (uint32_t j = 0; j < W.n_cl; ++j) {
      const uint32_t sym = W.cl_sym[j] & 0xffu, extra = (uint32_t)W.cl_sym[j] >> 8, s = sym < 20u ? sym : 19u;
      dfl_put(T, W.buf, at, W.cl_code[s], W.cl_len[s]); at += W.cl_len[s];
      const uint32_t eb = sym == 16u ? 2u : sym == 17u ? 3u : sym == 18u ? 7u : 0u;
      dfl_put(T, W.buf, at, extra, eb); at += eb;
    }
    for (uint32_t t = 0; t < DFL_BATCH; ++t) { const uint32_t s = W.part[t]; W.part[t] = at; at += s; }     // exclusive sums, behind the header
    dfl_put(T, W.buf, at, W.lit_code[256], W.lit_len[256]);        // end of block
  }
  T.sync();
  for (uint32_t t = tid; t < DFL_BATCH; t += Team::N) {
    const uint32_t s = t * per < ntok ? t * per : ntok, e = s + per < ntok ? s + per : ntok;
    uint32_t at = W.part[t];
    for (uint32_t i = s; i < e; ++i) {
      const uint32_t k = tok[i];
      if (!(k & 0x80000000u)) {
        dfl_put(T, W.buf, at, W.lit_code[k & 0xffu], W.lit_len[k & 0xffu]); at += W.lit_len[k & 0xffu];
        continue;
      }
      uint32_t sym, eb, ev;
      dfl_len_sym((k >> 16) & 0xffu, sym, eb, ev);
      sym = sym < 288u ? sym : 287u;
      dfl_put(T, W.buf, at, (uint32_t)W.lit_code[sym] | ev << W.lit_len[sym], W.lit_len[sym] + eb); at += W.lit_len[sym] + eb;
      dfl_dist_sym(k & 0x7fffu, sym, eb, ev);
      sym &= 31u;
      dfl_put(T, W.buf, at, (uint32_t)W.dist_code[sym] | ev << W.dist_len[sym], W.dist_len[sym] + eb); at += W.dist_len[sym] + eb;
    }
  }
  T.sync();
  for (uint32_t i = tid; i < body; i += Team::N) out[18u + i] = b[i];
  T.sync();
  *stored = 0;
  return size;
}

// the output bytes that always suffice: every member stored
inline uint64_t dfl_bound(uint64_t in_bytes, uint32_t block_bytes) {
  if (!block_bytes) return 0;
  const uint64_t nb = in_bytes / block_bytes, rem = in_bytes % block_bytes;
  return nb * ((uint64_t)block_bytes + DFL_MEMBER_EXTRA) + (rem ? rem + DFL_MEMBER_EXTRA : 0);
}

inline const DflCrc &dfl_crc_tables() {
  static const DflCrc T = [] { DflCrc t; dfl_crc_make(t); return t; }();
  return T;
}

// strl_bgzf_deflate_host without the error text: the members of in[0, in_bytes) back to back on the calling thread;
// with the rule and the team named (the tests run the lanes' side of the dense rule on one thread this way)
template <class Rule, class Team = DflSerial>
inline int dfl_deflate_host_as(const uint8_t *in, uint64_t in_bytes, uint32_t block_bytes, uint8_t *out, uint64_t out_cap, uint64_t *out_bytes, uint32_t *csize,
                               uint32_t *n_stored) {
  if (block_bytes < 1u || block_bytes > DFL_MAX_BLOCK || !out_bytes || (in_bytes && (!in || !out))) return STRL_ERR_ARG;
  if (out_cap < dfl_bound(in_bytes, block_bytes)) return STRL_ERR_CAPACITY;
  *out_bytes = 0;
  if (n_stored) *n_stored = 0;
  if (!in_bytes) return STRL_OK;
  std::unique_ptr<DflWorkT<Rule>> W(new DflWorkT<Rule>);
  std::vector<uint32_t> tok(block_bytes);
  std::vector<uint8_t> slot((size_t)block_bytes + DFL_MEMBER_EXTRA);
  const Team T;
  uint64_t at = 0, k = 0;
  for (uint64_t off = 0; off < in_bytes; off += block_bytes, ++k) {
    const uint32_t n = (uint32_t)(in_bytes - off < block_bytes ? in_bytes - off : block_bytes);
    uint32_t st = 0;
    const uint32_t size = dfl_block(T, *W, dfl_crc_tables(), in + off, n, tok.data(), slot.data(), &st);
    memcpy(out + at, slot.data(), size);
    if (csize) csize[k] = size;
    if (n_stored) *n_stored += st;
    at += size;
  }
  *out_bytes = at;
  return STRL_OK;
}
inline int dfl_deflate_host(const uint8_t *in, uint64_t in_bytes, uint32_t block_bytes, uint8_t *out, uint64_t out_cap, uint64_t *out_bytes, uint32_t *csize,
                            uint32_t *n_stored) {
  return dfl_deflate_host_as<DflFast>(in, in_bytes, block_bytes, out, out_cap, out_bytes, csize, n_stored);
}
// ... with the rule as a value: STRL_DEFLATE_FAST or STRL_DEFLATE_DENSE, any other is STRL_ERR_ARG
inline int dfl_deflate_host_mode(int mode, const uint8_t *in, uint64_t in_bytes, uint32_t block_bytes, uint8_t *out, uint64_t out_cap, uint64_t *out_bytes,
                                 uint32_t *csize, uint32_t *n_stored) {
  if (mode == STRL_DEFLATE_FAST) return dfl_deflate_host_as<DflFast>(in, in_bytes, block_bytes, out, out_cap, out_bytes, csize, n_stored);
  if (mode == STRL_DEFLATE_DENSE) return dfl_deflate_host_as<DflDense>(in, in_bytes, block_bytes, out, out_cap, out_bytes, csize, n_stored);
  return STRL_ERR_ARG;
}

}  // namespace strl
