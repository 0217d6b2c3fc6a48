// markdup_core.h -- the rule of `strling sort --markdup` (flag 0x400 on duplicate pairs and fragments), one source for the device
// path (markdup.hip), the host path (cli/sort_cli.cpp), the library's host entry (strl_markdup_host) and the stand-alone test program
// (tests/emu/markdup_core_main.cpp).  DESIGN section 24.3.  The reference drops records that carry the flag when it collects
// spanning evidence (collect.nim:140), and so does `call` (F_DUP in call_logic.cpp, EVF_DUP in evidence_core.h).
//
// Picard's rule as `samtools markdup` applies it in template mode, without optical duplicates, libraries and read groups ignored:
//   eligible   0x4, 0x100, 0x200 and 0x800 all clear.  Every other record keeps its flag word, an incoming 0x400 included; an
//              eligible record has 0x400 cleared and then decided here.
//   signature  e = (tid, u, strand): strand = flag bit 0x10; forward u = pos - leading S/H lengths; reverse u = pos + reflen - 1 +
//              trailing S/H lengths (reflen over M, D, N, =, X; 0 without a CIGAR).  u is signed and compared as an integer.
//   score      the sum of the quality bytes >= 15; 0xFF (absent) counts as 0.
//   pair       a NAME whose eligible records are exactly two, one with 0x40 and one with 0x80, both with 0x1 set and 0x8 clear.
//              Every other eligible record is a fragment.
//   pairs      key (e_lo, e_hi), the two signatures in ascending order; template score = the two scores added.  Among equal keys
//              the highest template score is kept, ties to the lowest input ordinal of the 0x40 record; both records of every
//              other pair get 0x400.
//   fragments  where any record of any pair has the signature e, every fragment with e gets 0x400; else the fragment with the
//              highest score is kept (ties to the lowest ordinal) and the others get 0x400.
// A record whose name, CIGAR, bases and qualities do not fit its block_size is refused (the caller names its ordinal), and so is
// one whose unclipped end leaves 32 signed bits -- no position of a BAM is there, and the packed signature has 32 bits for it.
#pragma once
#include <stdint.h>
#include <string.h>
#if defined(__HIPCC__)
#define MDUP_HD __host__ __device__
#else
#define MDUP_HD
#endif
#include <algorithm>
#include <map>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

namespace strl {

constexpr uint32_t MDUP_DUP = 0x400;
constexpr uint32_t MDUP_RUN_MAX = 512;                   // records under one name hash the device resolves (the host has no limit)
// device bytes a record of the step: signature 8, score 4, mate 4, class 1, and the sorts' two key and two value buffers 8 + 8 + 4 + 4
constexpr uint64_t MDUP_RECORD_BYTES = 41;
constexpr uint32_t MDUP_FLAG_AT = 18;                   // the flag word behind a record's start (its block_size word included)
constexpr uint32_t MDUP_FIXED = 36;                      // block_size word + the 32 fixed bytes

// what the device keeps of a record between its kernels (one byte)
constexpr uint8_t MDUP_C_ELIGIBLE = 1, MDUP_C_PAIRABLE = 2, MDUP_C_FIRST = 4, MDUP_C_LAST = 8, MDUP_C_PAIRED = 16, MDUP_C_MARK = 32;

MDUP_HD inline uint32_t mdup_ld16(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }
MDUP_HD inline uint32_t mdup_ld32(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

MDUP_HD inline bool mdup_eligible(uint32_t flag) { return !(flag & (0x4u | 0x100u | 0x200u | 0x800u)); }
// the class byte of an eligible record's flag word
MDUP_HD inline uint8_t mdup_class(uint32_t flag) {
  if (!mdup_eligible(flag)) return 0;
  return (uint8_t)(MDUP_C_ELIGIBLE | ((flag & 0x1u) && !(flag & 0x8u) ? MDUP_C_PAIRABLE : 0) | (flag & 0x40u ? MDUP_C_FIRST : 0) | (flag & 0x80u ? MDUP_C_LAST : 0));
}
// two eligible records alone under one name: a pair?
MDUP_HD inline bool mdup_is_pair(uint8_t a, uint8_t b) {
  if (!(a & MDUP_C_PAIRABLE) || !(b & MDUP_C_PAIRABLE)) return false;
  const uint8_t ea = a & (MDUP_C_FIRST | MDUP_C_LAST), eb = b & (MDUP_C_FIRST | MDUP_C_LAST);
  return (ea == MDUP_C_FIRST && eb == MDUP_C_LAST) || (ea == MDUP_C_LAST && eb == MDUP_C_FIRST);
}

// where the parts of a record lie, from its start (the block_size word): false when they do not fit `len` = 4 + block_size
struct MdupFields { int32_t tid, pos; uint32_t flag, l_name, n_cigar, l_seq, cigar_at, qual_at; };
MDUP_HD inline bool mdup_fields(const uint8_t *rec, uint64_t len, MdupFields *f) {
  if (len < MDUP_FIXED || (uint64_t)mdup_ld32(rec) + 4u != len) return false;
  f->tid = (int32_t)mdup_ld32(rec + 4); f->pos = (int32_t)mdup_ld32(rec + 8);
  f->l_name = rec[12]; f->n_cigar = mdup_ld16(rec + 16); f->flag = mdup_ld16(rec + MDUP_FLAG_AT); f->l_seq = mdup_ld32(rec + 20);
  if (f->l_seq > 0x7fffffffu) return false;
  const uint64_t cigar_at = (uint64_t)MDUP_FIXED + f->l_name, seq_at = cigar_at + 4ull * f->n_cigar, qual_at = seq_at + ((uint64_t)f->l_seq + 1u) / 2u;
  if (qual_at + f->l_seq > len) return false;
  f->cigar_at = (uint32_t)cigar_at; f->qual_at = (uint32_t)qual_at;      // (below len, which is below 2^32 + 4; a caller holds records far below)
  return true;
}

// the unclipped end of the signature from the CIGAR words (little-endian, any alignment); false: it leaves 32 signed bits
MDUP_HD inline bool mdup_unclipped(const uint8_t *cigar, uint32_t n_cigar, int32_t pos, bool reverse, int32_t *u) {
  int64_t v = pos;
  if (!reverse) {
    for (uint32_t k = 0; k < n_cigar; ++k) {
      const uint32_t w = mdup_ld32(cigar + 4u * k), op = w & 15u;
      if (op != 4u && op != 5u) break;
      v -= (int64_t)(w >> 4);
    }
  } else {
    int64_t reflen = 0, tail = 0;
    for (uint32_t k = 0; k < n_cigar; ++k) {
      const uint32_t w = mdup_ld32(cigar + 4u * k), op = w & 15u;
      if (op == 0u || op == 2u || op == 3u || op == 7u || op == 8u) reflen += (int64_t)(w >> 4);
      if (op == 4u || op == 5u) tail += (int64_t)(w >> 4); else tail = 0;
    }
    v += reflen - 1 + tail;
  }
  if (v < -2147483648ll || v > 2147483647ll) return false;
  *u = (int32_t)v;
  return true;
}

// the signature as one word that orders as (tid, u, strand) orders: tid + 1 in 31 bits (tid >= -1), u + 2^31 in 32, the strand
MDUP_HD inline uint64_t mdup_sig(int32_t tid, int32_t u, uint32_t reverse) {
  return (uint64_t)(uint32_t)(tid + 1) << 33 | (uint64_t)((uint32_t)u ^ 0x80000000u) << 1 | (uint64_t)(reverse & 1u);
}
// the bits of a signature that can differ among records of a file with n_ref references
MDUP_HD inline int mdup_sig_bits(int32_t n_ref) { int b = 0; for (uint32_t x = (uint32_t)n_ref; x; x >>= 1) ++b; return 33 + b; }

MDUP_HD inline uint32_t mdup_qual(uint32_t b) { return b >= 15u && b != 0xffu ? b : 0u; }
// the four quality bytes of a word
MDUP_HD inline uint32_t mdup_qual4(uint32_t w) { return mdup_qual(w & 255u) + mdup_qual(w >> 8 & 255u) + mdup_qual(w >> 16 & 255u) + mdup_qual(w >> 24); }

// the name's 64-bit hash: FNV-1a over its l_read_name bytes, mixed.  Only the device path joins by it, and decides by the names.
MDUP_HD inline uint64_t mdup_name_hash(const uint8_t *name, uint32_t l_name) {
  uint64_t h = 0xcbf29ce484222325ull;
  for (uint32_t k = 0; k < l_name; ++k) { h ^= name[k]; h *= 0x100000001b3ull; }
  h ^= h >> 33; h *= 0xff51afd7ed558ccdull; h ^= h >> 33; h *= 0xc4ceb9fe1a85ec53ull; h ^= h >> 33;
  return h;
}
MDUP_HD inline bool mdup_same_name(const uint8_t *a, uint32_t la, const uint8_t *b, uint32_t lb) {
  if (la != lb) return false;
  for (uint32_t k = 0; k < la; ++k) if (a[k] != b[k]) return false;
  return true;
}

// the sorts' tiebreak words: an ascending sort puts the element to keep first.  score_bits = the bits the largest score of the file
// needs (a template's one more); the field lies above the 32 bits of the ordinal, a fragment's class bit above the field
MDUP_HD inline uint64_t mdup_tiebreak(uint64_t score, int score_bits, uint32_t ordinal) {
  const uint64_t top = score_bits >= 31 ? 0x7fffffffull : (1ull << score_bits) - 1ull;
  return (top - (score < top ? score : top)) << 32 | ordinal;
}

struct MdupCounts { uint64_t pairs, dup_pairs, fragments, dup_fragments, ineligible; };

// ---- the host path ----------------------------------------------------------------------------------------------------------------
// The rule over records back to back in input order (each with its block_size word), with dictionaries keyed by NAME.
// flags[i] = the flag word record i leaves with.  -> -1, or the ordinal of the first record refused (`why` says for what).
inline int64_t mdup_host(const uint8_t *raw, uint64_t bytes, std::vector<uint16_t> &flags, MdupCounts *counts, std::string &why) {
  struct Rec { uint64_t sig; uint64_t score; uint8_t cls; };
  std::vector<Rec> R;
  std::unordered_map<std::string, std::vector<uint32_t>> by_name;      // eligible records of a name, in input order
  flags.clear();
  MdupCounts C{0, 0, 0, 0, 0};
  for (uint64_t q = 0; q < bytes;) {
    const int64_t ord = (int64_t)R.size();
    if (bytes - q < 4 || (uint64_t)mdup_ld32(raw + q) + 4u > bytes - q) { why = "it does not lie inside the bytes given"; return ord; }
    const uint64_t len = (uint64_t)mdup_ld32(raw + q) + 4u;
    MdupFields f;
    if (!mdup_fields(raw + q, len, &f)) { why = "its name, CIGAR, bases and qualities do not fit its block_size"; return ord; }
    Rec r{0, 0, mdup_class(f.flag)};
    flags.push_back((uint16_t)f.flag);
    if (r.cls) {
      int32_t u = 0;
      if (!mdup_unclipped(raw + q + f.cigar_at, f.n_cigar, f.pos, (f.flag & 0x10u) != 0, &u)) { why = "its unclipped end is no 32-bit position"; return ord; }
      r.sig = mdup_sig(f.tid, u, f.flag >> 4 & 1u);
      for (uint32_t k = 0; k < f.l_seq; ++k) r.score += mdup_qual(raw[q + f.qual_at + k]);
      by_name[std::string(reinterpret_cast<const char *>(raw + q + MDUP_FIXED), f.l_name)].push_back((uint32_t)ord);
      flags.back() = (uint16_t)(f.flag & ~MDUP_DUP);
    } else ++C.ineligible;
    R.push_back(r);
    q += len;
  }
  // pairs: the best of every key; fragments: everything else that is eligible
  struct Best { uint64_t score; uint32_t first, last; };
  std::map<std::pair<uint64_t, uint64_t>, Best> best_pair;
  std::vector<Best> pairs;
  std::vector<uint8_t> paired(R.size(), 0);
  for (const auto &kv : by_name) {
    const std::vector<uint32_t> &v = kv.second;
    if (v.size() != 2 || !mdup_is_pair(R[v[0]].cls, R[v[1]].cls)) continue;
    const uint32_t first = R[v[0]].cls & MDUP_C_FIRST ? v[0] : v[1], last = first == v[0] ? v[1] : v[0];
    paired[first] = paired[last] = 1;
    pairs.push_back(Best{R[first].score + R[last].score, first, last});
  }
  auto better = [](const Best &a, const Best &b) { return a.score != b.score ? a.score > b.score : a.first < b.first; };
  auto key_of = [&](const Best &p) { return std::make_pair(std::min(R[p.first].sig, R[p.last].sig), std::max(R[p.first].sig, R[p.last].sig)); };
  std::unordered_map<uint64_t, char> pair_end;
  for (const Best &p : pairs) {
    pair_end[R[p.first].sig] = 1; pair_end[R[p.last].sig] = 1;
    auto it = best_pair.find(key_of(p));
    if (it == best_pair.end()) best_pair.emplace(key_of(p), p);
    else if (better(p, it->second)) it->second = p;
  }
  C.pairs = pairs.size();
  for (const Best &p : pairs)
    if (best_pair.find(key_of(p))->second.first != p.first) { flags[p.first] |= MDUP_DUP; flags[p.last] |= MDUP_DUP; ++C.dup_pairs; }
  std::unordered_map<uint64_t, Best> best_frag;
  for (uint32_t i = 0; i < R.size(); ++i) {
    if (!R[i].cls || paired[i]) continue;
    ++C.fragments;
    const Best b{R[i].score, i, i};
    auto it = best_frag.find(R[i].sig);
    if (it == best_frag.end()) best_frag.emplace(R[i].sig, b);
    else if (better(b, it->second)) it->second = b;
  }
  for (uint32_t i = 0; i < R.size(); ++i) {
    if (!R[i].cls || paired[i]) continue;
    if (pair_end.count(R[i].sig) || best_frag.find(R[i].sig)->second.first != i) { flags[i] |= MDUP_DUP; ++C.dup_fragments; }
  }
  if (counts) *counts = C;
  return -1;
}

}  // namespace strl
