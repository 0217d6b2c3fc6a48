// fastq_core.h -- the rule of `strling fastq` (a BAM's reads back to paired FASTQ, the step in front of the aligner), one source for
// the device path (fastq.hip), the host path (cli/sort_cli.cpp), the library's host entry (strl_fastq_host) and the stand-alone test
// program (tests/emu/fastq_core_main.cpp).  DESIGN section 24.4.  What `samtools collate | samtools fastq` is used for in front of
// `bwa mem -p`; agreement with samtools is unverified (no machine of the project has it).
//
//   kept        a record with flag & F == 0 and l_seq > 0.  F = 0x900 unless -F INT replaces it.
//   counted     a record that F leaves out is `filtered`; one that F keeps and whose l_seq is 0 is `empty`.  Neither is written.
//   refused     a record whose name, CIGAR, bases and qualities do not fit its block_size (mdup_fields' check), with its ordinal.
//   read number r = (flag >> 6) & 3.
//   pair        a NAME with exactly two kept records, one with r == 1 and one with r == 2.  No other flag bit matters.
//   single      every other kept record.
//   entry       @NAME[/1|/2]\n SEQ\n +\n QUAL\n   -- l_name - 1 + 2 l_seq + 6 bytes, 2 more with a suffix
//   NAME        the l_read_name - 1 name bytes as they are (none when l_read_name is 0); the suffix only with -N and r in {1, 2}.
//   SEQ         the 4-bit codes through "=ACMGRSVTWYHKDBN".
//   QUAL        min(q, 93) + 33 a byte.  A first quality byte of 0xFF says the qualities are absent: every position then gets
//               min(v, 93) + 33, v = -v INT (default 1: '"').  A 0xFF behind a valid first byte is a value like any other (clamped).
//   reverse     with flag 0x10 the read is written as it was sequenced: the bases reversed and complemented, the qualities reversed.
//               The complement of a 4-bit code is its four bits in reverse order (A=1 <-> T=8, C=2 <-> G=4; = and N stay).
//   order       of first appearance: a pair stands where the earlier of its two records stood in the input, R1 before R2; singles
//               stand in input order.
//   streams     p1, p2 and s.  Split (-1 A -2 B): R1 entries to p1, R2 entries to p2.  Interleaved (-o): R1, R2, R1, R2 ... in p1,
//               p2 empty.  Singles go to s, which is laid out only when it is written (-s FILE); else they are counted as not written
//               and never mixed into the pairs: an interleaved stream that `bwa mem -p` reads must hold pairs only.
#pragma once
#include <stdint.h>
#include <string.h>
#include <string>
#include <unordered_map>
#include <vector>
#include "markdup_core.h"

namespace strl {

constexpr uint32_t FASTQ_FILTER_DEFAULT = 0x900;
constexpr uint32_t FASTQ_QUAL_MAX = 93;
// what the device keeps of a record between its kernels (one byte); FASTQ_C_SEEN is the runs kernel's
constexpr uint8_t FASTQ_C_KEPT = 1, FASTQ_C_R1 = 2, FASTQ_C_R2 = 4, FASTQ_C_REVERSE = 8, FASTQ_C_PAIRED = 16, FASTQ_C_SEEN = 64;
constexpr int FASTQ_P1 = 0, FASTQ_P2 = 1, FASTQ_S = 2;
// device bytes a record while the step runs: class 1, entry length 4, mate 4, the join's two key and two value buffers 8 + 8 + 4 + 4
// and up to three streams' offsets 3 x 8; behind the plan the key and value buffers are gone
constexpr uint64_t FASTQ_RECORD_BYTES = 57;

struct FastqOpts {
  uint32_t filter;        // F
  uint32_t suffix;        // -N
  uint32_t default_qual;  // -v
  uint32_t interleaved;   // -o: R2 behind its R1 in p1
  uint32_t singles;       // -s: s is laid out
};
struct FastqCounts { uint64_t kept, filtered, empty, pairs, singles, singles_unwritten; };

MDUP_HD inline uint32_t fastq_read_number(uint32_t flag) { return flag >> 6 & 3u; }
// the class byte of a record: 0 when it is not kept
MDUP_HD inline uint8_t fastq_class(uint32_t flag, uint32_t l_seq, uint32_t filter) {
  if ((flag & filter) || !l_seq) return 0;
  const uint32_t r = fastq_read_number(flag);
  return (uint8_t)(FASTQ_C_KEPT | (r == 1u ? FASTQ_C_R1 : 0) | (r == 2u ? FASTQ_C_R2 : 0) | (flag & 0x10u ? FASTQ_C_REVERSE : 0));
}
// two kept records alone under one name: a pair?
MDUP_HD inline bool fastq_is_pair(uint8_t a, uint8_t b) {
  const uint8_t ea = a & (FASTQ_C_R1 | FASTQ_C_R2), eb = b & (FASTQ_C_R1 | FASTQ_C_R2);
  return (ea == FASTQ_C_R1 && eb == FASTQ_C_R2) || (ea == FASTQ_C_R2 && eb == FASTQ_C_R1);
}
MDUP_HD inline uint32_t fastq_name_bytes(uint32_t l_name) { return l_name ? l_name - 1u : 0u; }
MDUP_HD inline uint64_t fastq_entry_len(uint32_t l_name, uint32_t l_seq, uint32_t flag, uint32_t suffix) {
  const uint32_t r = fastq_read_number(flag);
  return (uint64_t)fastq_name_bytes(l_name) + 2ull * l_seq + 6u + (suffix && (r == 1u || r == 2u) ? 2u : 0u);
}

// the letter of a 4-bit code ("=ACMGRSVTWYHKDBN" as two words: no table in memory) and the code's complement
MDUP_HD inline uint8_t fastq_base(uint32_t code) {
  constexpr uint64_t lo = (uint64_t)'=' | (uint64_t)'A' << 8 | (uint64_t)'C' << 16 | (uint64_t)'M' << 24 | (uint64_t)'G' << 32 | (uint64_t)'R' << 40 | (uint64_t)'S' << 48 | (uint64_t)'V' << 56;
  constexpr uint64_t hi = (uint64_t)'T' | (uint64_t)'W' << 8 | (uint64_t)'Y' << 16 | (uint64_t)'H' << 24 | (uint64_t)'K' << 32 | (uint64_t)'D' << 40 | (uint64_t)'B' << 48 | (uint64_t)'N' << 56;
  return (uint8_t)((code & 8u ? hi : lo) >> ((code & 7u) * 8u));
}
MDUP_HD inline uint32_t fastq_complement(uint32_t code) { return (code & 1u) << 3 | (code & 2u) << 1 | (code & 4u) >> 1 | (code & 8u) >> 3; }
MDUP_HD inline uint8_t fastq_qual(uint32_t q) { return (uint8_t)((q < FASTQ_QUAL_MAX ? q : FASTQ_QUAL_MAX) + 33u); }

// a record ready to be written: where its parts lie from its start (the block_size word), and what the options make of it
struct FastqRec {
  uint32_t name_at, n_name, seq_at, qual_at, l_seq, flag;
  uint8_t cls, suffix;       // suffix: 0, or '1' / '2'
  uint8_t absent, fill;      // the qualities are absent | the byte every position then gets
  uint64_t len;              // of the entry
};
// false: the record's parts do not fit `len` = 4 + block_size (mdup_fields' check)
MDUP_HD inline bool fastq_rec(const uint8_t *rec, uint64_t len, const FastqOpts &o, FastqRec *R) {
  MdupFields f;
  if (!mdup_fields(rec, len, &f)) return false;
  R->name_at = MDUP_FIXED; R->n_name = fastq_name_bytes(f.l_name); R->l_seq = f.l_seq; R->flag = f.flag;
  R->qual_at = f.qual_at; R->seq_at = f.qual_at - (f.l_seq + 1u) / 2u;
  R->cls = fastq_class(f.flag, f.l_seq, o.filter);
  const uint32_t r = fastq_read_number(f.flag);
  R->suffix = o.suffix && (r == 1u || r == 2u) ? (uint8_t)('0' + r) : 0;
  R->absent = f.l_seq && rec[f.qual_at] == 0xffu;
  R->fill = fastq_qual(o.default_qual);
  R->len = fastq_entry_len(f.l_name, f.l_seq, f.flag, o.suffix);
  return true;
}

// The bytes [first, first + count) of a record's entry, each handed to emit(index in [0, count), byte) in ascending order; a window
// that reaches past the entry's end is cut there.  Every text the project writes comes from here: the kernel packs the bytes of a
// 16-byte word into registers, the host path and the test program store them.  Nothing outside the record is read: base i of the
// entry is nibble j = reverse ? l_seq - 1 - i : i of the bases (byte j / 2, the high nibble for an even j -- for an odd l_seq the
// last base sits in a high nibble and the low nibble beside it is padding, which no j names).
template <typename Emit> MDUP_HD inline void fastq_entry_emit(const uint8_t *rec, const FastqRec &R, uint64_t first, uint64_t count, Emit &&emit) {
  const uint64_t l = R.l_seq, name_end = 1u + (uint64_t)R.n_name, head_end = name_end + (R.suffix ? 2u : 0u) + 1u, seq_end = head_end + l, sep_end = seq_end + 3u,
                 qual_end = sep_end + l, end = first + count < R.len ? first + count : R.len;
  const bool rev = (R.flag & 0x10u) != 0;
  uint64_t k = first;
  for (; k < end && k < head_end; ++k) {
    uint8_t b;
    if (k == 0) b = '@';
    else if (k < name_end) b = rec[R.name_at + (k - 1u)];
    else if (k + 1u == head_end) b = '\n';
    else b = k == name_end ? (uint8_t)'/' : R.suffix;
    emit((uint32_t)(k - first), b);
  }
  const uint8_t *seq = rec + R.seq_at, *qual = rec + R.qual_at;
  for (const uint64_t e = end < seq_end ? end : seq_end; k < e; ++k) {
    const uint64_t i = k - head_end, j = rev ? l - 1u - i : i;
    const uint32_t code = (uint32_t)(seq[j >> 1] >> ((~j & 1u) << 2)) & 15u;
    emit((uint32_t)(k - first), fastq_base(rev ? fastq_complement(code) : code));
  }
  for (const uint64_t e = end < sep_end ? end : sep_end; k < e; ++k) emit((uint32_t)(k - first), k - seq_end == 1u ? (uint8_t)'+' : (uint8_t)'\n');
  for (const uint64_t e = end < qual_end ? end : qual_end; k < e; ++k) {
    const uint64_t i = k - sep_end, j = rev ? l - 1u - i : i;
    emit((uint32_t)(k - first), R.absent ? R.fill : fastq_qual(qual[j]));
  }
  if (k < end) emit((uint32_t)(k - first), (uint8_t)'\n');      // (k == qual_end == R.len - 1)
}
// ... stored to out[0, count)
MDUP_HD inline void fastq_entry_bytes(const uint8_t *rec, const FastqRec &R, uint64_t first, uint64_t count, uint8_t *out) {
  fastq_entry_emit(rec, R, first, count, [out](uint32_t at, uint8_t b) { out[at] = b; });
}

// ---- the host path ----------------------------------------------------------------------------------------------------------------
// The rule over records back to back in input order (each with its block_size word), with a dictionary keyed by NAME.
// stream[FASTQ_P1 / _P2 / _S] = the three byte streams.  -> -1, or the ordinal of the first record refused (`why` says for what).
inline int64_t fastq_host(const uint8_t *raw, uint64_t bytes, const FastqOpts &o, std::vector<uint8_t> stream[3], FastqCounts *counts, std::string &why) {
  struct Rec { uint64_t at; FastqRec R; uint32_t mate; };
  std::vector<Rec> V;
  std::unordered_map<std::string, std::vector<uint32_t>> by_name;      // kept records of a name, in input order
  FastqCounts C{0, 0, 0, 0, 0, 0};
  for (int s = 0; s < 3; ++s) stream[s].clear();
  for (uint64_t q = 0; q < bytes;) {
    const int64_t ord = (int64_t)V.size();
    if (bytes - q < 4 || (uint64_t)mdup_ld32(raw + q) + 4u > bytes - q) { why = "it does not lie inside the bytes given"; return ord; }
    const uint64_t len = (uint64_t)mdup_ld32(raw + q) + 4u;
    Rec r{q, FastqRec{}, 0xffffffffu};
    if (!fastq_rec(raw + q, len, o, &r.R)) { why = "its name, CIGAR, bases and qualities do not fit its block_size"; return ord; }
    if (r.R.cls) { ++C.kept; by_name[std::string(reinterpret_cast<const char *>(raw + q + r.R.name_at), r.R.n_name)].push_back((uint32_t)ord); }
    else if (r.R.flag & o.filter) ++C.filtered;
    else ++C.empty;
    V.push_back(r);
    q += len;
  }
  for (const auto &kv : by_name) {
    const std::vector<uint32_t> &v = kv.second;
    if (v.size() == 2 && fastq_is_pair(V[v[0]].R.cls, V[v[1]].R.cls)) { V[v[0]].mate = v[1]; V[v[1]].mate = v[0]; }
  }
  auto put = [&](std::vector<uint8_t> &out, const Rec &r) {
    const size_t at = out.size();
    out.resize(at + (size_t)r.R.len);
    fastq_entry_bytes(raw + r.at, r.R, 0, r.R.len, out.data() + at);
  };
  for (uint32_t i = 0; i < V.size(); ++i) {
    if (!V[i].R.cls) continue;
    if (V[i].mate == 0xffffffffu) {
      ++C.singles;
      if (o.singles) put(stream[FASTQ_S], V[i]); else ++C.singles_unwritten;
    } else if (i < V[i].mate) {
      ++C.pairs;
      const Rec &a = V[i].R.cls & FASTQ_C_R1 ? V[i] : V[V[i].mate], &b = V[i].R.cls & FASTQ_C_R1 ? V[V[i].mate] : V[i];
      put(stream[FASTQ_P1], a);
      put(stream[o.interleaved ? FASTQ_P1 : FASTQ_P2], b);
    }
  }
  if (counts) *counts = C;
  return -1;
}

}  // namespace strl
