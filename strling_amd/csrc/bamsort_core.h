// bamsort_core.h -- the rule of `strling sort` (coordinate order of a BAM), one source for the host path (cli/sort_cli.cpp), the
// device path (bamsort.hip), the library's host entries (strl_bamsort_key / strl_bamsort_header) and the stand-alone test
// program (tests/emu/bamsort_core_main.cpp): the key of a record, the output's header, and where the records that touch a piece
// [lo, hi) of the output stream lie.  DESIGN section 24.
//
//   key    = tid_u << 33 | (uint32)(pos + 1) << 1 | reverse strand,  tid_u = refID < 0 ? n_ref : refID
//            -> (reference, position, forward before reverse), records without a reference last; a STABLE sort keeps the
//            input order among equal keys.  This is the comparator samtools documents for `sort` without -n / -t.
//   stream = header bytes || records in sorted order, each with its block_size word; cut into BGZF members of 0xFF00 bytes.
#pragma once
#include <stdint.h>
#include <string.h>
#if defined(__HIPCC__)
#define BSORT_HD __host__ __device__
#else
#define BSORT_HD
#endif
#include <string>
#include <vector>

namespace strl {

constexpr uint32_t BSORT_BLK = 0xFF00;                   // input bytes of a BGZF member of the output (write_bgzf's cut)
constexpr uint64_t BSORT_MAX_RECORDS = 0xfffffffeull;    // radix_sort_pairs counts in 32 bits
constexpr uint32_t BSORT_KEY_BYTES = 20;                 // bytes behind block_size the key is made from
constexpr uint32_t BSORT_MIN_REC = 36;                   // block_size word + the 32 fixed bytes of a record

BSORT_HD inline uint32_t bsort_ld32(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

// bits needed to write x (0 for 0)
BSORT_HD inline int bsort_bits(uint32_t x) { int b = 0; while (x) { ++b; x >>= 1; } return b; }
// the key bits that can differ: what the sort runs over
BSORT_HD inline int bsort_key_bits(int32_t n_ref) { return 33 + bsort_bits((uint32_t)n_ref); }

// key of the record whose first 20 bytes behind block_size are `body` (refID, pos, l_read_name, mapq, bin, n_cigar_op, flag, l_seq).
// false: the refID is not one of the header's (refID >= n_ref or refID < -1); *key is then the key of a record without a reference
BSORT_HD inline bool bsort_key(const uint8_t *body, int32_t n_ref, uint64_t *key) {
  const int32_t tid = (int32_t)bsort_ld32(body), pos = (int32_t)bsort_ld32(body + 4);
  const uint32_t flag = (uint32_t)body[14] | (uint32_t)body[15] << 8;
  const bool ok = tid >= -1 && tid < n_ref;
  const uint64_t tid_u = (tid < 0 || !ok) ? (uint64_t)(uint32_t)n_ref : (uint64_t)(uint32_t)tid;
  *key = tid_u << 33 | (uint64_t)(uint32_t)(pos + 1) << 1 | (uint64_t)(flag >> 4 & 1u);
  return ok;
}

// ---- pieces of the output stream -------------------------------------------------------------------------------------------
// off[0 .. n]: off[j] = stream offset of the record of rank j, off[n] = the stream's end (ascending; every record has bytes).
// The records that touch [lo, hi), lo < hi: ranks [bsort_first_touch, bsort_end_touch).
BSORT_HD inline uint64_t bsort_first_touch(const uint64_t *off, uint64_t n, uint64_t lo) {      // the first j with off[j + 1] > lo (n: none)
  uint64_t a = 0, b = n;
  while (a < b) { const uint64_t m = a + (b - a) / 2; if (off[m + 1] > lo) b = m; else a = m + 1; }
  return a;
}
BSORT_HD inline uint64_t bsort_end_touch(const uint64_t *off, uint64_t n, uint64_t hi) {        // the first j with off[j] >= hi (n: none)
  uint64_t a = 0, b = n;
  while (a < b) { const uint64_t m = a + (b - a) / 2; if (off[m] >= hi) b = m; else a = m + 1; }
  return a;
}
// the part of a record [beg, end) of the stream that lies inside the piece: bytes to skip at its start, where they go in the
// piece, how many
struct BsortPart { uint64_t skip, dst, bytes; };
BSORT_HD inline BsortPart bsort_part(uint64_t beg, uint64_t end, uint64_t lo, uint64_t hi) {
  const uint64_t a = beg > lo ? beg : lo, b = end < hi ? end : hi;
  BsortPart p;
  p.skip = a - beg; p.dst = a - lo; p.bytes = b > a ? b - a : 0;
  return p;
}

// ---- windows of the output stream (`sort --windowed`) --------------------------------------------------------------------------------
// A file larger than device memory: pass 0 keeps key and length of every record and sorts; dest[ordinal] = the record's first byte
// in the stream.  Every later pass reads the input again and places the records that touch the window [lo, hi) of the stream
// straight where they belong; the window is then a finished piece of the stream.
//   W = max(piece_bytes, limit_bytes / piece_bytes * piece_bytes),  n_windows = ceil(stream_bytes / W),  window w = [w W, min(stream_bytes, (w + 1) W))
// piece_bytes is a multiple of 0xFF00, so every window starts on a member boundary and no piece straddles two windows.
struct BsortWindowPlan { uint64_t window_bytes, n_windows; };
BSORT_HD inline BsortWindowPlan bsort_window_plan(uint64_t stream_bytes, uint64_t limit_bytes, uint64_t piece_bytes) {
  if (!piece_bytes) piece_bytes = BSORT_BLK;
  const uint64_t whole = limit_bytes / piece_bytes * piece_bytes;
  BsortWindowPlan p;
  p.window_bytes = whole > piece_bytes ? whole : piece_bytes;
  p.n_windows = stream_bytes / p.window_bytes + (stream_bytes % p.window_bytes ? 1u : 0u);      // (no sum that could wrap)
  return p;
}
// the scatter's rule for one record: dest = its first byte in the stream and len = its 4 + block_size, both from pass 0; bs_now = the
// block_size word read in this pass -> the part inside the window.  false: bs_now + 4 != len, the file is not the one pass 0 read
BSORT_HD inline bool bsort_scatter_part(uint64_t dest, uint32_t len, uint32_t bs_now, uint64_t lo, uint64_t hi, BsortPart *part) {
  if ((uint64_t)bs_now + 4u != (uint64_t)len) return false;
  *part = bsort_part(dest, dest + len, lo, hi);
  return true;
}
// header bytes inside the window, and the window's completeness: the bytes the scatter placed and those of the header fill it
BSORT_HD inline uint64_t bsort_window_header(uint64_t header_bytes, uint64_t lo, uint64_t hi) {
  return lo < header_bytes ? (hi < header_bytes ? hi : header_bytes) - lo : 0;
}
BSORT_HD inline bool bsort_window_complete(uint64_t placed, uint64_t header_bytes, uint64_t lo, uint64_t hi) {
  return hi >= lo && placed + bsort_window_header(header_bytes, lo, hi) == hi - lo;
}

// ---- virtual offsets of the output (`sort --write-index`) ------------------------------------------------------------------------
// The stream is cut into members of exactly BSORT_BLK bytes, so where a stream offset lies in the file is arithmetic and one load:
// member_off[0 .. n_members] = file offset of every member, the last entry the EOF block's; n_members = ceil(stream_bytes / 0xFF00).
//   voff(s) = member_off[s / 0xFF00] << 16 | s % 0xFF00,  0 <= s < stream_bytes;   voff(stream_bytes) = member_off[n_members] << 16
// A byte on a member boundary belongs to the member that starts there, and the stream's end to the EOF block (offset 0) -- whether
// or not the stream is a multiple of 0xFF00 long: what bai_voff (bamindex.hip) gives for the byte behind the last record of a file,
// and what htslib's bgzf_tell gives there, so the index is `strling bamindex OUT.bam`'s byte for byte.  (bamio.write_bai names the
// last member and its ISIZE instead when the last member is short: the same place, as tests that compare structures see it.)
BSORT_HD inline uint64_t bsort_n_members(uint64_t stream_bytes) { return (stream_bytes + BSORT_BLK - 1) / BSORT_BLK; }
BSORT_HD inline uint64_t bsort_voff(const uint64_t *member_off, uint64_t n_members, uint64_t stream_bytes, uint64_t s) {
  if (s >= stream_bytes) return member_off[n_members] << 16;      // (s > stream_bytes is not asked for; nothing behind the table is read)
  const uint64_t k = s / BSORT_BLK;                                // < n_members
  return member_off[k] << 16 | (s - k * BSORT_BLK);
}
// a table the rule can use: n_members as the stream's length gives it, the offsets ascending, each below 2^48
inline bool bsort_member_table_ok(const uint64_t *member_off, uint64_t n_members, uint64_t stream_bytes) {
  if (!member_off || n_members != bsort_n_members(stream_bytes)) return false;
  for (uint64_t k = 0; k <= n_members; ++k)
    if (member_off[k] >> 48 || (k && member_off[k] <= member_off[k - 1])) return false;
  return true;
}
// the BGZF members in p[0, n), which the writer puts at file offset `at`: each one's file offset is appended to member_off (BSIZE
// at byte 16 of a member: zlib's members and the device compressor's alike).  -> the file offset behind them; false: not whole members
inline bool bsort_walk_members(const uint8_t *p, size_t n, uint64_t *at, std::vector<uint64_t> &member_off) {
  size_t o = 0;
  while (o < n) {
    if (n - o < 18 || p[o] != 0x1f || p[o + 1] != 0x8b) return false;
    const size_t bsize = ((size_t)p[o + 16] | (size_t)p[o + 17] << 8) + 1;
    if (bsize < 26 || bsize > n - o) return false;
    member_off.push_back(*at + o);
    o += bsize;
  }
  *at += n;
  return true;
}

// what the index step reads of a finished sort (bamsort.hip hands it to bamindex.hip): device pointers
constexpr int BSORT_SLAB_SHIFT = 40;                         // src = slab << 40 | offset in the slab
constexpr uint64_t BSORT_SLAB_MASK = (1ull << BSORT_SLAB_SHIFT) - 1ull;
struct BsortView {
  const uint64_t *off, *src;   // off[0 .. n]: stream offsets in sorted order; src[ordinal]
  const uint32_t *perm, *len;  // perm[rank] = ordinal; len[ordinal] = 4 + block_size
  uint8_t *const *slab;        // [n_slabs] bases
  const uint64_t *slab_used;   // [n_slabs] bytes of records in each
  uint32_t n_slabs;
  int32_t n_ref;
  uint64_t n_records, stream_bytes;
};

// ---- the header (host) ------------------------------------------------------------------------------------------------------------
// The text of the output: the input's, with the @HD line's SO: set to coordinate (added at the end of the line when the line has
// none), GO: and SS: dropped, the line's other fields and every other line byte for byte; a text whose first line is not @HD
// gets "@HD\tVN:1.6\tSO:coordinate\n" in front.
inline std::string bsort_header_text(const std::string &text) {
  const bool hd = text.size() >= 3 && !text.compare(0, 3, "@HD") && (text.size() == 3 || text[3] == '\t' || text[3] == '\n');
  if (!hd) return "@HD\tVN:1.6\tSO:coordinate\n" + text;
  size_t eol = text.find('\n');
  const bool has_nl = eol != std::string::npos;
  if (!has_nl) { eol = text.size(); while (eol > 3 && text[eol - 1] == '\0') --eol; }      // (NUL padding behind a last line without \n stays behind it)
  std::string line = "@HD";
  bool so = false;
  size_t at = 3;
  while (at < eol) {                         // text[at] == '\t'
    size_t e = text.find('\t', at + 1);
    if (e == std::string::npos || e > eol) e = eol;
    const std::string f = text.substr(at + 1, e - at - 1);
    if (!f.compare(0, 3, "SO:")) { if (!so) line += "\tSO:coordinate"; so = true; }
    else if (f.compare(0, 3, "GO:") && f.compare(0, 3, "SS:")) line += "\t" + f;
    at = e;
  }
  if (!so) line += "\tSO:coordinate";
  return line + text.substr(eol);
}

// The output's header bytes (magic, l_text, text, n_ref, the reference list) from the input's: the text by the rule above,
// l_text to match, the binary reference list byte for byte.  `in` may hold bytes behind the header (records); *used = bytes of the
// input's header.  false: `err` says what is wrong with the input's header.
inline bool bsort_header(const uint8_t *in, size_t in_bytes, std::vector<uint8_t> &out, int32_t *n_ref, size_t *used, std::string &err) {
  if (in_bytes < 12 || memcmp(in, "BAM\1", 4)) { err = "not a BAM header (magic)"; return false; }
  const uint32_t l_text = bsort_ld32(in + 4);
  if ((uint64_t)l_text + 12 > in_bytes) { err = "BAM header: l_text reaches past the bytes given"; return false; }
  size_t at = 8 + (size_t)l_text;
  const int32_t nr = (int32_t)bsort_ld32(in + at);
  if (nr < 0) { err = "BAM header: negative n_ref"; return false; }
  const size_t refs = at;
  at += 4;
  for (int32_t t = 0; t < nr; ++t) {
    if (at + 4 > in_bytes) { err = "BAM header: the reference list reaches past the bytes given"; return false; }
    const uint32_t l_name = bsort_ld32(in + at);
    if ((uint64_t)at + 8 + l_name > in_bytes) { err = "BAM header: the reference list reaches past the bytes given"; return false; }
    at += 8 + (size_t)l_name;
  }
  const std::string text = bsort_header_text(std::string(reinterpret_cast<const char *>(in + 8), l_text));
  if (text.size() > 0x7fffffffu) { err = "BAM header: text of more than 2^31 bytes"; return false; }
  out.clear();
  out.reserve(8 + text.size() + (at - refs));
  out.insert(out.end(), in, in + 4);
  const uint32_t lt = (uint32_t)text.size();
  for (int k = 0; k < 4; ++k) out.push_back((uint8_t)(lt >> (8 * k)));
  out.insert(out.end(), text.begin(), text.end());
  out.insert(out.end(), in + refs, in + at);
  if (n_ref) *n_ref = nr;
  if (used) *used = at;
  return true;
}

}  // namespace strl
