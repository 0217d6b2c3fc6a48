// bamsort_core_main.cpp -- the rule of `strling sort` (strling_amd/csrc/bamsort_core.h) as a stand-alone program, built with
// -fsanitize=address,undefined by tests/test_sort_bam_cases.py and run directly.
//   bamsort_core_main                      the built-in checks: keys at their edges, header texts, the piece arithmetic against a
//                                          byte-by-byte walk with offsets around 2^32
//   bamsort_core_main IN.raw OUT PIECE     IN.raw = the inflated bytes of a BAM; OUT = the sorted stream, assembled in pieces of
//                                          PIECE bytes, every piece in a buffer exact to the byte
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <numeric>
#include <string>
#include <vector>
#include "../../strling_amd/csrc/bamsort_core.h"

using namespace strl;

static int g_bad = 0;
#define EXPECT(c) do { if (!(c)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); ++g_bad; } } while (0)

static std::vector<uint8_t> body20(int32_t tid, int32_t pos, uint16_t flag) {
  std::vector<uint8_t> b(20, 0);                      // exactly the 20 bytes the key may read
  memcpy(b.data(), &tid, 4); memcpy(b.data() + 4, &pos, 4); memcpy(b.data() + 14, &flag, 2);
  return b;
}
static uint64_t key_of(int32_t tid, int32_t pos, uint16_t flag, int32_t n_ref, bool *ok = nullptr) {
  uint64_t k = 0;
  const std::vector<uint8_t> b = body20(tid, pos, flag);
  const bool r = bsort_key(b.data(), n_ref, &k);
  if (ok) *ok = r;
  return k;
}

static void check_keys() {
  EXPECT(key_of(0, 0, 0, 3) == 2);
  EXPECT(key_of(0, 0, 16, 3) == 3);
  EXPECT(key_of(0, -1, 0, 3) == 0);                                      // pos -1 on a placed record sorts first within its reference
  EXPECT(key_of(2, 0x7ffffffe, 16, 3) == (2ull << 33 | 0xffffffffull));  // the largest position: the field is full, the reference untouched
  EXPECT(key_of(-1, -1, 4, 3) == 3ull << 33);                            // no reference: behind every reference
  EXPECT(key_of(-1, 12345, 0, 0) > key_of(-1, -1, 0, 0));
  EXPECT(key_of(1, -1, 0, 3) > key_of(0, 0x7ffffffe, 16, 3));
  EXPECT(key_of(0, 5, 0x10 | 0x400, 3) == key_of(0, 5, 16, 3));           // only the strand bit of the flag
  bool ok = true;
  key_of(3, 0, 0, 3, &ok); EXPECT(!ok);
  key_of(-2, 0, 0, 3, &ok); EXPECT(!ok);
  key_of(0, 0, 0, 0, &ok); EXPECT(!ok);
  key_of(-1, 0, 0, 0, &ok); EXPECT(ok);
  key_of(0x7ffffffe, 0, 0, 0x7fffffff, &ok); EXPECT(ok);
  EXPECT(key_of(0x7ffffffe, 0x7ffffffe, 16, 0x7fffffff) < key_of(-1, -1, 0, 0x7fffffff));      // 64 bits hold the widest key
  const int want[][2] = {{0, 33}, {1, 34}, {2, 35}, {3, 35}, {4, 36}, {255, 41}, {256, 42}, {0x7fffffff, 64}};
  for (auto &w : want) EXPECT(bsort_key_bits(w[0]) == w[1]);
  for (int32_t n_ref : {1, 3, 4, 255, 256}) EXPECT(key_of(-1, 0x7ffffffe, 16, n_ref) >> bsort_key_bits(n_ref) == 0);
}

static void check_header_texts() {
  EXPECT(bsort_header_text("") == "@HD\tVN:1.6\tSO:coordinate\n");
  EXPECT(bsort_header_text("@SQ\tSN:a\tLN:5\n") == "@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:a\tLN:5\n");
  EXPECT(bsort_header_text("@HD\tVN:1.5\tSO:unsorted\tGO:query\n@SQ\tSN:a\tLN:5\n") == "@HD\tVN:1.5\tSO:coordinate\n@SQ\tSN:a\tLN:5\n");
  EXPECT(bsort_header_text("@HD\tVN:1.6\n@CO\tSO:unsorted\n") == "@HD\tVN:1.6\tSO:coordinate\n@CO\tSO:unsorted\n");
  EXPECT(bsort_header_text("@HD\tVN:1.6\tSS:x\tXY:z\tSO:queryname") == "@HD\tVN:1.6\tXY:z\tSO:coordinate");
  EXPECT(bsort_header_text("@HD") == "@HD\tSO:coordinate");
  EXPECT(bsort_header_text("@HD\n") == "@HD\tSO:coordinate\n");
  EXPECT(bsort_header_text(std::string("@HD\tVN:1.6\0\0", 12)) == std::string("@HD\tVN:1.6\tSO:coordinate\0\0", 26));
  EXPECT(bsort_header_text("@HDX\tVN:1\n") == "@HD\tVN:1.6\tSO:coordinate\n@HDX\tVN:1\n");
  // truncated headers are refused, never read past
  const char full[] = "BAM\1\4\0\0\0@CO\n\1\0\0\0\2\0\0\0a\0\7\0\0\0";
  for (size_t n = 0; n < sizeof full - 1; ++n) {
    std::vector<uint8_t> in(full, full + n), out;
    std::string err;
    EXPECT(!bsort_header(in.data(), in.size(), out, nullptr, nullptr, err));
  }
  std::vector<uint8_t> in(full, full + sizeof full - 1), out;
  std::string err;
  int32_t n_ref = -1;
  size_t used = 0;
  EXPECT(bsort_header(in.data(), in.size(), out, &n_ref, &used, err) && n_ref == 1 && used == in.size());
  const std::string text = "@HD\tVN:1.6\tSO:coordinate\n@CO\n";
  EXPECT(out.size() == 8 + text.size() + 14 && bsort_ld32(out.data() + 4) == text.size() && !memcmp(out.data() + 8, text.data(), text.size()) &&
         !memcmp(out.data() + 8 + text.size(), full + 12, 14));
}

// the piece arithmetic against a walk over every byte of the stream
static void check_pieces() {
  uint32_t seed = 12345;
  auto rnd = [&] { seed = seed * 1664525u + 1013904223u; return seed >> 8; };
  for (uint64_t base : {0ull, 37ull, (1ull << 32) - 100ull}) {
    const uint64_t n = 40;
    std::vector<uint64_t> off(n + 1);
    off[0] = base;
    for (uint64_t j = 0; j < n; ++j) off[j + 1] = off[j] + 36 + rnd() % 50;
    const uint64_t end = off[n];
    std::vector<uint64_t> cuts = {0, 1, base ? base - 1 : 0, base, base + 1, off[1] - 1, off[1], off[1] + 1, off[7], off[7] + 3, off[n - 1], end - 1, end};
    for (uint64_t lo : cuts)
      for (uint64_t hi : cuts) {
        if (lo >= hi || hi > end) continue;
        const uint64_t a = bsort_first_touch(off.data(), n, lo), b = bsort_end_touch(off.data(), n, hi);
        uint64_t covered = 0;
        for (uint64_t j = 0; j < n; ++j) {
          const bool touches = off[j + 1] > lo && off[j] < hi;
          EXPECT(touches == (j >= a && j < b));
          if (!touches) continue;
          const BsortPart p = bsort_part(off[j], off[j + 1], lo, hi);
          EXPECT(p.bytes > 0 && off[j] + p.skip >= lo && off[j] + p.skip + p.bytes <= hi && off[j] + p.skip - lo == p.dst && p.skip + p.bytes <= off[j + 1] - off[j]);
          EXPECT(p.skip == 0 || p.dst == 0);
          covered += p.bytes;
        }
        const uint64_t want = hi > base ? hi - std::max(lo, base) : 0;      // the bytes of the piece that lie behind the header
        EXPECT(covered == want);
      }
    EXPECT(bsort_first_touch(off.data(), 0, 5) == 0 && bsort_end_touch(off.data(), 0, 5) == 0);
  }
}

static int sort_file(const char *in_path, const char *out_path, uint64_t piece) {
  FILE *f = fopen(in_path, "rb");
  if (!f) { perror(in_path); return 2; }
  std::vector<uint8_t> raw;
  uint8_t tmp[65536];
  for (size_t got; (got = fread(tmp, 1, sizeof tmp, f)) > 0;) raw.insert(raw.end(), tmp, tmp + got);
  fclose(f);
  std::vector<uint8_t> header;
  std::string err;
  int32_t n_ref = 0;
  size_t used = 0;
  if (!bsort_header(raw.data(), raw.size(), header, &n_ref, &used, err)) { fprintf(stderr, "%s\n", err.c_str()); return 3; }
  std::vector<uint64_t> at, key;
  for (size_t q = used; q < raw.size();) {
    if (raw.size() - q < BSORT_MIN_REC) return 4;
    const uint32_t bs = bsort_ld32(raw.data() + q);
    if (bs < 32 || bs > raw.size() - q - 4) return 4;
    uint64_t k;
    if (!bsort_key(raw.data() + q + 4, n_ref, &k)) { fprintf(stderr, "record %zu: refID\n", at.size()); return 5; }
    at.push_back(q); key.push_back(k);
    q += 4 + (size_t)bs;
  }
  const size_t n = at.size();
  std::vector<uint32_t> perm(n);
  std::iota(perm.begin(), perm.end(), 0u);
  std::stable_sort(perm.begin(), perm.end(), [&](uint32_t a, uint32_t b) { return key[a] < key[b]; });
  std::vector<uint64_t> off(n + 1);
  uint64_t run = header.size();
  for (size_t j = 0; j < n; ++j) { off[j] = run; run += 4 + (uint64_t)bsort_ld32(raw.data() + at[perm[j]]); }
  off[n] = run;
  FILE *o = fopen(out_path, "wb");
  if (!o) { perror(out_path); return 2; }
  for (uint64_t lo = 0; lo < run; lo += piece) {
    const uint64_t hi = std::min(run, lo + piece);
    std::vector<uint8_t> buf((size_t)(hi - lo));                         // exact to the byte
    if (lo < header.size()) memcpy(buf.data(), header.data() + lo, (size_t)(std::min<uint64_t>(hi, header.size()) - lo));
    const uint64_t a = bsort_first_touch(off.data(), n, lo), b = bsort_end_touch(off.data(), n, hi);
    for (uint64_t j = a; j < b; ++j) {
      const BsortPart p = bsort_part(off[j], off[j + 1], lo, hi);
      memcpy(buf.data() + p.dst, raw.data() + at[perm[j]] + p.skip, (size_t)p.bytes);
    }
    if (fwrite(buf.data(), 1, buf.size(), o) != buf.size()) return 2;
  }
  return fclose(o) ? 2 : 0;
}

int main(int argc, char **argv) {
  if (argc == 4) return sort_file(argv[1], argv[2], strtoull(argv[3], nullptr, 10));
  check_keys();
  check_header_texts();
  check_pieces();
  if (g_bad) { printf("%d checks failed\n", g_bad); return 1; }
  printf("all cases passed\n");
  return 0;
}
