// bamindex_host_main.cpp -- the host index builder (csrc/bamindex_host.cpp) and the rules it shares with the device
// (csrc/bamindex_core.h, the virtual-offset rule and the member walk of csrc/bamsort_core.h) as a stand-alone program, built with
// -fsanitize=address,undefined by tests/test_sort_index.py.
//   bamindex_host_main                                   self-checks; prints "all cases passed"
//   bamindex_host_main STREAM MEMBERS OUT MIN_SHIFT      STREAM: the inflated bytes of a coordinate-sorted BAM; MEMBERS: the file offset
//                                                        of each of its members as little-endian 64-bit words, the EOF block's last;
//                                                        OUT: the index's bytes (a .bai for MIN_SHIFT -1, else the CSI payload).
//                                                        A refusal: its words on stderr, exit 1.
// Every record is handed over from a heap copy exact to the byte, so a read behind a record's end is one the sanitizer sees.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "../../strling_amd/csrc/bamindex_host.h"
#include "../../strling_amd/csrc/bamsort_core.h"

using namespace strl;

static int fails = 0;
#define EXPECT(c) do { if (!(c)) { fprintf(stderr, "line %d: %s\n", __LINE__, #c); ++fails; } } while (0)

static bool slurp(const char *path, std::vector<uint8_t> &v) {
  FILE *f = fopen(path, "rb");
  if (!f) return false;
  uint8_t b[65536];
  size_t n;
  while ((n = fread(b, 1, sizeof b, f)) > 0) v.insert(v.end(), b, b + n);
  fclose(f);
  return true;
}

static std::vector<uint8_t> record(int32_t tid, int32_t pos, uint16_t flag, const std::vector<uint32_t> &cigar, uint32_t l_seq) {
  const std::string name = "r";
  std::vector<uint8_t> r(36 + name.size() + 1 + 4 * cigar.size() + (l_seq + 1) / 2 + l_seq, 0);
  auto p32 = [&](size_t at, uint32_t v) { memcpy(r.data() + at, &v, 4); };
  p32(0, (uint32_t)r.size() - 4); p32(4, (uint32_t)tid); p32(8, (uint32_t)pos);
  r[12] = (uint8_t)(name.size() + 1);
  const uint16_t nc = (uint16_t)cigar.size();
  memcpy(r.data() + 16, &nc, 2); memcpy(r.data() + 18, &flag, 2);
  p32(20, l_seq); p32(24, (uint32_t)-1); p32(28, (uint32_t)-1);
  memcpy(r.data() + 36, name.c_str(), name.size() + 1);
  if (!cigar.empty()) memcpy(r.data() + 36 + name.size() + 1, cigar.data(), 4 * cigar.size());
  return r;
}

static void self_checks() {
  // the rule at the edges: a boundary byte belongs to the member that starts there, the stream's end to the EOF block
  const std::vector<uint64_t> tab = {0, 100, 250, 300};               // three members and the EOF block
  const uint64_t B = BSORT_BLK;
  EXPECT(bsort_n_members(0) == 0 && bsort_n_members(1) == 1 && bsort_n_members(B) == 1 && bsort_n_members(B + 1) == 2);
  EXPECT(bsort_member_table_ok(tab.data(), 3, 3 * B) && bsort_member_table_ok(tab.data(), 3, 2 * B + 1));
  EXPECT(!bsort_member_table_ok(tab.data(), 3, 2 * B) && !bsort_member_table_ok(tab.data(), 2, 3 * B) && !bsort_member_table_ok(nullptr, 0, 0));
  const std::vector<uint64_t> down = {0, 250, 100, 300}, wide = {0, 100, 250, 1ull << 48}, same = {0, 100, 100, 300};
  EXPECT(!bsort_member_table_ok(down.data(), 3, 3 * B) && !bsort_member_table_ok(wide.data(), 3, 3 * B) && !bsort_member_table_ok(same.data(), 3, 3 * B));
  EXPECT(bsort_voff(tab.data(), 3, 3 * B, 0) == 0 && bsort_voff(tab.data(), 3, 3 * B, B - 1) == (B - 1));
  EXPECT(bsort_voff(tab.data(), 3, 3 * B, B) == (100ull << 16) && bsort_voff(tab.data(), 3, 3 * B, 2 * B + 5) == ((250ull << 16) | 5));
  EXPECT(bsort_voff(tab.data(), 3, 3 * B, 3 * B) == (300ull << 16));
  EXPECT(bsort_voff(tab.data(), 3, 2 * B + 9, 2 * B + 8) == ((250ull << 16) | 8) && bsort_voff(tab.data(), 3, 2 * B + 9, 2 * B + 9) == (300ull << 16));      // the end: the EOF block
  const std::vector<uint64_t> none = {0};
  EXPECT(bsort_member_table_ok(none.data(), 0, 0) && bsort_voff(none.data(), 0, 0, 0) == 0);
  // the walk: two members of 30 and 26 bytes, then bytes that are none
  std::vector<uint8_t> m(56, 0);
  m[0] = 0x1f; m[1] = 0x8b; m[16] = 29; m[30] = 0x1f; m[31] = 0x8b; m[46] = 25;
  std::vector<uint64_t> got;
  uint64_t at = 1000;
  EXPECT(bsort_walk_members(m.data(), m.size(), &at, got) && at == 1056 && got == (std::vector<uint64_t>{1000, 1030}));
  std::vector<uint8_t> cut(m.begin(), m.begin() + 50);
  got.clear(); at = 0;
  EXPECT(!bsort_walk_members(cut.data(), cut.size(), &at, got));
  // a record whose CIGAR does not lie inside its length is not walked
  BaiRec r;
  std::vector<uint8_t> rec = record(0, 100, 0, {(50u << 4) | 0u, (1000u << 4) | 3u, (50u << 4) | 0u}, 100);
  EXPECT(bai_read_bounded(rec.data(), (uint32_t)rec.size(), r) && r.tid == 0 && r.pos == 100 && r.end == 1200);
  { std::vector<uint8_t> exact(rec.begin(), rec.begin() + 36 + 2 + 8); EXPECT(!bai_read_bounded(exact.data(), (uint32_t)exact.size(), r)); }
  { std::vector<uint8_t> exact(rec.begin(), rec.begin() + 35); EXPECT(!bai_read_bounded(exact.data(), (uint32_t)exact.size(), r)); }
  EXPECT(bai_reg2bin(0, 1) == 4681 && bai_reg2bin(16383, 16385) == 585 && bai_reg2bin((1 << 26) - 1, (1 << 26) + 1) == 0);
  for (int32_t b : {0, 16383, 16384, 1 << 20, (1 << 29) - 40})
    for (int32_t l : {1, 40, 20000, 1 << 21})
      if ((int64_t)b + l <= (1 << 29)) EXPECT(csi_reg2bin(b, b + l, 14, 5) == bai_reg2bin(b, b + l));
  // three records, two references: bins, linear index, pseudo-bins, n_no_coor; a bin left and entered again is two chunks
  const int32_t l_ref[2] = {1 << 20, 1 << 20};
  HostIndex H;
  std::string err;
  EXPECT(H.begin(2, l_ref, -1, -1, err));
  const std::vector<uint8_t> a = record(0, 10, 0, {(30u << 4)}, 30), b = record(0, 11, 0, {(10u << 4), (40000u << 4) | 3u, (10u << 4)}, 20), c = record(0, 12, 4, {}, 30),
                             d = record(-1, -1, 4, {}, 30);
  uint64_t s = 500;
  for (const auto *x : {&a, &b, &c, &d}) { std::vector<uint8_t> copy(*x); H.add(copy.data(), (uint32_t)copy.size(), s << 16, (s + 1) << 16, s, s + 1); ++s; }
  std::vector<uint8_t> bytes;
  EXPECT(H.finish(bytes, err) == 0 && H.n_records == 4 && H.n_no_coor == 1 && H.n_runs == 4 && H.n_chunks == 3);
  EXPECT(bytes.size() > 8 && !memcmp(bytes.data(), "BAI\1", 4));
  // refusals: their words
  EXPECT(H.begin(2, l_ref, -1, -1, err));
  { std::vector<uint8_t> copy = record(0, -1, 0, {(30u << 4)}, 30); H.add(copy.data(), (uint32_t)copy.size(), 0, 1, 0, 1); }
  EXPECT(H.finish(bytes, err) == STRL_ERR_FORMAT && err == "record 0 has a reference but a negative position; not indexed");
  EXPECT(H.begin(2, l_ref, -1, -1, err));
  { std::vector<uint8_t> x = record(0, 50, 0, {(30u << 4)}, 30), y = record(0, 49, 0, {(30u << 4)}, 30); H.add(x.data(), (uint32_t)x.size(), 0, 1, 0, 1); H.add(y.data(), (uint32_t)y.size(), 1, 2, 1, 2); }
  EXPECT(H.finish(bytes, err) == STRL_ERR_FORMAT && err.find("not coordinate sorted: record 1 ") != std::string::npos);
  EXPECT(!H.begin(2, l_ref, 7, -1, err) && !H.begin(2, l_ref, 25, -1, err) && H.begin(2, l_ref, 8, -1, err) && H.begin(0, nullptr, 14, -1, err));
}

int main(int argc, char **argv) {
  if (argc == 1) {
    self_checks();
    if (fails) { fprintf(stderr, "%d checks failed\n", fails); return 1; }
    puts("all cases passed");
    return 0;
  }
  if (argc != 5) { fprintf(stderr, "usage: bamindex_host_main [STREAM MEMBERS OUT MIN_SHIFT]\n"); return 2; }
  std::vector<uint8_t> u, tabb;
  if (!slurp(argv[1], u) || !slurp(argv[2], tabb) || tabb.size() % 8 || tabb.empty()) { fprintf(stderr, "cannot read the inputs\n"); return 2; }
  std::vector<uint64_t> tab(tabb.size() / 8);
  memcpy(tab.data(), tabb.data(), tabb.size());
  const uint64_t nm = tab.size() - 1;
  if (!bsort_member_table_ok(tab.data(), nm, u.size())) { fprintf(stderr, "the member table does not match the stream\n"); return 2; }
  if (u.size() < 12) return 2;
  size_t at = 8 + (size_t)bsort_ld32(u.data() + 4);
  const int32_t n_ref = (int32_t)bsort_ld32(u.data() + at);
  at += 4;
  std::vector<int32_t> l_ref;
  for (int32_t t = 0; t < n_ref; ++t) { const uint32_t ln = bsort_ld32(u.data() + at); l_ref.push_back((int32_t)bsort_ld32(u.data() + at + 4 + ln)); at += 8 + ln; }
  l_ref.push_back(0);
  HostIndex H;
  std::string err;
  if (!H.begin(n_ref, l_ref.data(), atoi(argv[4]), -1, err)) { fprintf(stderr, "%s\n", err.c_str()); return 2; }
  while (at < u.size()) {
    const uint64_t len = 4 + (uint64_t)bsort_ld32(u.data() + at);
    if (len > u.size() - at) { fprintf(stderr, "the stream ends inside a record\n"); return 2; }
    std::vector<uint8_t> copy(u.begin() + (ptrdiff_t)at, u.begin() + (ptrdiff_t)(at + len));      // exact to the byte
    H.add(copy.data(), (uint32_t)len, bsort_voff(tab.data(), nm, u.size(), at), bsort_voff(tab.data(), nm, u.size(), at + len), at, at + len);
    at += len;
  }
  std::vector<uint8_t> bytes;
  const int rc = H.finish(bytes, err);
  if (rc) { fprintf(stderr, "%s (status %d)\n", err.c_str(), rc); return 1; }
  FILE *f = fopen(argv[3], "wb");
  if (!f || fwrite(bytes.data(), 1, bytes.size(), f) != bytes.size() || fclose(f)) { fprintf(stderr, "cannot write %s\n", argv[3]); return 2; }
  return 0;
}
