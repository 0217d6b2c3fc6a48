// fastq_core_main.cpp -- the rule of `strling fastq` (strling_amd/csrc/fastq_core.h) as a stand-alone program, built plainly and with
// -fsanitize=address,undefined by tests/test_fastq_cases.py and run directly.
//   fastq_core_main                                     the built-in checks: codes, complements, qualities, classes, lengths
//   fastq_core_main IN.raw OUT F N V INTERLEAVED SINGLES IN.raw = the inflated bytes of a BAM.  Every record is copied into a buffer of
//                                                       its own, exact to the byte, and fastq_entry_bytes is run for EVERY window
//                                                       (first, count) of its entry, into a buffer of exactly `count` bytes, against
//                                                       the whole entry.  Then fastq_host over the records (a buffer exact to the
//                                                       byte): OUT.p1, OUT.p2, OUT.s, and on stdout "counts K F E P S U" and
//                                                       "windows N".  A refused record: exit 3 and "record N: why" on stderr
#include <stdio.h>
#include <stdlib.h>
#include <memory>
#include <string>
#include <vector>
#include "../../strling_amd/csrc/fastq_core.h"

using namespace strl;

static int g_bad = 0;
#define EXPECT(c) do { if (!(c)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); ++g_bad; } } while (0)

static void checks() {
  const char *codes = "=ACMGRSVTWYHKDBN";
  for (uint32_t c = 0; c < 16; ++c) EXPECT(fastq_base(c) == (uint8_t)codes[c]);
  EXPECT(fastq_complement(1) == 8 && fastq_complement(8) == 1 && fastq_complement(2) == 4 && fastq_complement(4) == 2 && fastq_complement(0) == 0 && fastq_complement(15) == 15);
  for (uint32_t c = 0; c < 16; ++c) EXPECT(fastq_complement(fastq_complement(c)) == c);
  EXPECT(fastq_base(fastq_complement(3)) == 'K' && fastq_base(fastq_complement(5)) == 'Y' && fastq_base(fastq_complement(7)) == 'B');      // M <-> K, R <-> Y, V <-> B
  EXPECT(fastq_qual(0) == '!' && fastq_qual(93) == '~' && fastq_qual(94) == '~' && fastq_qual(254) == '~' && fastq_qual(255) == '~' && fastq_qual(1) == '"');
  EXPECT(fastq_class(0x100, 5, 0x900) == 0 && fastq_class(0x800, 5, 0x900) == 0 && fastq_class(0, 0, 0x900) == 0 && fastq_class(0x100, 5, 0) == FASTQ_C_KEPT);
  EXPECT(fastq_class(0x41, 5, 0x900) == (FASTQ_C_KEPT | FASTQ_C_R1) && fastq_class(0x91, 5, 0x900) == (FASTQ_C_KEPT | FASTQ_C_R2 | FASTQ_C_REVERSE) && fastq_class(0xc0, 5, 0x900) == FASTQ_C_KEPT);
  EXPECT(fastq_is_pair(fastq_class(0x40, 1, 0), fastq_class(0x80, 1, 0)) && fastq_is_pair(fastq_class(0x80, 1, 0), fastq_class(0x40, 1, 0)));
  EXPECT(!fastq_is_pair(fastq_class(0x40, 1, 0), fastq_class(0x40, 1, 0)) && !fastq_is_pair(fastq_class(0xc0, 1, 0), fastq_class(0x80, 1, 0)) && !fastq_is_pair(fastq_class(0, 1, 0), fastq_class(0x80, 1, 0)));
  EXPECT(fastq_entry_len(5, 10, 0x40, 0) == 4 + 20 + 6 && fastq_entry_len(5, 10, 0x40, 1) == 4 + 20 + 8 && fastq_entry_len(5, 10, 0xc0, 1) == 30 && fastq_entry_len(5, 10, 0, 1) == 30);
  EXPECT(fastq_entry_len(0, 1, 0, 0) == 8 && fastq_entry_len(1, 1, 0, 0) == 8);
}

int main(int argc, char **argv) {
  if (argc == 1) {
    checks();
    if (!g_bad) puts("all cases passed");
    return g_bad ? 1 : 0;
  }
  if (argc != 8) { fputs("usage: fastq_core_main [IN.raw OUT F N V INTERLEAVED SINGLES]\n", stderr); return 2; }
  const FastqOpts o{(uint32_t)strtoul(argv[3], nullptr, 0), (uint32_t)atoi(argv[4]), (uint32_t)atoi(argv[5]), (uint32_t)atoi(argv[6]), (uint32_t)atoi(argv[7])};
  FILE *f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  fseek(f, 0, SEEK_END);
  const long size = ftell(f);
  fseek(f, 0, SEEK_SET);
  std::vector<uint8_t> all((size_t)size);
  if (size && fread(all.data(), 1, (size_t)size, f) != (size_t)size) { perror("read"); return 2; }
  fclose(f);
  // the header: magic, l_text, text, n_ref, the reference list
  if (all.size() < 12 || memcmp(all.data(), "BAM\1", 4)) { fputs("not a BAM\n", stderr); return 2; }
  size_t at = 8 + (size_t)mdup_ld32(all.data() + 4);
  const uint32_t n_ref = mdup_ld32(all.data() + at);
  at += 4;
  for (uint32_t t = 0; t < n_ref; ++t) at += 8 + (size_t)mdup_ld32(all.data() + at);
  const std::vector<uint8_t> recs(all.begin() + (long)at, all.end());              // exact to the byte: a read behind the last record is caught
  // every window of every entry
  unsigned long long windows = 0;
  for (size_t q = 0, ord = 0; q + 4 <= recs.size(); ++ord) {
    const size_t len = (size_t)mdup_ld32(recs.data() + q) + 4u;
    if (len > recs.size() - q) break;                           // (fastq_host refuses it below)
    std::unique_ptr<uint8_t[]> one(new uint8_t[len]);           // the record alone: a read outside it is caught
    memcpy(one.get(), recs.data() + q, len);
    q += len;
    FastqRec R;
    if (!fastq_rec(one.get(), len, o, &R) || !R.cls) continue;
    if (R.len != fastq_entry_len(one[12], R.l_seq, R.flag, o.suffix)) { fprintf(stderr, "record %zu: entry length\n", ord); return 1; }
    std::unique_ptr<uint8_t[]> whole(new uint8_t[R.len]);
    fastq_entry_bytes(one.get(), R, 0, R.len, whole.get());
    for (uint64_t first = 0; first < R.len; ++first)
      for (uint64_t count = 1; first + count <= R.len; ++count, ++windows) {
        std::unique_ptr<uint8_t[]> part(new uint8_t[count]);
        fastq_entry_bytes(one.get(), R, first, count, part.get());
        if (memcmp(part.get(), whole.get() + first, count)) { fprintf(stderr, "record %zu: window (%llu, %llu) differs from the entry\n", ord, (unsigned long long)first, (unsigned long long)count); return 1; }
      }
    uint8_t past[4] = {0x5a, 0x5a, 0x5a, 0x5a};                  // a window that reaches past the entry's end is cut there
    fastq_entry_bytes(one.get(), R, R.len - 1, 3, past);
    if (past[0] != '\n' || past[1] != 0x5a || past[2] != 0x5a) { fprintf(stderr, "record %zu: a window past the end wrote past the end\n", ord); return 1; }
  }
  std::vector<uint8_t> stream[3];
  FastqCounts C{};
  std::string why;
  static const uint8_t none = 0;
  const int64_t bad = fastq_host(recs.empty() ? &none : recs.data(), recs.size(), o, stream, &C, why);
  if (bad >= 0) { fprintf(stderr, "record %lld: %s\n", (long long)bad, why.c_str()); return 3; }
  const char *ext[3] = {".p1", ".p2", ".s"};
  for (int s = 0; s < 3; ++s) {
    FILE *out = fopen((std::string(argv[2]) + ext[s]).c_str(), "wb");
    if (!out) { perror(argv[2]); return 2; }
    if (!stream[s].empty() && fwrite(stream[s].data(), 1, stream[s].size(), out) != stream[s].size()) { perror("write"); return 2; }
    fclose(out);
  }
  printf("counts %llu %llu %llu %llu %llu %llu\nwindows %llu\n", (unsigned long long)C.kept, (unsigned long long)C.filtered, (unsigned long long)C.empty, (unsigned long long)C.pairs,
         (unsigned long long)C.singles, (unsigned long long)C.singles_unwritten, windows);
  return 0;
}
