// markdup_core_main.cpp -- the rule of `strling sort --markdup` (strling_amd/csrc/markdup_core.h) as a stand-alone program, built
// plainly and with -fsanitize=address,undefined by tests/test_markdup_cases.py and run directly.
//   markdup_core_main                 the built-in checks: signatures at their edges, the packed word's order, scores, the tiebreak
//   markdup_core_main IN.raw OUT      IN.raw = the inflated bytes of a BAM, copied into a buffer exact to the byte; OUT = one line
//                                     "counts P DP F DF I", then the flag word of every record in input order, one a line.  A refused
//                                     record: exit 3 and "record N: why" on stderr
#include <stdio.h>
#include <stdlib.h>
#include <string>
#include <vector>
#include "../../strling_amd/csrc/markdup_core.h"

using namespace strl;

static int g_bad = 0;
#define EXPECT(c) do { if (!(c)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); ++g_bad; } } while (0)

static std::vector<uint8_t> cigar(std::initializer_list<uint32_t> ops) {      // op | len << 4 words in an exact buffer
  std::vector<uint8_t> b;
  for (uint32_t w : ops) for (int k = 0; k < 4; ++k) b.push_back((uint8_t)(w >> (8 * k)));
  return b;
}
static uint32_t op(char c, uint32_t len) { return (uint32_t)std::string("MIDNSHP=X").find(c) | len << 4; }
static int64_t unclipped(std::initializer_list<uint32_t> ops, int32_t pos, bool rev) {
  const std::vector<uint8_t> c = cigar(ops);
  int32_t u = 0;
  return mdup_unclipped(c.data(), (uint32_t)(c.size() / 4), pos, rev, &u) ? (int64_t)u : INT64_MIN;
}

static void checks() {
  EXPECT(unclipped({op('M', 50)}, 100, false) == 100);
  EXPECT(unclipped({op('S', 5), op('M', 45)}, 105, false) == 100);
  EXPECT(unclipped({op('H', 3), op('S', 5), op('M', 45)}, 108, false) == 100);
  EXPECT(unclipped({op('S', 10), op('M', 40)}, 2, false) == -8);                  // u < 0
  EXPECT(unclipped({op('M', 50)}, 100, true) == 149);
  EXPECT(unclipped({op('M', 20), op('D', 3), op('M', 10), op('N', 100), op('M', 20), op('S', 4), op('H', 2)}, 100, true) == 100 + 153 - 1 + 6);
  EXPECT(unclipped({op('S', 7), op('M', 20), op('I', 5), op('=', 10), op('X', 2)}, 10, true) == 10 + 32 - 1);      // I takes no reference, leading S is not trailing
  EXPECT(unclipped({}, 77, true) == 76);                                          // no CIGAR: reflen 0
  EXPECT(unclipped({}, 77, false) == 77);
  EXPECT(unclipped({op('S', 0xfffffff), op('S', 0xfffffff), op('S', 0xfffffff), op('S', 0xfffffff), op('S', 0xfffffff), op('S', 0xfffffff), op('S', 0xfffffff),
                    op('S', 0xfffffff), op('S', 0xfffffff), op('M', 1)}, 0, false) == INT64_MIN);                  // beyond 32 signed bits: refused, not wrapped
  EXPECT(unclipped({op('M', 0xfffffff)}, 0x7ffffff0, true) == INT64_MIN);
  // the packed word orders as (tid, u, strand)
  EXPECT(mdup_sig(0, -8, 0) < mdup_sig(0, -7, 0) && mdup_sig(0, -1, 1) < mdup_sig(0, 0, 0) && mdup_sig(0, 5, 0) < mdup_sig(0, 5, 1));
  EXPECT(mdup_sig(-1, 2147483647, 1) < mdup_sig(0, -2147483647 - 1, 0) && mdup_sig(0, 2147483647, 1) < mdup_sig(1, -2147483647 - 1, 0));
  EXPECT(mdup_sig(0x7ffffffd, 2147483647, 1) == ~0ull - (1ull << 33) && mdup_sig_bits(0x7ffffffe) == 64 && mdup_sig_bits(3) == 35 && mdup_sig_bits(0) == 33);
  EXPECT(mdup_sig(2, 2147483647, 1) >> mdup_sig_bits(3) == 0);
  // scores
  EXPECT(mdup_qual(14) == 0 && mdup_qual(15) == 15 && mdup_qual(0xff) == 0 && mdup_qual(0xfe) == 0xfe);
  EXPECT(mdup_qual4(0xff0f0e28u) == 0x28 + 0x0f);
  // eligibility and pairs
  EXPECT(mdup_eligible(0x400 | 0x1 | 0x40) && !mdup_eligible(0x4) && !mdup_eligible(0x100) && !mdup_eligible(0x200) && !mdup_eligible(0x800));
  EXPECT(mdup_is_pair(mdup_class(0x41), mdup_class(0x81)) && mdup_is_pair(mdup_class(0x81), mdup_class(0x41)));
  EXPECT(!mdup_is_pair(mdup_class(0x41), mdup_class(0x41)) && !mdup_is_pair(mdup_class(0x49), mdup_class(0x81)) && !mdup_is_pair(mdup_class(0x40), mdup_class(0x81)));
  EXPECT(!mdup_is_pair(mdup_class(0xc1), mdup_class(0x81)));
  // the tiebreak: the higher score first, then the lower ordinal; inside its bit field
  EXPECT(mdup_tiebreak(100, 7, 5) < mdup_tiebreak(99, 7, 4) && mdup_tiebreak(100, 7, 4) < mdup_tiebreak(100, 7, 5));
  EXPECT(mdup_tiebreak(0, 7, 0xffffffffu) >> (32 + 7) == 0 && mdup_tiebreak(127, 7, 9) == 9);
}

int main(int argc, char **argv) {
  if (argc == 1) {
    checks();
    if (!g_bad) puts("all cases passed");
    return g_bad ? 1 : 0;
  }
  if (argc != 3) { fputs("usage: markdup_core_main [IN.raw OUT]\n", stderr); return 2; }
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
  std::vector<uint16_t> flags;
  MdupCounts C{};
  std::string why;
  static const uint8_t none = 0;
  const int64_t bad = mdup_host(recs.empty() ? &none : recs.data(), recs.size(), flags, &C, why);
  if (bad >= 0) { fprintf(stderr, "record %lld: %s\n", (long long)bad, why.c_str()); return 3; }
  FILE *o = fopen(argv[2], "w");
  if (!o) { perror(argv[2]); return 2; }
  fprintf(o, "counts %llu %llu %llu %llu %llu\n", (unsigned long long)C.pairs, (unsigned long long)C.dup_pairs, (unsigned long long)C.fragments, (unsigned long long)C.dup_fragments,
          (unsigned long long)C.ineligible);
  for (uint16_t v : flags) fprintf(o, "%u\n", v);
  fclose(o);
  return 0;
}
