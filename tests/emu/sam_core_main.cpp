// sam_core_main.cpp -- csrc/sam_core.h as a stand-alone program, built with -fsanitize=address,undefined and run on the CPU
// (tests/test_sort_sam_cases.py).  Every line is copied into a heap block exact to the byte before it is encoded, and the tags are
// encoded once more into a block exact to the byte, so a read behind the line or a store behind the record is the sanitizer's to see.
//   sam_core_main                  the built-in cases
//   sam_core_main IN.sam OUT       the header function and the encoder over a file: OUT = the BAM header || the records in input order;
//                                  a refusal: its words on stderr, exit 1
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <memory>
#include <string>
#include <vector>
#include "../../strling_amd/csrc/sam_core.h"
#include "../../strling_amd/csrc/bamsort_core.h"

using namespace strl;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++failures; } } while (0)

// the line in a block of exactly its bytes; the record checked against a second walk of the tags into a block of exactly theirs
static uint32_t encode_exact(const uint8_t *line, size_t len, const SamRefs &R, std::vector<uint8_t> &out, std::string &why) {
  std::unique_ptr<uint8_t[]> copy(new uint8_t[len ? len : 1]);
  memcpy(copy.get(), line, len);
  const size_t before = out.size();
  const uint32_t er = sam_encode_line(copy.get(), (uint32_t)len, R, out, why);
  if (er) { CHECK(out.size() == before); return er; }
  const uint32_t l = sam_strip_cr(copy.get(), (uint32_t)len);
  SamPlan P;
  CHECK(sam_plan_line<true>(copy.get(), l, R, P) == SAM_OK);
  CHECK(out.size() - before == P.rec_len);
  if (P.tab[10] < l && P.tag_bytes) {
    // the device's walk of the tags (the fast path of the floats) takes the same bytes, and one byte less of room is an overrun, not a store
    std::unique_ptr<uint8_t[]> tags(new uint8_t[P.tag_bytes]);
    uint32_t nb = 0, nh = 0;
    CHECK(sam_tags<false>(copy.get() + P.tab[10] + 1, l - P.tab[10] - 1, tags.get(), P.tag_bytes, &nb, &nh) == SAM_OK && nb == P.tag_bytes);
    if (!nh) CHECK(!memcmp(tags.get(), out.data() + out.size() - P.tag_bytes, P.tag_bytes));
    std::unique_ptr<uint8_t[]> less(new uint8_t[P.tag_bytes - 1 ? P.tag_bytes - 1 : 1]);
    CHECK(sam_tags<false>(copy.get() + P.tab[10] + 1, l - P.tab[10] - 1, less.get(), P.tag_bytes - 1, &nb, &nh) == SAM_E_OVERRUN && nb == P.tag_bytes);
  }
  return SAM_OK;
}

static int run_file(const char *in, const char *out_path) {
  FILE *f = fopen(in, "rb");
  if (!f) { fprintf(stderr, "cannot read %s\n", in); return 2; }
  std::vector<uint8_t> text;
  uint8_t buf[1 << 16];
  for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;) text.insert(text.end(), buf, buf + n);
  fclose(f);
  SamHeader H;
  std::string err;
  if (!sam_header(text.data(), text.size(), H, err)) { fprintf(stderr, "%s\n", err.c_str()); return 1; }
  SamRefTable T;
  T.build(H.names.data(), H.name_off.data(), (int32_t)H.l_ref.size(), nullptr);
  std::vector<uint8_t> out = H.bam;
  uint64_t n = 0;
  for (size_t at = H.used; at < text.size(); ++n) {
    const uint8_t *nl = static_cast<const uint8_t *>(memchr(text.data() + at, '\n', text.size() - at));
    const size_t end = nl ? (size_t)(nl - text.data()) : text.size();
    std::string why;
    if (encode_exact(text.data() + at, end - at, T.view(), out, why)) { fprintf(stderr, "%s\n", sam_refusal(n + 1, why).c_str()); return 1; }
    at = end + 1;
  }
  f = fopen(out_path, "wb");
  if (!f || fwrite(out.data(), 1, out.size(), f) != out.size()) { fprintf(stderr, "cannot write %s\n", out_path); return 2; }
  fclose(f);
  return failures ? 3 : 0;
}

static float fast(const char *s, bool *took) { float f = -1.f; *took = sam_float_fast(reinterpret_cast<const uint8_t *>(s), (uint32_t)strlen(s), &f); return f; }

int main(int argc, char **argv) {
  if (argc == 3) return run_file(argv[1], argv[2]);
  // the floats: where the fast path answers it answers as strtod and the cast do, and it declines what it must
  const char *spell[] = {"0", "-0", "1", "+7", ".5", "5.", "1e-3", "0.1", "3.14", "123456789012345", "1e22", "123456789012345e22", "1e-22", "16777217", "0.000001", "-2.5E+3",
                         "00000000000000000001.5", "0e400", "4.35", "0.3", "2.675", "1.0000001", "8.5e-5"};
  for (const char *s : spell) {
    bool took;
    const float a = fast(s, &took), b = (float)strtod(s, nullptr);
    CHECK(took && !memcmp(&a, &b, 4));
  }
  for (const char *s : {"1234567890123456", "1e23", "1e-23", "inf", "nan", "-inf", "", "-", ".", "1e", "1e+", "1.5x", " 1", "0x10", "1.17549435e-38"}) { bool took; fast(s, &took); CHECK(!took); }
  unsigned seed = 12345;
  for (int k = 0; k < 200000; ++k) {                               // random spellings inside the fast path's conditions
    seed = seed * 1664525u + 1013904223u;
    char s[64];
    const unsigned long long w = ((unsigned long long)seed * 2654435761u) % 1000000000000000ull;
    const int e = (int)(seed >> 8) % 23 - (int)(seed >> 20) % 23;
    snprintf(s, sizeof s, "%llue%d", w, e);
    bool took;
    const float a = fast(s, &took), b = (float)strtod(s, nullptr);
    CHECK(took && !memcmp(&a, &b, 4));
  }
  // the table: names that share a first slot, a prefix of another, a name that is not there
  const char *names = "chrchr1chr10x";
  const uint32_t off[5] = {0, 3, 7, 12, 13};
  SamRefTable T;
  int32_t dup = -1;
  CHECK(T.build(reinterpret_cast<const uint8_t *>(names), off, 4, &dup));
  const SamRefs R = T.view();
  CHECK(sam_ref_find(R, (const uint8_t *)"chr1", 4) == 1 && sam_ref_find(R, (const uint8_t *)"chr", 3) == 0 && sam_ref_find(R, (const uint8_t *)"chr10", 5) == 2);
  CHECK(sam_ref_find(R, (const uint8_t *)"chr100", 6) == -2 && sam_ref_find(R, (const uint8_t *)"ch", 2) == -2 && sam_ref_find(R, (const uint8_t *)"", 0) == -2);
  const uint32_t off2[3] = {0, 3, 6};
  CHECK(!T.build(reinterpret_cast<const uint8_t *>("abcabc"), off2, 2, &dup) && dup == 1);
  SamRefTable none;
  CHECK(none.build(nullptr, off, 0, nullptr) && sam_ref_find(none.view(), (const uint8_t *)"a", 1) == -2);
  // lines: a record's length is the plan's, a refusal appends nothing
  CHECK(T.build(reinterpret_cast<const uint8_t *>(names), off, 4, &dup));
  std::vector<uint8_t> out;
  std::string why;
  const std::string ok = "r\t0\tchr1\t5\t30\t4M\t=\t9\t-3\tACGT\tIIII\tNM:i:-40000\tXB:B:f,1.5,inf\tXZ:Z:\r";
  CHECK(encode_exact((const uint8_t *)ok.data(), ok.size(), T.view(), out, why) == SAM_OK && out.size() > 36 && bsort_ld32(out.data()) + 4 == out.size());
  CHECK((int32_t)bsort_ld32(out.data() + 4) == 1 && (int32_t)bsort_ld32(out.data() + 24) == 1 && (int32_t)bsort_ld32(out.data() + 32) == -3);
  for (const char *bad : {"", "r", "r\t0\tchr1\t5\t30\t4M\t=\t9\t-3\tACGT", "r\t0\tchr2\t5\t30\t4M\t=\t9\t-3\tACGT\tIIII", "r\t0\tchr1\t5\t30\t4M\t=\t9\t-3\tACGT\tIIII\t", "r\t0\tchr1\t5\t30\t4M\t=\t9\t-3\tACGT\tIIII\tXX",
                          "r\t0\tchr1\t5\t30\t4\t=\t9\t-3\tACGT\tIIII", "r\t0\tchr1\t5\t30\tM\t=\t9\t-3\tACGT\tIIII", "r\t0\tchr1\t5\t30\t4M\t=\t9\t-3\t\tIIII", "r\t0\tchr1\t5\t30\t4M\t=\t9\t-\tACGT\tIIII",
                          "r\t0\tchr1\t5\t30\t4M\t=\t9\t-3\tACGT\tIIII\tXB:B:", "r\t0\tchr1\t5\t30\t4M\t=\t9\t-3\tACGT\tIIII\tXB:B:c1", "r\t0\tchr1\t5\t30\t4M\t=\t9\t-3\tACGT\tIIII\tXB:B:c,", "r\t0\tchr1\t5\t30\t4M\t=\t9\t-3\tACGT\tIIII\tXA:A:"}) {
    const size_t before = out.size();
    CHECK(encode_exact((const uint8_t *)bad, strlen(bad), T.view(), out, why) != SAM_OK && out.size() == before && !why.empty());
  }
  if (failures) { printf("%d checks failed\n", failures); return 1; }
  printf("all cases passed\n");
  return 0;
}
