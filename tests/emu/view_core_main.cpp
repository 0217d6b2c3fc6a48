// view_core_main.cpp -- the rule of `strling view` (strling_amd/csrc/view_core.h) as a stand-alone program: g++, no device, nothing
// loaded into Python; tests/test_view_cases.py builds it plain and with -fsanitize=address,undefined.
//   view_core_main                                    200 000 seeded random float bit patterns (and the edges of the stated range) through
//                                                     view_float_g against snprintf("%g"): every answer identical or "not mine", "not
//                                                     mine" only outside the range; the same for doubles that are floats
//   view_core_main IN.raw OUT f F G q [tid beg end]   IN.raw = a BAM's inflated bytes.  Every kept record's line is written twice: by the
//                                                     host rule (view_host) and, part by part, by the sinks the kernels use (ViewCount for
//                                                     the sizes, ViewStore into a buffer of exactly the line's bytes); the two must
//                                                     agree to the byte.  OUT gets the text; stdout the counts.  A refusal: exit code 3,
//                                                     "record N: WORDS" on stderr.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "../../strling_amd/csrc/view_core.h"

using namespace strl;

static int fail(const char *what, const std::string &a, const std::string &b) {
  fprintf(stderr, "FAILED %s: got [%s] want [%s]\n", what, a.c_str(), b.c_str());
  return 1;
}

static int check_float(uint32_t bits, uint64_t *mine, uint64_t *not_mine) {
  float v;
  memcpy(&v, &bits, 4);
  char got[16], want[64];
  const uint32_t n = view_float_g(v, got);
  snprintf(want, sizeof want, "%g", (double)v);
  const uint32_t E = bits >> 23 & 255u;
  const bool in_range = !(bits & 0x7fffffffu) || (E >= VIEW_G_EXP_LO && E <= VIEW_G_EXP_HI);
  if (!n) {
    ++*not_mine;
    if (in_range) return fail("a float inside the stated range was passed on", "not mine", want);
    return 0;
  }
  ++*mine;
  if (!in_range) return fail("a float outside the stated range was answered", std::string(got, n), want);
  if (n > 15 || std::string(got, n) != want) return fail("view_float_g", std::string(got, n), want);
  return 0;
}

static int floats() {
  uint64_t mine = 0, not_mine = 0, x = 0x9e3779b97f4a7c15ull;
  for (int i = 0; i < 200000; ++i) {
    x ^= x << 13; x ^= x >> 7; x ^= x << 17;
    uint32_t bits = (uint32_t)(x >> 16);
    if (i & 1) bits = (bits & 0x807fffffu) | ((VIEW_G_EXP_LO - 3u + (uint32_t)(x >> 50) % (VIEW_G_EXP_HI - VIEW_G_EXP_LO + 7u)) << 23);      // half of them in and around the range
    if (check_float(bits, &mine, &not_mine)) return 1;
  }
  // the edges of every exponent of the range and its neighbours, the powers of ten, ties
  for (uint32_t E = VIEW_G_EXP_LO - 2u; E <= VIEW_G_EXP_HI + 2u; ++E)
    for (uint32_t f : {0u, 1u, 2u, 0x400000u, 0x7ffffeu, 0x7fffffu})
      for (uint32_t s : {0u, 1u})
        if (check_float(s << 31 | E << 23 | f, &mine, &not_mine)) return 1;
  const float named[] = {0.f, -0.f, 1.f, 0.5f, 0.1f, 0.0123f, 0.0001f, 1e-05f, 100000.f, 999999.5f, 123456.7f, 1000005.f, 1000015.f, 16777216.f, 1.234565e-05f, 999999.4f, 99999.95f,
                         9.999995e-05f, 0.00099999995f, 1e10f, 1e15f, 9.5e18f, 3.4028235e38f, 1e-45f};
  for (float v : named) {
    uint32_t bits;
    memcpy(&bits, &v, 4);
    for (int d = -2; d <= 2; ++d) if (check_float(bits + (uint32_t)d, &mine, &not_mine)) return 1;
  }
  for (int k = -7; k <= 19; ++k) {
    char t[32];
    snprintf(t, sizeof t, "1e%d", k);
    const float v = strtof(t, nullptr);
    uint32_t bits;
    memcpy(&bits, &v, 4);
    for (int d = -1; d <= 1; ++d) if (check_float(bits + (uint32_t)d, &mine, &not_mine)) return 1;
  }
  // doubles: the float's bytes where the double is one, else passed on
  struct Arr { char o[32]; uint32_t n; void put(uint8_t b) { o[n++] = (char)b; } };
  for (double v : {0.5, -0.0, 1000015.0, 0.1, 1e300, 123456.7}) {
    Arr a{{0}, 0};
    const bool ok = view_double_g_emit(a, v);
    char want[64];
    snprintf(want, sizeof want, "%g", v);
    if ((double)(float)v == v ? !ok || std::string(a.o, a.n) != want : ok) return fail("view_double_g_emit", std::string(a.o, a.n), want);
  }
  printf("floats answered %llu passed on %llu\nall cases passed\n", (unsigned long long)mine, (unsigned long long)not_mine);
  return 0;
}

int main(int argc, char **argv) {
  if (argc < 7) return floats();
  FILE *f = fopen(argv[1], "rb");
  if (!f) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
  std::vector<uint8_t> raw;
  uint8_t buf[65536];
  for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;) raw.insert(raw.end(), buf, buf + n);
  fclose(f);
  ViewOpts o{(uint32_t)strtoul(argv[3], nullptr, 0), (uint32_t)strtoul(argv[4], nullptr, 0), (uint32_t)strtoul(argv[5], nullptr, 0), (uint32_t)strtoul(argv[6], nullptr, 0), VIEW_NO_REGION, 0, 0};
  if (argc >= 10) { o.tid = atoi(argv[7]); o.beg = atoi(argv[8]); o.end = atoi(argv[9]); }
  // the header: magic, text, references
  size_t p = 4;
  p += 4 + (size_t)mdup_ld32(raw.data() + p);
  const int32_t n_ref = (int32_t)mdup_ld32(raw.data() + p);
  p += 4;
  std::vector<uint8_t> names;
  std::vector<uint32_t> name_off{0};
  for (int32_t r = 0; r < n_ref; ++r) {
    const uint32_t l = mdup_ld32(raw.data() + p);
    names.insert(names.end(), raw.data() + p + 4, raw.data() + p + 4 + l - 1);
    name_off.push_back((uint32_t)names.size());
    p += 4 + l + 4;
  }
  names.push_back(0);
  const ViewRefs F{names.data(), name_off.data(), n_ref};
  // the records exactly to the byte, so that a read past them is seen
  const size_t nrec = raw.size() - p;
  uint8_t *recs = static_cast<uint8_t *>(malloc(nrec ? nrec : 1));
  memcpy(recs, raw.data() + p, nrec);
  std::vector<uint8_t> text;
  ViewCounts C{};
  uint32_t code = 0;
  const int64_t bad = view_host(recs, nrec, F, o, text, &C, 0, &code);
  if (bad >= 0) { fprintf(stderr, "record %lld: %s\n", (long long)bad, view_refusal_text(code)); free(recs); return 3; }
  // again through the kernels' sinks, a line at a time into a buffer of exactly its bytes
  size_t at = 0;
  uint64_t lines = 0;
  for (size_t q = 0; q < nrec;) {
    const uint64_t len = (uint64_t)mdup_ld32(recs + q) + 4u;
    const uint8_t *rec = recs + q;
    q += len;
    ViewRec R;
    if (!view_rec(rec, len, &R)) { fprintf(stderr, "view_rec refuses what view_host took\n"); return 1; }
    uint64_t reflen = 0;
    ViewCount cg;
    for (uint32_t k = 0; k < R.f.n_cigar; ++k) { const uint32_t w = mdup_ld32(rec + R.f.cigar_at + 4u * k); if (view_cigar_on_ref(w & 15u)) reflen += w >> 4; }
    if (!view_kept(R, o, reflen)) continue;
    ViewCount head, mid, tags;
    uint32_t hard = 0;
    view_head_emit(head, rec, R, F); view_cigar_emit(cg, rec, R); view_mid_emit(mid, R, F);
    if (view_tags_emit(tags, rec + R.tags_at, R.n_tags, &hard)) { fprintf(stderr, "the tag walk refuses what view_host took\n"); return 1; }
    const uint32_t sl = view_seq_len(R), ql = view_qual_len(rec, R);
    const ViewParts pt{(uint32_t)head.n, (uint32_t)(head.n + cg.n), (uint32_t)(head.n + cg.n + mid.n), (uint32_t)(head.n + cg.n + mid.n + sl + 1u + ql)};
    const uint64_t L = pt.tags_at + tags.n + 1u;
    if (at + L > text.size()) { fprintf(stderr, "line %llu: the sizes give %llu bytes, the text has %zu left\n", (unsigned long long)lines, (unsigned long long)L, text.size() - at); return 1; }
    uint8_t *d = static_cast<uint8_t *>(malloc(L));
    memset(d, 0, L);
    ViewStore s0{d, d + pt.cigar_at}, s1{d + pt.cigar_at, d + pt.mid_at}, s2{d + pt.mid_at, d + pt.seq_at}, s3{d + pt.tags_at, d + (L - 1u)};
    view_head_emit(s0, rec, R, F); view_cigar_emit(s1, rec, R); view_mid_emit(s2, R, F);
    (void)view_tags_emit(s3, rec + R.tags_at, R.n_tags, &hard);
    if (s0.p != s0.end || s1.p != s1.end || s2.p != s2.end || s3.p != s3.end) { fprintf(stderr, "line %llu: a part does not fill its bytes\n", (unsigned long long)lines); return 1; }
    if (!R.f.l_seq) d[pt.seq_at] = '*';
    for (uint32_t j = 0; j < R.f.l_seq; ++j) d[pt.seq_at + j] = view_base((uint32_t)(rec[R.seq_at + (j >> 1)] >> ((~j & 1u) << 2)) & 15u);
    d[pt.seq_at + sl] = '\t';
    if (ql != R.f.l_seq || !R.f.l_seq) d[pt.seq_at + sl + 1u] = '*';
    else for (uint32_t j = 0; j < ql; ++j) d[pt.seq_at + sl + 1u + j] = view_qual(rec[R.f.qual_at + j]);
    d[L - 1u] = '\n';
    const bool same = !memcmp(d, text.data() + at, L);
    free(d);
    if (!same) { fprintf(stderr, "line %llu: the sinks' bytes differ from the host rule's\n", (unsigned long long)lines); return 1; }
    at += L;
    ++lines;
  }
  free(recs);
  if (at != text.size() || lines != C.written) { fprintf(stderr, "the lines' sizes add up to %zu, the text holds %zu\n", at, text.size()); return 1; }
  FILE *out = fopen(argv[2], "wb");
  if (!out || (!text.empty() && fwrite(text.data(), 1, text.size(), out) != text.size()) || fclose(out)) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
  printf("counts %llu %llu %llu %llu\n", (unsigned long long)C.records, (unsigned long long)C.written, (unsigned long long)C.dropped, (unsigned long long)C.text_bytes);
  return 0;
}
