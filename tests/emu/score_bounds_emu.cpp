// score_bounds_emu.cpp -- TEST-ONLY host build of the device scorer (strling_amd/csrc/score_core.h with STRL_EMU) whose entry
// takes the wave's length bounds EXPLICITLY.  On the device the bounds are the minimum and maximum of the segment lengths of a
// wave's 64 lanes; they only decide which work is skipped (end-of-read masks below `lo`, windows / words / batches at or past
// `hi`), never what a lane computes.  One emulated lane scored under every legal pair lo <= len <= hi <= 16 NW must therefore
// give the same two words: tests/test_emu_bounds.py checks them against the oracle.
//
// With -DSTRL_BOUNDS_MAIN the file is a stand-alone program (for -fsanitize=address,undefined; link oracle/strling_oracle.c):
// a few thousand generated segments, every pair of bounds, compared with the oracle's get_repeat.
#define STRL_EMU 1
#include "../../strling_amd/csrc/score_core.h"
#include "../../strling_amd/csrc/score_tables.h"
#include <string.h>

using namespace strl;

static std::vector<uint16_t> g_lut;
static std::vector<uint64_t> g_thr;
static std::vector<uint32_t> g_clut, g_ta;

template <int NW> static void new_seg(Seg<NW> &sg, uint32_t *inv_lds, uint32_t *inv_mem) {
  sg.inv_lds = inv_lds;
  sg.inv = inv_mem;
  sg.inv_stride = 1;
  sg.inv_nslots = INV_SLOTS;
}

// fused: stage B on the Seg stage A used (the soft-clip launch of the short-read class); else hand over and convert again
template <int NW, int SLOTS>
static void run(const uint8_t *seq4, int s0, int len, LenBounds lb, int row0, int row1, bool whole, bool fused, uint32_t *o0, uint32_t *o1) {
  static uint32_t tab[SLOTS + 8];
  constexpr int MAXCH = (16 * NW + 62) / 32;
  const int s0l = s0 & 31;
  const int nch = (s0l + len + 31) >> 5;
  const uint8_t *src = seq4 + (size_t)(s0 >> 5) * 16;
  auto stage_raw = [&]() {
    memset(tab, 0, sizeof tab);
    for (int c = 0; c < MAXCH && c < nch; ++c) memcpy(&tab[4 * c], src + 16 * c, 16);
  };
  stage_raw();
  Seg<NW> sg;
  uint32_t inv_mem[NW];
  static uint32_t inv_lds[INV_SLOTS * NW];
  new_seg<NW>(sg, inv_lds, inv_mem);
  if (whole && s0 == 0) {
    uint32_t raw[4 * MAXCH];
    for (int i = 0; i < 4 * MAXCH; ++i) raw[i] = i < 4 * nch ? tab[i] : 0u;
    seg_from_words<NW>(raw, g_clut.data(), len, lb, sg);
  } else {
    seg_from_raw<NW>(tab, g_clut.data(), s0l, len, sg);
  }
  ScoreState st;
  LaneThr lt;
  load_thr(g_thr.data(), row0, row1, len, lt);
  score_stage_a<NW, SLOTS>(sg, true, tab, tab, 0, g_ta.data(), lt, lb, st);
  if (st.alive) {
    if (fused) {
      score_stage_b<NW, SLOTS>(sg, tab, 0, g_lut.data(), lt, lb, st);
    } else {
      stage_raw();
      Seg<NW> sg2;
      new_seg<NW>(sg2, inv_lds, inv_mem);
      seg_from_raw<NW>(tab, g_clut.data(), s0l, len, sg2);
      score_stage_b<NW, SLOTS>(sg2, tab, 0, g_lut.data(), lt, lb, st);
    }
  }
  *o0 = reduce_packed(st.res0);
  *o1 = reduce_packed(st.res1);
}

extern "C" {
void bemu_set_p(double p) {
  strl_opts o{};
  o.proportion_repeat = p;
  build_lut(g_lut);
  build_thr(o, g_thr);
  build_conv_lut(g_clut);
  build_stage_a_tables(g_lut, g_ta);
}
// mode 0: whole read (threshold p); mode 1: soft clip (p - 0.07 / min(p, 0.6)).  klass 0 | 1 | 2 = NW 10 | 16 | 32.
// lo <= len <= hi <= 16 NW or the call is refused (-1).  seq4 must have 32 B slack.
int bemu_score(const uint8_t *seq4, int s0, int len, int lo, int hi, int mode, int klass, int fused, uint32_t *o0, uint32_t *o1) {
  const int nw = klass == 0 ? 10 : klass == 1 ? 16 : 32;
  if (!(0 <= lo && lo <= len && len <= hi && hi <= 16 * nw)) return -1;
  const int r0 = mode == 0 ? 1 : 2, r1 = mode == 0 ? 1 : 3;
  LenBounds lb;
  lb.lo = lo;
  lb.hi = hi;
  if (klass == 0) run<10, 64>(seq4, s0, len, lb, r0, r1, mode == 0, fused != 0, o0, o1);
  else if (klass == 1) run<16, 128>(seq4, s0, len, lb, r0, r1, mode == 0, fused != 0, o0, o1);
  else run<32, 256>(seq4, s0, len, lb, r0, r1, mode == 0, fused != 0, o0, o1);
  return 0;
}
}

#ifdef STRL_BOUNDS_MAIN
#include <stdio.h>
#include <stdlib.h>
#include <string>
extern "C" void orc_get_repeat(const char *read, int len, double proportion_repeat, char rep[6], int *repeat_count);

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t n) {   // xorshift64*: [0, n)
  g_rng ^= g_rng >> 12; g_rng ^= g_rng << 25; g_rng ^= g_rng >> 27;
  return (uint32_t)(((g_rng * 0x2545F4914F6CDD1Dull) >> 33) % n);
}
static char pick(const char *set) { return set[rnd((uint32_t)strlen(set))]; }

// the generator style of tests/test_emu_parity.py: random, k = 1..6 repeats at several purities and phases, two-unit mixes, not-ACGT
static std::string segment(int L) {
  std::string s((size_t)L, 'A');
  const uint32_t kind = rnd(100);
  if (kind < 25) {
    for (auto &c : s) c = pick("ACGT");
  } else if (kind < 80) {
    const int k = 1 + (int)rnd(6), ph = (int)rnd((uint32_t)k + 1);
    static const int purity[6] = {100, 98, 95, 90, 85, 70};
    const int pur = purity[rnd(6)];
    char u[6];
    for (int j = 0; j < k; ++j) u[j] = pick("ACGT");
    for (int i = 0; i < L; ++i) s[(size_t)i] = (int)rnd(100) < pur ? u[(i + ph) % k] : pick("ACGT");
  } else if (kind < 90) {
    const int k1 = 2 + (int)rnd(5), k2 = 2 + (int)rnd(5), cut = (int)rnd((uint32_t)L + 1);
    char u1[6], u2[6];
    for (int j = 0; j < k1; ++j) u1[j] = pick("ACGT");
    for (int j = 0; j < k2; ++j) u2[j] = pick("AC");
    for (int i = 0; i < L; ++i) s[(size_t)i] = i < cut ? u1[i % k1] : u2[(i - cut) % k2];
  } else {
    for (auto &c : s) c = pick("ACGTNNMR=");
  }
  if (rnd(100) < 15 && L > 0)
    for (int n = 1 + (int)rnd(25); n > 0; --n) s[rnd((uint32_t)L)] = pick("NNNMRY");
  return s;
}

static uint32_t pack_word(const char rep[6], int count) {
  static const char *bases = "CATG";
  uint32_t code = 0, k = 0;
  for (; k < 6 && rep[k]; ++k) code = (code << 2) | (uint32_t)(strchr(bases, rep[k]) - bases);
  return code | (k << 12) | ((uint32_t)count << 16);
}

int main() {
  static const int lens[] = {0, 1, 4, 5, 6, 19, 20, 21, 23, 24, 25, 29, 30, 31, 95, 96, 100, 149, 150, 151, 160};
  static const char *nt16 = "=ACMGRSVTWYHKDBN";
  const double p = 0.8;
  bemu_set_p(p);
  long n_seg = 0, n_run = 0;
  for (int rep = 0; rep < 8; ++rep) {
    for (int L : lens) {
      for (int q = 0; q < 20; ++q) {
        const int pre = (int)rnd(40);                       // bases in front of the segment: every staging phase
        const std::string s = segment(pre + L);
        std::vector<uint8_t> seq4((size_t)(pre + L + 1) / 2 + 64, 0);
        for (int i = 0; i < pre + L; ++i)
          seq4[(size_t)i / 2] |= (uint8_t)((strchr(nt16, s[(size_t)i]) - nt16) << ((i & 1) ? 0 : 4));
        char r0[6], r1[6];
        int c0, c1;
        orc_get_repeat(s.data() + pre, L, p - 0.07, r0, &c0);
        orc_get_repeat(s.data() + pre, L, p < 0.6 ? p : 0.6, r1, &c1);
        const uint32_t e0 = pack_word(r0, c0), e1 = pack_word(r1, c1);
        int his[6] = {L, L + 1, (L + 19) / 20 * 20, (L + 23) / 24 * 24, (L + 15) / 16 * 16, 160};
        ++n_seg;
        for (int hi : his) {
          if (hi > 160) hi = 160;
          for (int lo : {0, L}) {
            for (int fused = 0; fused < 2; ++fused) {
              uint32_t o0 = 0, o1 = 0;
              if (bemu_score(seq4.data(), pre, L, lo, hi, 1, 0, fused, &o0, &o1)) { printf("refused: len %d lo %d hi %d\n", L, lo, hi); return 1; }
              ++n_run;
              if (o0 != e0 || o1 != e1) {
                printf("MISMATCH len %d lo %d hi %d fused %d: %08x %08x, oracle %08x %08x: %s\n", L, lo, hi, fused, o0, o1, e0, e1, s.c_str() + pre);
                return 1;
              }
            }
          }
        }
      }
    }
  }
  printf("score_bounds_emu: %ld segments, %ld bounded runs, all equal to the oracle\n", n_seg, n_run);
  return 0;
}
#endif
