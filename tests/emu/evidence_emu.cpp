// Host build of the evidence kernel's per-record rule (strling_amd/csrc/evidence_core.h with STRL_EMU): the walk with the header
// test, the keep test, the row fill, the depth array and the median, in plain loops, one region after the other.  What belongs
// to a workgroup in evidence.hip (the LDS window, ballots and ranks, the row reservation, the scan, the hash table) is NOT here:
// qname identity is the first kept record with equal name bytes, found by plain search.  A stand-alone program, so that the CPU
// suite can run the rule itself -- under -fsanitize=address,undefined -- without a device (tests/test_evidence_cases.py).
//
//   evidence_emu FILE
// FILE (binary, little endian):
//   u32 n_tables, then n_tables x 4096 float32     the cd[] tables (spanning.nim:7-20), made by the test
//   u32 n_regions, then per region
//     i32 window, u32 min_mapq, u32 table          the table's index
//     i32 tid, u32 left, u32 right, char unit[8]   the bound (strl_bounds' fields)
//     u64 len, then len bytes                      the region's record bytes; held in a heap block of exactly len bytes, so that a
//                                                  read behind the range is an AddressSanitizer report
// Output, per region:  "region R status S median M rows N", then one line per row:
//   "row ORD NAME_ID HASH PROB(float32 bits) START STOP ISIZE FLAGS TYPE REPEAT_COUNT CIGAR_INS CIGAR_DEL"
// The kernel's rules hold: more than EV_MAX_RECORDS records, bytes that do not parse, a CIGAR that names bases the SEQ does not
// hold, or a bound beyond the capacity rule give status 2 and no rows.
#define STRL_EMU 1
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <memory>
#include <vector>
#include "../../strling_amd/csrc/evidence_core.h"

using namespace strl;

template <class T> static bool rd(FILE *f, T *v, size_t n = 1) { return fread(v, sizeof(T), n, f) == n; }

static void run_region(uint32_t r, const uint8_t *u, uint64_t len, const EvBound &B, uint32_t min_mapq, const float *cd) {
  auto pass_on = [&] { printf("region %u status 2 median 0 rows 0\n", r); };
  if (B.status) return pass_on();
  // 1. the records' offsets
  std::vector<uint64_t> off;
  for (uint64_t p = 0; p < len;) {
    uint32_t bs;
    if (p + 36 > len || !ev_header_ok(u + p, len - p, &bs) || off.size() == EV_MAX_RECORDS) return pass_on();
    off.push_back(p);
    p += 4ull + bs;
  }
  // 2. the filters and the depth differences
  const int64_t D = B.depth_n;
  std::vector<int64_t> depth((size_t)D, 0);
  std::vector<uint32_t> kept;
  for (uint32_t i = 0; i < off.size(); ++i) {
    EvRec R;
    R.load(u + off[i]);
    int32_t a, b;
    if (!ev_keep(R, R.stop(), B, min_mapq, &a, &b)) continue;
    depth.at((size_t)a) += 1;
    depth.at((size_t)b) -= 1;
    kept.push_back(i);
  }
  // 3. one row per kept record
  std::vector<EvRow> rows;
  bool bad = false;
  for (uint32_t k = 0; k < kept.size(); ++k) {
    EvRec R;
    R.load(u + off[kept[k]]);
    rows.push_back(ev_row(R, R.stop(), B, cd, kept[k], k, &bad));
  }
  if (bad) return pass_on();
  // 4. depths, their histogram, the median (utils.nim:148-158)
  std::vector<uint64_t> hist(1048, 0);
  int64_t run = 0;
  for (int64_t i = 0; i < D; ++i) {
    run += depth[(size_t)i];
    hist[(size_t)(run < 0 ? 0 : (run > 1047 ? 1047 : run))] += 1;
  }
  int median = 0;
  uint64_t s = 0;
  for (int i = 0; i < 1048; ++i) { s += hist[(size_t)i]; if ((double)s > (double)D / 2.0) { median = i; break; } }
  // 5. qname identity: the first row with the same qname bytes
  for (uint32_t k = 0; k < rows.size(); ++k) {
    const uint8_t *me = u + off[rows[k].ord];
    for (uint32_t e = 0; e < k; ++e) {
      const uint8_t *ot = u + off[rows[e].ord];
      if (ot[12] == me[12] && (me[12] < 2 || !memcmp(ot + 36, me + 36, me[12] - 1u))) { rows[k].name_id = e; break; }
    }
  }
  printf("region %u status 0 median %d rows %zu\n", r, median, rows.size());
  for (const EvRow &w : rows) {
    uint32_t bits;
    memcpy(&bits, &w.prob, 4);
    printf("row %u %u %u %u %d %lld %d %u %u %u %u %u\n", w.ord, w.name_id, w.hash, bits, w.start, (long long)w.stop, w.isize, w.flags, w.type, w.repeat_count,
           w.cigar_ins, w.cigar_del);
  }
}

int main(int argc, char **argv) {
  if (argc != 2) { fprintf(stderr, "usage: evidence_emu FILE\n"); return 2; }
  FILE *f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  uint32_t n_tables = 0, n_regions = 0;
  if (!rd(f, &n_tables) || n_tables > 64) return 2;
  std::vector<float> cd((size_t)n_tables * 4096);
  if (n_tables && !rd(f, cd.data(), cd.size())) return 2;
  if (!rd(f, &n_regions)) return 2;
  for (uint32_t r = 0; r < n_regions; ++r) {
    int32_t window, tid;
    uint32_t min_mapq, table, left, right;
    char unit[8];
    uint64_t len;
    if (!rd(f, &window) || !rd(f, &min_mapq) || !rd(f, &table) || !rd(f, &tid) || !rd(f, &left) || !rd(f, &right) || !rd(f, unit, 8) || !rd(f, &len)) return 2;
    if (table >= n_tables || len > (1ull << 31)) return 2;
    std::unique_ptr<uint8_t[]> u(new uint8_t[len]);            // exactly len bytes
    if (len && !rd(f, u.get(), len)) return 2;
    strl_bounds b;
    memset(&b, 0, sizeof b);
    b.tid = tid; b.left = left; b.right = right;
    memcpy(b.repeat, unit, 6);
    if (b.left > b.right) return 2;                             // (evidence_run refuses the call)
    run_region(r, u.get(), len, ev_bound_make(b, window, 0), min_mapq, cd.data() + (size_t)table * 4096);
  }
  fclose(f);
  return 0;
}
