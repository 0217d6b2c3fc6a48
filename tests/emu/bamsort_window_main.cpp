// bamsort_window_main.cpp -- the rule of `strling sort --windowed` (strling_amd/csrc/bamsort_core.h: bsort_window_plan, bsort_scatter_part,
// bsort_window_complete) as a stand-alone program, built with -fsanitize=address,undefined by tests/test_sort_windowed_cases.py and
// run directly.
//   bamsort_window_main plan STREAM_BYTES LIMIT PIECE     prints "window_bytes n_windows"
//   bamsort_window_main IN.raw STREAM                     IN.raw = the inflated bytes of a BAM, STREAM = the sorted stream expected.
//                                                         Pass 0 (keys, a stable sort, dest[]), then for windows of 1 block, 3 blocks
//                                                         and the whole stream, and the input walked in chunks of 1, 2 and all records,
//                                                         the scatter into a window buffer exact to the byte; the windows, concatenated,
//                                                         against STREAM
//   bamsort_window_main IN.raw STREAM withhold K          the same with record K left out of every pass: exit 3, "incomplete"
//   bamsort_window_main IN.raw STREAM alter K             the same with record K's block_size word one more in every pass: exit 4,
//                                                         "record K"
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <numeric>
#include <string>
#include <vector>
#include "../../strling_amd/csrc/bamsort_core.h"

using namespace strl;

static bool read_file(const char *path, std::vector<uint8_t> &out) {
  FILE *f = fopen(path, "rb");
  if (!f) { perror(path); return false; }
  uint8_t tmp[65536];
  for (size_t got; (got = fread(tmp, 1, sizeof tmp, f)) > 0;) out.insert(out.end(), tmp, tmp + got);
  fclose(f);
  return true;
}

int main(int argc, char **argv) {
  if (argc == 5 && std::string(argv[1]) == "plan") {
    const BsortWindowPlan p = bsort_window_plan(strtoull(argv[2], nullptr, 10), strtoull(argv[3], nullptr, 10), strtoull(argv[4], nullptr, 10));
    printf("%llu %llu\n", (unsigned long long)p.window_bytes, (unsigned long long)p.n_windows);
    return 0;
  }
  if (argc != 3 && argc != 5) { fprintf(stderr, "usage: see the head of bamsort_window_main.cpp\n"); return 2; }
  std::vector<uint8_t> raw, want;
  if (!read_file(argv[1], raw) || !read_file(argv[2], want)) return 2;
  const std::string mode = argc == 5 ? argv[3] : "";
  const uint64_t victim = argc == 5 ? strtoull(argv[4], nullptr, 10) : ~0ull;
  // pass 0: key and length of every record, the stable sort, the layout, dest[ordinal]
  std::vector<uint8_t> header;
  std::string err;
  int32_t n_ref = 0;
  size_t used = 0;
  if (!bsort_header(raw.data(), raw.size(), header, &n_ref, &used, err)) { fprintf(stderr, "%s\n", err.c_str()); return 2; }
  std::vector<uint64_t> at, key;
  std::vector<uint32_t> len;
  for (size_t q = used; q < raw.size();) {
    if (raw.size() - q < BSORT_MIN_REC) return 2;
    const uint32_t bs = bsort_ld32(raw.data() + q);
    if (bs < 32 || bs > raw.size() - q - 4) return 2;
    uint64_t k;
    if (!bsort_key(raw.data() + q + 4, n_ref, &k)) { fprintf(stderr, "record %zu: refID\n", at.size()); return 2; }
    at.push_back(q); key.push_back(k); len.push_back(bs + 4);
    q += 4 + (size_t)bs;
  }
  const size_t n = at.size();
  std::vector<uint32_t> perm(n);
  std::iota(perm.begin(), perm.end(), 0u);
  std::stable_sort(perm.begin(), perm.end(), [&](uint32_t a, uint32_t b) { return key[a] < key[b]; });
  std::vector<uint64_t> dest(n);
  uint64_t total = header.size();
  for (size_t j = 0; j < n; ++j) { dest[perm[j]] = total; total += len[perm[j]]; }
  if (total != want.size()) { fprintf(stderr, "the stream is %llu bytes, %zu expected\n", (unsigned long long)total, want.size()); return 1; }
  // the passes
  for (uint64_t limit : {(uint64_t)BSORT_BLK, (uint64_t)3 * BSORT_BLK + 77, total + 5 * (uint64_t)BSORT_BLK})
    for (size_t chunk : {(size_t)1, (size_t)2, std::max<size_t>(n, 1)}) {
      const BsortWindowPlan plan = bsort_window_plan(total, limit, BSORT_BLK);
      if (plan.window_bytes % BSORT_BLK || plan.window_bytes > std::max<uint64_t>(limit, BSORT_BLK)) { fprintf(stderr, "plan: window of %llu bytes\n", (unsigned long long)plan.window_bytes); return 1; }
      uint64_t covered = 0;
      for (uint64_t w = 0; w < plan.n_windows; ++w) {
        const uint64_t lo = w * plan.window_bytes, hi = std::min(total, lo + plan.window_bytes);
        if (lo != covered || lo >= hi) { fprintf(stderr, "plan: window %llu is [%llu, %llu)\n", (unsigned long long)w, (unsigned long long)lo, (unsigned long long)hi); return 1; }
        std::vector<uint8_t> buf((size_t)(hi - lo), 0xAA);                 // exact to the byte
        const uint64_t hb = bsort_window_header(header.size(), lo, hi);
        if (hb) memcpy(buf.data(), header.data() + lo, (size_t)hb);
        uint64_t placed = 0, ord0 = 0;
        for (size_t c0 = 0; c0 < n; c0 += chunk) {                         // a chunk of the input: its records' ordinals are ord0 + i
          const size_t nc = std::min(chunk, n - c0);
          for (size_t i = 0; i < nc; ++i) {
            const uint64_t ord = ord0 + i;
            if (mode == "withhold" && ord == victim) continue;
            uint32_t bs_now = bsort_ld32(raw.data() + at[c0 + i]);
            if (mode == "alter" && ord == victim) ++bs_now;
            BsortPart p;
            if (!bsort_scatter_part(dest[ord], len[ord], bs_now, lo, hi, &p)) { printf("the input changed between passes: record %llu\n", (unsigned long long)ord); return 4; }
            if (!p.bytes) continue;
            memcpy(buf.data() + p.dst, raw.data() + at[c0 + i] + p.skip, (size_t)p.bytes);
            placed += p.bytes;
          }
          ord0 += nc;
        }
        if (!bsort_window_complete(placed, header.size(), lo, hi)) { printf("incomplete window %llu\n", (unsigned long long)w); return 3; }
        if (memcmp(buf.data(), want.data() + lo, buf.size())) { fprintf(stderr, "window %llu (limit %llu, chunks of %zu) differs\n", (unsigned long long)w, (unsigned long long)limit, chunk); return 1; }
        covered = hi;
      }
      if (covered != total) { fprintf(stderr, "plan: the windows end at %llu of %llu\n", (unsigned long long)covered, (unsigned long long)total); return 1; }
    }
  printf("all windows equal\n");
  return 0;
}
