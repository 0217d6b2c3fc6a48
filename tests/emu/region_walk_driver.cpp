// Stand-alone driver of region_walk (cli/region_feed.cpp, the host's stand-in for region_walk_kernel) for
// tests/test_region_cases.py: every request's run of inflated bytes is copied into a vector of exactly its size, so that
// AddressSanitizer sees a read behind the run, and walked.  Built with -fsanitize=address,undefined.
//   driver IN
// IN:  u64 stream bytes, n_requests | the stream | per request u64 base, lim, in_block; i32 tid, beg, end, 0
//      (the run is stream[base, lim), the walk starts at in_block inside it)
// Out: one line per request: stopped keep stop (offsets inside the run)
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "region_feed.h"

using namespace strl;

int main(int argc, char **argv) {
  if (argc != 2) { fprintf(stderr, "usage: see the head of region_walk_driver.cpp\n"); return 1; }
  FILE *f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  uint64_t head[2];
  if (fread(head, 8, 2, f) != 2) { fprintf(stderr, "short file\n"); return 2; }
  std::vector<uint8_t> stream((size_t)head[0]);
  if (head[0] && fread(stream.data(), 1, stream.size(), f) != stream.size()) { fprintf(stderr, "short stream\n"); return 2; }
  for (uint64_t r = 0; r < head[1]; ++r) {
    struct { uint64_t base, lim, in_block; int32_t tid, beg, end, pad; } q;
    if (fread(&q, sizeof q, 1, f) != 1) { fprintf(stderr, "short request %llu\n", (unsigned long long)r); return 2; }
    if (q.base > q.lim || q.lim > stream.size()) { fprintf(stderr, "request %llu leaves the stream\n", (unsigned long long)r); return 2; }
    const std::vector<uint8_t> u(stream.begin() + (ptrdiff_t)q.base, stream.begin() + (ptrdiff_t)q.lim);
    size_t keep = 0, stop = 0;
    const bool stopped = region_walk(u, (size_t)q.in_block, q.tid, q.beg, q.end, keep, stop);
    printf("%d %zu %zu\n", stopped ? 1 : 0, keep, stop);
  }
  fclose(f);
  return 0;
}
