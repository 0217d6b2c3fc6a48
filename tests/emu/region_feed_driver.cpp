// Stand-alone driver of cli/region_feed.{h,cpp} for tests/test_region_feed.py: plans the regions of a BAM, adds every planned one
// to one RegionBlocks, reads the slices -- in groups of 16 regions, as `strling call` does -- into a malloc'ed buffer of exactly
// comp_bytes + 64 bytes (what `strling call` allocates at the least) and dumps the tables, the buffer and, per region, what the
// host's stand-in for the device makes of it.  Built with -fsanitize=address,undefined.
//   driver BAM MORE OUT TID:BEG:END ...
// Dump: u64 n_regions, n_blocks, comp_bytes, inflated, read_ok | per block u64 coff; u32 clen, isize, crc | the buffer |
//   per region i64 ok, c_beg, c_end, plan blocks; a planned one goes on with u64 first_block, n_blocks, in_block, file_off, len, at;
//   i64 inflate (0 = fine), stopped, keep, stop, inflated bytes; the bytes [keep, stop) if the walk stopped
#include <fcntl.h>
#include <stdio.h>
#include <stdlib.h>
#include <unistd.h>
#include <algorithm>
#include <string>
#include <vector>
#include "region_feed.h"

using namespace strl;

static void put(FILE *f, const void *p, size_t n) { if (n && fwrite(p, 1, n, f) != n) { perror("write"); exit(2); } }
static void put64(FILE *f, int64_t v) { put(f, &v, 8); }

int main(int argc, char **argv) {
  if (argc < 5) { fprintf(stderr, "usage: see the head of region_feed_driver.cpp\n"); return 1; }
  BamReader rd;
  std::string err;
  if (!rd.open(argv[1], err) || !rd.load_index(argv[1], err)) { fprintf(stderr, "open: %s\n", err.c_str()); return 3; }
  const int fd = open(argv[1], O_RDONLY), more = atoi(argv[2]);
  FILE *f = fopen(argv[3], "wb");
  if (fd < 0 || !f) { perror(argv[3]); return 2; }
  struct Region { int32_t tid; long long beg, end; RegionPlan P; size_t at = 0; };      // at: its place among the planned ones
  std::vector<Region> regions((size_t)argc - 4);
  RegionBlocks B;
  for (size_t r = 0; r < regions.size(); ++r) {
    Region &R = regions[r];
    if (sscanf(argv[4 + r], "%d:%lld:%lld", &R.tid, &R.beg, &R.end) != 3) { fprintf(stderr, "region %s\n", argv[4 + r]); return 1; }
    plan_region(rd, fd, R.tid, R.beg, R.end, R.P, more);
    if (!R.P.ok) continue;
    R.at = B.req.size();
    strl_region_req q{};
    q.tid = R.tid; q.beg = (int32_t)R.beg; q.end = (int32_t)R.end;
    B.add(R.P, q);
  }
  uint8_t *comp = (uint8_t *)malloc((size_t)B.comp_bytes + 64);
  bool read_ok = true;
  for (size_t k = 0; k < B.slices.size(); k += 16) read_ok = B.read(fd, comp, k, std::min(B.slices.size(), k + 16)) && read_ok;
  put64(f, (int64_t)regions.size()); put64(f, (int64_t)B.clen.size()); put64(f, (int64_t)B.comp_bytes); put64(f, (int64_t)B.inflated); put64(f, read_ok);
  for (size_t k = 0; k < B.clen.size(); ++k) { put(f, &B.coff[k], 8); put(f, &B.clen[k], 4); put(f, &B.isize[k], 4); put(f, &B.crc[k], 4); }
  put(f, comp, (size_t)B.comp_bytes);
  for (const Region &R : regions) {
    put64(f, R.P.ok); put64(f, (int64_t)R.P.c_beg); put64(f, (int64_t)R.P.c_end); put64(f, (int64_t)R.P.bsize.size());
    if (!R.P.ok) continue;
    const RegionBlocks::Slice &s = B.slices[R.at];
    const strl_region_req &q = B.req[R.at];
    put64(f, q.first_block); put64(f, q.n_blocks); put64(f, q.in_block); put64(f, (int64_t)s.file_off); put64(f, (int64_t)s.len); put64(f, (int64_t)s.at);
    std::vector<uint8_t> u;
    size_t keep = 0, stop = 0;
    const char *bad = read_ok ? region_inflate(B, R.at, comp, u) : "read";
    const bool stopped = !bad && region_walk(u, q.in_block, R.tid, R.beg, R.end, keep, stop);
    if (bad) fprintf(stderr, "region %s: %s\n", argv[4 + (&R - regions.data())], bad);
    put64(f, bad != nullptr); put64(f, stopped); put64(f, (int64_t)keep); put64(f, (int64_t)stop); put64(f, (int64_t)u.size());
    if (stopped) put(f, u.data() + keep, stop - keep);
  }
  free(comp);
  fclose(f);
  close(fd);
  return 0;
}
