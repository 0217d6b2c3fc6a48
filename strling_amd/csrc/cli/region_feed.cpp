// region_feed.cpp -- the planner, the block layout, the host stand-in and nothing of the device (region_feed.h)
#include "region_feed.h"
#include <string.h>
#include <zlib.h>

namespace strl {

void plan_region(const BamReader &rd, int fd, int32_t tid, int64_t beg, int64_t end, RegionPlan &P, int more) {
  uint64_t c_hint = 0;
  P.ok = false;
  if (!rd.region_span(tid, beg, end, P.c_beg, P.in_block, c_hint)) return;
  uint64_t o = P.c_beg, infl = 0;
  int beyond = 0;
  bool good = true;
  while (beyond < 2 * more && infl < ((uint64_t)8 << 20) * (uint64_t)more && P.bsize.size() < (size_t)4096 * (size_t)more) {   // (a window of 30x data is ~1 MB)
    uint8_t h[18], tr[8];
    if (pread(fd, h, 18, (off_t)o) != 18) break;                                  // end of the file
    const uint32_t xlen = h[10] | (h[11] << 8);
    if (h[0] != 0x1f || h[1] != 0x8b || h[2] != 8 || !(h[3] & 4) || xlen != 6 || h[12] != 'B' || h[13] != 'C') { good = false; break; }
    const uint32_t bsize = (h[16] | (h[17] << 8)) + 1u;
    if (bsize < 26 || pread(fd, tr, 8, (off_t)(o + bsize - 8)) != 8) { good = false; break; }
    uint32_t crc, isz;
    memcpy(&crc, tr, 4); memcpy(&isz, tr + 4, 4);
    if (isz > 65536u) { good = false; break; }
    P.hdr.push_back(18); P.bsize.push_back(bsize); P.isz.push_back(isz); P.crc.push_back(crc);
    infl += isz;
    if (o >= c_hint) ++beyond;
    o += bsize;
  }
  P.c_end = o;
  // the first block must hold the index offset; a run that did not reach the hinted block goes to the host reader
  P.ok = good && beyond >= 1 && !P.bsize.empty() && P.in_block <= P.isz[0];
}

const char *region_inflate(const RegionBlocks &B, size_t r, const uint8_t *comp, std::vector<uint8_t> &u) {
  for (size_t k = B.req[r].first_block; k < (size_t)B.req[r].first_block + B.req[r].n_blocks; ++k) {
    const size_t at = u.size();
    u.resize(at + B.isize[k]);
    z_stream zs = {};
    if (inflateInit2(&zs, -15) != Z_OK) return "zlib";
    zs.next_in = const_cast<uint8_t *>(comp + B.coff[k]); zs.avail_in = B.clen[k];
    zs.next_out = u.data() + at; zs.avail_out = B.isize[k];
    const bool whole = inflate(&zs, Z_FINISH) == Z_STREAM_END && zs.total_out == B.isize[k];
    inflateEnd(&zs);
    if (!whole) return "inflate";
    if ((uint32_t)crc32(0, u.data() + at, B.isize[k]) != B.crc[k]) return "crc";
  }
  return nullptr;
}

bool region_walk(const std::vector<uint8_t> &u, size_t p, int32_t tid, int64_t beg, int64_t end, size_t &keep, size_t &stop) {
  bool stopped = false;
  keep = SIZE_MAX;
  while (p + 36 <= u.size()) {
    int32_t bs, ref, pos;
    memcpy(&bs, &u[p], 4); memcpy(&ref, &u[p + 4], 4); memcpy(&pos, &u[p + 8], 4);
    if (bs < 32 || bs > (1 << 28)) break;                                        // not a record: the blocks "end" here, as on the device
    if (ref != tid || pos >= end) { stopped = true; break; }
    if (p + 4 + (size_t)bs > u.size()) break;
    if (keep == SIZE_MAX) {
      const uint32_t l_name = u[p + 12];
      uint16_t n_cig;
      memcpy(&n_cig, &u[p + 16], 2);
      int64_t span = 1;
      if (36 + (size_t)l_name + 4 * (size_t)n_cig <= 4 + (size_t)bs)
        for (uint32_t k = 0; k < n_cig; ++k) { uint32_t c; memcpy(&c, &u[p + 36 + l_name + 4 * k], 4); span += c >> 4; }
      else span = (int64_t)1 << 40;              // a cigar that leaves its record is never read: the record is kept, and the parser behind the walk reports it
      if ((int64_t)pos + span > beg) keep = p;
    }
    p += 4 + (size_t)bs;
  }
  if (keep == SIZE_MAX) keep = p;
  stop = p;
  return stopped;
}

}  // namespace strl
