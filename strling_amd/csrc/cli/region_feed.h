// region_feed.h -- how the region entry points (strl_regions_fetch, strl_regions_evidence, strl_pull_select, strl_pull_mates) are
// fed, written once and with no device call in it: the index names a region's run of BGZF blocks (plan_region), the runs of many
// regions are laid out as the block tables those calls take (RegionBlocks::add) and read, still compressed, into the caller's
// buffer (RegionBlocks::read: page-locked in `strling call`, a vector in `strling pull`, plain memory in the host test).  Beside
// them the host's stand-in for the device (`strling _region ... plan`) and the retry ladder of `strling pull`'s two passes.
#pragma once
#include <unistd.h>
#include "bam_reader.h"

namespace strl {

// The run of BGZF blocks the walk of one region query (BamReader::read_region) passes through, as far as the index can bound it:
// from the block of the index offset of `beg`'s window up to the block that holds the first record overlapping a later window
// than `end`'s -- and the one behind it --, their sizes read from the block headers and trailers (18 + 8 bytes per block).
// ok = false: the index does not bound the region, the file is laid out unusually (other extra subfields than BC), the run did
// not reach the hinted block within its caps: such a region is read by the host reader.
struct RegionPlan { bool ok = false; uint64_t c_beg = 0, c_end = 0; uint32_t in_block = 0; std::vector<uint32_t> hdr, bsize, isz, crc; };
// `more` (1 = the plan `strling call` uses): that many times the inflated bytes (8 MB) and blocks (4096), and blocks behind the
// hinted one (2)
void plan_region(const BamReader &rd, int fd, int32_t tid, int64_t beg, int64_t end, RegionPlan &P, int more = 1);

// The blocks of several regions as the region entry points take them.  Region r's run lies in the buffer as it lies in the file,
// gzip headers and trailers included, from slices[r].at on: a multiple of 16, so no two runs share a 16-byte line even when
// they name the same file blocks.  Block k of the run has its payload at
//   coff = slices[r].at + (bsize of the run's blocks before k) + hdr[k],  clen = bsize[k] - hdr[k] - 8
// and the region's request req[r] names its rows: first_block, n_blocks, and in_block (<= isize[first_block]) from the plan.
struct RegionBlocks {
  struct Slice { uint64_t file_off, len, at; };
  std::vector<uint64_t> coff;
  std::vector<uint32_t> clen, isize, crc;
  std::vector<strl_region_req> req;           // one per region added: what the caller asked (tid, beg, end) and where its blocks are
  std::vector<Slice> slices;                  // ... and where its run lies in the file and in the buffer
  uint64_t comp_bytes = 0, inflated = 0;      // the buffer read() fills (callers give the device 64 bytes of slack behind it) / the ISIZE sum
  // an ok plan's rows appended, and `q` with its first_block, n_blocks and in_block filled in
  void add(const RegionPlan &P, strl_region_req q) {
    q.first_block = (uint32_t)clen.size(); q.n_blocks = (uint32_t)P.bsize.size(); q.in_block = P.in_block;
    uint64_t o = 0;
    for (size_t k = 0; k < P.bsize.size(); ++k) {
      coff.push_back(comp_bytes + o + P.hdr[k]); clen.push_back(P.bsize[k] - P.hdr[k] - 8); isize.push_back(P.isz[k]); crc.push_back(P.crc[k]);
      inflated += P.isz[k];
      o += P.bsize[k];
    }
    req.push_back(q);
    slices.push_back(Slice{P.c_beg, o, comp_bytes});
    comp_bytes += (o + 15) & ~(uint64_t)15;
  }
  // the region q.tid, q.beg, q.end planned and, if the plan is ok (the value), added
  bool plan_add(const BamReader &rd, int fd, const strl_region_req &q, int more) { RegionPlan P; plan_region(rd, fd, q.tid, q.beg, q.end, P, more); if (P.ok) add(P, q); return P.ok; }
  // the slices of regions [k0, k1) from fd into buf (comp_bytes at least); false: the file ended first or could not be read
  bool read(int fd, uint8_t *buf, size_t k0, size_t k1) const {
    for (size_t k = k0; k < k1; ++k)
      for (uint64_t got = 0; got < slices[k].len;) {
        const ssize_t r = pread(fd, buf + slices[k].at + got, (size_t)(slices[k].len - got), (off_t)(slices[k].file_off + got));
        if (r <= 0) return false;
        got += (uint64_t)r;
      }
    return true;
  }
};

// The host in the device's place.  region_inflate: the blocks of region r by zlib, their CRCs checked, appended to `u`;
// nullptr, or what failed ("zlib", "inflate", "crc").  region_walk: strl_regions_fetch's rule over those bytes from p (the request's in_block) on --
// keep from the first record whose cigar could reach past `beg`, stop at the first record on another reference or at / behind
// `end` -- the records are u[keep, stop); false: the blocks end before the query does (the device passes such a region on).
// As on the device a block_size outside 32 .. 2^28 ends the bytes, and a record whose cigar would leave it is kept without its
// cigar being read: the parser behind the walk reports it (tests/test_region_cases.py holds the two side by side).
const char *region_inflate(const RegionBlocks &B, size_t r, const uint8_t *comp, std::vector<uint8_t> &u);
bool region_walk(const std::vector<uint8_t> &u, size_t p, int32_t tid, int64_t beg, int64_t end, size_t &keep, size_t &stop);

// The ladder an item (a tile, a mate window) of `strling pull` goes down: the device with the plain plan; once more with eight
// times the blocks if its blocks ended before its query did (a pile-up larger than the plan's run) and the index can bound it
// at all; then the host reader.  device_pass(which, more, failed) appends what it could not answer to `failed`.  Returns the
// items left to the host; *retried = how many took the second step.
template <class Bounded, class DevicePass>
std::vector<size_t> region_ladder(const std::vector<size_t> &items, Bounded bounded, DevicePass device_pass, uint64_t *retried = nullptr) {
  std::vector<size_t> failed, again, host;
  device_pass(items, 1, failed);
  for (size_t t : failed) (bounded(t) ? again : host).push_back(t);
  if (retried) *retried = again.size();
  if (!again.empty()) device_pass(again, 8, host);
  return host;
}

}  // namespace strl
