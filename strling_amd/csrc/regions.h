// regions.h -- what the region entry points (bgzf.hip: strl_regions_fetch; evidence.hip: strl_evidence_records,
// strl_regions_evidence) and the host side of the evidence (call_logic.cpp) share.
#pragma once
#include <vector>
#include "common.h"
#include "evidence_core.h"

namespace strl {

struct RegionWalk { uint64_t start, stop; };   // bytes [start, stop) of the inflated stream: the records one region query returns

// A region slot of the context held for one call: its stream and its buffers (kept between calls: freeing gigabytes
// synchronises the device).  Two calls of different host threads run side by side, one per slot.  The slot's stream is
// drained before the slot -- and the host memory its copies read and write: the members below -- is given up, whichever way
// the caller is left: an early error return must not leave DMA pending on destroyed memory.
struct RegionJob {
  strl_ctx *c = nullptr;
  strl_ctx::RegionSlot *slot = nullptr;
  std::vector<uint64_t> uoff;           // where every block's inflated bytes start in slot->u
  std::vector<RegionWalk> range;        // per region, after regions_inflate_walk
  uint64_t tot = 0;                     // inflated bytes of all blocks
  uint32_t err = 0;                     // IW_ERR_* flags of the blocks
  RegionWalk *d_range = nullptr;        // device copies (in slot->rq)
  uint64_t *d_off = nullptr;
  uint8_t *d_status = nullptr;
  int acquire(strl_ctx *ctx, bool want_crc);
  hipStream_t stream() const { return slot->st; }
  ~RegionJob();
};
// copy the blocks in, inflate them, check their CRC-32 (crc32 != NULL), walk every region (region_walk_kernel), and wait:
// J.range / status[] hold the result.  STRL_ERR_CRC / STRL_ERR_FORMAT as strl_regions_fetch documents them.
int regions_inflate_walk(RegionJob &J, const uint8_t *comp, uint64_t comp_bytes, const uint64_t *coff, const uint32_t *clen, const uint32_t *isize,
                         const uint32_t *crc32, uint32_t n_blocks, const strl_region_req *req, uint32_t n_regions, uint8_t *status);

// ---- evidence around a bound (evidence.hip) ----
// (EV_MAX_RECORDS, EV_MAX_SPAN, EvRow: evidence_core.h, which the host emulation of the per-record rule reads too)

// call_logic.cpp: the tables spanners() derives from the fragment histogram (made once per histogram and thread), and the
// order-dependent steps of spanners() -- the fold per qname in record order, the float32 sum in Table slot order, the pair
// list, the spanning fragments in slot order -- over the rows of one region.  Returns 0, or 2 where the reference's doAssert
// L.start <= R.start would fire (the host path reports that one).
const float *frag_cd(const uint32_t frag[4096]);
int evidence_finish(const EvRow *rows, uint32_t n, const strl_bounds &b, const uint32_t frag[4096], strl_support *out, uint64_t cap, uint64_t *n_out,
                    float *expected_spanners);
// evidence.hip: the evidence of n_regions regions whose record bytes are u[range[r].start, range[r].stop) on the device
// (h_count, if given: the number of records in each range, from which the rows are reserved instead of from the bytes)
int evidence_run(RegionJob &J, const uint8_t *d_u, uint64_t u_readable, const RegionWalk *d_range, const RegionWalk *h_range, uint32_t n_regions,
                 const strl_bounds *bounds, int32_t window, const uint32_t frag[4096], uint8_t min_mapq, strl_support *out, uint64_t cap,
                 uint64_t *support_off, strl_span_summary *summary, uint8_t *status, double *kernel_ms, const uint32_t *h_count = nullptr);

}  // namespace strl
