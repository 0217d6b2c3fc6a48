// score.h -- what score.hip shares with the translation units around it (context.hip, extract.hip, front_abi.hip).
#pragma once
#include "common.h"

namespace strl {

// per-tid view of the genome STR table (32 B, one or two cache lines for a whole genome's contigs)
struct TidInfo {
  int64_t iv_off;    // first interval of the tid in g_start
  int64_t bin_off;   // first bin of the tid in g_bins
  int32_t n_iv;      // intervals of the tid
  int32_t n_bins;    // bins of the tid (bin b covers starts in [b << BIN_SHIFT, (b+1) << BIN_SHIFT))
  int32_t has;       // chromosome is a key of the table (extract.nim:30)
  int32_t pad;
};
constexpr int BIN_SHIFT = 12;

constexpr uint64_t RING = 256;
// events per recorded strl_score_reads call: start | classify | stage A, compaction, stage B (whole reads) | soft-item
// compaction | stage A, compaction, stage B (segments)
constexpr int EV_PER = 9;

// grid of a compaction kernel (compact_kernel, soft_compact_kernel, pair_soft_items_kernel): STRL_GRID_K when set, else `dflt`
int compact_grid(int dflt);

}  // namespace strl

// one scoring pass over a device-resident batch (classify, scorer, segments, the long reads), enqueued on the context's stream
int score_device(strl_ctx *c, const strl_read_soa *s, uint32_t *whole, strl_soft_rec *soft, uint64_t soft_cap, uint64_t *n_soft,
                 strl_score_stats *stats, bool sync_counts, const strl_pair_soa *pp = nullptr, bool fresh_bloom = true,
                 bool side_busy_ok = false);
// host-memory batch -> staging buffers in HBM (asynchronous copies on the context stream)
int stage_batch(strl_ctx *c, const strl_read_soa *s, const strl_pair_soa *pp, strl_read_soa *d, strl_pair_soa *dpp);
// Bloom bitmap of the hot qname groups, sized for n reads and zeroed
int bloom_reset(strl_ctx *c, uint64_t n);
