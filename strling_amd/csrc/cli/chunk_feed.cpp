// chunk_feed.cpp -- staging a chunk of BGZF blocks for the device, the read-ahead ring, the fragment-length accumulator (chunk_feed.h)
#include "chunk_feed.h"
#include <stdio.h>
#include <algorithm>
#include <atomic>
#include <chrono>

namespace strl {

StagedChunk stage_chunk(BgzfFeed &feed, ThreadPool &pool, size_t max_blocks, size_t max_bytes, uint8_t *data, uint8_t *meta, size_t chunk_blocks, bool want_last) {
  auto now = [] { return std::chrono::steady_clock::now(); };
  auto secs = [](std::chrono::steady_clock::time_point x, std::chrono::steady_clock::time_point y) { return std::chrono::duration<double>(y - x).count(); };
  const auto ta = now();
  StagedChunk S;
  std::vector<BgzfFeed::Block> bl;
  S.nb = feed.next(bl, max_blocks, max_bytes, S.err, want_last ? &S.last : nullptr);
  if (S.nb <= 0) return S;
  const auto tb = now();
  S.lo = bl.front().c_off; S.hi = bl.back().c_off + bl.back().clen;
  const size_t lo = S.lo, hi = S.hi, piece = (size_t)4 << 20, pieces = (hi - lo + piece - 1) / piece;
  std::atomic<int> short_reads{0};
  pool.parallel_for(pieces, [&](size_t k) { if (!feed.copy_at(data + k * piece, lo + k * piece, std::min(piece, hi - lo - k * piece))) ++short_reads; });
  feed.done_with(lo, hi - lo);        // (once per chunk, by this thread: per 4 MB piece it was a round of TLB shoot-downs per piece on every copying CPU)
  S.short_read = short_reads.load() != 0;
  const ChunkTables t = tables_of(meta, chunk_blocks);
  for (size_t k = 0; k < (size_t)S.nb; ++k) {      // a block starts at its gzip header (boff); coff is where its payload sits in `data`
    t.coff[k] = bl[k].c_off - lo; t.boff[k] = bl[k].c_off - bl[k].hdr; t.clen[k] = bl[k].clen; t.isz[k] = bl[k].isize; t.crc[k] = bl[k].crc;
  }
  S.t_walk = secs(ta, tb); S.t_copy = secs(tb, now());
  return S;
}

void ChunkAhead::stage(uint64_t ci, size_t slot) {
  // (a short first chunk gets the device going while the second is being copied)
  const size_t max_blocks = ci == 0 && first_blocks ? std::min(chunk_blocks_, first_blocks) : chunk_blocks_;
  StagedChunk &S = ring_[ci % 3];
  S = stage_chunk(feed_, pool_, max_blocks, chunk_bytes_, data_[slot], meta_[slot], chunk_blocks_, want_last_);
  S.slot = slot;
  t_walk += S.t_walk; t_copy += S.t_copy;
  if (S.nb > 0) { bytes += S.bytes(); ++chunks; }
}

void FragLengths::finish(uint32_t out[4096]) {
  uint64_t sum = 0;
  for (int k = 0; k < 4096; ++k) sum += frag[k];
  if ((uint32_t)sum == 0) {
    fprintf(stderr, "using first reads in fragment_length_distribution calculation as there were not enough\n");
    for (int32_t is : skipped) frag[is]++;
  }
  std::copy(frag, frag + 4096, out);
}

}  // namespace strl
