// chunk_feed.h -- how every device pass over a BAM (extract, bamindex, call's fragment sample) is fed, written once and with no
// device call in it: BgzfFeed names a run of consecutive blocks, their bytes are copied -- still compressed -- into one buffer in
// 4 MB pieces on a thread pool, the block table goes into a second buffer, and a thread stages a later chunk beside the push of
// the current one (ChunkAhead).  The buffers are the caller's (page-locked in `strling`, plain memory in the host test).
#pragma once
#include <stdint.h>
#include <string>
#include <thread>
#include <vector>
#include "bam_reader.h"
#include "bgzf_feed.h"

namespace strl {

// The block table of a chunk of at most chunk_blocks blocks, one layout for every caller:
//   coff u64 (payload offset in the data buffer) | boff u64 (file offset of the block's gzip header) | clen | isize | crc u32
struct ChunkTables { uint64_t *coff, *boff; uint32_t *clen, *isz, *crc; };
inline size_t chunk_table_bytes(size_t chunk_blocks) { return chunk_blocks * 28 + 64; }
inline size_t chunk_data_bytes(size_t chunk_bytes) { return chunk_bytes + 64; }
inline ChunkTables tables_of(uint8_t *meta, size_t chunk_blocks) {
  uint64_t *coff = reinterpret_cast<uint64_t *>(meta), *boff = coff + chunk_blocks;
  uint32_t *clen = reinterpret_cast<uint32_t *>(boff + chunk_blocks);
  return ChunkTables{coff, boff, clen, clen + chunk_blocks, clen + 2 * chunk_blocks};
}

struct StagedChunk {
  int64_t nb = 0;               // blocks; 0 at the end of the file / share, < 0: a malformed file (err)
  size_t lo = 0, hi = 0;        // file offsets: first block's payload .. last block's payload end
  size_t slot = 0;              // the buffer it was staged into (ChunkAhead)
  bool last = false, short_read = false;     // last: the run reaches the end of the share (only when asked for)
  std::string err;
  double t_walk = 0, t_copy = 0;                 // seconds waiting for the header walker / copying and filling the table
  size_t end_off() const { return hi + 8; }      // CRC-32 and ISIZE close the last block
  size_t bytes() const { return hi - lo; }
};

// The next run of at most max_blocks blocks / max_bytes of file from `feed` into data (chunk_data_bytes(max_bytes) at least) and
// its table into meta (chunk_table_bytes(chunk_blocks), chunk_blocks >= max_blocks).  want_last: waits until the walker can tell
// whether the run is the share's last.
StagedChunk stage_chunk(BgzfFeed &feed, ThreadPool &pool, size_t max_blocks, size_t max_bytes, uint8_t *data, uint8_t *meta, size_t chunk_blocks, bool want_last);

// The read-ahead every pass shares: chunk ci sits in ring[ci % 3] while it is handed to the device, a thread stages a later chunk
// (one or two ahead, into the buffer `slot`: the caller says which) into another entry meanwhile and is joined before the next turn.
class ChunkAhead {
 public:
  ChunkAhead(BgzfFeed &feed, ThreadPool &pool, uint8_t *const *data, uint8_t *const *meta, size_t chunk_blocks, size_t chunk_bytes, bool want_last = false)
      : feed_(feed), pool_(pool), data_(data), meta_(meta), chunk_blocks_(chunk_blocks), chunk_bytes_(chunk_bytes), want_last_(want_last) {}
  ~ChunkAhead() { join(); }
  size_t first_blocks = 0;                          // > 0: chunk 0 is cut short at that many blocks
  void stage(uint64_t ci, size_t slot);             // on the calling thread
  void stage_ahead(uint64_t ci, size_t slot) { ahead_ = std::thread([this, ci, slot] { stage(ci, slot); }); }
  void join() { if (ahead_.joinable()) ahead_.join(); }
  void clear(uint64_t ci) { ring_[ci % 3] = StagedChunk{}; }
  const StagedChunk &at(uint64_t ci) const { return ring_[ci % 3]; }
  ChunkTables tables(const StagedChunk &S) const { return tables_of(meta_[S.slot], chunk_blocks_); }
  uint8_t *data(const StagedChunk &S) const { return data_[S.slot]; }
  double t_walk = 0, t_copy = 0;                    // summed over the chunks staged
  uint64_t bytes = 0, chunks = 0;

 private:
  BgzfFeed &feed_;
  ThreadPool &pool_;
  uint8_t *const *data_, *const *meta_;
  size_t chunk_blocks_, chunk_bytes_; bool want_last_;
  StagedChunk ring_[3];
  std::thread ahead_;
};

// fragment_length_distribution (utils.nim:86-111): the histogram of the insert sizes of proper pairs that are neither secondary nor
// supplementary, over 2 000 000 records behind the first 100 000 of the file; a file with nothing behind those takes the skipped
// ones.  `isize` is taken unsigned, so the host reader's `isize < 0 || isize > 4095` and the unsigned `> 4095` on the 16 bits the
// device's parse keeps of it are one test.
struct FragLengths {
  static constexpr int64_t n_reads = 2000000, skip_reads = 100000;
  uint32_t frag[4096] = {};
  std::vector<int32_t> skipped;
  int64_t counted = 0;
  uint64_t next = 0;            // add_words: the first record not looked at yet
  bool full = false;
  void add(uint32_t flag, uint32_t isize, int64_t record_index) {
    if (!(flag & 0x2) || (flag & (0x800 | 0x100)) || isize > 4095u) return;
    if (record_index < skip_reads) { skipped.push_back((int32_t)isize); return; }
    skipped.clear();
    frag[isize]++;
    if (++counted > n_reads) full = true;
  }
  // the device front end's words of records [first, first + n): flag | isize << 16
  void add_words(const uint32_t *fw, uint64_t first, uint64_t n) {
    for (uint64_t k = 0; k < n && !full; ++k) add(fw[k] & 0xffffu, fw[k] >> 16, (int64_t)(first + k));
    next = first + n;
  }
  bool done() const { return full; }
  void finish(uint32_t out[4096]);      // the histogram, or the skipped reads' with the reference's message
};

}  // namespace strl
