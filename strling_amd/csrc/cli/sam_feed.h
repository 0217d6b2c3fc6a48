// sam_feed.h -- `strling sort`'s reader of SAM text, from a file or from stdin: no mapping (a pipe has none), plain reads into the
// caller's buffers, each chunk cut behind its last newline and the rest carried into the next.  DESIGN section 24.2.
#pragma once
#include <stdint.h>
#include <string>
#include <vector>
#include "../sam_core.h"

namespace strl {

struct SamFeed {
  enum Kind { KIND_SAM, KIND_GZIP, KIND_OTHER, KIND_ERROR };
  ~SamFeed();
  // path "-" = stdin.  -> what the first bytes say: BGZF / gzip magic, `@` or another printable byte (SAM), anything else (an empty
  // file included).  The bytes read for it stay with the feed
  Kind open(const std::string &path, std::string &err);
  // the leading @ lines, read to their end -> H; what was read behind them is the first chunk's beginning
  bool read_header(SamHeader &H, std::string &err);
  // bytes a caller's buffer must hold: the chunk size (STRL_SAM_CHUNK_KB, fractions allowed; default 32 MiB), and at least a line
  // of SAM_LINE_MAX bytes -- a chunk is never less than one whole line
  size_t buffer_bytes() const;
  // the next chunk of whole lines into buf[0, buffer_bytes()), its last byte a newline (added behind a last line that has none).
  // A chunk takes lines up to the chunk size, or one line where that line alone is longer.  -> bytes; 0 at the end; -1: err
  int64_t next_chunk(uint8_t *buf, std::string &err);
  uint64_t bytes_read = 0;

 private:
  int fd_ = -1;
  bool own_ = false, eof_ = false, poisoned_ = false;
  size_t target_ = 0;
  std::vector<uint8_t> carry_;     // read, not yet handed out
  bool fill(std::vector<uint8_t> &v, size_t want, std::string &err);
};

}  // namespace strl
