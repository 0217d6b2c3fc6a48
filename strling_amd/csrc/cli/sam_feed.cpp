// sam_feed.cpp -- see sam_feed.h
#include "sam_feed.h"
#include <errno.h>
#include <fcntl.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#include <algorithm>

namespace strl {

namespace {
constexpr size_t STEP = 1 << 16;                 // bytes a read asks for while it looks for a line's end
size_t chunk_target() {
  const char *e = getenv("STRL_SAM_CHUNK_KB");   // tests: chunks of a line or two (fractions allowed)
  const double kb = e ? atof(e) : 0.0;
  return kb > 0 ? std::max<size_t>(1, (size_t)(kb * 1024.0)) : (size_t)32 << 20;
}
}  // namespace

SamFeed::~SamFeed() { if (own_ && fd_ >= 0) close(fd_); }

// up to `want` more bytes behind v's end; false: a read error.  Sets eof_
bool SamFeed::fill(std::vector<uint8_t> &v, size_t want, std::string &err) {
  const size_t at = v.size();
  v.resize(at + want);
  size_t got = 0;
  while (got < want && !eof_) {
    const ssize_t r = read(fd_, v.data() + at + got, want - got);
    if (r < 0) { if (errno == EINTR) continue; err = std::string("read: ") + strerror(errno); v.resize(at + got); return false; }
    if (!r) eof_ = true;
    got += (size_t)r;
  }
  v.resize(at + got);
  bytes_read += got;
  return true;
}

SamFeed::Kind SamFeed::open(const std::string &path, std::string &err) {
  if (path == "-") fd_ = 0;
  else {
    fd_ = ::open(path.c_str(), O_RDONLY);
    own_ = true;
    if (fd_ < 0) { err = "couldn't open " + path + ": " + strerror(errno); return KIND_ERROR; }
  }
  target_ = chunk_target();
  if (!fill(carry_, 4, err)) return KIND_ERROR;
  if (carry_.size() >= 2 && carry_[0] == 0x1f && carry_[1] == 0x8b) return KIND_GZIP;
  if (!carry_.empty() && (carry_[0] == '@' || (carry_[0] >= 0x20 && carry_[0] < 0x7f))) return KIND_SAM;
  return KIND_OTHER;
}

bool SamFeed::read_header(SamHeader &H, std::string &err) {
  // the header ends at the first line that does not begin with @, or at the end of the text
  size_t at = 0;
  for (;;) {
    bool more = false;
    while (at < carry_.size() && carry_[at] == '@') {
      const void *nl = memchr(carry_.data() + at, '\n', carry_.size() - at);
      if (!nl) { more = true; break; }
      at = (size_t)(static_cast<const uint8_t *>(nl) - carry_.data()) + 1;
    }
    if (at >= carry_.size()) more = true;
    if (!more || eof_) break;
    if (!fill(carry_, (size_t)1 << 20, err)) return false;
  }
  if (!sam_header(carry_.data(), carry_.size(), H, err)) return false;
  carry_.erase(carry_.begin(), carry_.begin() + (ptrdiff_t)H.used);
  return true;
}

size_t SamFeed::buffer_bytes() const { return std::max<size_t>(target_, (size_t)SAM_LINE_MAX + 16) + STEP + 64; }

int64_t SamFeed::next_chunk(uint8_t *buf, std::string &err) {
  if (poisoned_) { err = "SAM text: a line of more than " + std::to_string(SAM_LINE_MAX) + " bytes"; return -1; }
  const size_t line_limit = (size_t)SAM_LINE_MAX + 16;
  size_t have = 0;
  // what an earlier cut left (the first time: what was read behind the header, which may be more than a chunk)
  auto pull = [&](size_t want) -> bool {
    if (!carry_.empty()) {
      const size_t n = std::min(want, carry_.size());
      memcpy(buf + have, carry_.data(), n);
      carry_.erase(carry_.begin(), carry_.begin() + (ptrdiff_t)n);
      have += n;
      return true;
    }
    while (!eof_) {
      const ssize_t r = read(fd_, buf + have, want);
      if (r < 0) { if (errno == EINTR) continue; err = std::string("read: ") + strerror(errno); return false; }
      if (!r) eof_ = true;
      have += (size_t)r; bytes_read += (size_t)r;
      break;
    }
    return true;
  };
  while (have < target_ && !(eof_ && carry_.empty())) if (!pull(target_ - have)) return -1;
  if (!have) return 0;
  const uint8_t *last = static_cast<const uint8_t *>(memrchr(buf, '\n', have));
  size_t cut;                                                      // the chunk is buf[0, cut)
  if (last) cut = (size_t)(last - buf) + 1;
  else {
    // one line longer than a chunk: on to its end
    size_t seen = 0;
    const uint8_t *nl = nullptr;
    for (;;) {
      nl = static_cast<const uint8_t *>(memchr(buf + seen, '\n', have - seen));
      seen = have;
      if (nl || (eof_ && carry_.empty()) || have >= line_limit) break;
      if (!pull(std::min(STEP, line_limit + STEP - have))) return -1;
    }
    if (nl) cut = (size_t)(nl - buf) + 1;
    else if (have < line_limit) { buf[have++] = '\n'; cut = have; }      // the last line of the text, without a newline
    else {
      // the encoder refuses a line this long, and counts the lines before it: it gets the line's beginning as a line
      buf[line_limit - 1] = '\n';
      poisoned_ = true;
      return (int64_t)line_limit;
    }
  }
  if (cut < have) carry_.insert(carry_.begin(), buf + cut, buf + have);
  return (int64_t)cut;
}

}  // namespace strl
