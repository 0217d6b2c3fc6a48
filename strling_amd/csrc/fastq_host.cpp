// fastq_host.cpp -- the rule of `strling fastq` (fastq_core.h) through the library, without a device: what fastq.hip lays out and
// writes from the resident records, over a host buffer of records in input order (the Python mirror, tests).
#include <string>
#include <vector>
#include "common.h"
#include "fastq_core.h"

using namespace strl;

extern "C" int strl_fastq_host(const uint8_t *records, uint64_t bytes, const strl_fastq_opts *opts, uint8_t *const out[3], const uint64_t cap[3], strl_fastq_info *info) {
  if ((bytes && !records) || !opts || !info || !cap) { set_error("strl_fastq_host: null argument"); return STRL_ERR_ARG; }
  const FastqOpts o{opts->filter, opts->suffix ? 1u : 0u, opts->default_qual, opts->interleaved ? 1u : 0u, opts->singles ? 1u : 0u};
  std::vector<uint8_t> stream[3];
  FastqCounts C{};
  std::string why;
  static const uint8_t none = 0;
  const int64_t bad = fastq_host(bytes ? records : &none, bytes, o, stream, &C, why);
  if (bad >= 0) { set_error("malformed BAM record %lld: %s", (long long)bad, why.c_str()); return STRL_ERR_FORMAT; }
  *info = strl_fastq_info{};
  info->n_kept = C.kept; info->n_filtered = C.filtered; info->n_empty = C.empty; info->n_pairs = C.pairs; info->n_singles = C.singles; info->n_singles_unwritten = C.singles_unwritten;
  for (int s = 0; s < 3; ++s) info->stream_bytes[s] = stream[s].size();
  for (int s = 0; s < 3; ++s)
    if (cap[s] < stream[s].size() || (!stream[s].empty() && (!out || !out[s]))) {
      set_error("strl_fastq_host: stream %d holds %zu bytes, room for %llu", s, stream[s].size(), (unsigned long long)cap[s]);
      return STRL_ERR_CAPACITY;
    }
  for (int s = 0; s < 3; ++s) if (!stream[s].empty()) memcpy(out[s], stream[s].data(), stream[s].size());
  return STRL_OK;
}
