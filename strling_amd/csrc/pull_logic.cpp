// pull_logic.cpp -- the rules of `strling pull` (extract_region.nim) over raw BAM record bytes, on the host: what pull.hip
// computes on the device, for the tiles and windows the device passes on, for STRL_PULL=host and for machines without a device.
#include <string.h>
#include <algorithm>
#include <numeric>
#include <string>
#include <unordered_map>
#include <vector>
#include "common.h"
#include "nim_tables.h"
#include "pull_rec.h"

using namespace strl;

namespace {

// the record at `at` when it lies inside `left` bytes
bool load_rec(PlRec &R, const uint8_t *at, uint64_t left) {
  if (!pl_plausible(at, left)) return false;
  R.load(at);
  return true;
}

}  // namespace

// extract_region.nim:46-48 behind htslib's iterator filter, for one tile of a region
extern "C" int strl_pull_select_host(const uint8_t *bytes, uint64_t n_bytes, const strl_pull_tile *tile, uint64_t base_off, strl_pull_row *rows,
                                     uint64_t row_cap, uint64_t *n_rows) {
  if ((n_bytes && !bytes) || !tile || !n_rows || (row_cap && !rows)) { set_error("null argument"); return STRL_ERR_ARG; }
  uint64_t n = *n_rows;
  for (uint64_t at = 0; at < n_bytes;) {
    PlRec R;
    if (!load_rec(R, bytes + at, n_bytes - at)) { set_error("corrupt BAM record"); return STRL_ERR_FORMAT; }
    const bool kept = R.kept_by(*tile);
    if (kept) {
      if (n < row_cap) rows[n] = R.row(base_off + at, R.hash());
      ++n;
    }
    at += 4ull + R.bs;
  }
  *n_rows = n;
  if (n > row_cap) { set_error("pull: %llu rows, room for %llu", (unsigned long long)n, (unsigned long long)row_cap); return STRL_ERR_CAPACITY; }
  return STRL_OK;
}

// counts[qname] (:44,50): the table's key is the name's bytes
extern "C" int strl_pull_counts_host(const uint8_t *bytes, strl_pull_row *rows, uint64_t n) {
  if (n && (!bytes || !rows)) { set_error("null argument"); return STRL_ERR_ARG; }
  std::unordered_map<std::string, uint32_t> counts;
  counts.reserve((size_t)n * 2);
  auto name = [&](const strl_pull_row &r) { return std::string(reinterpret_cast<const char *>(bytes + r.off + 36), r.l_name ? r.l_name - 1u : 0u); };
  for (uint64_t i = 0; i < n; ++i) ++counts[name(rows[i])];
  for (uint64_t i = 0; i < n; ++i) rows[i].count = counts[name(rows[i])];
  return STRL_OK;
}

// get_mate (:7-19) for many requests over one stretch of records: the records are visited once, in file order, and a request
// keeps the first record that meets its rule
extern "C" int strl_pull_mates_host(const uint8_t *bytes, uint64_t n_bytes, int use_interval, int32_t tid, const strl_pull_req *reqs, uint32_t n_req,
                                    const uint8_t *names, uint64_t base_off, strl_pull_row *rows) {
  if ((n_bytes && !bytes) || (n_req && (!reqs || !rows))) { set_error("null argument"); return STRL_ERR_ARG; }
  std::unordered_multimap<uint32_t, uint32_t> open;          // hash -> request, the unanswered ones
  for (uint32_t k = 0; k < n_req; ++k) if (!rows[k].found) open.emplace(reqs[k].hash, k);
  for (uint64_t at = 0; at < n_bytes && !open.empty();) {
    PlRec R;
    if (!load_rec(R, bytes + at, n_bytes - at)) { set_error("corrupt BAM record"); return STRL_ERR_FORMAT; }
    if (!(R.flag & 0x900u) && (!use_interval || R.tid == tid)) {
      const uint32_t h = R.hash();
      int64_t stop = -1;
      for (auto it = open.find(h); it != open.end() && it->first == h;) {
        const strl_pull_req &Q = reqs[it->second];
        bool hit = ((R.flag ^ Q.flag) & 0x40u) && Q.name_len == R.name_len() && (Q.name_len == 0 || !memcmp(names + Q.name_off, R.p + 36, Q.name_len));
        if (hit && use_interval) {
          if (stop < 0) stop = R.stop();
          hit = R.pos < Q.end && stop > (int64_t)Q.beg;
        }
        if (hit) {
          rows[it->second] = R.row(base_off + at, h);
          it = open.erase(it);
        } else ++it;
      }
    }
    at += 4ull + R.bs;
  }
  return STRL_OK;
}

// records.sort (:65-68): tid, then start, as signed integers; Nim's sort is a stable merge sort
extern "C" int strl_pull_order(const strl_pull_row *rows, uint64_t n, uint32_t *order) {
  if (n && (!rows || !order)) { set_error("null argument"); return STRL_ERR_ARG; }
  if (n > 0xffffffffull) { set_error("pull: %llu records", (unsigned long long)n); return STRL_ERR_LIMIT; }
  std::iota(order, order + n, 0u);
  std::stable_sort(order, order + n, [&](uint32_t a, uint32_t b) {
    if (rows[a].tid != rows[b].tid) return rows[a].tid < rows[b].tid;
    return rows[a].pos < rows[b].pos;
  });
  return STRL_OK;
}
