// markdup_host.cpp -- the rule of `strling sort --markdup` (markdup_core.h) through the library, without a device: what markdup.hip
// decides on the resident records, over a host buffer of records in input order (the Python mirror, tests).
#include <string>
#include <vector>
#include "common.h"
#include "markdup_core.h"

using namespace strl;

extern "C" int strl_markdup_host(const uint8_t *records, uint64_t bytes, uint16_t *flags, uint64_t cap, uint64_t *n_records, strl_markdup_info *info) {
  if ((bytes && !records) || !n_records || (cap && !flags)) { set_error("strl_markdup_host: null argument"); return STRL_ERR_ARG; }
  std::vector<uint16_t> f;
  MdupCounts C{};
  std::string why;
  static const uint8_t none = 0;
  const int64_t bad = mdup_host(bytes ? records : &none, bytes, f, &C, why);
  if (bad >= 0) { set_error("malformed BAM record %lld: %s", (long long)bad, why.c_str()); return STRL_ERR_FORMAT; }
  *n_records = f.size();
  if (cap < f.size()) { set_error("strl_markdup_host: %zu records, room for %llu", f.size(), (unsigned long long)cap); return STRL_ERR_CAPACITY; }
  if (!f.empty()) memcpy(flags, f.data(), f.size() * 2);
  if (info) {
    *info = strl_markdup_info{};
    info->n_pairs = C.pairs; info->n_dup_pairs = C.dup_pairs; info->n_fragments = C.fragments; info->n_dup_fragments = C.dup_fragments; info->n_ineligible = C.ineligible;
  }
  return STRL_OK;
}
