// view_host.cpp -- the rule of `strling view` (view_core.h) through the library, without a device: what view.hip sizes and writes
// per chunk, over a host buffer of records (the host path of the command, the Python mirror, tests).
#include <string>
#include <vector>
#include "common.h"
#include "view_core.h"

using namespace strl;

extern "C" int strl_view_host(const uint8_t *records, uint64_t bytes, const uint8_t *names, const uint32_t *name_off, int32_t n_ref, const strl_view_opts *opts, uint8_t *out,
                              uint64_t cap, uint64_t *out_bytes, strl_view_info *info) {
  if ((bytes && !records) || !opts || !out_bytes || n_ref < 0 || (n_ref && (!names || !name_off))) { set_error("strl_view_host: bad argument"); return STRL_ERR_ARG; }
  const ViewOpts o{opts->require, opts->exclude, opts->exclude_all, opts->min_mapq, opts->tid, opts->beg, opts->end};
  const ViewRefs F{names, name_off, n_ref};
  std::vector<uint8_t> text;
  ViewCounts C{};
  uint32_t code = 0;
  static const uint8_t none = 0;
  const int64_t bad = view_host(bytes ? records : &none, bytes, F, o, text, &C, 0, &code);
  if (bad >= 0) { set_error("malformed BAM record %lld: %s", (long long)bad, view_refusal_text(code)); return STRL_ERR_FORMAT; }
  if (info) {
    *info = strl_view_info{};
    info->records = C.records; info->written = C.written; info->dropped = C.dropped; info->text_bytes = C.text_bytes;
  }
  *out_bytes = text.size();
  if (cap < text.size() || (!text.empty() && !out)) { set_error("strl_view_host: the text holds %zu bytes, room for %llu", text.size(), (unsigned long long)cap); return STRL_ERR_CAPACITY; }
  if (!text.empty()) memcpy(out, text.data(), text.size());
  return STRL_OK;
}
