// bamindex_host.cpp -- see bamindex_host.h.  One record at a time, in the file's order, what bamindex.hip's bai_record_body does a
// lane per record: refusals, bin, the linear index's windows, the per-reference span and counts, a run per change of (tid, bin);
// at the end the runs sorted by key (stable), runs that touch merged, and bai_pack.
#include "bamindex_host.h"
#include <algorithm>

namespace strl {

bool HostIndex::begin(int32_t n_ref, const int32_t *l_ref, int32_t csi_min_shift, int32_t csi_depth, std::string &err) {
  const int32_t csi[2] = {csi_min_shift, csi_depth};
  csi_ = csi_min_shift >= 0;
  auto_depth_ = csi_ && csi_depth < 0;
  if (n_ref < 0 || (n_ref && !l_ref)) { err = "bad argument"; return false; }
  if (!bai_scheme_make(csi_ ? csi : nullptr, n_ref, l_ref, sch_, err)) return false;
  n_ref_ = n_ref;
  bai_windows(sch_, n_ref, l_ref, win_off_);
  lin_.assign((size_t)win_off_[(size_t)n_ref], ~0ull);
  ref_beg_.assign((size_t)n_ref, ~0ull);
  ref_end_.assign((size_t)n_ref, 0);
  ref_cnt_.assign(2 * (size_t)n_ref, 0);
  for (uint64_t &e : err_ord_) e = ~0ull;
  runs_.clear();
  n_records = n_no_coor = n_runs = n_chunks = 0;
  pkey_ = BAI_KEY_NONE; ptid_ = 0; ppos_ = -1; pwin_ = -1; pend_v_ = pend_abs_ = 0;
  return true;
}

void HostIndex::add(const uint8_t *rec, uint32_t len, uint64_t beg_v, uint64_t end_v, uint64_t beg_abs, uint64_t end_abs) {
  const uint64_t ord = n_records++;
  const int32_t m = sch_.min_shift;
  BaiRec r;
  if (!bai_read_bounded(rec, len, r)) r = BaiRec{-2, -1, 0, 0, 0};
  const int bad = bai_refusal_rule(r.tid, r.pos, r.end, n_ref_, sch_.max_end, m, [&](int32_t t) { return win_off_[(size_t)t + 1] - win_off_[(size_t)t]; });
  if (bad >= 0 && err_ord_[bad] == ~0ull) err_ord_[bad] = ord;
  const bool placed = r.tid >= 0 && bad < 0;
  const bool bai = m == 14 && sch_.depth == 5;
  const uint64_t key = placed ? ((uint64_t)(uint32_t)r.tid << sch_.key_shift) | (bai ? bai_reg2bin(r.pos, r.end) : csi_reg2bin(r.pos, r.end, m, sch_.depth))
                              : (uint64_t)(uint32_t)n_ref_ << sch_.key_shift;
  const int32_t end_win = placed ? (r.end - 1) >> m : -1;
  // coordinate order: (tid, pos) does not decrease, tid = -1 only at the end
  const uint32_t uc = (uint32_t)r.tid, up = (uint32_t)ptid_;
  if (pkey_ != BAI_KEY_NONE && (uc < up || (uc == up && r.tid >= 0 && r.pos < ppos_)) && err_ord_[BAI_E_UNSORTED] == ~0ull) err_ord_[BAI_E_UNSORTED] = ord;
  if (placed) {
    const int32_t w0 = r.pos >> m, from = (ptid_ == r.tid && pwin_ >= w0) ? pwin_ + 1 : w0;
    uint64_t *lin = lin_.data() + win_off_[(size_t)r.tid];
    for (int32_t w = from; w <= end_win; ++w) lin[w] = std::min(lin[w], beg_v);
    ref_beg_[(size_t)r.tid] = std::min(ref_beg_[(size_t)r.tid], beg_v);
    ref_end_[(size_t)r.tid] = std::max(ref_end_[(size_t)r.tid], end_v);
    ++ref_cnt_[2 * (size_t)r.tid + ((r.flag & 4u) ? 1 : 0)];
  }
  if (r.tid < 0) ++n_no_coor;
  if (key != pkey_) {                          // a run starts, and the one in front ends where this record begins
    if (!runs_.empty()) { runs_.back().end_v = beg_v; runs_.back().end_abs = beg_abs; }
    runs_.push_back(Run{key, beg_v, 0, beg_abs, 0});
  }
  pkey_ = key; ptid_ = r.tid; ppos_ = r.pos; pwin_ = end_win; pend_v_ = end_v; pend_abs_ = end_abs;
}

int HostIndex::finish(std::vector<uint8_t> &bytes, std::string &err) {
  const uint32_t kind = bai_first_refusal(err_ord_);
  if (kind != BAI_ERR_KINDS) return bai_refusal_text(kind, err_ord_[kind], csi_, auto_depth_, sch_, n_ref_, err);
  if (!runs_.empty()) { runs_.back().end_v = pend_v_; runs_.back().end_abs = pend_abs_; }
  n_runs = runs_.size();
  std::stable_sort(runs_.begin(), runs_.end(), [](const Run &a, const Run &b) { return a.key < b.key; });
  // a chunk starts where the key changes or the run in front does not end here
  std::vector<BaiChunk> ch;
  for (size_t j = 0; j < runs_.size(); ++j) {
    const Run &R = runs_[j];
    if (j && R.key == runs_[j - 1].key && runs_[j - 1].end_abs == R.beg_abs) ch.back().end_v = R.end_v;
    else ch.push_back(BaiChunk{R.key, R.beg_v, R.end_v});
  }
  std::vector<uint64_t> lin = lin_;
  n_chunks = bai_pack(sch_, csi_, n_ref_, win_off_, ch, lin, ref_beg_, ref_end_, ref_cnt_, n_no_coor, bytes);
  return STRL_OK;
}

}  // namespace strl
