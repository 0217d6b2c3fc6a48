// bamindex_host.h -- the BAM index (.bai / CSI payload) of coordinate-sorted records in one sequential pass on the host: what
// `strling sort --write-index` writes with STRL_SORT=host or without a device.  No HIP: the rules are bamindex_core.h's, the ones the
// device builder (bamindex.hip) runs, and the bytes come from the same bai_pack -- the two paths write the same file.
#pragma once
#include <stdint.h>
#include <string>
#include <vector>
#include "bamindex_core.h"

namespace strl {

class HostIndex {
 public:
  // csi_min_shift < 0: a .bai; else the CSI scheme (csi_min_shift, csi_depth), csi_depth < 0 = samtools' rule.  false: err
  bool begin(int32_t n_ref, const int32_t *l_ref, int32_t csi_min_shift, int32_t csi_depth, std::string &err);
  // the next record of the sorted file: its bytes (block_size word first, len of them), the virtual offsets of its first byte
  // and of the byte behind it, and the same two as offsets in the inflated stream
  void add(const uint8_t *rec, uint32_t len, uint64_t beg_v, uint64_t end_v, uint64_t beg_abs, uint64_t end_abs);
  // the file's bytes; a refusal: the status and the words of strl_bamindex_finish
  int finish(std::vector<uint8_t> &bytes, std::string &err);
  uint64_t n_records = 0, n_no_coor = 0, n_runs = 0, n_chunks = 0;

 private:
  struct Run { uint64_t key, beg_v, end_v, beg_abs, end_abs; };
  BaiScheme sch_{14, 5, 16, BAI_MAX_POS};
  bool csi_ = false, auto_depth_ = false;
  int32_t n_ref_ = 0;
  std::vector<uint64_t> win_off_, lin_, ref_beg_, ref_end_, ref_cnt_;
  uint64_t err_ord_[BAI_ERR_KINDS];
  std::vector<Run> runs_;
  // the record in front
  uint64_t pkey_ = BAI_KEY_NONE, pend_v_ = 0, pend_abs_ = 0;
  int32_t ptid_ = 0, ppos_ = -1, pwin_ = -1;
};

}  // namespace strl
