// samparse.h -- SAM text encoded to BAM records on the device (samparse.hip): what bamsort.hip drives.  DESIGN section 24.2.
#pragma once
#include "common.h"
#include "sam_core.h"

namespace strl {

// a chunk's figures: device words, and the host's copy of them one chunk late
struct SamInfo {
  unsigned long long err_line;   // the chunk's first refused line (0-based inside the chunk); ~0 = none
  unsigned long long total;      // bytes of the chunk's records
  uint32_t n_lines, n_fix;       // lines of the chunk; lines whose float values the host finishes
  uint32_t overflow, pad;        // more lines than the tables hold: one of them is shorter than any valid line
};

// what the encode reads of the size kernel's walk of a line
struct SamMeta { uint32_t tab[11]; uint32_t len, n_cig, tag_bytes, flags, pad; };      // len: the line's, without \n and \r

struct SamSlot {
  DevBuf text, line_off, len, meta, recoff, rec, tile, fix, state;
  SamInfo *h_info = nullptr;                   // pinned
  hipEvent_t ev_copy = nullptr, ev_a = nullptr, ev_t[6] = {};
  uint64_t text_bytes = 0, line0 = 0;
  bool timed = false;
};

struct SamParser {
  SamRefTable refs;                            // the host's table; the device's copy below
  DevBuf d_names, d_off, d_slot;
  SamRefs d_refs{};
  SamSlot slot[2];
  uint64_t max_text = 0, rec_cap = 0;
  uint32_t line_cap = 0, lanes = 16;
  strl_bamsort_sam_figures fig{};
  std::vector<uint8_t> h_text, h_rec;          // the host-finish step's and a refusal's copies
  std::vector<uint32_t> h_fix, h_off, h_recoff;
};

int sam_parser_create(SamParser **out, const uint8_t *names, const uint32_t *name_off, int32_t n_ref, hipStream_t st);
void sam_parser_destroy(SamParser *p);
int sam_parser_reserve(SamParser *p, uint64_t max_text_bytes);
// chunk `text` (whole lines, the last byte a \n) into slot si: the copy, the three kernels and the figures' copy, all on st; the text
// may be reused on return.  line0: alignment lines before this chunk
int sam_parser_enqueue(SamParser *p, int si, const uint8_t *text, uint64_t bytes, uint64_t line0, hipStream_t st);
// waits for slot si's chunk: a refusal in the host's words (STRL_ERR_FORMAT), else the records complete in the slot's `rec` (the host
// has finished the floats the kernel left) with recoff[] beside them
int sam_parser_collect(SamParser *p, int si, hipStream_t st, SamInfo *info);

}  // namespace strl
