// Stand-alone driver of the host twins of `strling pull` (csrc/pull_logic.cpp: strl_pull_select_host, strl_pull_counts_host,
// strl_pull_mates_host) for tests/test_pull_cases.py: every tile's or window's bytes are copied into a vector of exactly their
// size, so that AddressSanitizer sees a read behind them.  Built with -fsanitize=address,undefined together with
// pull_logic.cpp; set_error, which the library defines beside its context, is defined here.
//   driver IN
// IN:  u64 stream bytes, n_items, kind (0 select, 1 mates), names bytes | the stream | the names | the items
//      select item: u64 s0, s1; i32 tid, beg, end, own_beg, own_end, 0           (the tile's bytes are stream[s0, s1))
//      mates item:  u64 s0, s1; i32 tid; u32 n_req; n_req x strl_pull_req        (the window's bytes are stream[s0, s1))
// Out: select: "T rc n_rows" per tile, then "C rc" and a line per row of all tiles, counted over the whole stream
//      mates:  "W rc" per window and a line per request
//      a row: off tid pos mtid mpos size hash flag l_name found count
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "../../include/strling_amd.h"

namespace strl {
void set_error(const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vfprintf(stderr, fmt, ap);
  va_end(ap);
  fputc('\n', stderr);
}
}  // namespace strl

static void print_row(const strl_pull_row &r) {
  printf("%llu %d %d %d %d %u %u %u %u %u %u\n", (unsigned long long)r.off, r.tid, r.pos, r.mtid, r.mpos, r.size, r.hash, (unsigned)r.flag, (unsigned)r.l_name,
         (unsigned)r.found, r.count);
}

int main(int argc, char **argv) {
  if (argc != 2) { fprintf(stderr, "usage: see the head of pull_logic_driver.cpp\n"); return 1; }
  FILE *f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  uint64_t head[4];
  if (fread(head, 8, 4, f) != 4) { fprintf(stderr, "short file\n"); return 2; }
  std::vector<uint8_t> stream((size_t)head[0]), names((size_t)head[3]);
  if (head[0] && fread(stream.data(), 1, stream.size(), f) != stream.size()) { fprintf(stderr, "short stream\n"); return 2; }
  if (head[3] && fread(names.data(), 1, names.size(), f) != names.size()) { fprintf(stderr, "short names\n"); return 2; }
  std::vector<strl_pull_row> all;
  for (uint64_t k = 0; k < head[1]; ++k) {
    uint64_t s[2];
    if (fread(s, 8, 2, f) != 2) { fprintf(stderr, "short item %llu\n", (unsigned long long)k); return 2; }
    if (s[0] > s[1] || s[1] > stream.size()) { fprintf(stderr, "item %llu leaves the stream\n", (unsigned long long)k); return 2; }
    const std::vector<uint8_t> u(stream.begin() + (ptrdiff_t)s[0], stream.begin() + (ptrdiff_t)s[1]);
    if (head[2] == 0) {
      struct { strl_pull_tile T; int32_t pad; } q;
      if (fread(&q, sizeof q, 1, f) != 1) { fprintf(stderr, "short tile %llu\n", (unsigned long long)k); return 2; }
      std::vector<strl_pull_row> rows(u.size() / 36 + 1);
      uint64_t n = 0;
      const int rc = strl_pull_select_host(u.data(), u.size(), &q.T, s[0], rows.data(), rows.size(), &n);
      if (rc) n = 0;
      printf("T %d %llu\n", rc, (unsigned long long)n);
      all.insert(all.end(), rows.begin(), rows.begin() + (ptrdiff_t)n);
    } else {
      struct { int32_t tid; uint32_t n_req; } q;
      if (fread(&q, sizeof q, 1, f) != 1) { fprintf(stderr, "short window %llu\n", (unsigned long long)k); return 2; }
      std::vector<strl_pull_req> reqs(q.n_req);
      if (q.n_req && fread(reqs.data(), sizeof(strl_pull_req), q.n_req, f) != q.n_req) { fprintf(stderr, "short requests %llu\n", (unsigned long long)k); return 2; }
      for (const strl_pull_req &r : reqs)
        if ((uint64_t)r.name_off + r.name_len > names.size()) { fprintf(stderr, "a name leaves the names\n"); return 2; }
      std::vector<strl_pull_row> rows(q.n_req);
      memset(rows.data(), 0, rows.size() * sizeof(strl_pull_row));
      const int rc = strl_pull_mates_host(u.data(), u.size(), 1, q.tid, reqs.data(), q.n_req, names.data(), s[0], rows.data());
      printf("W %d\n", rc);
      for (const strl_pull_row &r : rows) print_row(r);
    }
  }
  if (head[2] == 0) {
    printf("C %d\n", strl_pull_counts_host(stream.data(), all.data(), all.size()));
    for (const strl_pull_row &r : all) print_row(r);
  }
  fclose(f);
  return 0;
}
