// Stand-alone driver of cli/chunk_feed.{h,cpp} for tests/test_chunk_feed.py: stages a BAM chunk by chunk into malloc'ed buffers the
// way the device passes do (ChunkAhead, with or without the read-ahead thread) and dumps what was staged; runs FragLengths over
// records given in a file.  Built with -fsanitize=address,undefined.
//   driver stage BAM MAX_BLOCKS MAX_BYTES AHEAD OUT
//   driver shares BAM MAX_BLOCKS MAX_BYTES OUT0 OUT1        (two shares, cut at the index's record start nearest the middle)
//   driver frag RECORDS OUT                                  (RECORDS: u32 flag, i32 isize per record; OUT: 4096 u32)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <zlib.h>
#include <algorithm>
#include <string>
#include <vector>
#include "chunk_feed.h"

using namespace strl;

static void put(FILE *f, const void *p, size_t n) { if (fwrite(p, 1, n, f) != n) { perror("write"); exit(2); } }
static void put64(FILE *f, int64_t v) { put(f, &v, 8); }

// Dump, per chunk: i64 nb, lo, hi, last, short_read; per block u64 boff, coff; u32 clen, isz, crc; the block's raw-inflated bytes
// (as many as inflate gave: u32 in front).  The end of the feed is a chunk of nb <= 0.
static void dump_chunk(FILE *f, const StagedChunk &S, const ChunkTables &t, const uint8_t *data) {
  put64(f, S.nb); put64(f, (int64_t)S.lo); put64(f, (int64_t)S.hi); put64(f, S.last); put64(f, S.short_read);
  std::vector<uint8_t> out(65536 + 16);
  for (int64_t k = 0; k < S.nb; ++k) {
    put(f, &t.boff[k], 8); put(f, &t.coff[k], 8); put(f, &t.clen[k], 4); put(f, &t.isz[k], 4); put(f, &t.crc[k], 4);
    z_stream z;
    memset(&z, 0, sizeof z);
    uint32_t got = 0;
    if (!S.short_read && inflateInit2(&z, -15) == Z_OK) {
      z.next_in = const_cast<uint8_t *>(data + t.coff[k]); z.avail_in = t.clen[k];
      z.next_out = out.data(); z.avail_out = (uInt)out.size();
      if (inflate(&z, Z_FINISH) == Z_STREAM_END) got = (uint32_t)z.total_out;
      inflateEnd(&z);
    }
    put(f, &got, 4);
    put(f, out.data(), got);
  }
}

static int stage_all(BgzfFeed &feed, size_t max_blocks, size_t max_bytes, bool ahead, bool want_last, const char *out_path) {
  FILE *f = fopen(out_path, "wb");
  if (!f) { perror(out_path); return 2; }
  ThreadPool pool(3);
  uint8_t *data[3], *meta[3];
  for (int k = 0; k < 3; ++k) { data[k] = (uint8_t *)malloc(chunk_data_bytes(max_bytes)); meta[k] = (uint8_t *)malloc(chunk_table_bytes(max_blocks)); }
  {
    ChunkAhead ring(feed, pool, data, meta, max_blocks, max_bytes, want_last);
    ring.stage(0, 0);
    for (uint64_t ci = 0;; ++ci) {
      const StagedChunk cur = ring.at(ci);
      if (ahead && cur.nb > 0 && !cur.short_read) ring.stage_ahead(ci + 1, (ci + 1) % 3);
      dump_chunk(f, cur, ring.tables(cur), ring.data(cur));
      ring.join();
      if (cur.nb <= 0 || cur.short_read) { if (cur.nb < 0) fprintf(stderr, "feed: %s\n", cur.err.c_str()); break; }
      if (!ahead) ring.stage(ci + 1, (ci + 1) % 3);
    }
  }
  for (int k = 0; k < 3; ++k) { free(data[k]); free(meta[k]); }
  fclose(f);
  return 0;
}

int main(int argc, char **argv) {
  const std::string cmd = argc > 1 ? argv[1] : "";
  std::string err;
  if (cmd == "stage" && argc == 7) {
    BgzfFeed feed;
    if (!feed.open(argv[2], err)) { fprintf(stderr, "open: %s\n", err.c_str()); return 3; }
    printf("first_record_offset %llu\n", (unsigned long long)feed.first_record_offset());
    return stage_all(feed, (size_t)atol(argv[3]), (size_t)atol(argv[4]), atoi(argv[5]) != 0, false, argv[6]);
  }
  if (cmd == "shares" && argc == 7) {
    BgzfFeed feed;
    if (!feed.open(argv[2], err)) { fprintf(stderr, "open: %s\n", err.c_str()); return 3; }
    const std::vector<uint64_t> pts = BgzfFeed::split_points(argv[2]);
    const uint64_t first = (feed.first_block_offset() << 16) | feed.first_record_offset();
    auto it = std::lower_bound(pts.begin(), pts.end(), std::max<uint64_t>(first + 1, (uint64_t)(feed.file_bytes() / 2) << 16));
    if (it == pts.end()) { fprintf(stderr, "no record start to cut at\n"); return 4; }
    const uint64_t cut = *it;
    feed.halt();
    BgzfFeed s0, s1;
    if (!s0.open_share(feed, first >> 16, (uint32_t)(first & 0xffff), cut >> 16, (uint32_t)(cut & 0xffff), err) ||
        !s1.open_share(feed, cut >> 16, (uint32_t)(cut & 0xffff), 0, 0, err)) { fprintf(stderr, "open_share: %s\n", err.c_str()); return 3; }
    const size_t mb = (size_t)atol(argv[3]), my = (size_t)atol(argv[4]);
    if (int rc = stage_all(s0, mb, my, true, true, argv[5])) return rc;
    if (int rc = stage_all(s1, mb, my, true, true, argv[6])) return rc;
    printf("first_off %llu cut_uoff %llu tail_trim %u %u\n", (unsigned long long)(first & 0xffff), (unsigned long long)(cut & 0xffff), s0.tail_trim(), s1.tail_trim());
    return 0;
  }
  if (cmd == "frag" && argc == 4) {
    FILE *f = fopen(argv[2], "rb");
    if (!f) { perror(argv[2]); return 2; }
    FragLengths fl;
    std::vector<uint32_t> buf(2 << 16);
    int64_t i = 0, looked = 0;
    size_t n;
    while (!fl.done() && (n = fread(buf.data(), 8, buf.size() / 2, f)) > 0)
      for (size_t k = 0; k < n && !fl.done(); ++k, ++looked) fl.add(buf[2 * k], buf[2 * k + 1], i++);
    fclose(f);
    uint32_t frag[4096];
    fl.finish(frag);
    FILE *o = fopen(argv[3], "wb");
    if (!o) { perror(argv[3]); return 2; }
    put(o, frag, sizeof frag);
    fclose(o);
    printf("looked %lld\n", (long long)looked);
    return 0;
  }
  fprintf(stderr, "usage: see the head of chunk_feed_driver.cpp\n");
  return 1;
}
