// sort_cli.cpp -- `strling sort`: a BAM coordinate-sorted, the step between the aligner and `strling extract` (the reference's
// simulator shells out to `samtools sort` for it, simulate_reads.nim:178).  The rule is csrc/bamsort_core.h's.
//
// Device path: fed exactly as `strling bamindex` is (BgzfFeed, ChunkAhead, STRL_CHUNK_BLOCKS, the context brought up on a thread
// beside the first chunk's read); strl_bamsort_* keeps key, length and the records themselves on the device, sorts, and the output
// stream is fetched piece by piece -- the fetch of piece k + 1 beside the host's deflate / write of piece k.
// Host path (STRL_SORT=host, or no device): the host BAM reader, std::stable_sort on the same key, the same header, the same
// stream, the same member cuts -- with --deflate=host the two paths write the same bytes.
// The output is written under a temporary name and renamed at the end: a failed run leaves no file.
// --write-index: the index (.bai / .csi) from the same pass.  The members are walked as they are written (their file offsets), and
// behind the last piece the index is built from what the sort still holds -- the device's arena, order and offsets
// (strl_bamsort_index), or the host path's (bamindex_host.cpp) -- and written, through a temporary name, after the BAM's rename.
// --windowed (device path): a file larger than device memory.  Pass 0 feeds the file as above but keeps only key and length of a
// record; the stream is then cut into windows the device can hold (strl_bamsort_window_limit, bsort_window_plan), and for every
// window the file is fed again -- a fresh BgzfFeed and ChunkAhead over the same page-locked buffers -- and scattered into the
// window, which then goes through the same piece loop.  With --write-index the index is build_bai's over the file just written.
// SAM text, from a file or from stdin (`-`): the format is taken from the first bytes.  SamFeed (sam_feed.h) reads chunks of whole
// lines into page-locked buffers, chunk i + 1 beside the push of chunk i; the device encodes them to BAM records (samparse.hip) in
// place of the inflate, and everything behind the read phase is the BAM's.  On the host path the same lines go through the same
// header's host function (sam_core.h) into host memory and then through the host path's tail.  DESIGN section 24.2.
// --markdup: flag 0x400 on duplicate pairs and fragments (csrc/markdup_core.h; the reference drops such records, collect.nim:140).
// On the device the step runs over the resident records between the finish and the first fetch (strl_bamsort_markdup); the host path
// applies the same header's rule to its records before it writes.  DESIGN section 24.3.
#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#include <algorithm>
#include <chrono>
#include <functional>
#include <numeric>
#include <string>
#include <thread>
#include <vector>
#include "cli_shared.h"
#include "bam_reader.h"
#include "bgzf_feed.h"
#include "cram_reader.h"
#include "sam_feed.h"
#include "../bamindex_host.h"
#include "../bamsort_core.h"
#include "../markdup_core.h"
#include "../sam_core.h"
#include "../front.h"

using namespace strl;

namespace {

using Clock = std::chrono::steady_clock;
double since(Clock::time_point t) { return std::chrono::duration<double>(Clock::now() - t).count(); }

const char *USAGE =
    "strling sort\n\nUsage:\n  strling sort [options] -o OUT.bam IN.bam\n  strling sort [options] -o OUT.bam IN.sam\n  aligner ... | strling sort [options] -o OUT.bam -\n\n"
    "Arguments:\n  IN.bam           path to a bam file, in any order\n  IN.sam, -        SAM text instead, from a file or from stdin (told from a BAM by its first bytes)\n\nOptions:\n"
    "  -o, --output=OUT.bam       required; written through a temporary name, so a failed run leaves no file\n"
    "      --write-index          also write OUT.bam's index, built from the sort's own pass: no second read, inflate and scan of the file\n"
    "      --index-out=OUT.bai    where --write-index writes it (default: OUT.bam.bai; with --csi OUT.bam.csi)\n"
    "      --csi                  with --write-index: a CSI index (.csi), which also holds contigs longer than 2^29 bases\n"
    "  -m, --min-shift=N          with --csi: bases per window of the smallest bins = 2^N, N in [8, 24] (default: 14)\n"
    "      --windowed             sort a file larger than device memory: only 12 bytes a record stay on the device, and the file is read once\n"
    "                             more for every window of the output that the device can hold; the same bytes as without it.  With\n"
    "                             --write-index the index costs a second read of the output (it is built as `strling bamindex OUT.bam` builds it).\n"
    "                             Not with SAM input: a pipe cannot be read again\n"
    "      --markdup              set flag 0x400 on duplicate pairs and fragments (and clear it elsewhere), as samtools markdup does in\n"
    "                             template mode: mates are joined by name on the device, no fixmate, MC or ms tag is needed.  One line on\n"
    "                             stderr gives the counts.  Not with --windowed: the records are not resident\n"
    "      --deflate=host|device|dense  host (default): zlib at its default level on the pool, as pull.  device: the GPU's compressor (about\n"
    "                             1.15 x the bytes).  dense: the GPU's compressor with its chained, lazy match search (the default's size class)\n"
    "  -D, --device=K             GPU to use (default: 0)\n"
    "  -v, --verbose              one JSON line on stderr\n  -h, --help                 Show this help\n";

struct Seconds { double read = 0, sort = 0, gather = 0, deflate = 0, write = 0, window = 0; };      // window: the passes of --windowed behind pass 0

// the output file: members appended under a temporary name, the EOF block and the rename at the end
struct SortOut {
  std::string path, tmp;
  FILE *f = nullptr;
  bool track = false;                     // --write-index: the file offset of every member written, the EOF block's last
  std::vector<uint64_t> member_off;
  uint64_t at = 0;
  bool open(const std::string &out, std::string &why) {
    path = out;
    tmp = out + ".tmp." + std::to_string((long long)getpid());
    f = fopen(tmp.c_str(), "wb");
    if (!f) why = "cannot write " + tmp + ": " + strerror(errno);
    return f != nullptr;
  }
  bool put(const uint8_t *p, size_t n, std::string &why) {
    if (n && fwrite(p, 1, n, f) != n) { why = "cannot write " + tmp + ": " + strerror(errno); return false; }
    if (track && !bsort_walk_members(p, n, &at, member_off)) { why = "internal error: a piece written is not whole BGZF members"; return false; }
    return true;
  }
  bool close(std::string &why) {
    static const uint8_t eof[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    bool ok = put(eof, 28, why);
    ok = (fclose(f) == 0) && ok;
    f = nullptr;
    if (ok && rename(tmp.c_str(), path.c_str()) != 0) ok = false;
    if (!ok) { if (why.empty()) why = "cannot write " + path + ": " + strerror(errno); unlink(tmp.c_str()); }
    return ok;
  }
  void drop() { if (f) { fclose(f); f = nullptr; } if (!tmp.empty()) unlink(tmp.c_str()); }
};

// the members of a piece of the stream (whole 0xFF00 blocks but for the stream's last), on the pool: zlib, or the compressor's host
// twin with the rule `mode` (STRL_DEFLATE_FAST / _DENSE)
bool deflate_piece(const uint8_t *p, size_t n, bool core, int mode, ThreadPool &pool, std::vector<uint8_t> &out, uint32_t &stored, std::string &why) {
  const size_t nb = (n + BSORT_BLK - 1) / BSORT_BLK;
  std::vector<std::vector<uint8_t>> blocks(nb);
  std::vector<uint32_t> st(nb, 0);
  std::vector<int> bad(nb, 0);
  pool.parallel_for(nb, [&](size_t k) {
    const uint8_t *src = p + k * BSORT_BLK;
    const size_t len = std::min<size_t>(BSORT_BLK, n - k * BSORT_BLK);
    if (!core) { bad[k] = !bgzf_member_zlib(src, len, blocks[k]); return; }
    blocks[k].resize((size_t)strl_bgzf_deflate_bound(len, BSORT_BLK));
    uint64_t got = 0;
    bad[k] = strl_bgzf_deflate_host_mode(mode, src, len, BSORT_BLK, blocks[k].data(), blocks[k].size(), &got, nullptr, &st[k]) != 0;
    blocks[k].resize((size_t)got);
  });
  out.clear();
  for (size_t k = 0; k < nb; ++k) {
    if (bad[k]) { why = "deflate failed"; return false; }
    out.insert(out.end(), blocks[k].begin(), blocks[k].end());
    stored += st[k];
  }
  return true;
}

uint64_t piece_bytes() {
  const char *e = getenv("STRL_SORT_PIECE_KB");                // tests: pieces that cut records, block_size words and the header
  const uint64_t want = e && atof(e) > 0 ? (uint64_t)(atof(e) * 1024.0) : (uint64_t)128 << 20;
  return std::max<uint64_t>(BSORT_BLK, want / BSORT_BLK * BSORT_BLK);
}

// --write-index: what was asked for, and what the index step gave
struct Index {
  bool on = false;
  int min_shift = -1;                     // >= 0: a CSI index
  std::string out;
  std::vector<int32_t> l_ref;
  int rc = 0;                             // != 0: refused (the sorted file is complete all the same)
  std::string why;
  std::vector<uint8_t> bytes;
  uint64_t chunks = 0;
  double s = 0;
};

struct Result {
  uint64_t records = 0, no_ref = 0, stream_bytes = 0, slabs = 0, out_bytes = 0;
  uint64_t windows = 0, window_bytes = 0;     // --windowed on the device: passes behind pass 0, bytes of the stream each finishes
  bool already_sorted = false;
  uint64_t lines = 0, text_bytes = 0, host_finished = 0;
  double sam_ms[4] = {0, 0, 0, 0};            // HIP-event time of the chunks' copies, line scans, size kernels and encodes
  const char *deflate = "zlib";
  uint32_t stored = 0;
  Seconds s;
  bool markdup = false;                       // --markdup: asked for | the counts, and on the device the step's times
  strl_markdup_info md{};
  double markdup_s = 0;
};

// ---- the host path ---------------------------------------------------------------------------------------------------------------
// SAM text on the host: what the feed reads, line by line through sam_core.h's host function
struct SamInput { SamFeed feed; SamHeader header; };

bool sort_on_host(const std::string &bam, SamInput *sam, const std::vector<uint8_t> &header, int32_t n_ref, bool core, int mode, SortOut &out, Result &R, Index &X, std::string &why, int &status) {
  auto t0 = Clock::now();
  std::string err;
  status = STRL_ERR_FORMAT;
  std::vector<uint8_t> raw;
  if (sam) {
    SamRefTable table;
    table.build(sam->header.names.data(), sam->header.name_off.data(), n_ref, nullptr);      // (sam_header has refused a name that occurs twice)
    const SamRefs refs = table.view();
    std::vector<uint8_t> text(sam->feed.buffer_bytes());
    for (;;) {
      const int64_t got = sam->feed.next_chunk(text.data(), err);
      if (got < 0) { why = err; return false; }
      if (!got) break;
      R.text_bytes += (uint64_t)got;
      for (size_t q = 0; q < (size_t)got; ++R.lines) {
        const size_t e = (size_t)(static_cast<const uint8_t *>(memchr(text.data() + q, '\n', (size_t)got - q)) - text.data());
        std::string w;
        if (sam_encode_line(text.data() + q, (uint32_t)(e - q), refs, raw, w)) { why = sam_refusal(R.lines + 1, w); return false; }
        q = e + 1;
      }
    }
  } else {
    BamReader rd;
    if (!rd.open(bam, err)) { why = err.empty() ? "couldn't open bam" : err; return false; }
    for (;;) {
      const int64_t got = rd.read_raw(raw, 1 << 20, err);
      if (got < 0) { why = err.empty() ? "malformed BAM (truncated file or invalid BGZF block)" : err; return false; }
      if (!got) break;
    }
  }
  std::vector<uint64_t> at, key;
  for (size_t q = 0; q < raw.size();) {
    const uint32_t bs = bsort_ld32(raw.data() + q);
    if ((uint64_t)bs + 4 > FRONT_CARRY_MAX) { why = "BAM record of more than " + std::to_string(FRONT_CARRY_MAX) + " bytes"; return false; }
    uint64_t k = 0;
    if (!bsort_key(raw.data() + q + 4, n_ref, &k)) {
      why = "malformed BAM record " + std::to_string(at.size()) + ": its refID is not one of the header's " + std::to_string(n_ref) + " references";
      return false;
    }
    if (at.size() >= BSORT_MAX_RECORDS) { why = "more than 2^32 - 2 records: beyond one sort"; status = STRL_ERR_LIMIT; return false; }
    R.no_ref += (int32_t)bsort_ld32(raw.data() + q + 4) < 0;
    at.push_back(q); key.push_back(k);
    q += 4 + (size_t)bs;
  }
  R.s.read = since(t0);
  t0 = Clock::now();
  if (R.markdup) {                                              // the rule over the records in input order; the decided words into them
    std::vector<uint16_t> flags;
    MdupCounts C{};
    std::string w;
    const int64_t bad = mdup_host(raw.data(), raw.size(), flags, &C, w);
    if (bad >= 0) { why = "malformed BAM record " + std::to_string(bad) + ": " + w; return false; }
    for (size_t i = 0; i < at.size(); ++i) { raw[at[i] + MDUP_FLAG_AT] = (uint8_t)flags[i]; raw[at[i] + MDUP_FLAG_AT + 1] = (uint8_t)(flags[i] >> 8); }
    R.md.n_pairs = C.pairs; R.md.n_dup_pairs = C.dup_pairs; R.md.n_fragments = C.fragments; R.md.n_dup_fragments = C.dup_fragments; R.md.n_ineligible = C.ineligible;
    R.markdup_s = since(t0);
    t0 = Clock::now();
  }
  const size_t n = at.size();
  std::vector<uint32_t> perm(n);
  std::iota(perm.begin(), perm.end(), 0u);
  std::stable_sort(perm.begin(), perm.end(), [&](uint32_t a, uint32_t b) { return key[a] < key[b]; });
  R.already_sorted = true;
  std::vector<uint64_t> off(n + 1);
  uint64_t run = header.size();
  for (size_t j = 0; j < n; ++j) {
    off[j] = run;
    run += 4 + (uint64_t)bsort_ld32(raw.data() + at[perm[j]]);
    if (perm[j] != j) R.already_sorted = false;
  }
  off[n] = run;
  R.records = n; R.stream_bytes = run;
  R.s.sort = since(t0);
  ThreadPool pool(std::min(decode_threads(), 16));
  const uint64_t piece = piece_bytes();
  std::vector<uint8_t> buf, members;
  status = STRL_ERR_IO;
  for (uint64_t lo = 0; lo < run; lo += piece) {
    const uint64_t hi = std::min(run, lo + piece);
    t0 = Clock::now();
    buf.resize((size_t)(hi - lo));
    if (lo < header.size()) memcpy(buf.data(), header.data() + lo, (size_t)(std::min<uint64_t>(hi, header.size()) - lo));
    const uint64_t a = bsort_first_touch(off.data(), n, lo), b = bsort_end_touch(off.data(), n, hi);
    for (uint64_t j = a; j < b; ++j) {
      const BsortPart p = bsort_part(off[j], off[j + 1], lo, hi);
      memcpy(buf.data() + p.dst, raw.data() + at[perm[j]] + p.skip, (size_t)p.bytes);
    }
    R.s.gather += since(t0);
    t0 = Clock::now();
    if (!deflate_piece(buf.data(), buf.size(), core, mode, pool, members, R.stored, why)) return false;
    R.s.deflate += since(t0);
    t0 = Clock::now();
    if (!out.put(members.data(), members.size(), why)) return false;
    R.out_bytes += members.size();
    R.s.write += since(t0);
  }
  R.deflate = !core ? "zlib" : mode == STRL_DEFLATE_DENSE ? "core-host-dense" : "core-host";
  if (X.on) {                                                   // one pass over the sorted records (bamindex_host.cpp)
    t0 = Clock::now();
    out.member_off.push_back(out.at);                           // the EOF block
    const uint64_t *mo = out.member_off.data(), nm = out.member_off.size() - 1;
    HostIndex H;
    if (!bsort_member_table_ok(mo, nm, run)) { X.rc = STRL_ERR_ARG; X.why = "internal error: the member table does not match the stream"; }
    else if (!H.begin(n_ref, X.l_ref.data(), X.min_shift, -1, X.why)) X.rc = STRL_ERR_ARG;
    else {
      for (size_t j = 0; j < n; ++j)
        H.add(raw.data() + at[perm[j]], (uint32_t)(off[j + 1] - off[j]), bsort_voff(mo, nm, run, off[j]), bsort_voff(mo, nm, run, off[j + 1]), off[j], off[j + 1]);
      X.rc = H.finish(X.bytes, X.why);
      X.chunks = H.n_chunks;
    }
    X.s = since(t0);
  }
  status = 0;
  return true;
}

// ---- the device path -------------------------------------------------------------------------------------------------------------
// windowed: `sort --windowed`.  Pass 0 keeps key and length of every record; the file is then read once more for every window of
// the output stream, and each finished window goes through the piece loop the resident sort's whole stream goes through.
bool sort_on_device(const std::function<strl_ctx *(std::string &)> &get_ctx, const std::string &bam, SamInput *sam, const std::vector<uint8_t> &header, bool core, int mode, bool windowed,
                    SortOut &out, Result &R, Index &X, std::string &why, int &status) {
  auto t0 = Clock::now();
  status = STRL_ERR_IO;
  BgzfFeed feed;
  std::string err;
  if (!sam && !feed.open(bam, err)) { why = err.empty() ? "couldn't open bam" : "couldn't open bam: " + err; return false; }
  static const char *env_blocks = getenv("STRL_CHUNK_BLOCKS");     // tests: tiny chunks put records across pushes
  const size_t auto_blocks = std::min<size_t>(16384, std::max<size_t>(2048, (sam ? 0 : feed.file_bytes()) / 16384 / 12));
  const size_t chunk_blocks = env_blocks && atoi(env_blocks) > 0 ? (size_t)atoi(env_blocks) : auto_blocks;
  const size_t chunk_bytes = std::max<size_t>((size_t)1 << 20, chunk_blocks * 20000);
  PinnedRing pins;
  if (!sam) {
    pins.alloc(3, chunk_blocks, chunk_bytes);
    if (!pins.ok()) { why = "page-locked memory for the chunks"; pins.release(); return false; }
  }
  strl_ctx *ctx = nullptr;
  auto fail = [&](int rc) { why = strl_last_error(); status = rc; (void)strl_bamsort_end(ctx); pins.release(); return false; };
  ThreadPool pool(std::min(decode_threads(), 12));
  // one pass over the file `fd`: every chunk through `push`, chunk ci + 1 read beside the push of chunk ci.  `begin` runs behind
  // the first chunk's read (pass 0 takes the context there); its rc < 0 is the library's, 1 = it has said why itself
  auto feed_pass = [&](BgzfFeed &fd, const std::function<int()> &begin, decltype(&strl_bamsort_push) push) {
    ChunkAhead ring(fd, pool, pins.data.data(), pins.meta.data(), chunk_blocks, chunk_bytes);
    ring.stage(0, 0);
    int rc = begin();
    if (rc > 0) { pins.release(); return false; }
    if (rc) return fail(rc);
    for (uint64_t ci = 0;; ++ci) {
      const StagedChunk cur = ring.at(ci);
      if (cur.nb < 0 || cur.short_read) { why = cur.nb < 0 ? cur.err : "short read"; status = STRL_ERR_FORMAT; (void)strl_bamsort_end(ctx); pins.release(); return false; }
      if (cur.nb == 0) break;
      ring.stage_ahead(ci + 1, (ci + 1) % 3);
      const ChunkTables t = ring.tables(cur);
      rc = push(ctx, ring.data(cur), cur.bytes(), t.coff, t.clen, t.isz, t.crc, (uint32_t)cur.nb);
      ring.join();
      if (rc) return fail(rc);
    }
    return true;
  };
  // SAM text: chunks of whole lines from the feed into two page-locked buffers, chunk ci + 1 read beside the push of chunk ci (the
  // push returns when its text has been copied, so the buffer is free again)
  auto sam_pass = [&]() {
    const size_t cap = sam->feed.buffer_bytes();
    uint8_t *tb[2] = {static_cast<uint8_t *>(strl_pinned_alloc(cap)), static_cast<uint8_t *>(strl_pinned_alloc(cap))};
    if (!tb[0] || !tb[1]) { why = "page-locked memory for the chunks"; status = STRL_ERR_NOMEM; return false; }
    int64_t got[2] = {0, 0};
    std::string rerr[2];
    got[0] = sam->feed.next_chunk(tb[0], rerr[0]);
    if (!(ctx = get_ctx(why))) { status = STRL_ERR_NO_DEVICE; return false; }
    const char *cap_mb = getenv("STRL_SORT_ARENA_MB");
    const uint64_t limit = cap_mb && atof(cap_mb) > 0 ? (uint64_t)(atof(cap_mb) * 1048576.0) : 0;
    const SamHeader &H = sam->header;
    int rc = strl_bamsort_sam_begin(ctx, H.names.data(), H.name_off.data(), (int32_t)H.l_ref.size(), limit);
    if (!rc && R.markdup) rc = strl_bamsort_markdup_mode(ctx, 1);
    if (!rc) rc = strl_bamsort_sam_reserve(ctx, cap);
    if (rc) return fail(rc);
    for (uint64_t ci = 0;; ++ci) {
      const int b = (int)(ci & 1);
      if (got[b] < 0) { why = rerr[b]; status = STRL_ERR_FORMAT; (void)strl_bamsort_end(ctx); return false; }
      if (!got[b]) break;
      std::thread ahead([&, b] { got[b ^ 1] = sam->feed.next_chunk(tb[b ^ 1], rerr[b ^ 1]); });
      rc = strl_bamsort_push_sam(ctx, tb[b], (uint64_t)got[b]);
      ahead.join();
      if (rc) return fail(rc);
    }
    return true;
  };
  const bool read_ok = sam ? sam_pass() : feed_pass(feed, [&]() -> int {
    if (!(ctx = get_ctx(why))) { status = STRL_ERR_NO_DEVICE; return 1; }
    const char *cap = getenv("STRL_SORT_ARENA_MB");                // tests of the refusal
    const uint64_t limit = cap && atof(cap) > 0 ? (uint64_t)(atof(cap) * 1048576.0) : 0;
    int rc = windowed ? strl_bamsort_begin_windowed(ctx, (int32_t)feed.targets().size(), feed.first_record_offset())
                      : strl_bamsort_begin(ctx, (int32_t)feed.targets().size(), feed.first_record_offset(), limit);
    if (!rc && R.markdup) rc = strl_bamsort_markdup_mode(ctx, 1);
    if (!rc) rc = strl_bamsort_reserve(ctx, (uint32_t)chunk_blocks, chunk_bytes);
    return rc;
  }, strl_bamsort_push);
  if (!read_ok) return false;
  R.s.read = since(t0);
  t0 = Clock::now();
  strl_bamsort_info info;
  int rc = strl_bamsort_finish(ctx, header.data(), header.size(), &info);
  if (rc) return fail(rc);
  R.s.sort = since(t0);
  if (R.markdup) {                                              // every record lies on the device: the flags before the first piece is gathered
    t0 = Clock::now();
    if ((rc = strl_bamsort_markdup(ctx, &R.md))) return fail(rc);
    R.markdup_s = since(t0);
  }
  if (core && (rc = strl_bamsort_deflate_mode(ctx, mode))) return fail(rc);      // the rule of every fetch_bgzf below
  R.records = info.n_records; R.no_ref = info.n_no_ref; R.stream_bytes = info.stream_bytes; R.already_sorted = info.already_sorted != 0; R.slabs = info.n_slabs;
  if (sam) {
    strl_bamsort_sam_figures f{};
    if (!strl_bamsort_sam_info(ctx, &f)) { R.lines = f.lines; R.text_bytes = f.text_bytes; R.host_finished = f.host_finished; R.sam_ms[0] = f.copy_ms; R.sam_ms[1] = f.scan_ms; R.sam_ms[2] = f.size_ms; R.sam_ms[3] = f.encode_ms; }
  }
  // pieces: the fetch of piece k + 1 on a thread beside the deflate / write of piece k
  const uint64_t total = info.stream_bytes;
  uint64_t piece = piece_bytes();
  BsortWindowPlan plan{0, 0};
  if (windowed) {
    uint64_t limit = 0;
    const char *kb = getenv("STRL_SORT_WINDOW_KB");                // tests: windows of a few members (fractions allowed)
    if (kb && atof(kb) > 0) limit = (uint64_t)(atof(kb) * 1024.0);
    else if ((rc = strl_bamsort_window_limit(ctx, &limit))) return fail(rc);
    // a window the device cannot hold helps nobody: where the limit is below a piece, the pieces shrink to the members that fit it
    piece = std::min(piece, std::max<uint64_t>(BSORT_BLK, limit / BSORT_BLK * BSORT_BLK));
    plan = bsort_window_plan(total, limit, piece);
    R.windows = plan.n_windows; R.window_bytes = plan.window_bytes;
  }
  const uint64_t room = core ? strl_bgzf_deflate_bound(std::min(piece, total), BSORT_BLK) : std::min(piece, total);
  uint8_t *buf[2] = {static_cast<uint8_t *>(strl_pinned_alloc(room + 64)), static_cast<uint8_t *>(strl_pinned_alloc(room + 64))};
  if (!buf[0] || !buf[1]) { why = "page-locked memory for the pieces"; status = STRL_ERR_NOMEM; (void)strl_bamsort_end(ctx); return false; }
  struct Fetched { int rc = 0; std::string err; uint64_t bytes = 0; uint32_t stored = 0; double s = 0; } got[2];
  std::vector<uint8_t> members;
  ThreadPool zpool(std::min(decode_threads(), 16));              // the deflate's pool, as the host path's and pull's
  // the pieces of [from, to) of the stream, `from` a multiple of the piece: fetched, deflated, written
  auto write_pieces = [&](uint64_t from, uint64_t to) {
    const uint64_t n_pieces = (to - from + piece - 1) / piece;
    auto fetch = [&](uint64_t k) {
      Fetched &F = got[k & 1];
      const auto f0 = Clock::now();
      const uint64_t lo = from + k * piece, len = std::min(piece, to - lo);
      F = Fetched{};
      if (core) F.rc = strl_bamsort_fetch_bgzf(ctx, lo, len, buf[k & 1], room, &F.bytes, &F.stored);
      else { F.rc = strl_bamsort_fetch(ctx, lo, len, buf[k & 1]); F.bytes = len; }
      if (F.rc) F.err = strl_last_error();
      F.s = since(f0);
    };
    if (n_pieces) fetch(0);
    for (uint64_t k = 0; k < n_pieces; ++k) {
      std::thread ahead;
      if (k + 1 < n_pieces) ahead = std::thread(fetch, k + 1);
      const Fetched &F = got[k & 1];
      bool ok = !F.rc;
      if (!ok) { why = F.err; status = F.rc; }
      R.s.gather += F.s;
      const uint8_t *p = buf[k & 1];
      size_t n = (size_t)F.bytes;
      if (ok && !core) {
        t0 = Clock::now();
        status = STRL_ERR_IO;
        ok = deflate_piece(p, n, false, mode, zpool, members, R.stored, why);
        p = members.data(); n = members.size();
        R.s.deflate += since(t0);
      } else if (ok) R.stored += F.stored;
      if (ok) {
        t0 = Clock::now();
        status = STRL_ERR_IO;
        ok = out.put(p, n, why);
        R.out_bytes += n;
        R.s.write += since(t0);
      }
      if (ahead.joinable()) ahead.join();
      if (!ok) { (void)strl_bamsort_end(ctx); return false; }
    }
    return true;
  };
  if (!windowed) {
    if (!write_pieces(0, total)) return false;
    if (core) { strl_bamsort_info now; if (!strl_bamsort_info_now(ctx, &now)) { R.s.deflate = std::max(0.0, R.s.gather - now.gather_ms / 1e3); R.s.gather = now.gather_ms / 1e3; } }
  } else {
    for (uint64_t w = 0; w < plan.n_windows; ++w) {
      const uint64_t lo = w * plan.window_bytes, hi = std::min(total, lo + plan.window_bytes);
      const auto w0 = Clock::now();
      BgzfFeed again;                                            // the same file from its first block
      status = STRL_ERR_IO;
      if (!again.open(bam, err)) { why = err.empty() ? "couldn't open bam" : "couldn't open bam: " + err; (void)strl_bamsort_end(ctx); pins.release(); return false; }
      if (!feed_pass(again, [&]() -> int { return strl_bamsort_window_begin(ctx, lo, hi); }, strl_bamsort_window_push)) return false;
      if ((rc = strl_bamsort_window_end(ctx))) return fail(rc);
      R.s.window += since(w0);
      if (!write_pieces(lo, hi)) return false;
    }
    if (core) { R.s.deflate = R.s.gather; R.s.gather = 0; }      // (a fetch of a window's piece is the compressor's run and its copy)
  }
  R.deflate = !core ? "zlib" : mode == STRL_DEFLATE_DENSE ? "device-dense" : "device";
  if (X.on && !windowed) {                                      // the records, their order and their offsets are still on the device
    t0 = Clock::now();
    out.member_off.push_back(out.at);                           // the EOF block
    uint64_t nbytes = 0;
    strl_bamindex_info ii{};
    X.rc = strl_bamsort_index(ctx, X.l_ref.data(), X.min_shift, -1, out.member_off.data(), out.member_off.size() - 1, &nbytes, &ii);
    if (!X.rc) { X.bytes.resize((size_t)nbytes + 1); X.rc = strl_bamsort_index_fetch(ctx, X.bytes.data(), X.bytes.size()); X.bytes.resize((size_t)nbytes); }
    if (X.rc) X.why = strl_last_error();
    X.chunks = ii.n_chunks;
    X.s = since(t0);
  }
  (void)strl_bamsort_end(ctx);
  // (the page-locked buffers are left to the end of the process: unlocking them stalls the device, as `bamindex` leaves its own)
  status = 0;
  return true;
}

}  // namespace

int sort_main(int argc, char **argv) {
  if (argc <= 2) { fputs(USAGE, stdout); return 0; }
  const Args a = parse(argc, argv, 2, {{"output", 'o', true}, {"deflate", 0, true}, {"device", 'D', true}, {"verbose", 'v', false},
                                       {"write-index", 0, false}, {"index-out", 0, true}, {"csi", 0, false}, {"min-shift", 'm', true}, {"windowed", 0, false}, {"markdup", 0, false}}, USAGE);
  if (a.pos.size() != 1) quit("expected 1 argument (bam, sam or - for SAM text on stdin)\n%s", USAGE);
  if (!a.flag("output")) quit("[strling] sort: -o OUT.bam is required\n%s", USAGE);
  if (a.flag("index-out") && !a.flag("write-index")) quit("--index-out needs --write-index\n%s", USAGE);
  if (a.flag("csi") && !a.flag("write-index")) quit("--csi needs --write-index\n%s", USAGE);
  if (a.flag("markdup") && a.flag("windowed")) quit("[strling] sort: --markdup --windowed: the records are not resident; sort without --windowed or mark with samtools (status %d)", STRL_ERR_ARG);
  Index X;
  X.on = a.flag("write-index");
  X.min_shift = csi_min_shift(a, USAGE);
  const std::string bam = a.pos[0], out_path = a.get("output", ""), form = a.get("deflate", "host");
  if (form != "host" && form != "device" && form != "dense") quit("--deflate must be host or device, or dense (the device with its dense rule) (got %s)", form.c_str());
  const bool core = form != "host";
  const int mode = form == "dense" ? STRL_DEFLATE_DENSE : STRL_DEFLATE_FAST;
  const bool from_stdin = bam == "-";
  if (!from_stdin && CramFile::is_cram(bam)) quit("[strling] sort: %s is a CRAM; sorting one is out of scope: this command sorts a BAM", bam.c_str());
  if (!from_stdin && !file_exists(bam)) quit("couldn't open bam");
  const auto t_all = Clock::now();
  // the format, from the first bytes: BGZF magic is a BAM (from a file), `@` or anything else printable is SAM text
  SamInput sam_in;
  std::string sniff_err;
  const SamFeed::Kind kind = sam_in.feed.open(bam, sniff_err);
  if (kind == SamFeed::KIND_ERROR && from_stdin) quit("[strling] sort: %s (status %d)", sniff_err.c_str(), STRL_ERR_IO);
  if (from_stdin && kind == SamFeed::KIND_GZIP) quit("[strling] sort: a BAM on stdin is not read; write it to a file (status %d)", STRL_ERR_ARG);
  if (from_stdin && kind != SamFeed::KIND_SAM) quit("[strling] sort: stdin holds no SAM text (status %d)", STRL_ERR_FORMAT);
  SamInput *sam = kind == SamFeed::KIND_SAM ? &sam_in : nullptr;
  if (sam && a.flag("windowed")) quit("[strling] sort: --windowed reads its input once more for every window, and SAM text is read once (a pipe cannot be read again): sort a BAM in windows (status %d)", STRL_ERR_ARG);
  // the header, by the host reader, and the output's from it
  std::vector<uint8_t> header;
  int32_t n_ref = 0;
  if (sam) {
    std::string err;
    if (!sam->feed.read_header(sam->header, err)) quit("[strling] sort: %s (status %d)", err.c_str(), STRL_ERR_FORMAT);
    if (!bsort_header(sam->header.bam.data(), sam->header.bam.size(), header, &n_ref, nullptr, err)) quit("[strling] sort: %s (status %d)", err.c_str(), STRL_ERR_FORMAT);
  } else {
    BamReader rd;
    std::string err;
    if (!rd.open(bam, err)) quit("[strling] sort: %s (status %d)", err.empty() ? "malformed BAM header (truncated file or invalid BGZF block)" : err.c_str(), STRL_ERR_FORMAT);
    const std::vector<uint8_t> &h = rd.header_bytes();
    if (!bsort_header(h.data(), h.size(), header, &n_ref, nullptr, err)) quit("[strling] sort: %s (status %d)", err.c_str(), STRL_ERR_FORMAT);
  }
  if (X.on) {                              // what no index of the kind asked for can hold is refused before anything is read
    X.out = a.get("index-out", (out_path + (X.min_shift >= 0 ? ".csi" : ".bai")).c_str());
    size_t at = 12 + (size_t)bsort_ld32(header.data() + 4);      // (bsort_header has walked the list)
    for (int32_t t = 0; t < n_ref; ++t) {
      const uint32_t l_name = bsort_ld32(header.data() + at);
      const int32_t len = (int32_t)bsort_ld32(header.data() + at + 4 + l_name);
      if (X.min_shift < 0 && len > BAI_MAX_POS)
        quit("[strling] sort: --write-index: reference %s is %d bases long, past 2^29 = 536870912, which a .bai cannot address; a CSI index can: --csi (status %d)",
             std::string(reinterpret_cast<const char *>(header.data() + at + 4), l_name ? l_name - 1 : 0).c_str(), len, STRL_ERR_LIMIT);
      X.l_ref.push_back(len);
      at += 8 + (size_t)l_name;
    }
    X.l_ref.push_back(0);                  // (n_ref = 0: the builders still get a pointer)
  }
  const char *where = getenv("STRL_SORT");
  const bool on_host = (where && !strcmp(where, "host")) || strl_device_count() <= 0;
  // --windowed on the host path changes nothing: that path holds the file in host memory anyway.  On the device the records are
  // never resident in sorted order, so the index comes from the builder over the file just written, behind its rename
  const bool windowed = a.flag("windowed") && !on_host;
  SortOut out;
  out.track = X.on && !windowed;
  std::string why;
  int status = 0;
  Result R;
  R.markdup = a.flag("markdup");
  strl_ctx *ctx = nullptr;
  std::function<strl_ctx *(std::string &)> ctx_again = [&](std::string &) { return ctx; };      // the context once it is up
  bool ok;
  if (on_host) {
    if (!out.open(out_path, why)) quit("[strling] sort: %s (status %d)", why.c_str(), STRL_ERR_IO);
    ok = sort_on_host(bam, sam, header, n_ref, core, mode, out, R, X, why, status);
  } else {
    set_device0(a.get("device", ""));
    // the HIP runtime and the context come up on a thread beside the header walk, the page-locked buffers and the first chunk's read
    int ctx_rc = 0;
    std::string ctx_err;
    std::thread ctx_thread([&] { ctx_rc = strl_ctx_create(device_of(0), &ctx); if (ctx_rc) ctx_err = strl_last_error(); });
    g_bg_init = &ctx_thread;
    auto get_ctx = [&](std::string &w) -> strl_ctx * { if (ctx_thread.joinable()) ctx_thread.join(); if (ctx_rc) w = ctx_err; return ctx_rc ? nullptr : ctx; };
    ok = out.open(out_path, why);
    if (!ok) status = STRL_ERR_IO;
    else ok = sort_on_device(get_ctx, bam, sam, header, core, mode, windowed, out, R, X, why, status);
    if (ctx_thread.joinable()) ctx_thread.join();
    g_bg_init = nullptr;
  }
  if (ok && !out.close(why)) { ok = false; status = STRL_ERR_IO; }
  if (!ok) {
    out.drop();
    if (ctx) strl_ctx_destroy(ctx);
    if (status == STRL_ERR_NOMEM) quit("[strling] sort: %s; sort this file with samtools, or on a device with more memory (status %d)", why.c_str(), status);
    quit("[strling] sort: %s (status %d)", why.c_str(), status);
  }
  // the index behind the BAM's rename.  A refusal (the records' own: a negative position, a record past the end of its reference
  // or past what the scheme addresses) leaves the sorted file, which is complete and valid, and no index
  uint64_t index_bytes = 0;
  if (X.on && windowed) {                  // a second read of the output: the bytes `strling bamindex OUT.bam` writes, by the same function
    const auto t0 = Clock::now();
    int st = 0;
    if (!build_bai(ctx_again, out_path, X.out, false, false, X.why, st, X.min_shift)) X.rc = st ? st : STRL_ERR_IO;
    else if (FILE *f = fopen(X.out.c_str(), "rb")) { fseek(f, 0, SEEK_END); index_bytes = (uint64_t)ftell(f); fclose(f); }
    X.s = since(t0);
  } else if (X.on && !X.rc) {
    index_bytes = X.bytes.size();
    const auto t0 = Clock::now();
    ThreadPool pool(std::min(decode_threads(), 4));
    if (!write_index_file(X.out, X.bytes, X.min_shift >= 0, X.why, &pool)) X.rc = STRL_ERR_IO;
    X.s += since(t0);
  }
  const bool indexed = X.on && !X.rc;
  if (R.markdup)
    fprintf(stderr, "[strling] sort: markdup: %llu pairs, %llu duplicate pairs, %llu fragments, %llu duplicate fragments, %llu ineligible records\n", (unsigned long long)R.md.n_pairs,
            (unsigned long long)R.md.n_dup_pairs, (unsigned long long)R.md.n_fragments, (unsigned long long)R.md.n_dup_fragments, (unsigned long long)R.md.n_ineligible);
  if (a.flag("verbose"))
    fprintf(stderr,
            "{\"command\": \"sort\", \"path\": \"%s\", \"records\": %llu, \"no_reference\": %llu, \"stream_bytes\": %llu, \"out_bytes\": %llu, \"already_sorted\": %s, \"slabs\": %llu, "
            "\"seconds\": %.3f, \"read_s\": %.3f, \"sort_s\": %.3f, \"gather_s\": %.3f, \"deflate_s\": %.3f, \"write_s\": %.3f, \"deflate\": \"%s\", \"stored\": %u, "
            "\"index\": \"%s\", \"index_bytes\": %llu, \"index_chunks\": %llu, \"index_s\": %.3f, \"windows\": %llu, \"window_bytes\": %llu, \"window_s\": %.3f, "
            "\"input\": \"%s\", \"lines\": %llu, \"text_bytes\": %llu, \"host_finished\": %llu, \"sam_copy_ms\": %.3f, \"sam_scan_ms\": %.3f, \"sam_size_ms\": %.3f, "
            "\"sam_encode_ms\": %.3f, \"markdup\": %s, \"markdup_s\": %.3f, \"markdup_record_ms\": %.3f, \"markdup_join_ms\": %.3f, \"markdup_pairs_ms\": %.3f, "
            "\"markdup_fragments_ms\": %.3f, \"markdup_flag_ms\": %.3f}\n",
            on_host ? "host" : "device", (unsigned long long)R.records, (unsigned long long)R.no_ref, (unsigned long long)R.stream_bytes, (unsigned long long)R.out_bytes,
            R.already_sorted ? "true" : "false", (unsigned long long)R.slabs, since(t_all), R.s.read, R.s.sort, R.s.gather, R.s.deflate, R.s.write, R.deflate, R.stored,
            !indexed ? "none" : X.min_shift >= 0 ? "csi" : "bai", (unsigned long long)(indexed ? index_bytes : 0), (unsigned long long)(indexed ? X.chunks : 0), X.s,
            (unsigned long long)R.windows, (unsigned long long)R.window_bytes, R.s.window, sam ? "sam" : "bam", (unsigned long long)R.lines, (unsigned long long)R.text_bytes,
            (unsigned long long)R.host_finished, R.sam_ms[0], R.sam_ms[1], R.sam_ms[2], R.sam_ms[3], R.markdup ? "true" : "false", R.markdup_s, R.md.record_ms, R.md.join_ms,
            R.md.pairs_ms, R.md.fragments_ms, R.md.flag_ms);
  if (X.on && X.rc) {
    if (ctx) strl_ctx_destroy(ctx);
    quit("[strling] sort: sorted file written; index refused: %s (status %d)", X.why.c_str(), X.rc);
  }
  return end_process(ctx);
}
