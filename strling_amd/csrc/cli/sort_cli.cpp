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
// `strling fastq` (fastq_main below) is a mode of this driver: the same feeds fill the same arena, and behind the finish the reads go
// out as FASTQ text (strl_bamsort_fastq / _fastq_fetch; the rule is csrc/fastq_core.h's) instead of as a sorted BAM.  The host path
// (STRL_FASTQ=host, or no device) applies the same header's rule to its records.  DESIGN section 24.4.
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
#include "../fastq_core.h"
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

// ---- `strling fastq`: what was asked for, where the three streams go, what the step gave ------------------------------------------------
// one output: a file written under a temporary name and renamed at the end (a failed run leaves no file), or stdout
struct FastqOut {
  std::string path, tmp;
  FILE *f = nullptr;
  bool on = false, to_stdout = false;
  bool open(std::string &why) {
    if (to_stdout) { f = stdout; return true; }
    tmp = path + ".tmp." + std::to_string((long long)getpid());
    f = fopen(tmp.c_str(), "wb");
    if (!f) why = "cannot write " + tmp + ": " + strerror(errno);
    return f != nullptr;
  }
  bool put(const uint8_t *p, size_t n, std::string &why) {
    if (n && fwrite(p, 1, n, f) != n) { why = "cannot write " + (to_stdout ? std::string("stdout") : tmp) + ": " + strerror(errno); return false; }
    return true;
  }
  bool close(std::string &why) {
    if (!f) return true;
    bool ok = to_stdout ? fflush(stdout) == 0 : fclose(f) == 0;
    f = nullptr;
    if (ok && !to_stdout && rename(tmp.c_str(), path.c_str()) != 0) ok = false;
    if (!ok) { if (why.empty()) why = "cannot write " + (to_stdout ? std::string("stdout") : path) + ": " + strerror(errno); if (!to_stdout) unlink(tmp.c_str()); }
    return ok;
  }
  void drop() { if (f && !to_stdout) fclose(f); f = nullptr; if (!to_stdout && !tmp.empty()) unlink(tmp.c_str()); }
};
struct Fastq {
  strl_fastq_opts opts{FASTQ_FILTER_DEFAULT, 0, 1, 0, 0};
  FastqOut out[3];                            // by stream: p1 (or the interleaved pairs), p2, s
  strl_fastq_info info{};
  double plan_s = 0, fetch_s = 0, write_s = 0;
};

uint64_t fastq_piece_bytes() {
  const char *e = getenv("STRL_FASTQ_PIECE_KB");               // tests: pieces that cut entries anywhere
  return e && atof(e) > 0 ? std::max<uint64_t>(1, (uint64_t)(atof(e) * 1024.0)) : (uint64_t)128 << 20;
}

// the host path's: the rule over the records in input order, the three streams written whole
bool fastq_on_host(const std::vector<uint8_t> &raw, Fastq &Q, std::string &why, int &status) {
  auto t0 = Clock::now();
  const FastqOpts o{Q.opts.filter, Q.opts.suffix, Q.opts.default_qual, Q.opts.interleaved, Q.opts.singles};
  std::vector<uint8_t> stream[3];
  FastqCounts C{};
  std::string w;
  static const uint8_t none = 0;
  const int64_t bad = fastq_host(raw.empty() ? &none : raw.data(), raw.size(), o, stream, &C, w);
  if (bad >= 0) { why = "malformed BAM record " + std::to_string(bad) + ": " + w; status = STRL_ERR_FORMAT; return false; }
  Q.info.n_kept = C.kept; Q.info.n_filtered = C.filtered; Q.info.n_empty = C.empty; Q.info.n_pairs = C.pairs; Q.info.n_singles = C.singles; Q.info.n_singles_unwritten = C.singles_unwritten;
  for (int s = 0; s < 3; ++s) Q.info.stream_bytes[s] = stream[s].size();
  Q.plan_s = since(t0);
  t0 = Clock::now();
  status = STRL_ERR_IO;
  for (int s = 0; s < 3; ++s)
    if (Q.out[s].on && !Q.out[s].put(stream[s].data(), stream[s].size(), why)) return false;
  Q.write_s = since(t0);
  status = 0;
  return true;
}

// the device path's, behind strl_bamsort_finish: the plan, then every stream in pieces -- the fetch of piece k + 1 into one of two
// page-locked buffers on a thread beside the write of piece k, as the sorted stream's pieces go
bool fastq_on_device(strl_ctx *ctx, Fastq &Q, std::string &why, int &status) {
  auto t0 = Clock::now();
  int rc = strl_bamsort_fastq(ctx, &Q.opts, &Q.info);
  if (rc) { why = strl_last_error(); status = rc; return false; }
  Q.plan_s = since(t0);
  const uint64_t piece = fastq_piece_bytes();
  uint64_t room = 0;
  for (int s = 0; s < 3; ++s) if (Q.out[s].on) room = std::max(room, std::min(piece, (uint64_t)Q.info.stream_bytes[s]));
  uint8_t *buf[2] = {static_cast<uint8_t *>(strl_pinned_alloc(room + 64)), static_cast<uint8_t *>(strl_pinned_alloc(room + 64))};
  if (!buf[0] || !buf[1]) { why = "page-locked memory for the pieces"; status = STRL_ERR_NOMEM; return false; }
  struct Fetched { int rc = 0; std::string err; uint64_t bytes = 0; double s = 0; } got[2];
  for (int s = 0; s < 3; ++s) {
    if (!Q.out[s].on) continue;
    const uint64_t total = Q.info.stream_bytes[s], n_pieces = (total + piece - 1) / piece;
    auto fetch = [&](uint64_t k) {
      Fetched &F = got[k & 1];
      const auto f0 = Clock::now();
      const uint64_t lo = k * piece;
      F = Fetched{};
      F.bytes = std::min(piece, total - lo);
      F.rc = strl_bamsort_fastq_fetch(ctx, s, lo, F.bytes, buf[k & 1]);
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
      Q.fetch_s += F.s;
      if (ok) {
        t0 = Clock::now();
        status = STRL_ERR_IO;
        ok = Q.out[s].put(buf[k & 1], (size_t)F.bytes, why);
        Q.write_s += since(t0);
      }
      if (ahead.joinable()) ahead.join();
      if (!ok) return false;
    }
  }
  (void)strl_bamsort_fastq_info_now(ctx, &Q.info);             // (the text kernel's time over the fetches)
  status = 0;
  return true;
}

// ---- the host path ---------------------------------------------------------------------------------------------------------------
// SAM text on the host: what the feed reads, line by line through sam_core.h's host function
struct SamInput { SamFeed feed; SamHeader header; };

bool sort_on_host(const std::string &bam, SamInput *sam, const std::vector<uint8_t> &header, int32_t n_ref, bool core, int mode, SortOut &out, Result &R, Index &X, std::string &why, int &status,
                  Fastq *fq = nullptr) {
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
  if (fq) { R.records = at.size(); return fastq_on_host(raw, *fq, why, status); }      // `strling fastq`: the records in input order are all it needs
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
                    SortOut &out, Result &R, Index &X, std::string &why, int &status, Fastq *fq = nullptr) {
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
    if (!rc && fq) rc = strl_bamsort_fastq_mode(ctx, 1);
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
    if (!rc && fq) rc = strl_bamsort_fastq_mode(ctx, 1);
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
  if (fq) {                                                     // `strling fastq`: every record lies on the device; the text instead of the sorted stream
    R.records = info.n_records; R.slabs = info.n_slabs;
    const bool ok = fastq_on_device(ctx, *fq, why, status);
    (void)strl_bamsort_end(ctx);
    if (!ok) pins.release();
    return ok;
  }
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

// the input's format, from its first bytes: BGZF magic is a BAM (from a file), `@` or anything else printable is SAM text
// -> sam_in opened as the SAM feed, or null for a BAM; `cmd` names the command in the refusals
SamInput *sniff_input(const char *cmd, const std::string &bam, bool from_stdin, SamInput &sam_in) {
  std::string sniff_err;
  const SamFeed::Kind kind = sam_in.feed.open(bam, sniff_err);
  if (kind == SamFeed::KIND_ERROR && from_stdin) quit("[strling] %s: %s (status %d)", cmd, sniff_err.c_str(), STRL_ERR_IO);
  if (from_stdin && kind == SamFeed::KIND_GZIP) quit("[strling] %s: a BAM on stdin is not read; write it to a file (status %d)", cmd, STRL_ERR_ARG);
  if (from_stdin && kind != SamFeed::KIND_SAM) quit("[strling] %s: stdin holds no SAM text (status %d)", cmd, STRL_ERR_FORMAT);
  return kind == SamFeed::KIND_SAM ? &sam_in : nullptr;
}
// the header, by the host reader, and the output's from it
void read_header(const char *cmd, const std::string &bam, SamInput *sam, std::vector<uint8_t> &header, int32_t &n_ref) {
  if (sam) {
    std::string err;
    if (!sam->feed.read_header(sam->header, err)) quit("[strling] %s: %s (status %d)", cmd, err.c_str(), STRL_ERR_FORMAT);
    if (!bsort_header(sam->header.bam.data(), sam->header.bam.size(), header, &n_ref, nullptr, err)) quit("[strling] %s: %s (status %d)", cmd, err.c_str(), STRL_ERR_FORMAT);
  } else {
    BamReader rd;
    std::string err;
    if (!rd.open(bam, err)) quit("[strling] %s: %s (status %d)", cmd, err.empty() ? "malformed BAM header (truncated file or invalid BGZF block)" : err.c_str(), STRL_ERR_FORMAT);
    const std::vector<uint8_t> &h = rd.header_bytes();
    if (!bsort_header(h.data(), h.size(), header, &n_ref, nullptr, err)) quit("[strling] %s: %s (status %d)", cmd, err.c_str(), STRL_ERR_FORMAT);
  }
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
  SamInput sam_in;
  SamInput *sam = sniff_input("sort", bam, from_stdin, sam_in);
  if (sam && a.flag("windowed")) quit("[strling] sort: --windowed reads its input once more for every window, and SAM text is read once (a pipe cannot be read again): sort a BAM in windows (status %d)", STRL_ERR_ARG);
  std::vector<uint8_t> header;
  int32_t n_ref = 0;
  read_header("sort", bam, sam, header, n_ref);
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

// ---- `strling fastq` -----------------------------------------------------------------------------------------------------------------
namespace {
const char *FASTQ_USAGE =
    "strling fastq\n\nUsage:\n  strling fastq [options] -o OUT.fq|- IN.bam|IN.sam|-\n  strling fastq [options] -1 R1.fq -2 R2.fq IN.bam|IN.sam|-\n"
    "  strling fastq -o - old.bam | bwa mem -p ref.fa - | strling sort --markdup --write-index -o new.bam -\n\n"
    "A BAM's reads back to paired FASTQ, for realignment: mates are joined by name on the GPU, whatever the order of the file (what\n"
    "`samtools collate | samtools fastq` is used for).  A name with exactly two kept records, one first (0x40) and one last (0x80) read,\n"
    "is a pair; every other kept record is a single.  Pairs stand in the order of first appearance, R1 before R2.\n\n"
    "Arguments:\n  IN.bam           path to a bam file, in any order\n  IN.sam, -        SAM text instead, from a file or from stdin (told from a BAM by its first bytes)\n\nOptions:\n"
    "  -o, --output=FILE|-        the pairs interleaved (R1, R2, R1, R2 ...), to a file or to stdout: what `bwa mem -p` reads\n"
    "  -1 FILE -2 FILE            instead of -o: first reads to one file, last reads to the other\n"
    "  -s, --singles=FILE         the singles; without it they are counted and reported as left out, never mixed into the pairs\n"
    "  -F, --filter=INT           leave out records with any of these flag bits (default: 0x900, secondary and supplementary)\n"
    "  -N, --suffix               /1 and /2 behind the names of first and last reads\n"
    "  -v, --default-qual=INT     the quality of every base of a read that has none (default: 1)\n"
    "  -D, --device=K             GPU to use (default: 0)\n"
    "      --verbose              one JSON line on stderr with the step's times\n  -h, --help                 Show this help\n\n"
    "Out of scope: tags and barcodes in the header line (samtools' -T, CASAVA), compressed output (pipe through a compressor), CRAM\n"
    "input, and files larger than device memory (sort's --windowed has no counterpart here).  Reads without a sequence (l_seq 0) are\n"
    "counted and left out.  STRL_FASTQ=host (or a machine without a GPU) takes the host path: the same bytes.\n";
}  // namespace

int fastq_main(int argc, char **argv) {
  if (argc <= 2) { fputs(FASTQ_USAGE, stdout); return 0; }
  const Args a = parse(argc, argv, 2, {{"output", 'o', true}, {"out1", '1', true}, {"out2", '2', true}, {"singles", 's', true}, {"filter", 'F', true}, {"suffix", 'N', false},
                                       {"default-qual", 'v', true}, {"device", 'D', true}, {"verbose", 0, false}}, FASTQ_USAGE);
  if (a.pos.size() != 1) quit("expected 1 argument (bam, sam or - for SAM text on stdin)\n%s", FASTQ_USAGE);
  if (a.flag("output") && (a.flag("out1") || a.flag("out2"))) quit("[strling] fastq: -o writes the pairs interleaved and -1 / -2 write them to two files: give one or the other (status %d)", STRL_ERR_ARG);
  if (a.flag("out1") != a.flag("out2")) quit("[strling] fastq: -1 and -2 go together (status %d)", STRL_ERR_ARG);
  if (!a.flag("output") && !a.flag("out1")) quit("[strling] fastq: -o FILE|- or -1 FILE -2 FILE is required\n%s", FASTQ_USAGE);
  auto number = [&](const char *k, const char *dflt, unsigned long max) {
    const std::string v = a.get(k, dflt);
    char *end = nullptr;
    const unsigned long x = strtoul(v.c_str(), &end, 0);
    if (v.empty() || *end || v[0] == '-' || x > max) quit("[strling] fastq: --%s must be an integer in [0, %lu] (got %s) (status %d)", k, max, v.c_str(), STRL_ERR_ARG);
    return (uint32_t)x;
  };
  Fastq Q;
  Q.opts.filter = number("filter", "0x900", 0xffff);
  Q.opts.default_qual = number("default-qual", "1", 255);
  Q.opts.suffix = a.flag("suffix");
  Q.opts.interleaved = a.flag("output");
  Q.opts.singles = a.flag("singles");
  const std::string names[3] = {Q.opts.interleaved ? a.get("output", "") : a.get("out1", ""), a.get("out2", ""), a.get("singles", "")};
  for (int s = 0; s < 3; ++s) { Q.out[s].on = !names[s].empty(); Q.out[s].path = names[s]; }
  Q.out[0].to_stdout = Q.opts.interleaved && names[0] == "-";
  const std::string bam = a.pos[0];
  const bool from_stdin = bam == "-";
  if (!from_stdin && CramFile::is_cram(bam)) quit("[strling] fastq: %s is a CRAM; reading one is out of scope: this command reads a BAM", bam.c_str());
  if (!from_stdin && !file_exists(bam)) quit("couldn't open bam");
  const auto t_all = Clock::now();
  SamInput sam_in;
  SamInput *sam = sniff_input("fastq", bam, from_stdin, sam_in);
  std::vector<uint8_t> header;
  int32_t n_ref = 0;
  read_header("fastq", bam, sam, header, n_ref);
  const char *where = getenv("STRL_FASTQ");
  const bool on_host = (where && !strcmp(where, "host")) || strl_device_count() <= 0;
  std::string why;
  int status = 0;
  bool ok = true;
  for (int s = 0; s < 3 && ok; ++s) if (Q.out[s].on && !Q.out[s].open(why)) { ok = false; status = STRL_ERR_IO; }
  SortOut none;
  Result R;
  Index X;
  strl_ctx *ctx = nullptr;
  if (ok && on_host) ok = sort_on_host(bam, sam, header, n_ref, false, STRL_DEFLATE_FAST, none, R, X, why, status, &Q);
  else if (ok) {
    set_device0(a.get("device", ""));
    int ctx_rc = 0;
    std::string ctx_err;
    std::thread ctx_thread([&] { ctx_rc = strl_ctx_create(device_of(0), &ctx); if (ctx_rc) ctx_err = strl_last_error(); });
    g_bg_init = &ctx_thread;
    auto get_ctx = [&](std::string &w) -> strl_ctx * { if (ctx_thread.joinable()) ctx_thread.join(); if (ctx_rc) w = ctx_err; return ctx_rc ? nullptr : ctx; };
    ok = sort_on_device(get_ctx, bam, sam, header, false, STRL_DEFLATE_FAST, false, none, R, X, why, status, &Q);
    if (ctx_thread.joinable()) ctx_thread.join();
    g_bg_init = nullptr;
  }
  for (int s = 0; s < 3 && ok; ++s) if (Q.out[s].on && !Q.out[s].close(why)) { ok = false; status = STRL_ERR_IO; }
  if (!ok) {
    for (FastqOut &o : Q.out) o.drop();
    if (ctx) strl_ctx_destroy(ctx);
    if (status == STRL_ERR_NOMEM) quit("[strling] fastq: %s; the records of this file do not fit the device: STRL_FASTQ=host writes it on the host (status %d)", why.c_str(), status);
    quit("[strling] fastq: %s (status %d)", why.c_str(), status);
  }
  const strl_fastq_info &I = Q.info;
  fprintf(stderr, "[strling] fastq: %llu records kept, %llu filtered, %llu empty, %llu pairs, %llu singles, %llu singles not written\n", (unsigned long long)I.n_kept,
          (unsigned long long)I.n_filtered, (unsigned long long)I.n_empty, (unsigned long long)I.n_pairs, (unsigned long long)I.n_singles, (unsigned long long)I.n_singles_unwritten);
  if (a.flag("verbose"))
    fprintf(stderr,
            "{\"command\": \"fastq\", \"path\": \"%s\", \"input\": \"%s\", \"records\": %llu, \"slabs\": %llu, \"p1_bytes\": %llu, \"p2_bytes\": %llu, \"s_bytes\": %llu, \"seconds\": %.3f, "
            "\"read_s\": %.3f, \"sort_s\": %.3f, \"plan_s\": %.3f, \"fetch_s\": %.3f, \"write_s\": %.3f, \"record_ms\": %.3f, \"join_ms\": %.3f, \"layout_ms\": %.3f, \"text_ms\": %.3f, "
            "\"text_bytes\": %llu}\n",
            on_host ? "host" : "device", sam ? "sam" : "bam", (unsigned long long)R.records, (unsigned long long)R.slabs, (unsigned long long)I.stream_bytes[0],
            (unsigned long long)I.stream_bytes[1], (unsigned long long)I.stream_bytes[2], since(t_all), R.s.read, R.s.sort, Q.plan_s, Q.fetch_s, Q.write_s, I.record_ms, I.join_ms,
            I.layout_ms, I.text_ms, (unsigned long long)I.text_bytes);
  return end_process(ctx);
}
