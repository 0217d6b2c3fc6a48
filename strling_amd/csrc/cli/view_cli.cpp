// view_cli.cpp -- `strling view`: a BAM's records as SAM text (what `samtools view` is used for; the reference's simulator shells out
// to it, sim/sim_shared.groovy:94).  The rule is csrc/view_core.h's.  DESIGN section 24.5.
//
// Whole file, device path: fed exactly as `strling bamindex` is (BgzfFeed, ChunkAhead, STRL_CHUNK_BLOCKS, the context brought up on a
// thread beside the first chunk's read); strl_view_push hands back the lines of the chunk pushed before, which are written while the
// next chunk is fetched.  Regions (the .bai or .csi is needed): each in the order given -- the host reader's records of the region
// (BamReader::region_seek / region_next: every record from the first that can overlap it), a bounded batch at a time, through
// strl_view_records_at with the region in the options, which keeps the records that overlap; both paths so take a region of any size.
// A record that overlaps two given regions is written once for each.  -c: the size kernel's counts alone, no text.
// Host path (STRL_VIEW=host, or no device): the host BAM reader and the same header's function; the same bytes.
// A file goes out under a temporary name and is renamed at the end: a failed run leaves no file.
#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#include <algorithm>
#include <chrono>
#include <functional>
#include <string>
#include <thread>
#include <vector>
#include "cli_shared.h"
#include "bam_reader.h"
#include "bgzf_feed.h"
#include "cram_reader.h"
#include "../view_core.h"

using namespace strl;

namespace {

using Clock = std::chrono::steady_clock;
double since(Clock::time_point t) { return std::chrono::duration<double>(Clock::now() - t).count(); }

const char *USAGE =
    "strling view\n\nUsage:\n  strling view [options] IN.bam [REGION ...]\n\n"
    "Arguments:\n  IN.bam           path to a bam file; with regions, coordinate-sorted and with its .bai or .csi index\n"
    "  REGION           NAME, NAME:BEG or NAME:BEG-END (1-based, inclusive); a record that overlaps two regions is written for each\n\nOptions:\n"
    "  -h                         write the header's text in front of the records\n  -H                         write the header's text alone\n"
    "  -c                         print the count of kept records and no text\n"
    "  -f INT                     keep records with every one of these flag bits set\n  -F INT                     keep records with none of these flag bits set\n"
    "  -G INT                     drop records with every one of these flag bits set\n  -q INT                     keep records with MAPQ >= INT\n"
    "  -o FILE                    output (default: stdout); a file is written through a temporary name\n"
    "  -D, --device=K             GPU to use (default: 0)\n      --verbose              one JSON line on stderr\n      --help                 Show this help\n\n"
    "Not read or written by this command: SAM or CRAM input, -b and every other output format (-C, -1, -u), -@, read-group and tag\n"
    "filters (-r, -R, -d), -M, -s, -L.\n";

struct Out {
  std::string path, tmp;
  FILE *f = nullptr;
  bool to_stdout = true;
  uint64_t bytes = 0;
  bool open(std::string &why) {
    if (to_stdout) { f = stdout; return true; }
    tmp = path + ".tmp." + std::to_string((long)getpid());
    f = fopen(tmp.c_str(), "wb");
    if (!f) { why = "cannot write " + tmp + ": " + strerror(errno); return false; }
    return true;
  }
  bool put(const void *p, size_t n, std::string &why) {
    if (n && fwrite(p, 1, n, f) != n) { why = std::string("cannot write the output: ") + strerror(errno); return false; }
    bytes += n;
    return true;
  }
  bool close(std::string &why) {
    if (to_stdout) { if (fflush(stdout)) { why = std::string("cannot write the output: ") + strerror(errno); return false; } return true; }
    const bool ok = fclose(f) == 0;
    f = nullptr;
    if (!ok || rename(tmp.c_str(), path.c_str())) { why = "cannot write " + path + ": " + strerror(errno); return false; }
    tmp.clear();
    return true;
  }
  void drop() {
    if (f && !to_stdout) fclose(f);
    f = nullptr;
    if (!tmp.empty()) unlink(tmp.c_str());
  }
};

struct View {
  strl_view_opts opts{0, 0, 0, 0, VIEW_NO_REGION, 0, 0};
  bool count_only = false;
  Out out;
  std::vector<uint8_t> names;
  std::vector<uint32_t> name_off;
  strl_view_info info{};
  double read_s = 0, view_s = 0, write_s = 0;
};

void add_info(strl_view_info &a, const strl_view_info &b) {
  a.records += b.records; a.written += b.written; a.dropped += b.dropped; a.text_bytes += b.text_bytes;
  a.chunks += b.chunks; a.host_chunks += b.host_chunks; a.size_ms += b.size_ms; a.text_ms += b.text_ms;
}

bool write_text(View &V, const uint8_t *text, uint64_t bytes, std::string &why) {
  if (V.count_only || !bytes) return true;
  const auto t = Clock::now();
  const bool ok = V.out.put(text, (size_t)bytes, why);
  V.write_s += since(t);
  return ok;
}

// records back to back through the host twin; ord0: the ordinal of the first
bool host_records(View &V, const std::vector<uint8_t> &raw, const strl_view_opts &o, uint64_t ord0, std::vector<uint8_t> &text, std::string &why, int &status) {
  const ViewOpts vo{o.require, o.exclude, o.exclude_all, o.min_mapq, o.tid, o.beg, o.end};
  const ViewRefs F{V.names.data(), V.name_off.data(), (int32_t)V.name_off.size() - 1};
  text.clear();
  ViewCounts C{};
  uint32_t code = 0;
  static const uint8_t none = 0;
  const auto t = Clock::now();
  const int64_t bad = view_host(raw.empty() ? &none : raw.data(), raw.size(), F, vo, text, &C, ord0, &code);
  V.view_s += since(t);
  if (bad >= 0) { why = "malformed BAM record " + std::to_string(bad) + ": " + view_refusal_text(code); status = STRL_ERR_FORMAT; return false; }
  V.info.records += C.records; V.info.written += C.written; V.info.dropped += C.dropped; V.info.text_bytes += C.text_bytes;
  return true;
}

bool whole_on_host(const std::string &bam, View &V, std::string &why, int &status) {
  BamReader rd;
  std::string err;
  if (!rd.open(bam, err)) { why = "couldn't open bam" + (err.empty() ? "" : ": " + err); status = STRL_ERR_IO; return false; }
  std::vector<uint8_t> raw, text;
  uint64_t ord = 0;
  for (;;) {
    raw.clear();
    const auto t = Clock::now();
    const int64_t got = rd.read_raw(raw, 1 << 16, err);
    V.read_s += since(t);
    if (got < 0) { why = "error reading " + bam + ": " + err; status = STRL_ERR_FORMAT; return false; }
    if (!got) break;
    if (!host_records(V, raw, V.opts, ord, text, why, status)) return false;
    ord += (uint64_t)got;
    if (!write_text(V, text.data(), text.size(), why)) { status = STRL_ERR_IO; return false; }
  }
  return true;
}

bool whole_on_device(const std::function<strl_ctx *(std::string &)> &get_ctx, const std::string &bam, View &V, std::string &why, int &status) {
  status = STRL_ERR_IO;
  BgzfFeed feed;
  std::string err;
  if (!feed.open(bam, err)) { why = err.empty() ? "couldn't open bam" : "couldn't open bam: " + err; return false; }
  static const char *env_blocks = getenv("STRL_CHUNK_BLOCKS");     // tests: tiny chunks put records across pushes
  const size_t auto_blocks = std::min<size_t>(16384, std::max<size_t>(2048, feed.file_bytes() / 16384 / 12));
  const size_t chunk_blocks = env_blocks && atoi(env_blocks) > 0 ? (size_t)atoi(env_blocks) : auto_blocks;
  const size_t chunk_bytes = std::max<size_t>((size_t)1 << 20, chunk_blocks * 20000);
  PinnedRing pins;
  pins.alloc(3, chunk_blocks, chunk_bytes);
  if (!pins.ok()) { why = "page-locked memory for the chunks"; pins.release(); return false; }
  strl_ctx *ctx = nullptr;
  auto fail = [&](int rc) { why = strl_last_error(); status = rc; (void)strl_view_end(ctx); pins.release(); return false; };
  ThreadPool pool(std::min(decode_threads(), 12));
  ChunkAhead ring(feed, pool, pins.data.data(), pins.meta.data(), chunk_blocks, chunk_bytes);
  ring.stage(0, 0);
  if (!(ctx = get_ctx(why))) { status = STRL_ERR_NO_DEVICE; pins.release(); return false; }
  int rc = strl_view_begin(ctx, (int32_t)V.name_off.size() - 1, feed.first_record_offset(), V.names.data(), V.name_off.data(), &V.opts);
  if (!rc && V.count_only) rc = strl_view_count_only(ctx, 1);      // -c: the counts alone, no text kernel and no copy
  if (!rc) rc = strl_view_reserve(ctx, (uint32_t)chunk_blocks, chunk_bytes);
  if (rc) return fail(rc);
  const uint8_t *text = nullptr;
  uint64_t bytes = 0;
  for (uint64_t ci = 0;; ++ci) {
    const auto t = Clock::now();
    const StagedChunk cur = ring.at(ci);
    V.read_s += since(t);
    if (cur.nb < 0 || cur.short_read) { why = cur.nb < 0 ? cur.err : "short read"; status = STRL_ERR_FORMAT; (void)strl_view_end(ctx); pins.release(); return false; }
    if (cur.nb == 0) break;
    ring.stage_ahead(ci + 1, (ci + 1) % 3);
    const ChunkTables tb = ring.tables(cur);
    const auto tv = Clock::now();
    rc = strl_view_push(ctx, ring.data(cur), cur.bytes(), tb.coff, tb.clen, tb.isz, tb.crc, (uint32_t)cur.nb, &text, &bytes);
    V.view_s += since(tv);
    const bool wrote = rc || write_text(V, text, bytes, why);      // (the lines of chunk ci - 1, beside the fetch of chunk ci + 1)
    ring.join();
    if (rc) return fail(rc);
    if (!wrote) { status = STRL_ERR_IO; (void)strl_view_end(ctx); pins.release(); return false; }
  }
  const auto tv = Clock::now();
  rc = strl_view_finish(ctx, &text, &bytes, &V.info);
  V.view_s += since(tv);
  if (rc) return fail(rc);
  if (!write_text(V, text, bytes, why)) { status = STRL_ERR_IO; (void)strl_view_end(ctx); pins.release(); return false; }
  (void)strl_view_end(ctx);
  status = 0;
  return true;
}

// Records of a region a batch: what bounds the host memory (a batch of records and its text) and one strl_view_records call, whatever
// the region holds.  STRL_VIEW_BATCH_RECORDS (tests): a few records a batch, so that a region is cut many times.
int64_t batch_records() {
  static const char *e = getenv("STRL_VIEW_BATCH_RECORDS");
  return e && atoll(e) > 0 ? atoll(e) : (int64_t)1 << 18;
}

bool regions_view(strl_ctx *ctx, const std::string &bam, const std::vector<PullRegion> &regions, BamReader &rd, View &V, std::string &why, int &status) {
  std::vector<uint8_t> raw, text;
  const int32_t n_ref = (int32_t)V.name_off.size() - 1;
  const int64_t batch = batch_records();
  for (const PullRegion &r : regions) {
    std::string err;
    strl_view_opts o = V.opts;
    o.tid = r.tid; o.beg = (int32_t)r.beg; o.end = (int32_t)std::min<int64_t>(r.end, INT32_MAX);
    const int at = rd.region_seek(r.tid, r.beg, r.end, err);
    if (at < 0) { why = "error reading " + bam + ": " + err; status = STRL_ERR_FORMAT; return false; }
    uint64_t ord = 0;                                         // of the batch's first record among the records the region's walk reads
    for (int64_t got = at ? batch : 0; got == batch;) {
      raw.clear();
      const auto t = Clock::now();
      got = rd.region_next(raw, batch, r.tid, r.end, err);
      V.read_s += since(t);
      if (got < 0) { why = "error reading " + bam + ": " + err; status = STRL_ERR_FORMAT; return false; }
      if (!got) break;
      if (!ctx) { if (!host_records(V, raw, o, ord, text, why, status)) return false; }
      else {
        const auto tv = Clock::now();
        uint64_t need = 0;
        strl_view_info I{};
        int rc;
        if (V.count_only) {                                   // the counts alone: no text kernel, no copy
          rc = strl_view_records_at(ctx, raw.data(), raw.size(), V.names.data(), V.name_off.data(), n_ref, &o, ord, nullptr, 0, &need, &I);
          if (rc == STRL_ERR_CAPACITY) rc = STRL_OK;
          need = 0;
        } else {
          text.resize(std::max<size_t>(raw.size() * 2, 4096));
          rc = strl_view_records_at(ctx, raw.data(), raw.size(), V.names.data(), V.name_off.data(), n_ref, &o, ord, text.data(), text.size(), &need, &I);
          if (rc == STRL_ERR_CAPACITY) {
            text.resize((size_t)need);
            rc = strl_view_records_at(ctx, raw.data(), raw.size(), V.names.data(), V.name_off.data(), n_ref, &o, ord, text.data(), text.size(), &need, &I);
          }
        }
        V.view_s += since(tv);
        if (rc) { why = strl_last_error(); status = rc; return false; }
        text.resize((size_t)need);
        add_info(V.info, I);
      }
      ord += (uint64_t)got;
      if (!write_text(V, text.data(), text.size(), why)) { status = STRL_ERR_IO; return false; }
    }
  }
  return true;
}

}  // namespace

int view_main(int argc, char **argv) {
  if (argc <= 2) { fputs(USAGE, stdout); return 0; }
  View V;
  bool with_header = false, header_only = false, verbose = false;
  std::string device;
  std::vector<std::string> pos;
  auto number = [&](const char *k, const char *v, unsigned long max) {
    char *end = nullptr;
    const unsigned long x = strtoul(v, &end, 0);
    if (!*v || *end || v[0] == '-' || x > max) quit("[strling] view: %s must be an integer in [0, %lu] (got %s) (status %d)", k, max, v, STRL_ERR_ARG);
    return (uint32_t)x;
  };
  for (int i = 2; i < argc; ++i) {
    const std::string s = argv[i];
    auto value = [&]() -> const char * { if (i + 1 >= argc) quit("option %s needs a value", s.c_str()); return argv[++i]; };
    if (s == "--help") { fputs(USAGE, stdout); return 0; }
    else if (s == "-h") with_header = true;
    else if (s == "-H") header_only = true;
    else if (s == "-c") V.count_only = true;
    else if (s == "--verbose") verbose = true;
    else if (s == "-f") V.opts.require = number("-f", value(), 0xffff);
    else if (s == "-F") V.opts.exclude = number("-F", value(), 0xffff);
    else if (s == "-G") V.opts.exclude_all = number("-G", value(), 0xffff);
    else if (s == "-q") V.opts.min_mapq = number("-q", value(), 255);
    else if (s == "-o") { V.out.path = value(); V.out.to_stdout = V.out.path == "-"; }
    else if (s == "-D") device = value();
    else if (!s.compare(0, 9, "--device=")) device = s.substr(9);
    else if (s.size() > 1 && s[0] == '-') quit("[strling] view: option %s is not one of this command's\n%s", s.c_str(), USAGE);
    else pos.push_back(s);
  }
  if (pos.empty()) quit("expected a bam\n%s", USAGE);
  const std::string bam = pos[0];
  if (bam == "-") quit("[strling] view: SAM text on stdin is not read by this command (`strling sort` reads it)\n%s", USAGE);
  if (!file_exists(bam)) quit("couldn't open bam");
  if (CramFile::is_cram(bam)) quit("[strling] view: %s is a CRAM; this command reads a BAM", bam.c_str());
  {
    uint8_t magic[2] = {0, 0};
    FILE *f = fopen(bam.c_str(), "rb");
    const size_t got = f ? fread(magic, 1, 2, f) : 0;
    if (f) fclose(f);
    if (got != 2 || magic[0] != 0x1f || magic[1] != 0x8b) quit("[strling] view: %s is not a BAM (SAM text is not read by this command; `strling sort` reads it)", bam.c_str());
  }
  const auto t_all = Clock::now();
  BamReader rd;
  std::string err;
  if (!rd.open(bam, err)) quit("couldn't open bam%s%s", err.empty() ? "" : ": ", err.c_str());
  V.name_off.push_back(0);
  for (const BamTarget &t : rd.targets()) { V.names.insert(V.names.end(), t.name.begin(), t.name.end()); V.name_off.push_back((uint32_t)V.names.size()); }
  if (V.names.empty()) V.names.push_back(0);                  // (never read: a pointer for the ABI)
  std::vector<PullRegion> regions;
  if (pos.size() > 1) {
    if (!rd.load_index(bam, err)) quit("[strling] view: %s", err.c_str());
    for (size_t k = 1; k < pos.size(); ++k) regions.push_back(parse_pull_region(pos[k], rd.targets(), "view"));
  }
  const char *where = getenv("STRL_VIEW");
  const bool on_host = header_only || (where && !strcmp(where, "host")) || strl_device_count() <= 0;
  std::string why;
  int status = 0;
  bool ok = V.out.open(why);
  if (!ok) status = STRL_ERR_IO;
  if (ok && (with_header || header_only) && !V.count_only) {
    const std::string &text = rd.header_text();
    ok = V.out.put(text.data(), text.size(), why);
    if (!ok) status = STRL_ERR_IO;
  }
  strl_ctx *ctx = nullptr;
  if (ok && !header_only) {
    if (on_host) ok = regions.empty() ? whole_on_host(bam, V, why, status) : regions_view(nullptr, bam, regions, rd, V, why, status);
    else {
      set_device0(device);
      int ctx_rc = 0;
      std::string ctx_err;
      std::thread ctx_thread([&] { ctx_rc = strl_ctx_create(device_of(0), &ctx); if (ctx_rc) ctx_err = strl_last_error(); });
      g_bg_init = &ctx_thread;
      auto get_ctx = [&](std::string &w) -> strl_ctx * { if (ctx_thread.joinable()) ctx_thread.join(); if (ctx_rc) w = ctx_err; return ctx_rc ? nullptr : ctx; };
      if (regions.empty()) ok = whole_on_device(get_ctx, bam, V, why, status);
      else {
        strl_ctx *c = get_ctx(why);
        if (!c) { ok = false; status = STRL_ERR_NO_DEVICE; }
        else ok = regions_view(c, bam, regions, rd, V, why, status);
      }
      if (ctx_thread.joinable()) ctx_thread.join();
      g_bg_init = nullptr;
    }
  }
  if (ok && V.count_only) {
    const std::string line = std::to_string(V.info.written) + "\n";
    ok = V.out.put(line.data(), line.size(), why);
    if (!ok) status = STRL_ERR_IO;
  }
  if (ok && !V.out.close(why)) { ok = false; status = STRL_ERR_IO; }
  if (!ok) {
    V.out.drop();
    if (ctx) strl_ctx_destroy(ctx);
    quit("[strling] view: %s (status %d)", why.c_str(), status);
  }
  if (verbose) {
    const strl_view_info &I = V.info;
    fprintf(stderr,
            "{\"command\": \"view\", \"path\": \"%s\", \"regions\": %zu, \"records\": %llu, \"written\": %llu, \"dropped\": %llu, \"text_bytes\": %llu, \"chunks\": %llu, "
            "\"host_chunks\": %llu, \"size_ms\": %.3f, \"text_ms\": %.3f, \"seconds\": %.3f, \"read_s\": %.3f, \"view_s\": %.3f, \"write_s\": %.3f}\n",
            on_host ? "host" : "device", regions.size(), (unsigned long long)I.records, (unsigned long long)I.written, (unsigned long long)I.dropped, (unsigned long long)I.text_bytes,
            (unsigned long long)I.chunks, (unsigned long long)I.host_chunks, I.size_ms, I.text_ms, since(t_all), V.read_s, V.view_s, V.write_s);
  }
  return end_process(ctx);
}
