// cli_shared.h -- what the commands that live in files of their own (sort_cli.cpp) take from main.cpp: declarations, not copies.
#pragma once
#include <stdint.h>
#include <algorithm>
#include <functional>
#include <map>
#include <string>
#include <thread>
#include <vector>
#include "../../../include/strling_amd.h"
#include "chunk_feed.h"

// Nim `quit msg`: message on stderr, exit code 1 (waits for a device bring-up running on g_bg_init)
[[noreturn]] void quit(const char *fmt, ...);
extern std::thread *g_bg_init;   // device bring-up running beside the first host pass; quit() waits for it

struct Args {
  std::map<std::string, std::string> opt;
  std::vector<std::string> pos;
  bool flag(const char *k) const { return opt.count(k) != 0; }
  std::string get(const char *k, const char *dflt) const { auto it = opt.find(k); return it == opt.end() ? dflt : it->second; }
};
// long name -> (short name, takes value)
struct OptSpec { const char *longn; char shortn; bool value; };
Args parse(int argc, char **argv, int first, const std::vector<OptSpec> &specs, const char *usage);

void set_device0(const std::string &v);     // --device K (or STRL_DEVICE=K)
int device_of(int g);
int decode_threads();
bool file_exists(const std::string &p);
int end_process(strl_ctx *ctx);             // the end of a process whose outputs are closed
// one BGZF member of `len` <= 0xFF00 input bytes: zlib at its default level (what htslib writes, and `strling pull`)
bool bgzf_member_zlib(const uint8_t *src, size_t len, std::vector<uint8_t> &o);

// --csi [-m N]: min_shift of the CSI scheme, -1 without --csi; usage errors (-m without --csi, N outside [8, 24]) end the process
int csi_min_shift(const Args &a, const char *usage);
// the bytes of an index to `out` through a temporary name (a failed run leaves no half index); bgzf: in BGZF blocks with the EOF
// block, as samtools writes a .csi.  false: why
bool write_index_file(const std::string &out, const std::vector<uint8_t> &bytes, bool bgzf, std::string &why, strl::ThreadPool *pool = nullptr);

// N page-locked chunk buffers and their N block tables (chunk_feed.h), allocated on a thread per buffer: the time is the kernel's,
// faulting and locking the pages.  Nothing is freed unless release() is called: `call` and `bamindex` leave theirs to the end of
// the process on purpose.
struct PinnedRing {
  std::vector<uint8_t *> data, meta;
  void alloc(size_t n, size_t chunk_blocks, size_t chunk_bytes) {
    data.assign(n, nullptr); meta.assign(n, nullptr);
    auto one = [&](size_t k) {
      data[k] = static_cast<uint8_t *>(strl_pinned_alloc(strl::chunk_data_bytes(chunk_bytes)));
      meta[k] = static_cast<uint8_t *>(strl_pinned_alloc(strl::chunk_table_bytes(chunk_blocks)));
    };
    std::vector<std::thread> each;
    for (size_t k = 1; k < n; ++k) each.emplace_back(one, k);
    one(0);
    for (auto &t : each) t.join();
  }
  bool ok() const { return !data.empty() && !std::count(data.begin(), data.end(), nullptr) && !std::count(meta.begin(), meta.end(), nullptr); }
  void release_except(const void *a, const void *b) {      // (freeing twice is harmless: the pointers are nulled)
    for (auto *v : {&data, &meta})
      for (uint8_t *&q : *v) if (q && q != a && q != b) { strl_pinned_free(q); q = nullptr; }
  }
  void release() { release_except(nullptr, nullptr); }
};

// main.cpp: the index of the BAM at `bam` built on the device and written to `out` through a temporary name (`strling bamindex`;
// `sort --windowed --write-index` runs it over the file it has just written).  csi_min_shift >= 0: a CSI index.  false: why, status
bool build_bai(const std::function<strl_ctx *(std::string &)> &get_ctx, const std::string &bam, const std::string &out, bool verbose, bool last_use, std::string &why,
               int &status, int csi_min_shift);

// main.cpp: htslib's region forms as `strling pull` takes them (NAME, NAME:BEG, NAME:BEG-END, 1-based and inclusive) -> 0-based, half-open;
// what cannot be read ends the process with a message that names `cmd`
namespace strl { struct BamTarget; }
struct PullRegion { int32_t tid; int64_t beg, end; };
PullRegion parse_pull_region(const std::string &s, const std::vector<strl::BamTarget> &targets, const char *cmd = "pull");

int sort_main(int argc, char **argv);       // sort_cli.cpp
int fastq_main(int argc, char **argv);      // sort_cli.cpp: `strling fastq`, a mode of sort's driver
int view_main(int argc, char **argv);       // view_cli.cpp
