// context.hip -- what every translation unit of the library stands on: the error string, the device allocator behind DevBuf,
// the life cycle of a context (streams, events, tables, options, the genome STR table, timing), the rotation of its buffer
// sets, and page-locked host memory.
#include <stdarg.h>
#include <string.h>
#include <sys/mman.h>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <mutex>
#include <thread>
#include <vector>
#include "common.h"
#include "front.h"
#include "score.h"
#include "score_tables.h"

namespace strl {

static thread_local char g_err[512] = "";
void set_error(const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof g_err, fmt, ap);
  va_end(ap);
}

// Device memory: every buffer of the library comes from here.  A failed allocation is STRL_ERR_NOMEM with the sizes in the
// message, not a bare HIP error; STRL_DEVICE_MEM_LIMIT_MB (tests) makes the library refuse to go past that much.
static std::atomic<uint64_t> g_dev_bytes{0};
static int dev_alloc(void **p, size_t want) {
  static const uint64_t cap = getenv("STRL_DEVICE_MEM_LIMIT_MB") ? strtoull(getenv("STRL_DEVICE_MEM_LIMIT_MB"), nullptr, 10) << 20 : 0;
  hipError_t e = hipSuccess;
  if (cap && g_dev_bytes.load() + want > cap) e = hipErrorOutOfMemory;
  else {
    static const bool timing = getenv("STRL_ALLOC_TIMING") != nullptr;      // (diagnosis: where the start of a whole-genome run goes)
    const auto t0 = std::chrono::steady_clock::now();
    e = hipMalloc(p, want);
    if (timing && want >= ((size_t)64 << 20))
      fprintf(stderr, "[strling] hipMalloc %.2f GB: %.3f s\n", (double)want / 1e9, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
  }
  if (e == hipSuccess) { g_dev_bytes += want; return STRL_OK; }
  (void)hipGetLastError();
  size_t fr = 0, tot = 0;
  (void)hipMemGetInfo(&fr, &tot);
  set_error("out of device memory: %.2f GB more wanted, %.2f GB held by this process, %.2f of %.1f GB free on the device (%s)", (double)want / 1e9, (double)g_dev_bytes.load() / 1e9,
            (double)fr / 1e9, (double)tot / 1e9, e == hipErrorOutOfMemory ? "the input's per-read state does not fit" : hipGetErrorString(e));
  return e == hipErrorOutOfMemory ? STRL_ERR_NOMEM : STRL_ERR_HIP;
}
static void dev_free(void *p, size_t cap) {
  if (!p) return;
  (void)hipFree(p);
  g_dev_bytes -= cap;
}

int DevBuf::reserve(size_t bytes) {
  if (bytes <= cap && p) return STRL_OK;
  dev_free(p, cap);
  p = nullptr;
  cap = 0;
  size_t want = bytes + bytes / 8 + 256;
  const int rc = dev_alloc(&p, want);
  if (rc) { p = nullptr; return rc; }
  cap = want;
  return STRL_OK;
}
int DevBuf::grow(size_t bytes, size_t keep_bytes, hipStream_t st) {
  if (bytes <= cap && p) return STRL_OK;
  void *np = nullptr;
  size_t want = std::max(bytes + bytes / 8 + 256, cap * 2);
  int rc = dev_alloc(&np, want);
  if (rc == STRL_ERR_NOMEM && want > bytes + 256) { want = bytes + 256; rc = dev_alloc(&np, want); }     // (no room to double: exactly what is asked for)
  if (rc) return rc;
  if (p && keep_bytes) {
    STRL_HIP(hipMemcpyAsync(np, p, std::min(keep_bytes, cap), hipMemcpyDeviceToDevice, st));
    STRL_HIP(hipStreamSynchronize(st));
  } else if (p) {
    STRL_HIP(hipStreamSynchronize(st));
  }
  dev_free(p, cap);
  p = np;
  cap = want;
  return STRL_OK;
}
void DevBuf::release() {
  dev_free(p, cap);
  p = nullptr;
  cap = 0;
}

}  // namespace strl

using namespace strl;

int side_join(strl_ctx *c) {
  if (c->side_pending) {
    STRL_HIP(hipStreamWaitEvent(c->stream, c->ev_side_done, 0));
    c->side_pending = false;
  }
  for (auto &a : c->alt)
    if (a.side_pending) {
      STRL_HIP(hipStreamWaitEvent(c->stream, a.ev_side_done, 0));
      a.side_pending = false;
    }
  return STRL_OK;
}

int side_streams(strl_ctx *c) {
  if (c->stream2) return STRL_OK;
  STRL_HIP(hipSetDevice(c->device));
  STRL_HIP(hipStreamCreateWithFlags(&c->stream2, hipStreamNonBlocking));
  for (auto &a : c->alt) if (!a.stream2) STRL_HIP(hipStreamCreateWithFlags(&a.stream2, hipStreamNonBlocking));
  return STRL_OK;
}

// current -> alt[0] -> alt[1] -> ... -> current: the least recently used set (the last alternative) becomes current, the set
// that was current becomes alt[0].  N_SETS rotations restore the arrangement.
void rotate_tail(strl_ctx *c) {
  for (auto &a : c->alt) std::swap(static_cast<TailSet &>(*c), a);
  c->cl_where = (c->cl_where + 1) % N_SETS;
}
void rotate_head(strl_ctx *c) {
  for (auto &h : c->head_alt) std::swap(static_cast<HeadSet &>(*c), h);
  c->set = (c->set + 1) % N_SETS;
}

extern "C" {

int strl_version(void) { return 100; }
const char *strl_last_error(void) { return strl::g_err; }

int strl_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int strl_ctx_mem_info(strl_ctx *c, uint64_t *free_bytes, uint64_t *total_bytes) {
  if (!c) { set_error("null context"); return STRL_ERR_ARG; }
  STRL_HIP(hipSetDevice(c->device));
  size_t f = 0, t = 0;
  STRL_HIP(hipMemGetInfo(&f, &t));
  if (free_bytes) *free_bytes = f;
  if (total_bytes) *total_bytes = t;
  return STRL_OK;
}

int strl_ctx_create(int device_ordinal, strl_ctx **out) {
  if (!out) { set_error("ctx out pointer is NULL"); return STRL_ERR_ARG; }
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n == 0) {
    set_error("no HIP device available: strling_amd has no CPU fallback");
    return STRL_ERR_NO_DEVICE;
  }
  if (device_ordinal < 0 || device_ordinal >= n) { set_error("device ordinal %d out of range (%d devices)", device_ordinal, n); return STRL_ERR_ARG; }
  static const bool lap_on = getenv("STRL_CTX_TIMING") != nullptr;
  const auto lap0 = std::chrono::steady_clock::now();
  auto lap = [&](const char *what) { if (lap_on) fprintf(stderr, "[strl_ctx_create] %s at %.4f s\n", what, std::chrono::duration<double>(std::chrono::steady_clock::now() - lap0).count()); };
  lap("device count known (the runtime is up)");
  STRL_HIP(hipSetDevice(device_ordinal));
  strl_ctx *c = new strl_ctx();
  c->device = device_ordinal;
  lap("hipSetDevice");
  STRL_HIP(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
  lap("first stream");
  // (the side streams -- one per tail set, for the overlapped batches of strl_extract_device / an asynchronous clustering -- are
  // made when that mode is first asked for, side_streams(): a stream is ~9.5 ms here, and `strling extract / call / merge`,
  // which never overlap batches that way, waited for three of them at every start)
  for (auto &a : c->alt) STRL_HIP(hipEventCreateWithFlags(&a.ev_side_done, hipEventDisableTiming));
  STRL_HIP(hipEventCreateWithFlags(&c->ev_main_done, hipEventDisableTiming));
  STRL_HIP(hipEventCreateWithFlags(&c->ev_side_done, hipEventDisableTiming));
  STRL_HIP(hipEventCreateWithFlags(&c->ev_head_done, hipEventDisableTiming));
  for (auto &e : c->ev_set_free) STRL_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  for (auto &e : c->ev) STRL_HIP(hipEventCreate(&e));
  for (auto &e : c->pev) STRL_HIP(hipEventCreate(&e));
  lap("streams and events");
  std::vector<uint16_t> lut;
  build_lut(lut);
  std::vector<uint32_t> clut, ta;
  build_conv_lut(clut);
  build_stage_a_tables(lut, ta);
  lap("scorer tables built on the host");
  int rc = c->lut.reserve(lut.size() * 2 + clut.size() * 4 + ta.size() * 4);
  if (rc) return rc;
  lap("first hipMalloc");
  {   // (one copy for the three tables: each synchronous copy out of pageable memory is ~3 ms at a process' start)
    std::vector<uint8_t> all(lut.size() * 2 + clut.size() * 4 + ta.size() * 4);
    memcpy(all.data(), lut.data(), lut.size() * 2);
    memcpy(all.data() + lut.size() * 2, clut.data(), clut.size() * 4);
    memcpy(all.data() + lut.size() * 2 + clut.size() * 4, ta.data(), ta.size() * 4);
    STRL_HIP(hipMemcpy(c->lut.p, all.data(), all.size(), hipMemcpyHostToDevice));
  }
  rc = c->counters.reserve(CNT_WORDS * 4);
  if (rc) return rc;
  lap("tables on the device");
  *out = c;
  return STRL_OK;
}

void strl_ctx_destroy(strl_ctx *c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  if (c->stream2) (void)hipStreamSynchronize(c->stream2);
  for (auto &a : c->alt) if (a.stream2) (void)hipStreamSynchronize(a.stream2);
  (void)hipStreamSynchronize(c->stream);
  if (c->comm) { strl::comm_destroy(c->comm); c->comm = nullptr; }
  if (c->x_soft_seen_ev) (void)hipEventDestroy(c->x_soft_seen_ev);
  if (c->x_soft_seen) (void)hipHostFree(c->x_soft_seen);
  if (c->bai) { strl::bai_destroy(c->bai); c->bai = nullptr; }
  if (c->sweep) { strl::sweep_destroy(c->sweep); c->sweep = nullptr; }
  if (c->view) { strl::view_destroy(c->view); c->view = nullptr; }
  if (c->view_rec) { strl::view_destroy(c->view_rec); c->view_rec = nullptr; }
  if (c->bsort) { strl::bsort_destroy(c->bsort); c->bsort = nullptr; }
  if (c->front) { if (c->front->st_c) (void)hipStreamSynchronize(c->front->st_c); for (hipStream_t q : c->front->st_i) if (q) (void)hipStreamSynchronize(q); if (c->front->st_a) (void)hipStreamSynchronize(c->front->st_a); strl::front_destroy(c->front); c->front = nullptr; }
  for (auto &r : c->rg)
    if (r.st) { (void)hipStreamSynchronize(r.st); (void)hipStreamDestroy(r.st); }
  for (auto &e : c->ev) if (e) (void)hipEventDestroy(e);
  for (auto &e : c->pev) if (e) (void)hipEventDestroy(e);
  for (auto &e : c->ring) if (e) (void)hipEventDestroy(e);
  if (c->ev_main_done) (void)hipEventDestroy(c->ev_main_done);
  if (c->ev_side_done) (void)hipEventDestroy(c->ev_side_done);
  if (c->ev_head_done) (void)hipEventDestroy(c->ev_head_done);
  for (auto &e : c->ev_set_free) if (e) (void)hipEventDestroy(e);
  if (c->stream2) (void)hipStreamDestroy(c->stream2);
  for (auto &a : c->alt) {
    if (a.stream2) (void)hipStreamDestroy(a.stream2);
    if (a.ev_side_done) (void)hipEventDestroy(a.ev_side_done);
  }
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;      // (frees every device buffer of the context: DevBuf owns its memory)
}

void *strl_ctx_stream(strl_ctx *c) { return c ? (void *)c->stream : nullptr; }
int strl_ctx_sync(strl_ctx *c) {
  if (!c) return STRL_ERR_ARG;
  STRL_HIP(hipSetDevice(c->device));
  { const int rc = side_join(c); if (rc) return rc; }
  STRL_HIP(hipStreamSynchronize(c->stream));
  return STRL_OK;
}
int strl_ctx_enable_timing(strl_ctx *c, int on) {
  if (!c) return STRL_ERR_ARG;
  STRL_HIP(hipSetDevice(c->device));
  c->timing = on != 0;
  c->ring_pos = 0;
  if (c->timing && c->ring.empty()) {
    c->ring.resize(RING * EV_PER);
    for (auto &e : c->ring) STRL_HIP(hipEventCreate(&e));
  }
  return STRL_OK;
}
int strl_ctx_kernel_times_detail(strl_ctx *c, double ms_sum[8], uint64_t *n_launches) {
  if (!c || !ms_sum) return STRL_ERR_ARG;
  STRL_HIP(hipSetDevice(c->device));
  STRL_HIP(hipStreamSynchronize(c->stream));
  for (int k = 0; k < EV_PER - 1; ++k) ms_sum[k] = 0.0;
  const uint64_t n = std::min<uint64_t>(c->ring_pos, RING);
  for (uint64_t q = 0; q < n; ++q) {
    hipEvent_t *e = &c->ring[q * EV_PER];
    for (int k = 0; k < EV_PER - 1; ++k) {
      float ms = 0.f;
      STRL_HIP(hipEventElapsedTime(&ms, e[k], e[k + 1]));
      ms_sum[k] += ms;
    }
  }
  if (n_launches) *n_launches = n;
  return STRL_OK;
}

int strl_ctx_kernel_times(strl_ctx *c, double ms_sum[3], uint64_t *n_launches) {
  if (!c || !ms_sum) return STRL_ERR_ARG;
  double d[EV_PER - 1];
  const int rc = strl_ctx_kernel_times_detail(c, d, n_launches);
  if (rc) return rc;
  ms_sum[0] = d[0];
  ms_sum[1] = d[1] + d[2] + d[3];
  ms_sum[2] = d[4] + d[5] + d[6] + d[7];
  return STRL_OK;
}

int strl_ctx_set_opts(strl_ctx *c, const strl_opts *o) {
  if (!c || !o) { set_error("null argument"); return STRL_ERR_ARG; }
  STRL_HIP(hipSetDevice(c->device));
  c->opts = *o;
  std::vector<uint64_t> thr;
  build_thr(*o, thr);
  int rc = c->thr.reserve(thr.size() * 8);
  if (rc) return rc;
  STRL_HIP(hipMemcpyAsync(c->thr.p, thr.data(), thr.size() * 8, hipMemcpyHostToDevice, c->stream));
  STRL_HIP(hipStreamSynchronize(c->stream));
  c->have_opts = true;
  return STRL_OK;
}

int strl_ctx_set_genome(strl_ctx *c, const strl_genome_str *g) {
  if (!c) return STRL_ERR_ARG;
  STRL_HIP(hipSetDevice(c->device));
  STRL_HIP(hipStreamSynchronize(c->stream));     // a skip-predicate pass still in flight reads the tables replaced below
  if (!g || g->n_tid <= 0) {
    // empty table: no chromosome is a key, nothing is skipped.  The kernels still dereference entry 0 of each array for
    // lanes without a candidate read, so the arrays must exist.
    const TidInfo t0{};
    const int2 iv0 = make_int2(INT32_MAX, INT32_MIN);
    const uint2 b0 = make_uint2(0, 0);
    int rc0;
    if ((rc0 = c->g_tid.reserve(sizeof t0)) || (rc0 = c->g_bins.reserve(sizeof b0)) || (rc0 = c->g_start.reserve(sizeof iv0))) return rc0;
    STRL_HIP(hipMemcpy(c->g_tid.p, &t0, sizeof t0, hipMemcpyHostToDevice));
    STRL_HIP(hipMemcpy(c->g_bins.p, &b0, sizeof b0, hipMemcpyHostToDevice));
    STRL_HIP(hipMemcpy(c->g_start.p, &iv0, sizeof iv0, hipMemcpyHostToDevice));
    c->n_tid = 0; c->n_iv = 0;
    return STRL_OK;
  }
  const int32_t nt = g->n_tid;
  const int64_t niv = g->iv_off[nt];
  std::vector<int32_t> st((size_t)std::max<int64_t>(niv, 1));
  // per tid, n_iv + 1 elements sorted by start: element i = {start_i, max(stop_0..stop_{i-1})}; the last one is the
  // sentinel {INT32_MAX, max of all stops}.  One 8-byte load answers "does a start lie here" AND "does an earlier
  // interval reach past my start".
  std::vector<int2> ivs;
  ivs.reserve((size_t)niv + (size_t)nt);
  std::vector<TidInfo> ti((size_t)nt);
  std::vector<uint2> bins;   // bins[k] = {#starts < k << BIN_SHIFT, #starts < (k+1) << BIN_SHIFT}
  std::vector<int64_t> idx;
  for (int32_t t = 0; t < nt; ++t) {
    const int64_t a = g->iv_off[t], b = g->iv_off[t + 1];
    if (b - a > 0x7ffffff0ll) { set_error("too many intervals on tid %d", t); return STRL_ERR_ARG; }
    idx.resize((size_t)(b - a));
    for (int64_t i = a; i < b; ++i) idx[(size_t)(i - a)] = i;
    std::stable_sort(idx.begin(), idx.end(), [&](int64_t x, int64_t y) { return g->iv_start[x] < g->iv_start[y]; });
    TidInfo &x = ti[(size_t)t];
    x.iv_off = (int64_t)ivs.size();
    int32_t run = INT32_MIN;
    for (int64_t i = a; i < b; ++i) {
      const int64_t s = idx[(size_t)(i - a)];
      st[(size_t)i] = g->iv_start[s];
      ivs.push_back(make_int2(g->iv_start[s], run));
      run = std::max(run, g->iv_stop[s]);
    }
    ivs.push_back(make_int2(INT32_MAX, run));
    x.n_iv = (int32_t)(b - a);
    x.has = g->has_chrom[t] ? 1 : 0;
    x.pad = 0;
    x.bin_off = (int64_t)bins.size();
    const int32_t max_start = b > a ? std::max(0, st[(size_t)(b - 1)]) : 0;
    x.n_bins = b > a ? (max_start >> BIN_SHIFT) + 1 : 0;
    int64_t j = a;
    uint32_t prev = 0;
    for (int32_t k = 0; k <= x.n_bins; ++k) {
      const int64_t lim = (int64_t)k << BIN_SHIFT;
      while (j < b && (int64_t)st[(size_t)j] < lim) ++j;
      const uint32_t cntk = (uint32_t)(j - a);
      if (k > 0) bins.push_back(make_uint2(prev, cntk));
      prev = cntk;
    }
  }
  if (bins.empty()) bins.push_back(make_uint2(0, 0));
  int rc;
  if ((rc = c->g_tid.reserve(ti.size() * sizeof(TidInfo)))) return rc;
  if ((rc = c->g_bins.reserve(bins.size() * 8))) return rc;
  if ((rc = c->g_start.reserve(ivs.size() * 8))) return rc;
  STRL_HIP(hipMemcpy(c->g_tid.p, ti.data(), ti.size() * sizeof(TidInfo), hipMemcpyHostToDevice));
  STRL_HIP(hipMemcpy(c->g_bins.p, bins.data(), bins.size() * 8, hipMemcpyHostToDevice));
  STRL_HIP(hipMemcpy(c->g_start.p, ivs.data(), ivs.size() * 8, hipMemcpyHostToDevice));
  c->n_tid = nt;
  c->n_iv = (uint64_t)niv;
  return STRL_OK;
}

int strl_ctx_blocking_waits(strl_ctx *c, int on) {
  if (!c) { set_error("null argument"); return STRL_ERR_ARG; }
  c->blocking_waits = on != 0;
  return STRL_OK;
}

// waits for (and frees) an event an asynchronous entry point handed out (strl_front_fragwords_async)
int strl_event_wait(void *event) {
  if (!event) return STRL_OK;
  hipEvent_t ev = static_cast<hipEvent_t>(event);
  STRL_HIP(hipEventSynchronize(ev));
  (void)hipEventDestroy(ev);
  return STRL_OK;
}

// Page-locked host memory.  hipHostMalloc takes 0.25 s per GB here (4 KB pages faulted and pinned one by one: 0.36 s for the four
// chunk buffers of `strling extract`, longer than creating the device context beside it).  An anonymous mapping advised to use
// 2 MB pages, touched by a few threads and then registered takes 0.012 s for the same 1.3 GB, and copies from it run at 57 GB/s
// instead of 36 - 50 (tools/ubench/pin_probe.hip, profiles/r04/pin_probe.txt).  hipHostMalloc is the fallback.
namespace {
struct PinnedMap { void *base; size_t len; };
std::mutex g_pinned_mu;
std::vector<std::pair<void *, PinnedMap>> g_pinned;      // registered mappings by the pointer handed out
}  // namespace
void *strl_pinned_alloc(uint64_t bytes) {
  const size_t huge = (size_t)2 << 20;
  if (bytes >= huge && !getenv("STRL_PINNED_PLAIN")) {
    const size_t len = (((size_t)bytes + huge - 1) & ~(huge - 1)) + huge;
    void *base = mmap(nullptr, len, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
    if (base != MAP_FAILED) {
      char *a = reinterpret_cast<char *>((reinterpret_cast<uintptr_t>(base) + huge - 1) & ~(uintptr_t)(huge - 1));
      const size_t span = len - huge;
      (void)madvise(a, span, MADV_HUGEPAGE);
      const size_t T = std::min<size_t>(8, std::max<size_t>(1, span >> 26));      // a thread per 64 MB, up to 8
      std::vector<std::thread> th;
      for (size_t k = 0; k < T; ++k)
        th.emplace_back([=] { for (size_t o = span / T * k, e = k + 1 == T ? span : span / T * (k + 1); o < e; o += 4096) a[o] = 0; });
      for (auto &x : th) x.join();
      if (hipHostRegister(a, span, hipHostRegisterPortable) == hipSuccess) {      // (portable: contexts on every device of the process copy from it)
        std::lock_guard<std::mutex> lk(g_pinned_mu);
        g_pinned.push_back({a, PinnedMap{base, len}});
        return a;
      }
      (void)hipGetLastError();
      (void)munmap(base, len);
    }
  }
  void *p = nullptr;
  if (hipHostMalloc(&p, (size_t)bytes, hipHostMallocDefault) != hipSuccess) return nullptr;
  return p;
}
void strl_pinned_free(void *p) {
  if (!p) return;
  PinnedMap m{nullptr, 0};
  {
    std::lock_guard<std::mutex> lk(g_pinned_mu);
    for (size_t i = 0; i < g_pinned.size(); ++i)
      if (g_pinned[i].first == p) { m = g_pinned[i].second; g_pinned.erase(g_pinned.begin() + (long)i); break; }
  }
  if (m.base) { (void)hipHostUnregister(p); (void)munmap(m.base, m.len); }
  else (void)hipHostFree(p);
}

}  // extern "C"
