// extract.hip -- the extract step of a batch on the device behind the scorer (score.hip): strl_extract_device (scorer + pair
// logic of one batch, overlapped with the previous batch's tail), the same in chunks (strl_extract_begin / _add / _finish), the
// treads' way back to the host, and the gather of a multi-device extract on its first context.
#include <string.h>
#include <algorithm>
#include <vector>
#include "common.h"
#include "front.h"
#include "score.h"

using namespace strl;

extern "C" {      // (C linkage: the kernels keep the plain names the records under profiles/ have them by)
namespace strl {
__global__ void soft_append_kernel(const strl_soft_rec *src, const uint32_t *cnt, uint32_t src_cap, uint32_t read_base, strl_soft_rec *dst,
                                   uint32_t dst_cap, uint32_t *xc) {
  __shared__ uint32_t base_sh;
  uint32_t n = cnt[CNT_SOFT];
  if (n > src_cap) n = src_cap;                 // (cannot happen: the per-chunk queue holds two records per read)
  if (threadIdx.x == 0) {
    base_sh = atomicAdd(&xc[XC_SOFT], n);   // one block: this is the only writer of the counter
    xc[XC_SKIP] += cnt[CNT_SKIP]; xc[XC_QUEUE] += cnt[CNT_QUEUE]; xc[XC_SBW] += cnt[CNT_SBW]; xc[XC_SBS] += cnt[CNT_SBS];
    xc[XC_SOFT_ITEMS] += cnt[CNT_SOFT];
  }
  __syncthreads();
  const uint32_t base = base_sh;
  for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
    strl_soft_rec s = src[i];
    s.read_side += read_base << 1;
    if (base + i < dst_cap) dst[base + i] = s;
  }
  if (threadIdx.x == 0 && (cnt[CNT_SOFT] > src_cap || (uint64_t)base + n > dst_cap)) xc[XC_OVERFLOW] = 1;   // reported by strl_treads_fetch
}

// multi-GPU extract, gather of the contexts' per-read state on one of them: soft-clip records carry the index of their read
// in the context that scored them -> its index in the file.  lbase / gbase: first local / global record of that context's chunks.
__global__ void soft_rebase_kernel(strl_soft_rec *soft, uint32_t n, const uint32_t *lbase, const uint32_t *gbase, uint32_t n_chunks) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t rs = soft[i].read_side, r = rs >> 1;
  uint32_t lo = 0, hi = n_chunks;              // last chunk with lbase <= r
  while (hi - lo > 1) { const uint32_t mid = (lo + hi) / 2; if (lbase[mid] <= r) lo = mid; else hi = mid; }
  soft[i].read_side = ((gbase[lo] + (r - lbase[lo])) << 1) | (rs & 1u);
}
__global__ void qref_rebase_kernel(uint64_t *qref, uint32_t n, uint64_t arena_base) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) qref[i] += arena_base << 8;
}
__global__ void words_or_kernel(uint32_t *dst, const uint32_t *src, size_t n_words) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_words; i += (size_t)gridDim.x * blockDim.x) dst[i] |= src[i];
}
}  // namespace strl
}  // extern "C"

static int copy_between(void *dst, int dst_dev, const void *src, int src_dev, size_t bytes, hipStream_t st) {
  if (!bytes) return STRL_OK;
  if (dst_dev == src_dev) STRL_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, st));
  else STRL_HIP(hipMemcpyPeerAsync(dst, dst_dev, src, src_dev, bytes, st));
  return STRL_OK;
}

// ---- the chunked form of strl_extract_device (further down): a BAM being decoded hands over batches in file order, the pair logic runs once at the end ----
// n_now: reads the big per-read columns are sized for right away (0: the hint); the front end passes a fraction and has the
// rest allocated beside its first chunks (FrontBigAlloc)
int extract_begin_sized(strl_ctx *c, uint64_t n_reads_hint, uint64_t n_now) {
  if (!c) { set_error("null argument"); return STRL_ERR_ARG; }
  if (!c->have_opts) { set_error("strl_ctx_set_opts must be called before scoring"); return STRL_ERR_ARG; }
  STRL_HIP(hipSetDevice(c->device));
  int rc;
  const uint64_t hint = std::max<uint64_t>(n_reads_hint, 1 << 20), first = n_now ? std::min(n_now, hint) : hint;
  if ((rc = c->x_rows.grow((size_t)first * sizeof(strl_pair_rec), 0, c->stream)) || (rc = c->x_qhash.grow((size_t)first * 8, 0, c->stream)) ||
      (rc = c->x_whole.grow((size_t)first * 4, 0, c->stream)) || (rc = c->x_soft.grow((size_t)(hint / 8 + 65536) * sizeof(strl_soft_rec), 0, c->stream)) ||
      (rc = c->x_cnt.reserve(XC_WORDS * 4)))
    return rc;
  STRL_HIP(hipMemsetAsync(c->x_cnt.p, 0, XC_WORDS * 4, c->stream));
  if ((rc = bloom_reset(c, std::max<uint64_t>(hint, 1ull << 28)))) return rc;   // 16 MB: sized for a whole genome of reads
  c->x_n = 0; c->x_soft_cap = c->x_soft.cap / sizeof(strl_soft_rec); c->x_open = true; c->x_front = false;
  c->x_soft_known = 0; c->x_soft_known_at = 0;
  if (c->x_soft_pending) { STRL_HIP(hipEventSynchronize(c->x_soft_seen_ev)); c->x_soft_pending = false; }
  return STRL_OK;
}

// the per-chunk part shared by strl_extract_add and the device front end: score the device-resident chunk `d` whose rows and
// qname hashes already sit at x_rows / x_qhash [at, at + n), append its soft-clip records
int extract_add_scored(strl_ctx *c, const strl_read_soa *d, uint64_t at) {
  const uint64_t n = d->n;
  int rc;
  // Soft-clip records: a chunk can add two per read (its hard bound, which the per-chunk queue is sized for), the typical
  // rate is a few per cent.  The running total lives on the device; the host keeps an upper bound of it -- the last total it
  // has seen (read back asynchronously behind every chunk) plus two per read added since -- and grows x_soft ahead of that.
  if (c->x_soft_seen_ev) {
    while (c->x_soft_pending && hipEventQuery(c->x_soft_seen_ev) == hipSuccess) {
      c->x_soft_known = *c->x_soft_seen;
      c->x_soft_known_at = c->x_soft_seen_at;
      c->x_soft_pending = false;
    }
  }
  const uint64_t bound = c->x_soft_known + 2 * ((at + n) - c->x_soft_known_at) + 2;
  if (bound > c->x_soft_cap) {
    c->x_soft_cap = std::max<uint64_t>(bound, (at + n) / 4 + 65536);
    if ((rc = c->x_soft.grow((size_t)c->x_soft_cap * sizeof(strl_soft_rec), c->x_soft.cap, c->stream))) return rc;
  }
  const strl_pair_soa dp{c->x_rows.as<strl_pair_rec>() + at, c->x_qhash.as<uint64_t>() + at};
  const uint64_t chunk_soft = 2 * n + 2;
  if ((rc = c->st_soft.reserve((size_t)chunk_soft * sizeof(strl_soft_rec)))) return rc;
  // the skip-predicate pass stores its words 16 bytes at a time when the destination is aligned (its other variant is ~80x
  // slower): a chunk that starts at an index that is not a multiple of 4 is scored into a scratch array and copied over
  uint32_t *whole = c->x_whole.as<uint32_t>() + at;
  const bool bounce = (at & 3u) != 0;
  if (bounce) {
    if ((rc = c->st_whole.reserve((size_t)std::max<uint64_t>(n, 1) * 4))) return rc;
    whole = c->st_whole.as<uint32_t>();
  }
  if ((rc = score_device(c, d, whole, c->st_soft.as<strl_soft_rec>(), chunk_soft, nullptr, nullptr, false, &dp, false))) return rc;
  if (bounce && n) STRL_HIP(hipMemcpyAsync(c->x_whole.as<uint32_t>() + at, whole, (size_t)n * 4, hipMemcpyDeviceToDevice, c->stream));
  hipLaunchKernelGGL(strl::soft_append_kernel, dim3(1), dim3(1024), 0, c->stream, c->st_soft.as<strl_soft_rec>(), c->counters.as<uint32_t>(), (uint32_t)chunk_soft,
                     (uint32_t)at, c->x_soft.as<strl_soft_rec>(), (uint32_t)std::min<uint64_t>(c->x_soft_cap, 0xffffffffull), c->x_cnt.as<uint32_t>());
  STRL_HIP(hipGetLastError());
  if (!c->x_soft_seen_ev) {
    STRL_HIP(hipEventCreateWithFlags(&c->x_soft_seen_ev, hipEventDisableTiming));
    STRL_HIP(hipHostMalloc(reinterpret_cast<void **>(&c->x_soft_seen), 64, hipHostMallocDefault));
  }
  if (!c->x_soft_pending) {
    STRL_HIP(hipMemcpyAsync(c->x_soft_seen, c->x_cnt.as<uint32_t>() + XC_SOFT, 4, hipMemcpyDeviceToHost, c->stream));
    STRL_HIP(hipEventRecord(c->x_soft_seen_ev, c->stream));
    c->x_soft_seen_at = at + n;
    c->x_soft_pending = true;
  }
  c->x_n = at + n;
  return STRL_OK;
}

extern "C" {

int strl_extract_device(strl_ctx *c, const strl_read_soa *s, const strl_pair_soa *pp, int64_t n_tail, uint64_t item_cap, uint64_t tread_cap) {
  if (!c || !s || !pp) { set_error("null argument"); return STRL_ERR_ARG; }
  if (!c->have_opts) { set_error("strl_ctx_set_opts must be called before scoring"); return STRL_ERR_ARG; }
  if (s->n && (!pp->rec || !pp->qhash)) { set_error("strl_extract_device: incomplete strl_pair_soa"); return STRL_ERR_ARG; }
  STRL_HIP(hipSetDevice(c->device));
  const uint64_t n = s->n;
  if (n_tail < 0 || (uint64_t)n_tail > n) { set_error("strl_extract_device: n_tail must be in [0, n]"); return STRL_ERR_ARG; }
  if (!item_cap) item_cap = n / 8 + 65536;
  if (!tread_cap) tread_cap = n / 16 + 65536;
  item_cap = std::min<uint64_t>(item_cap, 3 * n + 16);    // every read and both of its clipped ends
  tread_cap = std::min<uint64_t>(tread_cap, 8 * n + 16);
  strl_read_soa d = *s;
  strl_pair_soa dp = *pp;
  int rc;
  if (s->mem != STRL_MEM_DEVICE && (rc = stage_batch(c, s, pp, &d, &dp))) return rc;
  const uint64_t soft_cap = std::min<uint64_t>(item_cap, 2 * n + 2);
  // Device-resident input: classify + scorer of this batch on the main stream, its pair logic on the side stream -- where
  // the previous batch's pair logic and clustering may still be running while this call's scorer already executes.
  static const bool no_overlap = getenv("STRL_NO_OVERLAP") != nullptr;
  const bool overlap = s->mem == STRL_MEM_DEVICE && !c->timing && !no_overlap;
  if (overlap) {
    if ((rc = side_streams(c))) return rc;
    rotate_head(c);                 // the scorer's output of this batch: the least recently used set
    rotate_tail(c);                 // this batch's pair logic and clustering: likewise, on that set's own side stream
    if ((rc = c->counters.reserve(CNT_WORDS * 4))) return rc;
    if (c->set_used[c->set]) STRL_HIP(hipStreamWaitEvent(c->stream, c->ev_set_free[c->set], 0));   // the side stream is done with this set
  }
  if ((rc = c->st_whole.reserve((size_t)std::max<uint64_t>(n, 1) * 4))) return rc;
  if ((rc = c->st_soft.reserve((size_t)std::max<uint64_t>(soft_cap, 1) * sizeof(strl_soft_rec)))) return rc;
  c->ex_n = n; c->ex_soft_cap = soft_cap; c->x_mode = false;
  if ((rc = score_device(c, &d, c->st_whole.as<uint32_t>(), c->st_soft.as<strl_soft_rec>(), soft_cap, nullptr, nullptr, false, &dp, true, overlap))) return rc;
  if (!overlap)
    return strl_pair_device(c, n, &dp, c->st_whole.as<uint32_t>(), c->st_soft.as<strl_soft_rec>(), c->counters.as<uint32_t>() + CNT_SOFT, soft_cap,
                            n_tail, item_cap, tread_cap);
  STRL_HIP(hipEventRecord(c->ev_head_done, c->stream));
  STRL_HIP(hipStreamWaitEvent(c->stream2, c->ev_head_done, 0));
  if ((rc = strl_pair_device(c, n, &dp, c->st_whole.as<uint32_t>(), c->st_soft.as<strl_soft_rec>(), c->counters.as<uint32_t>() + CNT_SOFT, soft_cap,
                             n_tail, item_cap, tread_cap, c->stream2)))
    return rc;
  STRL_HIP(hipEventRecord(c->ev_set_free[c->set], c->stream2));
  c->set_used[c->set] = true;
  STRL_HIP(hipEventRecord(c->ev_side_done, c->stream2));
  c->side_pending = true;
  c->pair_on_side = true;
  return STRL_OK;
}

int strl_extract_begin(strl_ctx *c, uint64_t n_reads_hint) { return extract_begin_sized(c, n_reads_hint, 0); }

int strl_extract_add(strl_ctx *c, const strl_read_soa *s, const strl_pair_soa *pp) {
  if (!c || !s || !pp) { set_error("null argument"); return STRL_ERR_ARG; }
  if (!c->x_open) { set_error("strl_extract_add without strl_extract_begin"); return STRL_ERR_ARG; }
  if (s->n && (!pp->rec || !pp->qhash)) { set_error("strl_extract_add: incomplete strl_pair_soa"); return STRL_ERR_ARG; }
  STRL_HIP(hipSetDevice(c->device));
  const uint64_t n = s->n, at = c->x_n;
  if (!n) return STRL_OK;
  if (at + n > strl_record_limit()) { set_error("chunked extract: more than %llu records in one device pass", (unsigned long long)strl_record_limit()); return STRL_ERR_LIMIT; }
  int rc;
  if ((rc = c->x_rows.grow((size_t)(at + n) * sizeof(strl_pair_rec), (size_t)at * sizeof(strl_pair_rec), c->stream)) ||
      (rc = c->x_qhash.grow((size_t)(at + n) * 8, (size_t)at * 8, c->stream)) || (rc = c->x_whole.grow((size_t)(at + n) * 4, (size_t)at * 4, c->stream)))
    return rc;
  strl_read_soa d = *s;
  const hipMemcpyKind kind = s->mem == STRL_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  if (s->mem != STRL_MEM_DEVICE && (rc = stage_batch(c, s, nullptr, &d, nullptr))) return rc;
  STRL_HIP(hipMemcpyAsync(c->x_rows.as<strl_pair_rec>() + at, pp->rec, (size_t)n * sizeof(strl_pair_rec), kind, c->stream));
  STRL_HIP(hipMemcpyAsync(c->x_qhash.as<uint64_t>() + at, pp->qhash, (size_t)n * 8, kind, c->stream));
  return extract_add_scored(c, &d, at);
}

int strl_extract_finish(strl_ctx *c, int64_t n_tail, uint64_t item_cap, uint64_t tread_cap) {
  if (!c) { set_error("null argument"); return STRL_ERR_ARG; }
  if (!c->x_open && !c->x_mode) { set_error("strl_extract_finish without strl_extract_begin"); return STRL_ERR_ARG; }   // (again after a capacity error: fine)
  STRL_HIP(hipSetDevice(c->device));
  const uint64_t n = c->x_n;
  if (n_tail < 0 || (uint64_t)n_tail > n) { set_error("strl_extract_finish: n_tail must be in [0, n]"); return STRL_ERR_ARG; }
  if (!item_cap) item_cap = n / 8 + 65536;
  if (!tread_cap) tread_cap = n / 16 + 65536;
  item_cap = std::min<uint64_t>(item_cap, 3 * n + 16);
  tread_cap = std::min<uint64_t>(tread_cap, 8 * n + 16);
  c->x_open = false; c->x_mode = true;
  c->ex_n = n; c->ex_soft_cap = c->x_soft_cap;
  const strl_pair_soa dp{c->x_rows.as<strl_pair_rec>(), c->x_qhash.as<uint64_t>()};
  return strl_pair_device(c, n, &dp, c->x_whole.as<uint32_t>(), c->x_soft.as<strl_soft_rec>(), c->x_cnt.as<uint32_t>() + XC_SOFT,
                          std::max<uint64_t>(c->x_soft_cap, 1), n_tail, item_cap, tread_cap);
}

int strl_treads_fetch(strl_ctx *c, strl_tread *out, uint64_t cap, uint64_t *n_out, strl_score_stats *stats) {
  if (!c) { set_error("null argument"); return STRL_ERR_ARG; }
  if (!c->n_treads_dev) { set_error("strl_treads_fetch: no strl_extract_device call on this context"); return STRL_ERR_ARG; }
  STRL_HIP(hipSetDevice(c->device));
  { const int rc0 = strl_pair_order(c); if (rc0) return rc0; }
  uint32_t raw[CNT_WORDS], pc[PC_WORDS], xc[XC_WORDS];
  STRL_HIP(hipMemcpyAsync(raw, c->counters.p, CNT_WORDS * 4, hipMemcpyDeviceToHost, c->stream));
  STRL_HIP(hipMemcpyAsync(pc, c->pair_cnt.p, PC_WORDS * 4, hipMemcpyDeviceToHost, c->stream));
  if (c->x_mode) STRL_HIP(hipMemcpyAsync(xc, c->x_cnt.p, XC_WORDS * 4, hipMemcpyDeviceToHost, c->stream));
  STRL_HIP(hipStreamSynchronize(c->stream));
  if (c->x_mode) {   // chunked extract: the sums over the chunks
    raw[CNT_SKIP] = xc[XC_SKIP]; raw[CNT_QUEUE] = xc[XC_QUEUE]; raw[CNT_SBW] = xc[XC_SBW]; raw[CNT_SBS] = xc[XC_SBS]; raw[CNT_SOFT] = xc[XC_SOFT];
  }
  if (stats) {
    memset(stats, 0, sizeof *stats);
    stats->n_reads = c->ex_n; stats->n_skipped = raw[CNT_SKIP]; stats->n_scored = raw[CNT_QUEUE]; stats->n_soft_items = raw[CNT_SOFT];
    stats->n_stage_b_whole = raw[CNT_SBW]; stats->n_stage_b_soft = raw[CNT_SBS];
  }
  if (n_out) *n_out = pc[PC_EMIT];
  if (c->x_mode && xc[XC_OVERFLOW]) { set_error("chunked extract: soft-clip records of a chunk were dropped (%u kept of %u)", xc[XC_SOFT], xc[XC_SOFT_ITEMS]); return STRL_ERR_CAPACITY; }
  if (raw[CNT_SOFT] > c->ex_soft_cap) { set_error("soft-clip queue overflow: %u items, capacity %llu (raise item_cap)", raw[CNT_SOFT], (unsigned long long)c->ex_soft_cap); return STRL_ERR_CAPACITY; }
  const uint32_t err = pc[PC_ERR];
  if (err & PAIR_ERR_ITEMS) { set_error("pair logic: %u join items, capacity %u (raise item_cap)", pc[PC_ITEMS], c->pair_item_cap); return STRL_ERR_CAPACITY; }
  if (err & PAIR_ERR_EMIT) { set_error("pair logic: %u treads, capacity %u (raise tread_cap)", pc[PC_EMIT], c->tread_cap); return STRL_ERR_CAPACITY; }
  if (err & PAIR_ERR_COLLISION) { set_error("pair logic: two different qnames share one 64-bit hash (use the host pair logic, strl_pair_reads: it keys on the string)"); return STRL_ERR_FORMAT; }
  if (err & (PAIR_ERR_RUN | PAIR_ERR_LOCAL)) { set_error("pair logic: more than %d join items share the low 32 bits of their qname hash (use the host pair logic, strl_pair_reads)", strl::PAIR_LONG_MAX_ITEMS); return STRL_ERR_FORMAT; }
  if (err & PAIR_ERR_ASSERT) { set_error("repeat_count >= 256 (doAssert extract.nim:72)"); return STRL_ERR_ASSERT; }
  const uint64_t n = pc[PC_EMIT];
  if (out) {
    if (n > cap) { set_error("tread capacity %llu too small, need %llu", (unsigned long long)cap, (unsigned long long)n); return STRL_ERR_CAPACITY; }
    if (n) STRL_HIP(hipMemcpy(out, c->treads.p, (size_t)n * sizeof(strl_tread), hipMemcpyDeviceToHost));
  }
  return STRL_OK;
}

int strl_ctx_pair_times(strl_ctx *c, double ms[5]) {
  if (!c || !ms) return STRL_ERR_ARG;
  STRL_HIP(hipSetDevice(c->device));
  STRL_HIP(hipStreamSynchronize(c->stream));
  for (int k = 0; k < 5; ++k) {
    float f = 0.f;
    if (c->timing) (void)hipEventElapsedTime(&f, c->pev[k], c->pev[k + 1]);
    ms[k] = f;
  }
  return STRL_OK;
}

// `strling extract --gpus N`: the chunks of one file went round-robin over n contexts (strl_front_push_after), each scored
// its chunks.  The pair logic needs every record of a qname group in one place, and what it needs of a record is small
// (32-byte row, hash, scorer word, name reference: 52 B against the ~290 B of the record and the work of inflating and
// scoring it): everything is gathered on ctxs[0] in FILE order -- per chunk copies over xGMI (peer DMA) --, soft-clip
// records and name references are re-based, the Bloom bitmaps OR-ed; ctxs[0] then is in the state of a one-GPU chunked
// extract of the whole file (strl_extract_finish, strl_front_fragwords, strl_front_qnames work as usual).
// chunk_owner[k] / chunk_records[k]: context and record count (strl_front_chunk.n_records) of the file's k-th chunk.
int strl_ctxs_extract_gather(strl_ctx **ctxs, int n, const uint32_t *chunk_owner, const uint64_t *chunk_records, uint64_t n_chunks) {
  using namespace strl;
  if (!ctxs || n < 1 || (n_chunks && (!chunk_owner || !chunk_records))) { set_error("strl_ctxs_extract_gather: bad argument"); return STRL_ERR_ARG; }
  for (int g = 0; g < n; ++g) {
    if (!ctxs[g] || !ctxs[g]->front || !ctxs[g]->x_open) { set_error("strl_ctxs_extract_gather: context %d has no open front end", g); return STRL_ERR_ARG; }
    if (ctxs[g]->bloom_mask != ctxs[0]->bloom_mask) { set_error("strl_ctxs_extract_gather: Bloom bitmaps differ in size"); return STRL_ERR_ARG; }
    STRL_HIP(hipSetDevice(ctxs[g]->device));
    STRL_HIP(hipStreamSynchronize(ctxs[g]->stream));
  }
  if (n == 1) return STRL_OK;
  strl_ctx *c0 = ctxs[0];
  strl_front *F0 = c0->front;
  std::vector<uint64_t> local_n((size_t)n, 0), gbase((size_t)n_chunks, 0), lbase((size_t)n_chunks, 0);
  uint64_t tot = 0;
  for (uint64_t k = 0; k < n_chunks; ++k) {
    if (chunk_owner[k] >= (uint32_t)n) { set_error("strl_ctxs_extract_gather: chunk owner out of range"); return STRL_ERR_ARG; }
    gbase[(size_t)k] = tot; lbase[(size_t)k] = local_n[chunk_owner[k]];
    tot += chunk_records[k]; local_n[chunk_owner[k]] += chunk_records[k];
  }
  for (int g = 0; g < n; ++g)
    if (local_n[(size_t)g] != ctxs[g]->x_n) { set_error("strl_ctxs_extract_gather: context %d holds %llu records, its chunks say %llu", g, (unsigned long long)ctxs[g]->x_n, (unsigned long long)local_n[(size_t)g]); return STRL_ERR_ARG; }
  if (tot > strl_record_limit()) { set_error("chunked extract: more than %llu records in one device pass", (unsigned long long)strl_record_limit()); return STRL_ERR_LIMIT; }
  // totals of the soft-clip records, the name arenas, the counters
  std::vector<uint32_t> xc((size_t)n * XC_WORDS);
  std::vector<uint64_t> soft_at((size_t)n + 1, 0), arena_at((size_t)n + 1, 0);
  for (int g = 0; g < n; ++g) {
    STRL_HIP(hipSetDevice(ctxs[g]->device));
    STRL_HIP(hipMemcpy(&xc[(size_t)g * XC_WORDS], ctxs[g]->x_cnt.p, XC_WORDS * 4, hipMemcpyDeviceToHost));
    if (xc[(size_t)g * XC_WORDS + XC_OVERFLOW]) { set_error("chunked extract: soft-clip records of a chunk were dropped"); return STRL_ERR_CAPACITY; }
    soft_at[(size_t)g + 1] = soft_at[(size_t)g] + xc[(size_t)g * XC_WORDS + XC_SOFT];
    arena_at[(size_t)g + 1] = arena_at[(size_t)g] + ctxs[g]->front->qarena_used;
  }
  STRL_HIP(hipSetDevice(c0->device));
  hipStream_t st = c0->stream;
  const uint64_t t1 = std::max<uint64_t>(tot, 1), s1 = std::max<uint64_t>(soft_at[(size_t)n], 1);
  // Shares (the first context holds the FIRST records of the file, all of them, and nothing else): its columns stay where
  // they are and the other contexts' shares are appended behind them -- no second copy of the per-read state, no copy of the
  // first share, and no allocation when strl_front_begin sized the first context for the whole file (the CLI does).
  bool in_place = true;
  {
    uint64_t own = 0;
    for (uint64_t k = 0; k < n_chunks; ++k) {
      if (chunk_owner[k] == 0) { if (gbase[(size_t)k] != lbase[(size_t)k]) in_place = false; own += chunk_records[k]; }
    }
    if (own != local_n[0]) in_place = false;
  }
  // the gathered columns: the first context's own where its share stays in place, new ones (which it adopts at the end) otherwise
  DevBuf *const mine[7] = {&c0->x_rows, &c0->x_qhash, &c0->x_whole, &F0->qref, &F0->fragw, &c0->x_soft, &F0->qarena};
  DevBuf fresh[7], tmp, tab;
  const size_t want[7] = {(size_t)t1 * sizeof(strl_pair_rec), (size_t)t1 * 8, (size_t)t1 * 4, (size_t)t1 * 8, (size_t)t1 * 4, (size_t)s1 * sizeof(strl_soft_rec),
                          (size_t)arena_at[(size_t)n] + 64};
  int rc;
  if (in_place) {
    const uint64_t n0 = local_n[0];
    const size_t keep[7] = {(size_t)n0 * sizeof(strl_pair_rec), (size_t)n0 * 8, (size_t)n0 * 4, (size_t)n0 * 8, (size_t)n0 * 4, (size_t)soft_at[1] * sizeof(strl_soft_rec),
                            (size_t)arena_at[1]};
    for (int k = 0; k < 7; ++k) if ((rc = mine[k]->grow(want[k], keep[k], st))) return rc;
  } else {
    for (int k = 0; k < 7; ++k) if ((rc = fresh[k].reserve(want[k]))) return rc;
  }
  DevBuf *col[7];
  for (int k = 0; k < 7; ++k) col[k] = in_place ? mine[k] : &fresh[k];
  DevBuf &rows = *col[0], &qhash = *col[1], &whole = *col[2], &qref = *col[3], &fragw = *col[4], &soft = *col[5], &arena = *col[6];
  if ((rc = tmp.reserve(std::max<size_t>((size_t)c0->bloom_mask / 8 + 64, (size_t)F0->n_ref + 64))) || (rc = tab.reserve((size_t)std::max<uint64_t>(n_chunks, 1) * 8 + 64))) return rc;
  // Runs of consecutive chunks of one owner (a share = one run) are contiguous on both sides: one copy per column.  A
  // context's columns, names and soft-clip records travel on ITS stream -- each source device drives its own link to the first,
  // the links work side by side -- and the first context's stream waits for one event per source before it re-bases.
  struct Run { uint32_t owner; uint64_t lo, go, m; };
  std::vector<Run> runs;
  for (uint64_t k = 0; k < n_chunks; ++k) {
    const uint64_t m = chunk_records[k];
    if (!m) continue;
    if (!runs.empty() && runs.back().owner == chunk_owner[k] && runs.back().lo + runs.back().m == lbase[(size_t)k] && runs.back().go + runs.back().m == gbase[(size_t)k]) runs.back().m += m;
    else runs.push_back(Run{chunk_owner[k], lbase[(size_t)k], gbase[(size_t)k], m});
  }
  std::vector<hipEvent_t> src_done((size_t)n, nullptr);
  auto drop_events = [&] { for (hipEvent_t e : src_done) if (e) (void)hipEventDestroy(e); };
  std::vector<std::vector<uint32_t>> tls((size_t)n), tgs((size_t)n);
  for (int g = 0; g < n; ++g) {
    strl_ctx *cg = ctxs[g];
    STRL_HIP(hipSetDevice(cg->device));
    hipStream_t sg = cg->stream;
    if (g == 0 && in_place) continue;            // its records, names and soft-clip records are where they belong already
    for (const Run &r : runs) {
      if (r.owner != (uint32_t)g) continue;
      if ((rc = copy_between(rows.as<strl_pair_rec>() + r.go, c0->device, cg->x_rows.as<strl_pair_rec>() + r.lo, cg->device, (size_t)r.m * sizeof(strl_pair_rec), sg)) ||
          (rc = copy_between(qhash.as<uint64_t>() + r.go, c0->device, cg->x_qhash.as<uint64_t>() + r.lo, cg->device, (size_t)r.m * 8, sg)) ||
          (rc = copy_between(whole.as<uint32_t>() + r.go, c0->device, cg->x_whole.as<uint32_t>() + r.lo, cg->device, (size_t)r.m * 4, sg)) ||
          (rc = copy_between(qref.as<uint64_t>() + r.go, c0->device, cg->front->qref.as<uint64_t>() + r.lo, cg->device, (size_t)r.m * 8, sg)) ||
          (rc = copy_between(fragw.as<uint32_t>() + r.go, c0->device, cg->front->fragw.as<uint32_t>() + r.lo, cg->device, (size_t)r.m * 4, sg))) { drop_events(); return rc; }
    }
    if ((rc = copy_between(arena.as<uint8_t>() + arena_at[(size_t)g], c0->device, cg->front->qarena.p, cg->device, (size_t)cg->front->qarena_used, sg))) { drop_events(); return rc; }
    const uint64_t ns = soft_at[(size_t)g + 1] - soft_at[(size_t)g];
    if (ns && (rc = copy_between(soft.as<strl_soft_rec>() + soft_at[(size_t)g], c0->device, cg->x_soft.p, cg->device, (size_t)ns * sizeof(strl_soft_rec), sg))) { drop_events(); return rc; }
    if (g) {      // (an event of the SOURCE's device on the source's stream; the wait below is the cross-device half, which is legal)
      STRL_HIP(hipEventCreateWithFlags(&src_done[(size_t)g], hipEventDisableTiming));
      STRL_HIP(hipEventRecord(src_done[(size_t)g], sg));
    }
  }
  STRL_HIP(hipSetDevice(c0->device));
  // re-basing on the first context, behind each source's copies
  size_t tab_at = 0;
  for (int g = 0; g < n; ++g) {
    strl_ctx *cg = ctxs[g];
    if (g) STRL_HIP(hipStreamWaitEvent(st, src_done[(size_t)g], 0));
    const uint64_t ab = arena_at[(size_t)g];
    if (ab)
      for (const Run &r : runs) {
        if (r.owner != (uint32_t)g) continue;
        hipLaunchKernelGGL(qref_rebase_kernel, dim3((unsigned)((r.m + 255) / 256)), dim3(256), 0, st, qref.as<uint64_t>() + r.go, (uint32_t)r.m, ab);
        STRL_HIP(hipGetLastError());
      }
    const uint64_t ns = soft_at[(size_t)g + 1] - soft_at[(size_t)g];
    if (ns && !(g == 0 && in_place)) {
      std::vector<uint32_t> &tl = tls[(size_t)g], &tg = tgs[(size_t)g];      // this context's chunks: first local / first global record
      for (uint64_t k = 0; k < n_chunks; ++k) if (chunk_owner[k] == (uint32_t)g) { tl.push_back((uint32_t)lbase[(size_t)k]); tg.push_back((uint32_t)gbase[(size_t)k]); }
      STRL_HIP(hipMemcpyAsync(tab.as<uint32_t>() + tab_at, tl.data(), tl.size() * 4, hipMemcpyHostToDevice, st));
      STRL_HIP(hipMemcpyAsync(tab.as<uint32_t>() + n_chunks + 8 + tab_at, tg.data(), tg.size() * 4, hipMemcpyHostToDevice, st));
      hipLaunchKernelGGL(soft_rebase_kernel, dim3((unsigned)((ns + 255) / 256)), dim3(256), 0, st, soft.as<strl_soft_rec>() + soft_at[(size_t)g], (uint32_t)ns,
                         tab.as<uint32_t>() + tab_at, tab.as<uint32_t>() + n_chunks + 8 + tab_at, (uint32_t)tl.size());
      STRL_HIP(hipGetLastError());
      tab_at += tl.size();
    }
    if (g) {       // contigs that had a primary record (the CLI's "extracting chromosome" lines)
      const size_t tw = ((size_t)std::min(F0->n_ref, cg->front->n_ref) + 3) / 4;
      if (tw) {
        if ((rc = copy_between(tmp.p, c0->device, cg->front->tid_seen.p, cg->device, tw * 4, st))) { drop_events(); return rc; }
        hipLaunchKernelGGL(words_or_kernel, dim3(16), dim3(256), 0, st, F0->tid_seen.as<uint32_t>(), tmp.as<uint32_t>(), tw);
        STRL_HIP(hipGetLastError());
      }
    }
    if (g) {
      const size_t bw = ((size_t)c0->bloom_mask + 1) / 32;
      if ((rc = copy_between(tmp.p, c0->device, cg->bloom.p, cg->device, bw * 4, st))) { drop_events(); return rc; }
      hipLaunchKernelGGL(words_or_kernel, dim3(1024), dim3(256), 0, st, c0->bloom.as<uint32_t>(), tmp.as<uint32_t>(), bw);
      STRL_HIP(hipGetLastError());
    }
  }
  uint32_t sum[XC_WORDS] = {0};
  for (int g = 0; g < n; ++g) for (int w = 0; w < XC_WORDS; ++w) sum[w] += xc[(size_t)g * XC_WORDS + w];
  STRL_HIP(hipStreamSynchronize(st));
  drop_events();
  STRL_HIP(hipMemcpy(c0->x_cnt.p, sum, XC_WORDS * 4, hipMemcpyHostToDevice));
  // ctxs[0] takes the gathered state over
  if (!in_place)
    for (int k = 0; k < 7; ++k) *mine[k] = std::move(fresh[k]);      // (the move frees what the context held)
  F0->qarena_used = arena_at[(size_t)n];
  c0->x_n = tot;
  c0->x_soft_cap = in_place ? c0->x_soft.cap / sizeof(strl_soft_rec) : s1;
  c0->x_soft_known = soft_at[(size_t)n]; c0->x_soft_known_at = tot;
  return STRL_OK;
}

}  // extern "C"
