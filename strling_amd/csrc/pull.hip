// pull.hip -- `strling pull` on the GPU (gfx950): the two batched passes of extract_region.nim over record bytes that stay in
// device memory where regions_inflate_walk (bgzf.hip) left them.
//
//   select (extract_region.nim:46-50) : ONE WORKGROUP (4 waves) per tile of a region.  Wave 0 walks the tile's bytes through a
//     4 KiB LDS window (the walk of region_walk_kernel / evidence_kernel) and notes the offsets of up to 256 records; one lane
//     per record then applies htslib's iterator filter (refID, pos < end, bam_endpos > beg), the flag filter (:47), the tile's
//     ownership rule and hashes the qname; the kept lanes get consecutive places (ballot prefix, one LDS word per batch and
//     wave).  The loop goes on until the tile's bytes end: a pile-up is many batches, never a tile passed on.  A first launch
//     counts, the host turns the counts into the tiles' bases, a second launch writes the rows -- in file order, whichever
//     workgroup runs first.
//   counts (:44,50) : (hash, row) through sort.hip's radix sort; one lane per run of equal hash compares the name bytes inside
//     its run and writes every row's count.
//   mates (:7-19)   : ONE WORKGROUP per distinct (next_refID, 16 KiB window).  The window's requests go, 256 a round, into an
//     LDS hash table keyed by the qname hash; every record of the window probes it and, where it meets a request's rule
//     (:16-18 behind the iterator filter of the request's own interval), folds its place in the stream into the request's
//     answer with a 64-bit integer atomicMin: the first match in file order.
//   gather : one wave per record copies its bytes into the buffer the rows index (16 bytes a lane).
// All stores are plain vector stores and integer atomics.
#include <string.h>
#include <algorithm>
#include <vector>
#include "common.h"
#include "nim_tables.h"
#include "pull_rec.h"
#include "regions.h"
#include "sort.h"

namespace strl {

constexpr uint32_t PL_THREADS = 256, PL_WIN = 4096, PL_BATCH = 256;
constexpr uint32_t PL_TAB_REQ = 256, PL_TAB_SLOTS = 1024;     // requests a round, slots of the LDS table (a quarter full at most)
constexpr uint32_t PLF_READ1 = 0x40, PLF_SKIP = 0x900;   // :47 / :10,16 secondary | supplementary

struct PlTileOut { uint32_t n_rows, status; };
struct PlCopy { uint64_t src, dst; uint32_t len, pad; };

// Wave 0's walk over u[s0, s1): up to PL_BATCH records from W.p on, their offsets behind s0 into off[]; every lane holds the
// same values.  *st = 2: bytes that do not parse as records.  Returns the records noted.
struct PlWalk { uint64_t p, w0, w1; };
__device__ uint32_t pl_walk(const uint8_t *u, uint64_t u_readable, uint64_t s0, uint64_t s1, PlWalk &W, uint8_t *win, uint32_t *off, uint32_t lane, uint32_t *st) {
  uint32_t n = 0;
  while (n < PL_BATCH && W.p < s1) {
    const uint64_t p = W.p;
    if (p + 36 > s1) { *st = 2; break; }
    if (p < W.w0 || p + 36 > W.w1) {
      __builtin_amdgcn_wave_barrier();
      W.w0 = p & ~(uint64_t)15;
      W.w1 = W.w0 + PL_WIN < u_readable ? W.w0 + PL_WIN : u_readable;
#pragma unroll
      for (uint32_t k = 0; k < PL_WIN / 1024; ++k) {
        const uint64_t o = W.w0 + 1024ull * k + 16ull * lane;
        if (o + 16 <= W.w1) *reinterpret_cast<uint4 *>(win + 1024u * k + 16u * lane) = *reinterpret_cast<const uint4 *>(u + o);
      }
      W.w1 &= ~(uint64_t)15;
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
      if (p + 36 > W.w1) { *st = 2; break; }
    }
    const uint8_t *h = win + (p - W.w0);
    if (!pl_plausible(h, s1 - p)) { *st = 2; break; }
    const uint32_t bs = pl_ld32(h);
    if (lane == 0) off[n] = (uint32_t)(p - s0);
    ++n;
    W.p = p + 4ull + bs;
  }
  return n;
}

struct PlSelParams {
  const uint8_t *u; uint64_t u_readable;
  const RegionWalk *range; const uint8_t *walk_status; const strl_pull_tile *tiles;
  PlTileOut *to; const uint32_t *base; strl_pull_row *rows;
};

template <bool WRITE>
__global__ __launch_bounds__(PL_THREADS) void pull_select_kernel(PlSelParams P) {
  __shared__ __attribute__((aligned(16))) uint8_t win[PL_WIN];
  __shared__ uint32_t off[PL_BATCH];
  __shared__ uint32_t wcnt[PL_THREADS / 64];
  __shared__ uint32_t s_n, s_st, s_more;
  const uint32_t r = blockIdx.x, t = threadIdx.x, lane = t & 63u, wave = t >> 6;
  const uint32_t st_in = WRITE ? P.to[r].status : (uint32_t)P.walk_status[r];
  if (st_in) {                                                 // (uniform)
    if (!WRITE && t == 0) P.to[r] = PlTileOut{0u, st_in};
    return;
  }
  const strl_pull_tile T = P.tiles[r];
  const uint64_t s0 = P.range[r].start, s1 = P.range[r].stop;
  const uint8_t *u = P.u;
  const uint32_t limit = WRITE ? P.to[r].n_rows : 0u;           // rows the counting launch found: nothing is written behind them
  strl_pull_row *rows = WRITE ? P.rows + P.base[r] : nullptr;
  PlWalk W{s0, 0, 0};
  uint32_t running = 0;
  if (s1 < s0 || s1 - s0 >= (1ull << 31) || s1 > P.u_readable) {   // (uniform)
    if (!WRITE && t == 0) P.to[r] = PlTileOut{0u, 2u};
    return;
  }
  for (;;) {
    if (t < 64u) {
      uint32_t st = 0;
      const uint32_t n = pl_walk(u, P.u_readable, s0, s1, W, win, off, lane, &st);
      if (t == 0) { s_n = n; s_st = st; s_more = W.p < s1; }
    }
    __syncthreads();
    const uint32_t n = s_n, more = s_more;
    if (s_st) {                                                // (uniform)
      if (!WRITE && t == 0) P.to[r] = PlTileOut{0u, 2u};
      return;
    }
    bool kept = false;
    PlRec R;
    if (t < n) {
      R.load(u + s0 + off[t]);
      kept = R.kept_by(T);
    }
    const unsigned long long m = __ballot(kept);
    if (lane == 0) wcnt[wave] = (uint32_t)__popcll(m);
    __syncthreads();
    uint32_t before = running, total = 0;
    for (uint32_t w = 0; w < PL_THREADS / 64; ++w) { if (w < wave) before += wcnt[w]; total += wcnt[w]; }
    if (WRITE && kept) {
      const uint32_t k = before + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
      if (k < limit) rows[k] = R.row(s0 + off[t], R.hash());
    }
    running += total;
    if (!more) break;
    __syncthreads();                                           // off[], wcnt[] and s_* are rewritten by the next batch
  }
  if (!WRITE && t == 0) P.to[r] = PlTileOut{running, 0u};
}

__global__ __launch_bounds__(256) void pull_keys_kernel(const strl_pull_row *rows, uint32_t n, uint64_t *keys, uint32_t *vals) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i < n) { keys[i] = rows[i].hash; vals[i] = i; }
}

__device__ bool pl_same_name(const uint8_t *u, const strl_pull_row &a, const strl_pull_row &b) {
  const uint32_t ln = a.l_name ? a.l_name - 1u : 0u;           // PlRec::name_len: l_read_name 0 and 1 both carry the name ""
  if (ln != (b.l_name ? b.l_name - 1u : 0u)) return false;
  const uint8_t *x = u + a.off + 36, *y = u + b.off + 36;
  for (uint32_t j = 0; j < ln; ++j) if (x[j] != y[j]) return false;
  return true;
}
// one lane per run of equal hash (the lane of the run's first element): counts[qname] over the name's BYTES
__global__ __launch_bounds__(256) void pull_count_kernel(const uint8_t *u, strl_pull_row *rows, uint32_t n, const uint64_t *keys, const uint32_t *vals) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n || (i && keys[i - 1] == keys[i])) return;
  uint32_t e = i + 1;
  while (e < n && keys[e] == keys[i]) ++e;
  for (uint32_t a = i; a < e; ++a) {
    const uint32_t ra = vals[a];
    if (rows[ra].count) continue;                              // (counted with an earlier row of the run)
    uint32_t c = 0;
    for (uint32_t b = a; b < e; ++b) c += pl_same_name(u, rows[ra], rows[vals[b]]) ? 1u : 0u;
    for (uint32_t b = a; b < e; ++b) if (pl_same_name(u, rows[ra], rows[vals[b]])) rows[vals[b]].count = c;
  }
}

// one wave per record: len bytes from u + src to out + dst; dst = src (mod 16), so the body moves in 16-byte pieces
__global__ __launch_bounds__(256) void pull_copy_kernel(const uint8_t *u, const PlCopy *items, uint32_t n, uint8_t *out) {
  const uint32_t lane = threadIdx.x & 63u;
  for (uint32_t i = blockIdx.x * 4u + (threadIdx.x >> 6); i < n; i += gridDim.x * 4u) {
    const PlCopy c = items[i];
    const uint8_t *src = u + c.src;
    uint8_t *dst = out + c.dst;
    const uint64_t len = c.len;
    uint64_t head = (16u - (uint32_t)(c.src & 15u)) & 15u;
    if (head > len) head = len;
    const uint64_t body = (len - head) >> 4, tail0 = head + (body << 4);
    if (lane < head) dst[lane] = src[lane];
    const uint4 *s4 = reinterpret_cast<const uint4 *>(src + head);
    uint4 *d4 = reinterpret_cast<uint4 *>(dst + head);
    for (uint64_t k = lane; k < body; k += 64) d4[k] = s4[k];
    if (tail0 + lane < len) dst[tail0 + lane] = src[tail0 + lane];
  }
}

struct PlMateParams {
  const uint8_t *u; uint64_t u_readable;
  const RegionWalk *range; uint8_t *status; const strl_region_req *req;   // status[w]: the walk's verdict in, 2 out for bytes that do not parse
  const uint32_t *win_off; const strl_pull_req *reqs; const uint8_t *names;
  unsigned long long *ans;
};

__global__ __launch_bounds__(PL_THREADS) void pull_mate_kernel(PlMateParams P) {
  __shared__ __attribute__((aligned(16))) uint8_t win[PL_WIN];
  __shared__ uint32_t off[PL_BATCH];
  __shared__ int32_t slot[PL_TAB_SLOTS];
  __shared__ uint32_t s_n, s_st, s_more;
  const uint32_t w = blockIdx.x, t = threadIdx.x, lane = t & 63u;
  if (P.status[w]) return;                                     // (uniform; the host searches this window)
  const uint32_t q0 = P.win_off[w], q1 = P.win_off[w + 1];
  const int32_t tid = P.req[w].tid;
  const uint64_t s0 = P.range[w].start, s1 = P.range[w].stop;
  const uint8_t *u = P.u;
  if (s1 < s0 || s1 - s0 >= (1ull << 31) || s1 > P.u_readable) {   // (uniform)
    if (t == 0) P.status[w] = 2;
    return;
  }
  for (uint32_t r0 = q0; r0 < q1; r0 += PL_TAB_REQ) {
    const uint32_t m = q1 - r0 < PL_TAB_REQ ? q1 - r0 : PL_TAB_REQ;
    for (uint32_t i = t; i < PL_TAB_SLOTS; i += PL_THREADS) slot[i] = -1;
    __syncthreads();
    if (t < m) {
      uint32_t at = (P.reqs[r0 + t].hash * 0x9E3779B1u) >> 22;
      while (atomicCAS(&slot[at], -1, (int32_t)t) != -1) at = (at + 1u) & (PL_TAB_SLOTS - 1u);
    }
    __syncthreads();
    PlWalk W{s0, 0, 0};
    for (;;) {
      if (t < 64u) {
        uint32_t st = 0;
        const uint32_t n = pl_walk(u, P.u_readable, s0, s1, W, win, off, lane, &st);
        if (t == 0) { s_n = n; s_st = st; s_more = W.p < s1; }
      }
      __syncthreads();
      if (s_st) {                                              // (uniform) bytes that do not parse: the host searches this window
        if (t == 0) P.status[w] = 2;
        return;
      }
      const uint32_t n = s_n, more = s_more;
      if (t < n) {
        PlRec R;
        R.load(u + s0 + off[t]);
        if (!(R.flag & PLF_SKIP) && R.tid == tid) {
          const uint32_t ln = R.name_len();
          const uint32_t h = R.hash();
          int64_t stop = -1;
          for (uint32_t at = (h * 0x9E3779B1u) >> 22;; at = (at + 1u) & (PL_TAB_SLOTS - 1u)) {
            const int32_t e = slot[at];
            if (e < 0) break;
            const strl_pull_req Q = P.reqs[r0 + (uint32_t)e];
            if (Q.hash != h || !((Q.flag ^ R.flag) & PLF_READ1) || Q.name_len != ln || R.pos >= Q.end) continue;
            if (stop < 0) stop = R.stop();
            if (stop <= (int64_t)Q.beg) continue;
            const uint8_t *nm = P.names + Q.name_off;
            bool same = true;
            for (uint32_t j = 0; j < ln && same; ++j) same = nm[j] == R.p[36 + j];
            if (same) atomicMin(&P.ans[r0 + (uint32_t)e], (unsigned long long)(s0 + off[t]));
          }
        }
      }
      if (!more) break;
      __syncthreads();
    }
    __syncthreads();                                           // slot[] is cleared for the next round
  }
}

// one lane per request: the row of the record its answer names
__global__ __launch_bounds__(256) void pull_mate_rows_kernel(const uint8_t *u, const unsigned long long *ans, const strl_pull_req *reqs, uint32_t n, strl_pull_row *rows) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  strl_pull_row r;
  if (ans[i] == ~0ull) { r.off = 0; r.tid = r.pos = r.mtid = r.mpos = 0; r.size = r.hash = 0; r.flag = 0; r.l_name = 0; r.found = 0; r.count = 0; }
  else {
    PlRec R;
    R.load(u + ans[i]);
    r = R.row(ans[i], reqs[i].hash);
  }
  rows[i] = r;
}

// The records the rows name, gathered: rows[i].off goes from the offset in `u` to the one in `bytes`.  Waits for the stream.
static int pull_gather(hipStream_t st, const uint8_t *d_u, strl_pull_row *rows, uint64_t n, DevBuf &d_items, DevBuf &d_out, uint8_t *bytes, uint64_t bytes_cap,
                       uint64_t *n_bytes, hipEvent_t e0, hipEvent_t e1) {
  std::vector<PlCopy> items;
  items.reserve((size_t)n);
  uint64_t at = 0;
  for (uint64_t i = 0; i < n; ++i) {
    if (!rows[i].found) continue;
    at = ((at + 15) & ~(uint64_t)15) + (rows[i].off & 15u);
    items.push_back(PlCopy{rows[i].off, at, rows[i].size, 0u});
    rows[i].off = at;
    at += rows[i].size;
  }
  *n_bytes = at;
  if (at > bytes_cap) { set_error("pull: %llu record bytes, room for %llu", (unsigned long long)at, (unsigned long long)bytes_cap); return STRL_ERR_CAPACITY; }
  if (items.empty()) return STRL_OK;
  if (items.size() > 0xfffffff0ull) { set_error("pull: %llu records in one call", (unsigned long long)items.size()); return STRL_ERR_LIMIT; }
  int rc;
  if ((rc = d_items.reserve(items.size() * sizeof(PlCopy))) || (rc = d_out.reserve(at + 64))) return rc;
  STRL_HIP(hipMemcpyAsync(d_items.p, items.data(), items.size() * sizeof(PlCopy), hipMemcpyHostToDevice, st));
  STRL_HIP(hipEventRecord(e0, st));
  hipLaunchKernelGGL(pull_copy_kernel, dim3((uint32_t)std::min<uint64_t>((items.size() + 3) / 4, 2048)), dim3(256), 0, st, d_u, d_items.as<PlCopy>(), (uint32_t)items.size(), d_out.as<uint8_t>());
  STRL_HIP(hipGetLastError());
  STRL_HIP(hipEventRecord(e1, st));
  STRL_HIP(hipMemcpyAsync(bytes, d_out.p, at, hipMemcpyDeviceToHost, st));
  STRL_HIP(hipStreamSynchronize(st));
  return STRL_OK;
}

struct PlEvents {
  hipEvent_t e[4] = {};
  int make() { for (auto &x : e) STRL_HIP(hipEventCreate(&x)); return STRL_OK; }
  ~PlEvents() { for (auto x : e) if (x) (void)hipEventDestroy(x); }
  double ms(int a, int b) const { float v = 0.f; return hipEventElapsedTime(&v, e[a], e[b]) == hipSuccess ? (double)v : 0.0; }
};

}  // namespace strl

using namespace strl;

// C ABI: extract_region.nim:46-50 for the tiles of many regions
extern "C" int strl_pull_select(strl_ctx *c, const uint8_t *comp, uint64_t comp_bytes, const uint64_t *coff, const uint32_t *clen, const uint32_t *isize,
                                const uint32_t *crc32, uint32_t n_blocks, const strl_region_req *req, const strl_pull_tile *tiles, uint32_t n_tiles,
                                strl_pull_row *rows, uint64_t row_cap, uint64_t *n_rows, uint64_t *tile_rows, uint8_t *bytes, uint64_t bytes_cap,
                                uint64_t *n_bytes, uint8_t *status, double *kernel_ms) {
  if (!c || !n_rows || !n_bytes || !tile_rows || (n_blocks && (!comp || !coff || !clen || !isize)) || (n_tiles && (!req || !tiles || !status)) || (row_cap && !rows) ||
      (bytes_cap && !bytes)) { set_error("null argument"); return STRL_ERR_ARG; }
  if (kernel_ms) *kernel_ms = 0;
  *n_rows = 0; *n_bytes = 0; tile_rows[0] = 0;
  if (!n_tiles) return STRL_OK;
  STRL_HIP(hipSetDevice(c->device));
  DevBuf d_par, d_k0, d_k1, d_v0, d_v1, d_sort, d_items;          // (declared before the job: the job's destructor drains the stream first,
  std::vector<PlTileOut> to(n_tiles);                             //  and so are the host arrays and events its copies use)
  std::vector<uint32_t> base(n_tiles);
  uint32_t n = 0;
  PlEvents ev;
  RegionJob J;
  int rc;
  if ((rc = J.acquire(c, crc32 != nullptr)) || (rc = regions_inflate_walk(J, comp, comp_bytes, coff, clen, isize, crc32, n_blocks, req, n_tiles, status))) return rc;
  strl_ctx::RegionSlot *slot = J.slot;
  hipStream_t st = J.stream();
  if ((rc = ev.make())) return rc;
  const size_t par_bytes = (size_t)n_tiles * (sizeof(strl_pull_tile) + sizeof(PlTileOut) + 4) + 64;
  if ((rc = d_par.reserve(par_bytes))) return rc;
  PlTileOut *d_to = d_par.as<PlTileOut>();
  uint32_t *d_base = reinterpret_cast<uint32_t *>(d_to + n_tiles);
  strl_pull_tile *d_tiles = reinterpret_cast<strl_pull_tile *>(d_base + n_tiles);
  uint32_t *d_n = reinterpret_cast<uint32_t *>(d_tiles + n_tiles);
  STRL_HIP(hipMemcpyAsync(d_tiles, tiles, (size_t)n_tiles * sizeof(strl_pull_tile), hipMemcpyHostToDevice, st));
  PlSelParams P{slot->u.as<uint8_t>(), (J.tot + 64) & ~(uint64_t)15, J.d_range, J.d_status, d_tiles, d_to, d_base, nullptr};
  STRL_HIP(hipEventRecord(ev.e[0], st));
  hipLaunchKernelGGL(pull_select_kernel<false>, dim3(n_tiles), dim3(PL_THREADS), 0, st, P);
  STRL_HIP(hipGetLastError());
  STRL_HIP(hipMemcpyAsync(to.data(), d_to, (size_t)n_tiles * sizeof(PlTileOut), hipMemcpyDeviceToHost, st));
  STRL_HIP(hipStreamSynchronize(st));
  uint64_t total = 0;
  for (uint32_t t = 0; t < n_tiles; ++t) {
    status[t] = (uint8_t)to[t].status;
    tile_rows[t] = total;
    base[t] = (uint32_t)total;
    total += to[t].status ? 0 : to[t].n_rows;
    if (total > 0xfffffff0ull) { set_error("pull: %llu rows in one call", (unsigned long long)total); return STRL_ERR_LIMIT; }
  }
  tile_rows[n_tiles] = total;
  *n_rows = total;
  if (total > row_cap) { set_error("pull: %llu rows, room for %llu", (unsigned long long)total, (unsigned long long)row_cap); return STRL_ERR_CAPACITY; }
  if (!total) return STRL_OK;
  n = (uint32_t)total;
  const size_t sb = radix_sort_scratch_bytes(n, 32);
  if ((rc = slot->ev_rows.reserve((size_t)n * sizeof(strl_pull_row))) || (rc = d_k0.reserve((size_t)n * 8)) || (rc = d_k1.reserve((size_t)n * 8)) ||
      (rc = d_v0.reserve((size_t)n * 4)) || (rc = d_v1.reserve((size_t)n * 4)) || (rc = d_sort.reserve(sb)))
    return rc;
  P.rows = slot->ev_rows.as<strl_pull_row>();
  STRL_HIP(hipMemcpyAsync(d_base, base.data(), (size_t)n_tiles * 4, hipMemcpyHostToDevice, st));
  STRL_HIP(hipMemcpyAsync(d_n, &n, 4, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(pull_select_kernel<true>, dim3(n_tiles), dim3(PL_THREADS), 0, st, P);
  hipLaunchKernelGGL(pull_keys_kernel, dim3((n + 255) / 256), dim3(256), 0, st, P.rows, n, d_k0.as<uint64_t>(), d_v0.as<uint32_t>());
  STRL_HIP(hipGetLastError());
  uint64_t *ok = nullptr;
  uint32_t *ov = nullptr;
  const int e = radix_sort_pairs(st, d_n, n, d_k0.as<uint64_t>(), d_v0.as<uint32_t>(), d_k1.as<uint64_t>(), d_v1.as<uint32_t>(), d_sort.p, sb, 0, 32, &ok, &ov);
  if (e) { set_error("radix_sort_pairs failed: %s", hipGetErrorString((hipError_t)e)); return STRL_ERR_HIP; }
  hipLaunchKernelGGL(pull_count_kernel, dim3((n + 255) / 256), dim3(256), 0, st, P.u, P.rows, n, ok, ov);
  STRL_HIP(hipGetLastError());
  STRL_HIP(hipEventRecord(ev.e[1], st));
  STRL_HIP(hipMemcpyAsync(rows, P.rows, (size_t)n * sizeof(strl_pull_row), hipMemcpyDeviceToHost, st));
  STRL_HIP(hipStreamSynchronize(st));
  if ((rc = pull_gather(st, P.u, rows, n, d_items, slot->out, bytes, bytes_cap, n_bytes, ev.e[2], ev.e[3]))) return rc;
  if (kernel_ms) *kernel_ms = ev.ms(0, 1) + ev.ms(2, 3);
  return STRL_OK;
}

// C ABI: get_mate (:15-19) for many requests, window by window
extern "C" int strl_pull_mates(strl_ctx *c, const uint8_t *comp, uint64_t comp_bytes, const uint64_t *coff, const uint32_t *clen, const uint32_t *isize,
                               const uint32_t *crc32, uint32_t n_blocks, const strl_region_req *req, const uint32_t *win_off, uint32_t n_windows,
                               const strl_pull_req *reqs, const uint8_t *names, uint64_t names_bytes, strl_pull_row *rows, uint8_t *bytes,
                               uint64_t bytes_cap, uint64_t *n_bytes, uint8_t *status, double *kernel_ms) {
  if (!c || !n_bytes || (n_blocks && (!comp || !coff || !clen || !isize)) || (n_windows && (!req || !win_off || !status)) || (bytes_cap && !bytes)) { set_error("null argument"); return STRL_ERR_ARG; }
  if (kernel_ms) *kernel_ms = 0;
  *n_bytes = 0;
  if (!n_windows) return STRL_OK;
  const uint32_t n_req = win_off[n_windows];
  if (n_req && (!reqs || !rows || (names_bytes && !names))) { set_error("null argument"); return STRL_ERR_ARG; }
  for (uint32_t w = 0; w < n_windows; ++w)
    if (win_off[w] > win_off[w + 1]) { set_error("window %u: request offsets run backwards", w); return STRL_ERR_ARG; }
  for (uint32_t k = 0; k < n_req; ++k)
    if ((uint64_t)reqs[k].name_off + reqs[k].name_len > names_bytes) { set_error("request %u: name outside the names", k); return STRL_ERR_ARG; }
  if (!n_req) { for (uint32_t w = 0; w < n_windows; ++w) status[w] = 0; return STRL_OK; }
  STRL_HIP(hipSetDevice(c->device));
  DevBuf d_par, d_items;
  PlEvents ev;
  RegionJob J;
  int rc;
  if ((rc = J.acquire(c, crc32 != nullptr)) || (rc = regions_inflate_walk(J, comp, comp_bytes, coff, clen, isize, crc32, n_blocks, req, n_windows, status))) return rc;
  strl_ctx::RegionSlot *slot = J.slot;
  hipStream_t st = J.stream();
  if ((rc = ev.make())) return rc;
  const size_t par_bytes = (size_t)n_req * (8 + sizeof(strl_pull_req)) + (size_t)n_windows * sizeof(strl_region_req) + ((size_t)n_windows + 1) * 4 + names_bytes + 64;
  if ((rc = d_par.reserve(par_bytes)) || (rc = slot->ev_rows.reserve((size_t)n_req * sizeof(strl_pull_row)))) return rc;
  unsigned long long *d_ans = d_par.as<unsigned long long>();
  strl_pull_req *d_reqs = reinterpret_cast<strl_pull_req *>(d_ans + n_req);
  strl_region_req *d_req = reinterpret_cast<strl_region_req *>(d_reqs + n_req);
  uint32_t *d_woff = reinterpret_cast<uint32_t *>(d_req + n_windows);
  uint8_t *d_names = reinterpret_cast<uint8_t *>(d_woff + n_windows + 1);
  STRL_HIP(hipMemsetAsync(d_ans, 0xff, (size_t)n_req * 8, st));
  STRL_HIP(hipMemcpyAsync(d_reqs, reqs, (size_t)n_req * sizeof(strl_pull_req), hipMemcpyHostToDevice, st));
  STRL_HIP(hipMemcpyAsync(d_req, req, (size_t)n_windows * sizeof(strl_region_req), hipMemcpyHostToDevice, st));
  STRL_HIP(hipMemcpyAsync(d_woff, win_off, ((size_t)n_windows + 1) * 4, hipMemcpyHostToDevice, st));
  if (names_bytes) STRL_HIP(hipMemcpyAsync(d_names, names, names_bytes, hipMemcpyHostToDevice, st));
  PlMateParams P{slot->u.as<uint8_t>(), (J.tot + 64) & ~(uint64_t)15, J.d_range, J.d_status, d_req, d_woff, d_reqs, d_names, d_ans};
  strl_pull_row *d_rows = slot->ev_rows.as<strl_pull_row>();
  STRL_HIP(hipEventRecord(ev.e[0], st));
  hipLaunchKernelGGL(pull_mate_kernel, dim3(n_windows), dim3(PL_THREADS), 0, st, P);
  hipLaunchKernelGGL(pull_mate_rows_kernel, dim3((n_req + 255) / 256), dim3(256), 0, st, P.u, d_ans, d_reqs, n_req, d_rows);
  STRL_HIP(hipGetLastError());
  STRL_HIP(hipEventRecord(ev.e[1], st));
  STRL_HIP(hipMemcpyAsync(rows, d_rows, (size_t)n_req * sizeof(strl_pull_row), hipMemcpyDeviceToHost, st));
  STRL_HIP(hipMemcpyAsync(status, J.d_status, n_windows, hipMemcpyDeviceToHost, st));
  STRL_HIP(hipStreamSynchronize(st));
  for (uint32_t w = 0; w < n_windows; ++w)
    if (status[w]) memset(rows + win_off[w], 0, (size_t)(win_off[w + 1] - win_off[w]) * sizeof(strl_pull_row));   // (answered on the host, all of them)
  if ((rc = pull_gather(st, P.u, rows, n_req, d_items, slot->out, bytes, bytes_cap, n_bytes, ev.e[2], ev.e[3]))) return rc;
  if (kernel_ms) *kernel_ms = ev.ms(0, 1) + ev.ms(2, 3);
  return STRL_OK;
}
