// evidence.hip -- `strling call`'s per-bound evidence on the GPU (gfx950): what spanners() (collect.nim:130-182, with
// spanning.nim:22-49 and utils.nim:148-158) reads out of the BAM records around one bound, computed over the record bytes
// where region_walk_kernel (bgzf.hip) left them -- in device memory -- so that no record travels back to the host.
//
//   evidence_kernel : ONE WORKGROUP (4 waves) per region.
//     1. wave 0 walks the region's bytes through a 4 KiB LDS window (the walk of region_walk_kernel) and notes every record's
//        byte offset; more than EV_MAX_RECORDS records, or bytes that do not parse, pass the region on (status 2).
//     2. one lane per record: bam_endpos from the CIGAR, htslib's iterator filter, the flag / mapq filter; a kept record
//        adds +1 / -1 to the depth difference array in LDS (integer atomics) and its wave notes a ballot of the kept lanes.
//     3. the kept records get consecutive rows (ballot prefix; one integer atomic per region reserves them) and every kept
//        lane fills its row: expected_spanning_probability from the uploaded cd[] table, overlapping_read with
//        find_read_position and the greedy unit count over the 4-bit SEQ, the wrapping cigar_ins / cigar_del sums, pair
//        eligibility, Nim's murmur hash of the qname.
//     4. prefix sum of the depth array, the 1048-bin histogram (LDS atomics), median_depth.
//     5. qname identity in an LDS hash table keyed by the murmur value: every kept record is entered, then looks through
//        its probe run for the smallest row whose qname BYTES equal its own -- the hash only narrows the compare.
//   What depends on the order of Nim's tables (the fold per qname, the float32 sum in slot order, the pair list, the
//   spanning fragments) is finished on the host from the rows (call_logic.cpp evidence_finish), a few dozen bytes a record.
// What the kernel decides about ONE record against ONE bound -- the header test of step 1, step 2's keep test with its depth
// slots, step 3's row -- is evidence_core.h, which compiles for the host too (tests/emu/evidence_emu.cpp); this file keeps what
// belongs to a workgroup: the window walk, the ballots and ranks, the row reservation, the depth scan, the hash table.
// Nothing here re-sums floats: cd[] comes from the host as frag_tables() makes it; the only floating-point operations on the
// device are the IEEE subtraction 1.0f - cd[dist], the double product / quotient of the 70 % cut and the median's compare.
#include <string.h>
#include <algorithm>
#include <vector>
#pragma clang fp contract(off)
#include "common.h"
#include "nim_tables.h"
#include "regions.h"
#include "bam_rec.h"
#include "evidence_core.h"   // the per-record rule: EvBound, EvRec, ev_header_ok, ev_keep, ev_row (host and device)

namespace strl {

constexpr uint32_t EV_THREADS = 256, EV_WIN = 4096, EV_SLOTS = 8192, EV_DEPTH_CAP = 9192;

struct EvOut { int32_t median; uint32_t n_rows, row_base, status; };
struct EvParams {
  const uint8_t *u; uint64_t u_readable;
  const RegionWalk *range; const EvBound *eb; const float *cd;
  EvRow *rows; uint32_t row_cap; uint32_t *cursor; EvOut *eo;
  uint32_t min_mapq;
};

__global__ __launch_bounds__(EV_THREADS) void evidence_kernel(EvParams P) {
  __shared__ uint32_t off[EV_MAX_RECORDS];                     // byte offset of every record behind the region's start
  __shared__ __attribute__((aligned(16))) union {
    uint8_t win[EV_WIN];                                       // step 1
    int32_t depth[EV_DEPTH_CAP];                               // steps 2 - 4
    int32_t slot[EV_SLOTS];                                    // step 5
  } U;
  __shared__ uint32_t hist[1048];
  __shared__ unsigned long long mask[EV_MAX_RECORDS / 64];     // kept records, 64 consecutive ones a word
  __shared__ uint32_t rank0[EV_MAX_RECORDS / 64];              // kept records in front of the word's
  __shared__ uint32_t part[EV_THREADS];
  __shared__ uint32_t s_n, s_st, s_base, s_total, s_bad;
  __shared__ int32_t s_median;
  const uint32_t r = blockIdx.x, t = threadIdx.x, lane = t & 63u;
  const EvBound B = P.eb[r];
  if (B.status) {                                              // (uniform)
    if (t == 0) P.eo[r] = EvOut{0, 0u, 0u, B.status};
    return;
  }
  const uint64_t s0 = P.range[r].start, s1 = P.range[r].stop;
  const uint8_t *u = P.u;
  // ---- 1. the records' offsets
  if (t < 64u) {
    uint32_t n = 0, st = 0;
    uint64_t p = s0, w0 = 0, w1 = 0;                           // the window holds u[w0, w1)
    if (s1 - s0 >= (1ull << 31) || s1 > P.u_readable) st = 2;
    while (!st && p < s1) {
      if (p + 36 > s1) { st = 2; break; }
      if (p < w0 || p + 36 > w1) {
        __builtin_amdgcn_wave_barrier();
        w0 = p & ~(uint64_t)15;
        w1 = w0 + EV_WIN < P.u_readable ? w0 + EV_WIN : P.u_readable;
#pragma unroll
        for (uint32_t k = 0; k < EV_WIN / 1024; ++k) {
          const uint64_t o = w0 + 1024ull * k + 16ull * lane;
          if (o + 16 <= w1) *reinterpret_cast<uint4 *>(U.win + 1024u * k + 16u * lane) = *reinterpret_cast<const uint4 *>(u + o);
        }
        w1 &= ~(uint64_t)15;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (p + 36 > w1) { st = 2; break; }
      }
      uint32_t bs;
      if (!ev_header_ok(U.win + (p - w0), s1 - p, &bs)) { st = 2; break; }
      if (n == EV_MAX_RECORDS) { st = 2; break; }
      if (lane == 0) off[n] = (uint32_t)(p - s0);
      ++n;
      p += 4ull + bs;
    }
    if (t == 0) { s_n = n; s_st = st; }
  }
  __syncthreads();
  const uint32_t n = s_n;
  if (s_st) {                                                  // (uniform)
    if (t == 0) P.eo[r] = EvOut{0, 0u, 0u, 2u};
    return;
  }
  const int32_t D = B.depth_n;
  for (uint32_t i = t; i < (uint32_t)D; i += EV_THREADS) U.depth[i] = 0;
  for (uint32_t i = t; i < 1048u; i += EV_THREADS) hist[i] = 0;
  __syncthreads();
  // ---- 2. the filters and the depth differences (collect.nim:138-141,154-155)
  const uint32_t iters = (n + EV_THREADS - 1) / EV_THREADS;
  for (uint32_t it = 0; it < iters; ++it) {
    const uint32_t i = it * EV_THREADS + t;
    bool kept = false;
    if (i < n) {
      EvRec R;
      R.load(u + s0 + off[i]);
      int32_t a, b;
      kept = ev_keep(R, R.stop(), B, P.min_mapq, &a, &b);
      if (kept) {
        atomicAdd(&U.depth[a], 1);
        atomicSub(&U.depth[b], 1);
      }
    }
    const unsigned long long m = __ballot(kept);
    if (lane == 0) mask[it * 4u + (t >> 6)] = m;
  }
  __syncthreads();
  if (t == 0) {
    uint32_t tot = 0;
    for (uint32_t w = 0; w < iters * 4u; ++w) { rank0[w] = tot; tot += (uint32_t)__popcll(mask[w]); }
    uint32_t st = 0, base = 0;
    if (tot) {
      base = atomicAdd(P.cursor, tot);
      if ((uint64_t)base + tot > P.row_cap) st = 2;            // (the host sizes the rows for every record of every region)
    }
    s_total = tot; s_base = base; s_st = st; s_bad = 0;
  }
  __syncthreads();
  if (s_st) {
    if (t == 0) P.eo[r] = EvOut{0, 0u, 0u, 2u};
    return;
  }
  const uint32_t total = s_total;
  EvRow *rows = P.rows + s_base;
  // ---- 3. one row per kept record
  bool bad = false;
  for (uint32_t it = 0; it < iters; ++it) {
    const uint32_t i = it * EV_THREADS + t, w = it * 4u + (t >> 6);
    if (i >= n || !((mask[w] >> lane) & 1ull)) continue;
    const uint32_t k = rank0[w] + (uint32_t)__popcll(mask[w] & ((1ull << lane) - 1ull));
    EvRec R;
    R.load(u + s0 + off[i]);
    rows[k] = ev_row(R, R.stop(), B, P.cd, i, k, &bad);
  }
  if (bad) s_bad = 1;                                           // (every writer stores the same value; read behind the barriers below)
  // ---- 4. depths, their histogram, the median (utils.nim:148-158)
  const uint32_t chunk = ((uint32_t)D + EV_THREADS - 1) / EV_THREADS;
  const uint32_t c0 = t * chunk < (uint32_t)D ? t * chunk : (uint32_t)D, c1 = c0 + chunk < (uint32_t)D ? c0 + chunk : (uint32_t)D;
  {
    int32_t s = 0;
    for (uint32_t i = c0; i < c1; ++i) s += U.depth[i];
    part[t] = (uint32_t)s;
  }
  __syncthreads();
  {
    int32_t run = 0;
    for (uint32_t q = 0; q < t; ++q) run += (int32_t)part[q];
    for (uint32_t i = c0; i < c1; ++i) {
      run += U.depth[i];
      const int32_t d = run < 0 ? 0 : (run > 1047 ? 1047 : run);   // (a depth is never negative: a record's -1 lies at or behind its +1)
      atomicAdd(&hist[d], 1u);
    }
  }
  __syncthreads();
  if (t == 0) {
    int32_t med = 0;
    uint64_t s = 0;
    for (int i = 0; i < 1048; ++i) { s += hist[i]; if ((double)s > (double)D / 2.0) { med = i; break; } }
    s_median = med;
  }
  // ---- 5. qname identity: the first row of the region with the same qname bytes
  for (uint32_t i = t; i < EV_SLOTS; i += EV_THREADS) U.slot[i] = -1;
  __syncthreads();
  if (s_bad) {
    if (t == 0) P.eo[r] = EvOut{0, 0u, 0u, 2u};
    return;
  }
  for (uint32_t k = t; k < total; k += EV_THREADS) {
    uint32_t at = (rows[k].hash * 0x9E3779B1u) >> 19;
    while (atomicCAS(&U.slot[at], -1, (int32_t)k) != -1) at = (at + 1u) & (EV_SLOTS - 1u);
  }
  __syncthreads();
  for (uint32_t k = t; k < total; k += EV_THREADS) {
    const uint32_t h = rows[k].hash;
    const uint8_t *me = u + s0 + off[rows[k].ord];
    const uint32_t ln = me[12];
    uint32_t best = k;
    for (uint32_t at = (h * 0x9E3779B1u) >> 19;; at = (at + 1u) & (EV_SLOTS - 1u)) {
      const int32_t e = U.slot[at];
      if (e < 0) break;
      if ((uint32_t)e >= best || rows[e].hash != h) continue;
      const uint8_t *ot = u + s0 + off[rows[e].ord];
      if (ot[12] != ln) continue;
      bool same = true;
      for (uint32_t j = 0; j + 1u < ln && same; ++j) same = ot[36 + j] == me[36 + j];
      if (same) best = (uint32_t)e;
    }
    rows[k].name_id = best;
  }
  if (t == 0) P.eo[r] = EvOut{s_median, total, s_base, 0u};
}

int evidence_run(RegionJob &J, const uint8_t *d_u, uint64_t u_readable, const RegionWalk *d_range, const RegionWalk *h_range, uint32_t n_regions,
                 const strl_bounds *bounds, int32_t window, const uint32_t frag[4096], uint8_t min_mapq, strl_support *out, uint64_t cap,
                 uint64_t *support_off, strl_span_summary *summary, uint8_t *status, double *kernel_ms, const uint32_t *h_count) {
  if (kernel_ms) *kernel_ms = 0;
  std::vector<EvBound> eb(n_regions);
  uint64_t row_cap = 0;
  for (uint32_t r = 0; r < n_regions; ++r) {
    const strl_bounds &b = bounds[r];
    if (b.left > b.right) { set_error("bound with left > right"); return STRL_ERR_ARG; }
    const EvBound &E = eb[r] = ev_bound_make(b, window, status[r]);   // (with the capacity rule: status 2 beyond it)
    // rows for every record the region can hold (a record is 37 bytes or more); more than EV_MAX_RECORDS pass the region on
    // (h_count: the caller knows the number of records in the range -- the sweep's i1 - i0 -- and the rows are reserved from it)
    if (!E.status) row_cap += std::min<uint64_t>(EV_MAX_RECORDS, h_count ? (uint64_t)h_count[r] : (h_range[r].stop - h_range[r].start) / 37 + 1);
  }
  if (row_cap > 0xfffffff0ull) { set_error("evidence: %llu rows in one call", (unsigned long long)row_cap); return STRL_ERR_LIMIT; }
  strl_ctx::RegionSlot *slot = J.slot;
  hipStream_t st = J.stream();
  int rc;
  const size_t par_bytes = (size_t)n_regions * (sizeof(EvBound) + sizeof(EvOut)) + 4096 * sizeof(float) + 64;
  if ((rc = slot->ev_par.reserve(par_bytes)) || (rc = slot->ev_rows.reserve((size_t)row_cap * sizeof(EvRow) + 64))) return rc;
  EvBound *d_eb = slot->ev_par.as<EvBound>();
  EvOut *d_eo = reinterpret_cast<EvOut *>(d_eb + n_regions);
  float *d_cd = reinterpret_cast<float *>(d_eo + n_regions);
  uint32_t *d_cursor = reinterpret_cast<uint32_t *>(d_cd + 4096);
  const float *cd = frag_cd(frag);                             // (this thread's table: it outlives the copy, which is waited for below)
  std::vector<EvOut> eo(n_regions);
  uint32_t used = 0;
  hipEvent_t e0, e1;
  STRL_HIP(hipEventCreate(&e0));
  STRL_HIP(hipEventCreate(&e1));
  struct Ev { hipEvent_t a, b; ~Ev() { (void)hipEventDestroy(a); (void)hipEventDestroy(b); } } evs{e0, e1};
  STRL_HIP(hipMemcpyAsync(d_eb, eb.data(), (size_t)n_regions * sizeof(EvBound), hipMemcpyHostToDevice, st));
  STRL_HIP(hipMemcpyAsync(d_cd, cd, 4096 * sizeof(float), hipMemcpyHostToDevice, st));
  STRL_HIP(hipMemsetAsync(d_cursor, 0, 4, st));
  EvParams P{d_u, u_readable, d_range, d_eb, d_cd, slot->ev_rows.as<EvRow>(), (uint32_t)row_cap, d_cursor, d_eo, (uint32_t)min_mapq};
  STRL_HIP(hipEventRecord(e0, st));
  hipLaunchKernelGGL(evidence_kernel, dim3(n_regions), dim3(EV_THREADS), 0, st, P);
  STRL_HIP(hipGetLastError());
  STRL_HIP(hipEventRecord(e1, st));
  STRL_HIP(hipMemcpyAsync(eo.data(), d_eo, (size_t)n_regions * sizeof(EvOut), hipMemcpyDeviceToHost, st));
  STRL_HIP(hipMemcpyAsync(&used, d_cursor, 4, hipMemcpyDeviceToHost, st));
  STRL_HIP(hipStreamSynchronize(st));
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, e0, e1);
  if (kernel_ms) *kernel_ms = ms;
  std::vector<EvRow> rows(std::min<uint64_t>(used, row_cap));
  if (!rows.empty()) {
    STRL_HIP(hipMemcpyAsync(rows.data(), slot->ev_rows.p, rows.size() * sizeof(EvRow), hipMemcpyDeviceToHost, st));
    STRL_HIP(hipStreamSynchronize(st));
  }
  // the table-order steps, region by region
  uint64_t total = 0;
  for (uint32_t r = 0; r < n_regions; ++r) {
    support_off[r] = total;
    summary[r].median_depth = 0; summary[r].expected_spanners = 0; summary[r].n_support = 0;
    status[r] = (uint8_t)eo[r].status;
    if (eo[r].status) continue;
    if ((uint64_t)eo[r].row_base + eo[r].n_rows > rows.size()) { set_error("evidence rows out of range"); return STRL_ERR_HIP; }
    uint64_t n_out = 0;
    float es = 0;
    const bool room = out && total < cap;
    if (evidence_finish(rows.data() + eo[r].row_base, eo[r].n_rows, bounds[r], frag, room ? out + total : nullptr, room ? cap - total : 0, &n_out, &es)) {
      status[r] = 2;
      continue;
    }
    summary[r].median_depth = eo[r].median;
    summary[r].expected_spanners = es;
    summary[r].n_support = n_out;
    total += n_out;
  }
  support_off[n_regions] = total;
  if (total > cap) { set_error("support capacity %llu too small, need %llu", (unsigned long long)cap, (unsigned long long)total); return STRL_ERR_CAPACITY; }
  return STRL_OK;
}

}  // namespace strl

using namespace strl;

// C ABI: spanners() (collect.nim:130-182; spanning.nim:7-49; utils.nim:129-158) for many bounds, over record bytes in host memory
extern "C" int strl_evidence_records(strl_ctx *c, const uint8_t *bytes, const uint64_t *off, const uint64_t *len, const strl_bounds *bounds, uint32_t n_regions,
                                     int32_t window, const uint32_t frag[4096], uint8_t min_mapq, strl_support *support_out, uint64_t support_cap,
                                     uint64_t *support_off, strl_span_summary *summary, uint8_t *status) {
  if (!c || !frag || (n_regions && (!off || !len || !bounds || !support_off || !summary || !status)) || (support_cap && !support_out)) { set_error("null argument"); return STRL_ERR_ARG; }
  if (!n_regions) { if (support_off) support_off[0] = 0; return STRL_OK; }
  STRL_HIP(hipSetDevice(c->device));
  // one copy: the bytes from the lowest to the highest region
  uint64_t lo = ~0ull, hi = 0;
  for (uint32_t r = 0; r < n_regions; ++r) {
    if (!len[r]) continue;
    if (!bytes || off[r] + len[r] < off[r]) { set_error("null argument"); return STRL_ERR_ARG; }
    lo = std::min(lo, off[r]); hi = std::max(hi, off[r] + len[r]);
  }
  if (lo > hi) lo = hi = 0;
  std::vector<RegionWalk> range(n_regions);
  for (uint32_t r = 0; r < n_regions; ++r) range[r] = len[r] ? RegionWalk{off[r] - lo, off[r] - lo + len[r]} : RegionWalk{0, 0};
  RegionJob J;
  int rc;
  if ((rc = J.acquire(c, false))) return rc;
  strl_ctx::RegionSlot *slot = J.slot;
  const uint64_t span = hi - lo;
  if ((rc = slot->u.reserve(span + 64)) || (rc = slot->rq.reserve((size_t)n_regions * sizeof(RegionWalk) + 64))) return rc;
  hipStream_t st = J.stream();
  if (span) STRL_HIP(hipMemcpyAsync(slot->u.p, bytes + lo, span, hipMemcpyHostToDevice, st));
  STRL_HIP(hipMemcpyAsync(slot->rq.p, range.data(), (size_t)n_regions * sizeof(RegionWalk), hipMemcpyHostToDevice, st));
  for (uint32_t r = 0; r < n_regions; ++r) status[r] = 0;
  return evidence_run(J, slot->u.as<uint8_t>(), (span + 64) & ~(uint64_t)15, slot->rq.as<RegionWalk>(), range.data(), n_regions, bounds, window, frag, min_mapq,
                      support_out, support_cap, support_off, summary, status, nullptr);
}

// C ABI: the fused form `strling call` uses -- inflate, CRC, walk and evidence on the region slot's stream; no record bytes come back
extern "C" int strl_regions_evidence(strl_ctx *c, const uint8_t *comp, uint64_t comp_bytes, const uint64_t *coff, const uint32_t *clen, const uint32_t *isize,
                                     const uint32_t *crc32, uint32_t n_blocks, const strl_region_req *req, const strl_bounds *bounds, uint32_t n_regions,
                                     int32_t window, const uint32_t frag[4096], uint8_t min_mapq, strl_support *support_out, uint64_t support_cap,
                                     uint64_t *support_off, strl_span_summary *summary, uint8_t *status, double *kernel_ms) {
  if (!c || !frag || (n_blocks && (!comp || !coff || !clen || !isize)) || (n_regions && (!req || !bounds || !support_off || !summary || !status)) ||
      (support_cap && !support_out)) { set_error("null argument"); return STRL_ERR_ARG; }
  if (kernel_ms) *kernel_ms = 0;
  if (!n_regions) { if (support_off) support_off[0] = 0; return STRL_OK; }
  STRL_HIP(hipSetDevice(c->device));
  RegionJob J;
  int rc;
  if ((rc = J.acquire(c, crc32 != nullptr)) || (rc = regions_inflate_walk(J, comp, comp_bytes, coff, clen, isize, crc32, n_blocks, req, n_regions, status))) return rc;
  return evidence_run(J, J.slot->u.as<uint8_t>(), (J.tot + 64) & ~(uint64_t)15, J.d_range, J.range.data(), n_regions, bounds, window, frag, min_mapq, support_out,
                      support_cap, support_off, summary, status, kernel_ms);
}
