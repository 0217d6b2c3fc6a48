// sweep.hip -- `strling call --sweep`: the evidence of every bound from ONE pass over the BAM (gfx950).  The per-bound path reads
// query(tid, left - window, right + window) bound by bound (collect.nim:130-182 through the index); its bytes grow with the
// number of bounds.  Here the file goes through the front end once, chunk by chunk, as for `strling bamindex`:
//   front_stage_a        (front.hip)   copy + inflate + CRC + record scan: recoff[] of the chunk, its records contiguous
//   sweep_keys_kernel                  one lane per record: tid, pos, end; the order check; the running maximum of end in its tile
//   sweep_tiles_kernel                 one workgroup: the tiles' prefixes, seeded with the carry of the chunks in front
//   sweep_ranges_kernel                one lane per open bound: the byte range [recoff[i0], recoff[i1]) of its records, or a seam
//   evidence_kernel      (evidence.hip) over those ranges, in the slot's inflated buffer, through evidence_run
// (the bodies and the rule: sweep_core.h).  push(i) enqueues chunk i's copy + inflate + scan and then sweeps chunk i - 1 beside
// it; the slot's buffer is given back (ev_b) behind the evidence kernel of its chunk.  What a bound costs no longer depends on
// how many bounds share its blocks.
#include <string.h>
#include <algorithm>
#include <numeric>
#include <vector>
#include "front.h"
#include "regions.h"
#include "sweep_core.h"

namespace strl {

__global__ __launch_bounds__(SW_THREADS) void sweep_keys_kernel(SweepParams P) {
  __shared__ SweepShared Sh;
  sweep_keys_body(SwGroup{threadIdx.x, blockIdx.x}, P, Sh);
}
__global__ __launch_bounds__(SW_THREADS) void sweep_tiles_kernel(SweepParams P) {
  __shared__ SweepShared Sh;
  sweep_tiles_body(SwGroup{threadIdx.x, blockIdx.x}, P, Sh);
}
__global__ __launch_bounds__(SW_THREADS) void sweep_ranges_kernel(SweepParams P) { sweep_ranges_body(SwGroup{threadIdx.x, blockIdx.x}, P); }

constexpr uint64_t SW_ROWS_PER_LAUNCH = 1ull << 22;   // rows (40 B) one evidence launch may reserve; a chunk with more runs several

struct strl_sweep {
  int32_t n_ref = 0, window = 0;
  uint8_t min_mapq = 0;
  uint32_t frag[4096];
  uint32_t nb = 0;
  std::vector<strl_bounds> bounds;          // sorted by (tid, beg)
  std::vector<uint32_t> order;              // sorted index -> the caller's index
  DevBuf d_bounds, d_dec, d_state, d_out, d_tid, d_pos, d_pmax, d_tile, d_rng;
  SweepState *h_state = nullptr;            // pinned
  std::vector<SweepDecision> dec;
  // results, by sorted index
  std::vector<uint8_t> status;
  std::vector<strl_span_summary> summary;
  std::vector<uint64_t> sup_at;             // where the bound's Support list starts in sup
  std::vector<strl_support> sup;
  uint64_t chunks = 0, done = 0, n_records = 0;
  uint32_t par = 0;
  bool last_pushed = false;
  int fail_rc = 0;                          // a push refused the file: every later call repeats it
  std::string fail;
  double ms_sweep = 0, ms_evidence = 0;
  hipEvent_t e0 = nullptr, e1 = nullptr;
};

void sweep_destroy(strl_sweep *W) {
  if (!W) return;
  if (W->h_state) (void)hipHostFree(W->h_state);
  if (W->e0) (void)hipEventDestroy(W->e0);
  if (W->e1) (void)hipEventDestroy(W->e1);
  delete W;
}

static int sweep_fail(strl_sweep *W, int rc) {
  W->fail_rc = rc; W->fail = strl_last_error();
  return rc;
}

// the chunk in slot si (its record scan was enqueued by the push before): keys, tiles, ranges, then the evidence of the bounds
// the chunk decided.  Waits on the host for the decisions: the rows are reserved from their record counts.
static int sweep_chunk(strl_ctx *c, strl_front *F, strl_sweep *W, int si, bool last) {
  FrontSlot &S = F->slot[si];
  STRL_HIP(hipEventSynchronize(S.ev_a));
  const FrontInfo I = S.h_info[0];
  if (I.err & FRONT_ERR_INFLATE) { set_error("invalid BGZF block (DEFLATE data or ISIZE)"); return STRL_ERR_FORMAT; }
  if (I.err & FRONT_ERR_CRC) { set_error("CRC32 checksum mismatch in a BGZF block"); return STRL_ERR_CRC; }
  if (I.err & FRONT_ERR_RECORD) { set_error("malformed BAM record"); return STRL_ERR_FORMAT; }
  if (I.err & FRONT_ERR_CARRY) { set_error("BAM record of more than %u bytes", FRONT_CARRY_MAX); return STRL_ERR_FORMAT; }
  if (last && I.carry_len) { set_error("the BAM ends inside a record (truncated file)"); return STRL_ERR_FORMAT; }
  const uint32_t n = I.n_records, tiles = (n + SW_THREADS - 1u) / SW_THREADS;
  hipStream_t st = c->stream;
  int rc;
  if (n || last) {
    if ((rc = W->d_tid.reserve((size_t)n * 4 + 64)) || (rc = W->d_pos.reserve((size_t)n * 4 + 64)) || (rc = W->d_pmax.reserve((size_t)n * 4 + 64)) ||
        (rc = W->d_tile.reserve((size_t)tiles * sizeof(SweepCarry) + 64)))
      return rc;
    SweepParams P{};
    P.U = S.infl.as<uint8_t>(); P.recoff = S.recoff.as<uint32_t>(); P.n = n; P.rec_end = I.carry_off;
    P.ord0 = W->n_records; P.n_ref = W->n_ref;
    P.tid = W->d_tid.as<int32_t>(); P.pos = W->d_pos.as<int32_t>(); P.pmax = W->d_pmax.as<int32_t>();
    P.tile = W->d_tile.as<SweepCarry>(); P.n_tiles = tiles;
    P.S = W->d_state.as<SweepState>(); P.par = W->par;
    P.bounds = W->d_bounds.as<SweepBound>(); P.n_bounds = W->nb;
    P.dec = W->d_dec.as<uint32_t>(); P.out = W->d_out.as<SweepDecision>();
    P.last_chunk = last ? 1u : 0u;
    STRL_HIP(hipEventRecord(W->e0, st));
    if (n) {
      hipLaunchKernelGGL(sweep_keys_kernel, dim3(tiles), dim3(SW_THREADS), 0, st, P);
      hipLaunchKernelGGL(sweep_tiles_kernel, dim3(1), dim3(SW_THREADS), 0, st, P);
    }
    if (W->nb) hipLaunchKernelGGL(sweep_ranges_kernel, dim3((W->nb + SW_THREADS - 1u) / SW_THREADS), dim3(SW_THREADS), 0, st, P);
    STRL_HIP(hipGetLastError());
    STRL_HIP(hipEventRecord(W->e1, st));
    STRL_HIP(hipMemcpyAsync(W->h_state, W->d_state.p, sizeof(SweepState), hipMemcpyDeviceToHost, st));
    STRL_HIP(hipMemsetAsync(&P.S->n_dec, 0, 4, st));
    STRL_HIP(hipStreamSynchronize(st));
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, W->e0, W->e1);
    W->ms_sweep += ms;
    const SweepState &H = *W->h_state;
    if (H.err_ord[SW_E_UNSORTED] != ~0ull && H.err_ord[SW_E_UNSORTED] <= H.err_ord[SW_E_TID]) {
      set_error("the BAM is not coordinate sorted: record %llu comes behind a record of a later position (or behind an unplaced one); sort it first", H.err_ord[SW_E_UNSORTED]);
      return STRL_ERR_FORMAT;
    }
    if (H.err_ord[SW_E_TID] != ~0ull) {
      set_error("malformed BAM record %llu: its refID is not one of the header's %d references", H.err_ord[SW_E_TID], W->n_ref);
      return STRL_ERR_FORMAT;
    }
    const uint32_t nd = H.n_dec;
    if (nd > W->nb) { set_error("sweep: %u decisions for %u bounds", nd, W->nb); return STRL_ERR_HIP; }
    W->dec.resize(nd);
    if (nd) STRL_HIP(hipMemcpy(W->dec.data(), W->d_out.p, (size_t)nd * sizeof(SweepDecision), hipMemcpyDeviceToHost));
    std::sort(W->dec.begin(), W->dec.end(), [](const SweepDecision &a, const SweepDecision &b) { return a.bound < b.bound; });   // (the lanes' arrival order is not kept)
    // the evidence of the ranges, as many bounds a launch as its rows allow
    const uint64_t u_readable = ((uint64_t)I.end + 64) & ~(uint64_t)15;
    std::vector<RegionWalk> rng;
    std::vector<uint32_t> cnt, who;
    std::vector<strl_bounds> bb;
    std::vector<strl_support> out;
    std::vector<uint64_t> off;
    std::vector<strl_span_summary> sm;
    std::vector<uint8_t> stv;
    size_t k = 0;
    while (k < W->dec.size()) {
      rng.clear(); cnt.clear(); who.clear(); bb.clear();
      uint64_t rows = 0;
      for (; k < W->dec.size(); ++k) {
        const SweepDecision &D = W->dec[k];
        if (D.bound >= W->nb || D.i0 > D.i1 || D.i1 > n || D.start > D.stop || D.stop > I.end) { set_error("sweep: decision out of range"); return STRL_ERR_HIP; }
        if (D.status) { W->status[D.bound] = 1; continue; }
        const uint32_t records = D.i1 - D.i0;
        const uint64_t need = std::min<uint64_t>(records, EV_MAX_RECORDS);
        if (!who.empty() && rows + need > SW_ROWS_PER_LAUNCH) break;
        rows += need;
        rng.push_back(records ? RegionWalk{D.start, D.stop} : RegionWalk{0, 0});
        cnt.push_back(records); who.push_back(D.bound); bb.push_back(W->bounds[D.bound]);
      }
      const uint32_t m = (uint32_t)who.size();
      if (!m) continue;
      RegionJob J;
      if ((rc = J.acquire(c, false))) return rc;
      if ((rc = W->d_rng.reserve((size_t)m * sizeof(RegionWalk) + 64))) return rc;
      STRL_HIP(hipMemcpyAsync(W->d_rng.p, rng.data(), (size_t)m * sizeof(RegionWalk), hipMemcpyHostToDevice, J.stream()));
      const uint64_t cap = 2 * rows + 16;     // (a kept record gives at most one read Support and half a fragment: evidence_finish)
      out.resize(cap); off.assign((size_t)m + 1, 0); sm.resize(m); stv.assign(m, 0);
      double ems = 0;
      if ((rc = evidence_run(J, S.infl.as<uint8_t>(), u_readable, W->d_rng.as<RegionWalk>(), rng.data(), m, bb.data(), W->window, W->frag, W->min_mapq, out.data(), cap,
                             off.data(), sm.data(), stv.data(), &ems, cnt.data())))
        return rc;
      W->ms_evidence += ems;
      for (uint32_t r = 0; r < m; ++r) {
        const uint32_t b = who[r];
        W->status[b] = stv[r]; W->summary[b] = sm[r]; W->sup_at[b] = W->sup.size();
        W->sup.insert(W->sup.end(), out.begin() + (ptrdiff_t)off[r], out.begin() + (ptrdiff_t)off[r + 1]);
      }
    }
    if (n) { W->n_records += n; W->par ^= 1u; }
  }
  STRL_HIP(hipEventRecord(S.ev_b, st));       // the slot's inflated bytes and record table may be overwritten behind this
  S.b_pending = true;
  return STRL_OK;
}

}  // namespace strl

using namespace strl;

extern "C" int strl_sweep_begin(strl_ctx *c, int32_t n_ref, uint64_t first_record_offset, const strl_bounds *bounds, uint32_t n_bounds, int32_t window,
                                const uint32_t frag[4096], uint8_t min_mapq) {
  if (!c || n_ref < 0 || !frag || (n_bounds && !bounds)) { set_error("strl_sweep_begin: bad argument"); return STRL_ERR_ARG; }
  for (uint32_t r = 0; r < n_bounds; ++r)
    if (bounds[r].left > bounds[r].right) { set_error("bound with left > right"); return STRL_ERR_ARG; }
  int rc;
  if ((rc = front_begin_scan(c, n_ref, first_record_offset))) return rc;
  if (c->sweep) { sweep_destroy(c->sweep); c->sweep = nullptr; }
  strl_sweep *W = new strl_sweep();
  c->sweep = W;
  W->n_ref = n_ref; W->window = window; W->min_mapq = min_mapq; W->nb = n_bounds;
  memcpy(W->frag, frag, sizeof W->frag);
  auto beg_of = [window](const strl_bounds &b) { return std::max<int64_t>(0, (int64_t)b.left - window); };
  W->order.resize(n_bounds);
  std::iota(W->order.begin(), W->order.end(), 0u);
  std::stable_sort(W->order.begin(), W->order.end(), [&](uint32_t x, uint32_t y) {
    if (bounds[x].tid != bounds[y].tid) return bounds[x].tid < bounds[y].tid;
    return beg_of(bounds[x]) < beg_of(bounds[y]);
  });
  W->bounds.resize(n_bounds);
  std::vector<SweepBound> sb(n_bounds);
  std::vector<uint32_t> dec(n_bounds, SW_OPEN);
  W->status.assign(n_bounds, 1);              // what stays open to the end (a reference that never closed) is read the old way
  W->summary.assign(n_bounds, strl_span_summary{0, 0.f, 0});
  W->sup_at.assign(n_bounds, 0);
  for (uint32_t k = 0; k < n_bounds; ++k) {
    const strl_bounds &b = bounds[W->order[k]];
    W->bounds[k] = b;
    const int64_t end = (int64_t)b.right + window;
    sb[k] = SweepBound{b.tid, (int32_t)std::min<int64_t>(beg_of(b), INT32_MAX), (int32_t)std::max<int64_t>(INT32_MIN, std::min<int64_t>(end, INT32_MAX)), 0};
    if (b.tid < 0 || b.tid >= n_ref) dec[k] = 1u;   // no such reference in the file: never swept
  }
  STRL_HIP(hipHostMalloc(reinterpret_cast<void **>(&W->h_state), sizeof(SweepState), hipHostMallocDefault));
  STRL_HIP(hipEventCreate(&W->e0));
  STRL_HIP(hipEventCreate(&W->e1));
  if ((rc = W->d_bounds.reserve((size_t)n_bounds * sizeof(SweepBound) + 64)) || (rc = W->d_dec.reserve((size_t)n_bounds * 4 + 64)) ||
      (rc = W->d_out.reserve((size_t)n_bounds * sizeof(SweepDecision) + 64)) || (rc = W->d_state.reserve(sizeof(SweepState))))
    return rc;
  SweepState &H = *W->h_state;
  memset(&H, 0, sizeof H);
  H.err_ord[0] = H.err_ord[1] = ~0ull;
  for (int k = 0; k < 2; ++k) { H.carry[k] = SweepCarry{SW_NO_TID, SW_NO_END}; H.last[k] = SweepLast{SW_NO_TID, -1}; }
  hipStream_t st = c->stream;
  STRL_HIP(hipMemcpyAsync(W->d_state.p, &H, sizeof H, hipMemcpyHostToDevice, st));
  if (n_bounds) {
    STRL_HIP(hipMemcpyAsync(W->d_bounds.p, sb.data(), (size_t)n_bounds * sizeof(SweepBound), hipMemcpyHostToDevice, st));
    STRL_HIP(hipMemcpyAsync(W->d_dec.p, dec.data(), (size_t)n_bounds * 4, hipMemcpyHostToDevice, st));
  }
  STRL_HIP(hipStreamSynchronize(st));
  return STRL_OK;
}

extern "C" int strl_sweep_reserve(strl_ctx *c, uint32_t max_blocks, uint64_t max_comp_bytes) {
  if (!c || !c->sweep || !c->front || !max_blocks) { set_error("strl_sweep_reserve: bad argument / no strl_sweep_begin"); return STRL_ERR_ARG; }
  STRL_HIP(hipSetDevice(c->device));
  strl_sweep *W = c->sweep;
  int rc;
  const uint64_t rec_cap = (uint64_t)max_blocks * 65280u / 36 + 16;      // no record is shorter than 36 bytes (front_reserve's bound)
  if ((rc = W->d_tid.reserve((size_t)rec_cap * 4 + 64)) || (rc = W->d_pos.reserve((size_t)rec_cap * 4 + 64)) || (rc = W->d_pmax.reserve((size_t)rec_cap * 4 + 64)) ||
      (rc = W->d_tile.reserve((size_t)(rec_cap / SW_THREADS + 2) * sizeof(SweepCarry) + 64)))
    return rc;
  return front_reserve(c, c->front, max_blocks, max_comp_bytes);
}

extern "C" int strl_sweep_push(strl_ctx *c, const uint8_t *comp, uint64_t comp_bytes, const uint64_t *coff, const uint32_t *clen, const uint32_t *isize,
                               const uint32_t *crc32, uint32_t n_blocks, int last_chunk) {
  if (!c || !c->sweep || !c->front || (n_blocks && (c->sweep->last_pushed || !comp || !coff || !clen || !isize)) || (!n_blocks && !last_chunk)) {
    set_error("strl_sweep_push: bad argument / no strl_sweep_begin / a chunk behind the last one");
    return STRL_ERR_ARG;
  }
  if (!n_blocks) { c->sweep->last_pushed = true; return STRL_OK; }      // the chunk pushed before was the file's last
  STRL_HIP(hipSetDevice(c->device));
  strl_front *F = c->front;
  strl_sweep *W = c->sweep;
  if (W->fail_rc) { set_error("%s", W->fail.c_str()); return W->fail_rc; }
  const int si = (int)(W->chunks & 1);
  FrontSlot &S = F->slot[si];
  int rc;
  if (S.b_pending) { STRL_HIP(hipEventSynchronize(S.ev_b)); S.b_pending = false; }     // the chunk two back has left the slot
  const FrontChunkDesc d{comp, comp_bytes, coff, clen, isize, crc32, n_blocks};
  if ((rc = front_stage_a(c, F, si, d, W->chunks == 0))) return sweep_fail(W, rc);
  ++W->chunks;
  W->last_pushed = last_chunk != 0;
  // ... and beside this chunk's inflate, the sweep of the previous one
  while (W->done + 1 < W->chunks) {
    if ((rc = sweep_chunk(c, F, W, (int)(W->done & 1), false))) return sweep_fail(W, rc);
    ++W->done;
  }
  return STRL_OK;
}

extern "C" int strl_sweep_finish(strl_ctx *c, strl_support *out, uint64_t cap, uint64_t *support_off, strl_span_summary *summary, uint8_t *status,
                                 strl_sweep_info *info) {
  if (!c || !c->sweep || !c->front || (cap && !out)) { set_error("strl_sweep_finish without strl_sweep_begin"); return STRL_ERR_ARG; }
  strl_sweep *W = c->sweep;
  if (W->nb && (!support_off || !summary || !status)) { set_error("null argument"); return STRL_ERR_ARG; }
  STRL_HIP(hipSetDevice(c->device));
  if (W->fail_rc) { set_error("%s", W->fail.c_str()); return W->fail_rc; }
  int rc;
  for (; W->done < W->chunks; ++W->done)
    if ((rc = sweep_chunk(c, c->front, W, (int)(W->done & 1), W->last_pushed && W->done + 1 == W->chunks))) return sweep_fail(W, rc);
  STRL_HIP(hipStreamSynchronize(c->stream));
  // the caller's order
  std::vector<uint32_t> at(W->nb);
  for (uint32_t k = 0; k < W->nb; ++k) at[W->order[k]] = k;
  uint64_t total = 0, n_st[3] = {0, 0, 0};
  for (uint32_t r = 0; r < W->nb; ++r) {
    const uint32_t k = at[r];
    const uint8_t s = W->status[k];
    status[r] = s; ++n_st[s < 3 ? s : 2];
    summary[r] = s ? strl_span_summary{0, 0.f, 0} : W->summary[k];
    support_off[r] = total;
    const uint64_t ns = s ? 0 : W->summary[k].n_support;
    if (ns && total + ns <= cap) memcpy(out + total, W->sup.data() + W->sup_at[k], (size_t)ns * sizeof(strl_support));
    total += ns;
  }
  if (support_off) support_off[W->nb] = total;
  if (info) {
    info->n_answered = n_st[0]; info->n_seam = n_st[1]; info->n_passed_on = n_st[2];
    info->n_chunks = W->chunks; info->n_records = W->n_records;
    info->sweep_ms = W->ms_sweep; info->evidence_ms = W->ms_evidence;
  }
  if (total > cap) { set_error("support capacity %llu too small, need %llu", (unsigned long long)cap, (unsigned long long)total); return STRL_ERR_CAPACITY; }
  return STRL_OK;
}

extern "C" int strl_sweep_end(strl_ctx *c) {
  if (!c) { set_error("null argument"); return STRL_ERR_ARG; }
  STRL_HIP(hipSetDevice(c->device));
  if (c->front) {
    for (hipStream_t q : c->front->st_i) if (q) (void)hipStreamSynchronize(q);
    if (c->front->st_a) (void)hipStreamSynchronize(c->front->st_a);
    if (c->front->st_c) (void)hipStreamSynchronize(c->front->st_c);
  }
  STRL_HIP(hipStreamSynchronize(c->stream));
  if (c->sweep) { sweep_destroy(c->sweep); c->sweep = nullptr; }
  return STRL_OK;
}
