// sweep_core.h -- the bodies of the sweep's kernels (sweep.hip): which byte range of a chunk's records answers which bound.
//
// The records of a coordinate-sorted BAM pass by chunk by chunk (the front end's record scan leaves recoff[] of a chunk).  For
// a bound with the query [beg, end) = [max(0, left - window), right + window) on reference tid (collect.nim:133-139):
//   i1 = the first record with tid > b.tid, or tid == b.tid and pos >= end           -- no record from there on overlaps
//   i0 = the first record of b.tid whose running maximum of bam_endpos exceeds beg    -- no record in front of it overlaps
// and every record htslib's iterator returns for the query lies in [i0, i1) (those in between that end at or in front of beg
// are dropped by evidence_kernel's own filter, as the iterator drops them).
//   sweep_keys_body    one lane per record: tid, pos, end (bam_rec_end), the order check against the record in front, and the
//                      segmented running maximum of end inside the 256 records of the workgroup with the tile's aggregate
//   sweep_tiles_body   one workgroup: exclusive segmented scan of the tile aggregates, seeded with the carry (tid, largest end so
//                      far) of the chunks in front; leaves the carry of the next chunk in the state words
//   sweep_ranges_body  one lane per bound still open: two binary searches; a bound is decided in the first chunk that holds its
//                      i1 (or in the file's last chunk), as a range or -- the carry of its reference exceeds beg -- as a seam
// The same source compiles for the host (STRL_EMU: a workgroup is a set of threads and a barrier, tests/emu/sweep_emu.cpp) so
// that the CPU suite runs the rule itself.  No wave intrinsics for that reason: the scans go through LDS.
#pragma once
#include <stdint.h>
#include "bam_rec.h"

#ifdef STRL_EMU
#define SW_FN inline
#else
#define SW_FN __device__ __forceinline__
#endif

namespace strl {

constexpr uint32_t SW_THREADS = 256;
constexpr uint32_t SW_OPEN = 0xffffffffu;          // SweepParams::dec[]: not decided yet
constexpr int32_t SW_NO_TID = -2, SW_NO_END = INT32_MIN;
constexpr uint32_t SW_E_UNSORTED = 0, SW_E_TID = 1;

struct SweepBound { int32_t tid, beg, end, pad; };  // the query of a bound; sorted by (tid, beg)
struct SweepCarry { int32_t tid, max_end; };       // records of `tid` in the chunks so far end at most at max_end
struct SweepLast { int32_t tid, pos; };            // the last record so far
struct SweepState {                                // device words of a sweep
  unsigned long long err_ord[2];                   // ordinal of the first record out of order / with a refID outside the header; ~0 = none
  SweepCarry carry[2];                             // [parity of the chunk]: read from one, written to the other
  SweepLast last[2];
  uint32_t n_dec, pad;                             // bounds decided in the chunk just swept
};
struct SweepDecision { uint32_t bound, i0, i1, status; uint64_t start, stop; };   // bytes [start, stop) of the chunk's buffer; status 0 | 1 (seam)

struct SweepParams {
  const uint8_t *U;           // the chunk's inflated bytes
  const uint32_t *recoff;     // [n] offsets of its complete records
  uint32_t n, rec_end;        // records; the offset behind the last complete one
  unsigned long long ord0;    // ordinal of the chunk's first record
  int32_t n_ref;
  int32_t *tid, *pos, *pmax;  // [n] keys; pmax: running maximum of end inside the tile (sweep_pmax completes it)
  SweepCarry *tile;           // [tiles] aggregate of each tile, then (in place) the exclusive prefix in front of it
  uint32_t n_tiles;
  SweepState *S;
  uint32_t par;
  const SweepBound *bounds;
  uint32_t n_bounds;
  uint32_t *dec;              // [n_bounds] SW_OPEN, or the status the bound was decided with
  SweepDecision *out;         // [n_bounds] the decisions of this chunk, in the order the lanes arrived
  uint32_t last_chunk;
};

struct SweepShared { int32_t tid[SW_THREADS], mx[SW_THREADS]; };

#ifdef STRL_EMU
struct SwGroup {              // a lane's view of its workgroup on the host
  uint32_t t, b;
  void *barrier;
  void (*wait)(void *);
  void sync() const { wait(barrier); }
};
inline void sw_atomic_min64(unsigned long long *p, unsigned long long v) {
  unsigned long long cur = __atomic_load_n(p, __ATOMIC_RELAXED);
  while (v < cur && !__atomic_compare_exchange_n(p, &cur, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
}
inline uint32_t sw_atomic_inc32(uint32_t *p) { return __atomic_fetch_add(p, 1u, __ATOMIC_RELAXED); }
#else
struct SwGroup {
  uint32_t t, b;
  __device__ void sync() const { __syncthreads(); }
};
__device__ __forceinline__ void sw_atomic_min64(unsigned long long *p, unsigned long long v) { atomicMin(p, v); }
__device__ __forceinline__ uint32_t sw_atomic_inc32(uint32_t *p) { return atomicAdd(p, 1u); }
#endif

// the operator of the segmented maximum: b comes behind a
SW_FN SweepCarry sw_join(SweepCarry a, SweepCarry b) {
  if (a.tid == b.tid && a.max_end > b.max_end) b.max_end = a.max_end;
  return b;
}

SW_FN void sweep_keys_body(const SwGroup &G, const SweepParams &P, SweepShared &Sh) {
  const uint32_t t = G.t, i = G.b * SW_THREADS + t;
  const bool act = i < P.n;
  int32_t tid = SW_NO_TID, end = SW_NO_END;
  if (act) {
    const uint8_t *R = P.U + P.recoff[i];
    tid = (int32_t)rec_ld32(R + 4);
    const int32_t pos = (int32_t)rec_ld32(R + 8);
    const int64_t e = bam_rec_end(R);
    end = e > 0x7fffffffll ? 0x7fffffff : (int32_t)e;
    P.tid[i] = tid; P.pos[i] = pos;
    // coordinate order: (tid, pos) does not decrease, tid = -1 only at the end (the index builder's rule)
    SweepLast L;
    if (i == 0) L = P.S->last[P.par];
    else { const uint8_t *Q = P.U + P.recoff[i - 1u]; L.tid = (int32_t)rec_ld32(Q + 4); L.pos = (int32_t)rec_ld32(Q + 8); }
    const uint32_t uc = (uint32_t)tid, up = (uint32_t)L.tid;
    if (L.tid != SW_NO_TID && (uc < up || (uc == up && tid >= 0 && pos < L.pos))) sw_atomic_min64(&P.S->err_ord[SW_E_UNSORTED], P.ord0 + i);
    if (tid < -1 || tid >= P.n_ref) sw_atomic_min64(&P.S->err_ord[SW_E_TID], P.ord0 + i);
    if (i == P.n - 1u) P.S->last[P.par ^ 1u] = SweepLast{tid, pos};
  }
  // inclusive segmented maximum over the tile (lanes behind the chunk's last record come last and reach no one)
  Sh.tid[t] = tid; Sh.mx[t] = end;
  G.sync();
  SweepCarry me{tid, end};
  for (uint32_t d = 1; d < SW_THREADS; d <<= 1) {
    SweepCarry lo{SW_NO_TID, SW_NO_END};
    if (t >= d) lo = SweepCarry{Sh.tid[t - d], Sh.mx[t - d]};
    G.sync();
    if (t >= d) { me = sw_join(lo, me); Sh.mx[t] = me.max_end; }
    G.sync();
  }
  if (act) {
    P.pmax[i] = me.max_end;
    if (t == SW_THREADS - 1u || i == P.n - 1u) P.tile[G.b] = me;
  }
}

// one workgroup; every lane owns a run of consecutive tiles
SW_FN void sweep_tiles_body(const SwGroup &G, const SweepParams &P, SweepShared &Sh) {
  const uint32_t t = G.t, n = P.n_tiles, per = (n + SW_THREADS - 1u) / SW_THREADS;
  const uint32_t a = t * per < n ? t * per : n, b = a + per < n ? a + per : n;
  SweepCarry s{SW_NO_TID, SW_NO_END};
  for (uint32_t k = a; k < b; ++k) s = sw_join(s, P.tile[k]);
  Sh.tid[t] = s.tid; Sh.mx[t] = s.max_end;
  G.sync();
  if (t == 0) {
    SweepCarry run = P.S->carry[P.par];
    for (uint32_t k = 0; k < SW_THREADS; ++k) {
      const SweepCarry v{Sh.tid[k], Sh.mx[k]};
      Sh.tid[k] = run.tid; Sh.mx[k] = run.max_end;
      if (v.tid != SW_NO_TID) run = sw_join(run, v);            // (a lane without tiles leaves the run as it is)
    }
    P.S->carry[P.par ^ 1u] = run;
  }
  G.sync();
  SweepCarry run{Sh.tid[t], Sh.mx[t]};
  for (uint32_t k = a; k < b; ++k) { const SweepCarry v = P.tile[k]; P.tile[k] = run; run = sw_join(run, v); }
}

// running maximum of end over the records of record i's reference up to i, the chunks in front included
SW_FN int32_t sweep_pmax(const SweepParams &P, uint32_t i) {
  const SweepCarry pre = P.tile[i / SW_THREADS];
  const int32_t m = P.pmax[i];
  return pre.tid == P.tid[i] && pre.max_end > m ? pre.max_end : m;
}

SW_FN void sweep_ranges_body(const SwGroup &G, const SweepParams &P) {
  const uint32_t j = G.b * SW_THREADS + G.t;
  if (j >= P.n_bounds || P.dec[j] != SW_OPEN) return;
  const SweepBound B = P.bounds[j];
  const uint32_t ub = (uint32_t)B.tid, n = P.n;
  uint32_t lo = 0, hi = n;                                       // i1
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1), ut = (uint32_t)P.tid[mid];
    if (ut > ub || (ut == ub && P.pos[mid] >= B.end)) hi = mid; else lo = mid + 1u;
  }
  const uint32_t i1 = lo;
  if (i1 == n && !P.last_chunk) return;                          // its end has not passed by: open
  const SweepCarry C = P.S->carry[P.par];                        // what came into this chunk
  const uint32_t status = (C.tid == B.tid && C.max_end > B.beg) ? 1u : 0u;
  lo = 0; hi = i1;                                               // the first record of the bound's reference
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if ((uint32_t)P.tid[mid] >= ub) hi = mid; else lo = mid + 1u;
  }
  hi = i1;                                                       // i0: the running maximum does not decrease inside a reference
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (sweep_pmax(P, mid) > B.beg) hi = mid; else lo = mid + 1u;
  }
  const uint32_t i0 = lo;
  SweepDecision D;
  D.bound = j; D.i0 = i0; D.i1 = i1; D.status = status;
  D.start = i0 < n ? P.recoff[i0] : P.rec_end;
  D.stop = i1 < n ? P.recoff[i1] : P.rec_end;
  P.out[sw_atomic_inc32(&P.S->n_dec)] = D;
  P.dec[j] = status;
}

}  // namespace strl
