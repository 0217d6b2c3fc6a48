// assign_core.h -- the bodies of the kernels of strl_assign_reads_loci_device (assign.hip): given loci take their reads
// (assign_reads_locus, callclusters.nim:14-50, for every locus in the caller's order).
//
// The rule.  Per locus j, in the caller's order, over the group of treads with the locus' tid and the same six repeat bytes;
// treads that arrive with split == STRL_SOFT_TAKEN and, in STRL_MODE_MERGE, treads with tid < 0 are in no group.  The group is
// sorted stably by position (uint32 order, ties in input order).  A tread is alive until a locus takes or loses it.
//   lo = left_most == 0 ? 0 : left_most - 1,  hi = max(lo, (uint64)right_most + 1)
//   alive treads with lo <= position < hi are ASSIGNED to j in sorted order and counted (n_total, n_left, n_right);
//   the first alive tread with position >= hi, if any, is LOST: it dies without a locus, also when nothing was assigned
//   (the reference's trs[ri], :34-36, with the ri < li clamp).
// p0 = lower_bound(lo) and p1 = lower_bound(hi) in the group's sorted array do not depend on what is alive, so only the taking
// is sequential, and only inside a group:
//   as_check_body    one lane per tread: its unit and tid are checked, the largest tid sizes the sort key
//   as_keys_body     one lane per tread: (group key, position) with cluster.hip's key layout; treads in no group get a key behind all
//   as_gather_body   one lane per sorted entry: group key, position and split in sorted order; every entry alive
//   as_lkeys_body    one lane per locus: its group key (a stable sort by it keeps the caller's order inside a group)
//   as_ranges_body   one lane per locus: p0, p1 and the end of the group by binary search; counts reset
//   as_take_body     one wave per group with loci: walks the group's loci in order; lanes stride over [p0, p1) and own what is
//                    alive, a wave sum gives the counts, then the wave looks from p1 on for the first alive entry and loses it.
//                    A barrier stands between one locus and the next: what a lane marked is read by other lanes then.
//   as_scan_body     one workgroup: exclusive sum of the counts in the caller's order = assigned_off
//   as_fill_body     one wave per locus: the entries of [p0, p1) it owns, compacted in order by ballot and prefix
//   as_marks_body    one lane per sorted entry: taken and lost treads get split = STRL_SOFT_TAKEN, and a byte in the mark column
// Integer work only; no result depends on the order in which lanes or waves arrive (every entry has one writer per launch).
// The same source compiles for the host (STRL_EMU: a wave is 64 threads and a barrier, tests/emu/assign_emu.cpp).
#pragma once
#include <stdint.h>
#include "../../include/strling_amd.h"

#ifdef STRL_EMU
#define AS_FN inline
#else
#define AS_FN __device__ __forceinline__
#endif

namespace strl {

constexpr uint32_t AS_WAVE = 64;
constexpr uint32_t AS_ALIVE = 0xffffffffu, AS_LOST = 0xfffffffeu;   // AsParams::owner[]; any other value: the locus that took the entry
constexpr uint32_t AS_E_UNIT = 1u, AS_E_TID = 2u;
constexpr uint32_t AS_SCAN_MAX = 1024;                               // lanes of the scan's workgroup at most

struct AsLocus { int32_t tid; uint32_t left_most, right_most; char rep[8]; };   // what the device needs of a strl_locus
struct AsStat { uint32_t err; int32_t max_tid; uint32_t n_groups, n_lost; };

struct AsParams {
  strl_tread *treads;         // [n] input order; as_marks_body writes split
  uint32_t n;
  int32_t mode;
  const AsLocus *loci;        // [n_loci] the caller's order
  uint32_t n_loci;
  int32_t max_tid;            // largest tid of a tread (-1: none placed)
  int32_t composite;          // 1: key = group key << 32 | position, one sort; 0: key = position, then a second sort by gk_in
  uint64_t excl;              // group key of what is in no group: behind every key a tread with tid <= max_tid can have
  uint64_t *key;              // [n] keys stage: what the sort reads
  uint32_t *val;              // [n]
  uint64_t *gk_in;            // [n] (two sorts only) group key by input index
  const uint64_t *skey;       // [n] sorted
  const uint32_t *sval;       // [n] sorted entry -> input index
  uint64_t *s_g;              // [n] group key, sorted order
  uint32_t *s_pos;            // [n]
  uint8_t *s_split;           // [n]
  uint32_t *owner;            // [n]
  uint64_t *lkey;             // [n_loci] keys of the loci: what their sort reads
  uint32_t *lval;
  const uint64_t *slkey;      // [n_loci] sorted by group key, the caller's order inside a group
  const uint32_t *slval;
  uint32_t *p0, *p1, *ge;     // [n_loci] by locus
  uint32_t *cnt;              // [3][n_loci] reads assigned, of them STRL_SOFT_LEFT, STRL_SOFT_RIGHT
  uint64_t *off;              // [n_loci + 1]
  uint32_t *assigned;         // [n] (a tread is assigned once at most)
  uint8_t *mark;              // [n] by input index: 1 = taken or lost in this call
  AsStat *stat;
};

#ifdef STRL_EMU
struct AsShared { uint32_t v[AS_WAVE]; };
struct AsWave {               // a lane's view of its wave on the host
  uint32_t lane;
  AsShared *sh;
  void *barrier;
  void (*wait)(void *);
  void sync() const { wait(barrier); }
  uint64_t ballot(bool p) const {
    sh->v[lane] = p ? 1u : 0u;
    sync();
    uint64_t m = 0;
    for (uint32_t i = 0; i < AS_WAVE; ++i) m |= (uint64_t)sh->v[i] << i;
    sync();
    return m;
  }
  uint32_t sum(uint32_t x) const {
    sh->v[lane] = x;
    sync();
    uint32_t s = 0;
    for (uint32_t i = 0; i < AS_WAVE; ++i) s += sh->v[i];
    sync();
    return s;
  }
};
struct AsBlock {
  uint32_t t, nt;
  void *barrier;
  void (*wait)(void *);
  void sync() const { wait(barrier); }
};
inline void as_atomic_add(uint32_t *p, uint32_t v) { __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }
inline uint32_t as_popc(uint64_t m) { return (uint32_t)__builtin_popcountll(m); }
inline uint32_t as_ctz(uint64_t m) { return (uint32_t)__builtin_ctzll(m); }
#else
struct AsWave {
  uint32_t lane;
  __device__ void sync() const { __syncthreads(); }          // the workgroup is this one wave
  __device__ uint64_t ballot(bool p) const { return __ballot(p); }
  __device__ uint32_t sum(uint32_t x) const {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) x += __shfl_xor(x, d);
    return x;
  }
};
struct AsBlock {
  uint32_t t, nt;
  __device__ void sync() const { __syncthreads(); }
};
__device__ __forceinline__ void as_atomic_add(uint32_t *p, uint32_t v) { atomicAdd(p, v); }
__device__ __forceinline__ uint32_t as_popc(uint64_t m) { return (uint32_t)__popcll(m); }
__device__ __forceinline__ uint32_t as_ctz(uint64_t m) { return (uint32_t)(__ffsll((unsigned long long)m) - 1); }
#endif

// len << 12 | code of a unit (cluster.hip tread_keys_kernel); strict: [0, 6) NUL-padded, else the first NUL ends it
AS_FN uint32_t as_unit_key(const char *rep, bool strict, bool &ok) {
  uint32_t len = 0, code = 0;
  bool ended = false;
  for (int j = 0; j < 6; ++j) {
    const char ch = rep[j];
    if (ch == 0) { if (!strict) break; ended = true; continue; }
    if (ended) { ok = false; continue; }
    uint32_t cd = 0;
    switch (ch) { case 'C': cd = 0; break; case 'A': cd = 1; break; case 'T': cd = 2; break; case 'G': cd = 3; break; default: ok = false; }
    code = (code << 2) | cd;
    ++len;
  }
  return (len << 12) | code;
}

AS_FN uint64_t as_group_key(int32_t tid, uint32_t unit_key) { return ((uint64_t)(uint32_t)(tid + 1) << 15) | unit_key; }

AS_FN bool as_in_group(const AsParams &P, const strl_tread &t) {
  return t.split != STRL_SOFT_TAKEN && !(P.mode == STRL_MODE_MERGE && t.tid < 0);
}

// -> the tread's tid; err: AS_E_* of it
AS_FN int32_t as_check_body(const AsParams &P, uint32_t i, uint32_t &err) {
  const strl_tread &t = P.treads[i];
  bool ok = true;
  (void)as_unit_key(t.repeat, true, ok);
  if (!ok) err |= AS_E_UNIT;
  if (t.tid < -1) err |= AS_E_TID;
  return t.tid;
}

AS_FN void as_keys_body(const AsParams &P, uint32_t i) {
  const strl_tread &t = P.treads[i];
  bool ok = true;
  const uint64_t g = as_in_group(P, t) ? as_group_key(t.tid, as_unit_key(t.repeat, true, ok)) : P.excl;
  P.val[i] = i;
  if (P.composite) P.key[i] = (g << 32) | t.position;
  else { P.key[i] = t.position; P.gk_in[i] = g; }
}

AS_FN void as_gather_body(const AsParams &P, uint32_t i) {
  const uint32_t src = P.sval[i];
  const uint64_t k = P.skey[i];
  P.s_g[i] = P.composite ? k >> 32 : k;
  P.s_pos[i] = P.composite ? (uint32_t)k : P.treads[src].position;
  P.s_split[i] = P.treads[src].split;
  P.owner[i] = AS_ALIVE;
}

AS_FN void as_lkeys_body(const AsParams &P, uint32_t j) {
  const AsLocus &L = P.loci[j];
  bool ok = L.tid >= -1 && L.tid <= P.max_tid && !(P.mode == STRL_MODE_MERGE && L.tid < 0);
  const uint32_t u = as_unit_key(L.rep, false, ok);
  P.lkey[j] = ok ? as_group_key(L.tid, u) : P.excl;
  P.lval[j] = j;
}

// the first sorted entry that is not in front of (g, pos); pos may be 2^32
AS_FN uint32_t as_lower_bound(const AsParams &P, uint64_t g, uint64_t pos) {
  uint32_t lo = 0, hi = P.n;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    const uint64_t mg = P.s_g[mid];
    if (mg < g || (mg == g && (uint64_t)P.s_pos[mid] < pos)) lo = mid + 1u; else hi = mid;
  }
  return lo;
}

AS_FN void as_ranges_body(const AsParams &P, uint32_t k) {
  const uint32_t j = P.slval[k];
  const uint64_t g = P.slkey[k];
  uint32_t p0 = 0, p1 = 0, ge = 0;
  if (g != P.excl) {
    const AsLocus &L = P.loci[j];
    const uint64_t lo = L.left_most == 0 ? 0u : L.left_most - 1u;
    const uint64_t up = (uint64_t)L.right_most + 1u, hi = up < lo ? lo : up;
    p0 = as_lower_bound(P, g, lo);
    p1 = as_lower_bound(P, g, hi);
    ge = as_lower_bound(P, g + 1u, 0);
  }
  P.p0[j] = p0; P.p1[j] = p1; P.ge[j] = ge;
  P.cnt[j] = 0; P.cnt[P.n_loci + j] = 0; P.cnt[2u * P.n_loci + j] = 0;
}

// k: a sorted locus, the same for the whole wave; only the wave at the first locus of a group works
AS_FN void as_take_body(const AsWave &W, const AsParams &P, uint32_t k) {
  const uint64_t g = P.slkey[k];
  if (g == P.excl || (k && P.slkey[k - 1u] == g)) return;
  const uint32_t ge0 = P.ge[P.slval[k]];
  if (ge0 == 0 || P.s_g[ge0 - 1u] != g) return;                       // no tread in the group: every range is empty
  uint32_t n_lost = 0;
  for (uint32_t kk = k; kk < P.n_loci && P.slkey[kk] == g; ++kk) {
    const uint32_t j = P.slval[kk];
    const uint32_t p0 = P.p0[j], p1 = P.p1[j], ge = P.ge[j];
    uint32_t c = 0, l = 0, r = 0;
    for (uint32_t i = p0 + W.lane; i < p1; i += AS_WAVE) {
      if (P.owner[i] != AS_ALIVE) continue;
      P.owner[i] = j;
      const uint8_t s = P.s_split[i];
      ++c; l += s == STRL_SOFT_LEFT ? 1u : 0u; r += s == STRL_SOFT_RIGHT ? 1u : 0u;
    }
    c = W.sum(c); l = W.sum(l); r = W.sum(r);
    if (W.lane == 0) { P.cnt[j] = c; P.cnt[P.n_loci + j] = l; P.cnt[2u * P.n_loci + j] = r; }
    for (uint32_t base = p1; base < ge; base += AS_WAVE) {            // (entries behind p1: not written in this round)
      const uint32_t i = base + W.lane;
      const bool alive = i < ge && P.owner[i] == AS_ALIVE;
      const uint64_t m = W.ballot(alive);
      if (m) {
        if (W.lane == as_ctz(m)) P.owner[i] = AS_LOST;
        ++n_lost;
        break;
      }
    }
    W.sync();                                                          // this locus' marks are visible to the lanes of the next
  }
  if (W.lane == 0) { as_atomic_add(&P.stat->n_groups, 1u); if (n_lost) as_atomic_add(&P.stat->n_lost, n_lost); }
}

// one workgroup of B.nt <= AS_SCAN_MAX lanes; every lane owns a run of consecutive loci
AS_FN void as_scan_body(const AsBlock &B, const AsParams &P, uint64_t *sh) {
  const uint32_t n = P.n_loci, per = (n + B.nt - 1u) / B.nt;
  const uint64_t a64 = (uint64_t)B.t * per;
  const uint32_t a = a64 < n ? (uint32_t)a64 : n, b = n - a < per ? n : a + per;
  uint64_t s = 0;
  for (uint32_t k = a; k < b; ++k) s += P.cnt[k];
  sh[B.t] = s;
  B.sync();
  if (B.t == 0) {
    uint64_t run = 0;
    for (uint32_t k = 0; k < B.nt; ++k) { const uint64_t v = sh[k]; sh[k] = run; run += v; }
    P.off[n] = run;
  }
  B.sync();
  uint64_t run = sh[B.t];
  for (uint32_t k = a; k < b; ++k) { P.off[k] = run; run += P.cnt[k]; }
}

AS_FN void as_fill_body(const AsWave &W, const AsParams &P, uint32_t j) {
  if (P.cnt[j] == 0) return;
  const uint32_t p0 = P.p0[j], p1 = P.p1[j];
  uint64_t at = P.off[j];
  for (uint32_t base = p0; base < p1; base += AS_WAVE) {
    const uint32_t i = base + W.lane;
    const bool mine = i < p1 && P.owner[i] == j;
    const uint64_t m = W.ballot(mine);
    if (mine) {
      const uint64_t o = at + as_popc(m & (((uint64_t)1 << W.lane) - 1u));
      if (o < P.n) P.assigned[o] = P.sval[i];
    }
    at += as_popc(m);
  }
}

AS_FN void as_marks_body(const AsParams &P, uint32_t i) {
  const uint32_t src = P.sval[i];
  const bool gone = P.owner[i] != AS_ALIVE;
  if (gone) P.treads[src].split = STRL_SOFT_TAKEN;
  P.mark[src] = gone ? 1u : 0u;
}

}  // namespace strl
