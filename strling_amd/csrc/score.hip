// score.hip -- HIP kernels + C-ABI entry points for the extract-side hot path (gfx950).
//
//  classify_kernel : eight reads per lane and iteration, a wave owns a contiguous range of reads; streams the
//                    13 B/read of coordinates + cigar class, evaluates the skip predicate of
//                    extract.nim:30-34 against the genome STR intervals (a wave-level merge join against a
//                    window of {start, running max stop} entries; bin directory + short scan for reads
//                    outside it), writes the "skipped" result word or stages the read for the scoring
//                    queue (one queue atomic per 512 staged reads).  A turn that lies, with the turn behind it, wholly
//                    inside the wave's range is FULL (classify_turn.h): no bounds test, no exec mask on a load or a
//                    store, and the next turn's eight loads stay in flight for the whole turn -- two register sets
//                    swap roles instead of a copy, the wait for the current vectors is a counted one.  The last two
//                    turns of a range, ragged ends and the scalar variant take the GENERAL turn.  Bound by neither
//                    HBM (3.6 TB/s) nor vector issue (profiles/classify).
//  score_kernel<0> : one queued read per lane -> utils.get_repeat on the whole read
//                    (score_core.h), writes the packed result, queues the soft-clipped ends
//                    add_soft (extract.nim:93-106) would look at.  Bound by integer VALU issue (0.75-0.87 of
//                    all issue slots, profiles/r02).
//  score_kernel<1> : one queued soft-clipped end per lane, scored once, evaluated against both
//                    lowered thresholds (extract.nim:207-211 and :241-244).
// Host side: the kernels' launch code, the pass that hands reads of more than STRL_DEVICE_READ_LEN bases to the host twin
// (long_reads_pass), one scoring pass over a batch (score_device, stage_batch), strl_score_reads and strl_index_chrom.  What the
// translation units around it use of this is declared in score.h.
#include <string.h>
#include <algorithm>
#include <thread>
#include <type_traits>
#include <vector>
#include "common.h"
#include "classify_turn.h"
#include "host_score.h"
#include "device_util.h"
#include "score_core.h"
#include "score_tables.h"
#include "score.h"

namespace strl {

// Work items are self-contained 16-byte queue entries, so the scorer never chases metadata pointers:
//   whole read : id = read index            | seq_off | l_seq | clip_l << 16 | clip_r | cig << 16 | mapq << 24
//   segment    : id (read index << 1 | side, or a window index) | seq_off | first base | length
// Stage-B items are 32 bytes: the entry + {slot, best, res0, res1}.
constexpr uint32_t EMPTY = 0xffffffffu;

struct ScoreParams {
  const uint4 *meta;      // optional: strl_read_meta rows (seq_off | l_seq, clip_l | clip_r, cig, mapq | pad): what a queue entry carries of a read
  uint64_t n;
  const int32_t *tid, *pos, *end;
  const uint32_t *seq_off;
  const uint16_t *l_seq, *clip_l, *clip_r;
  const uint8_t *mapq, *cig;
  const uint8_t *seq4;
  const TidInfo *g_tid;
  const int2 *g_iv;         // per tid, sorted by start: {start_i, max stop of the earlier intervals} + sentinel
  const uint2 *g_bins;      // per tid and 4 KiB bin: {#starts below the bin, #starts below the next bin}
  int32_t n_tid;
  const uint16_t *lut;
  const uint32_t *ta;    // stage A's tables (score_core.h TA_*)
  uint32_t *inv_spill;   // [NW][threads of the launch]: Seg::inv of the waves that need it
  const uint64_t *thr;
  uint32_t *whole;
  uint32_t *queue_id;  // [n]      ids of the reads to score (classify -> stage A)
  uint4 *queue;        // [n]      their 16-byte entries (stage A, which gathers them -> compaction kernels)
  uint8_t *soft_flag;  // [n]      per scored read: bit 0 / 1 = its left / right clip has to be scored (add_soft gates)
  uint4 *soft_queue;   // [scap]   compacted soft-clip items
  uint4 *sb_state[2];  // dense hand-over of stage A: {best | EMPTY, res0, res1, -} per item
  uint4 *sb_queue[2];  // compacted stage-B items (2 x uint4 each)
  uint32_t scap;
  uint32_t *counters;  // CNT_* layout
  strl_soft_rec *soft_out;
  uint32_t soft_cap;
  uint32_t min_mapq;
  int32_t seg_row0, seg_row1;   // threshold rows of the segment scorer: (2,3) for soft clips, (1,1) for genome windows
  // pair logic (pair.hip): a whole read with a repeat marks its qname group in the Bloom bitmap; nullptr = no pairing
  const uint64_t *qhash;
  uint32_t *bloom;
  uint32_t bloom_mask;
};

constexpr int LUT_DWORDS = LUT_ENTRIES / 2;
constexpr int LUT_A_DWORDS = TA_WORDS;       // stage A reads its own tables (k <= 4)
constexpr int CL_STAGE = 512;    // queue entries a wave stages in LDS before one bulk append (16 KB per block: 8 blocks per CU)
constexpr int CL_ILP = 8;        // reads per lane per iteration (independent lookup chains in flight)

// extract.nim:30-34: single-M cigar, chromosome in the table, no interval overlapping [start, stop)
// The predicate for N independent reads of one lane, written as straight-line PHASES (all directory loads, then all
// bin loads, then all interval loads) so that the N lookup chains are in flight together: N separately inlined
// while-loops serialise their chains, and the kernel is bound by exactly that latency.
// One read against the table, the general way: bin directory, then a short scan inside the bin.  Out of line on purpose:
// it serves the rare wave iteration the merge join below cannot (a contig boundary, unsorted input, a very dense
// stretch), and inlining N copies of its three dependent loads costs the common path ~90 VGPRs (a wave less per SIMD).
__device__ __noinline__ bool skip_one(const TidInfo *g_tid, const uint2 *g_bins, const int2 *g_iv, int32_t t, int32_t start, int32_t stop) {
  const TidInfo ti = g_tid[t];
  if (!ti.has) return false;
  const int32_t b = stop > 0 ? (stop >> BIN_SHIFT) : 0;
  int32_t idx = ti.n_iv;                 // idx = number of intervals with iv.start < stop
  if (b < ti.n_bins) idx = (int32_t)g_bins[ti.bin_off + b].x;
  int2 c = g_iv[ti.iv_off + idx];
  while (c.x < stop) {                   // a start inside the bin below `stop`: rare, and the sentinel ends it
    ++idx;
    c = g_iv[ti.iv_off + idx];
  }
  return !(c.y > start);                 // c.y = longest reach of the intervals starting before `stop`
}

// The merge join's wave-uniform state, carried ACROSS the iterations of a wave: the contig entry and a window of WIN
// consecutive {start, running max stop} entries.  Consecutive iterations of a coordinate-sorted wave advance a few
// kilobases, a window spans tens of kilobases: most iterations reuse it and issue no table load at all.
constexpr int JOIN_WIN = 8;
struct JoinState {
  int32_t t;              // contig the entry / window belong to (-2: none yet)
  int32_t lo;             // every table entry before the window starts below `lo`
  int32_t valid;
  TidInfo tu;
  int2 e[JOIN_WIN];
};

// ALL_IN: every one of the N reads exists (a full turn, classify_turn.h): `in` is not looked at.  n_tid: max(P.n_tid, 0).
template <int N, bool ALL_IN>
__device__ __forceinline__ void skip_predicate_n(const ScoreParams &P, JoinState &J, uint32_t n_tid, const uint32_t (&cg)[N], const int32_t (&t)[N],
                                                 const int32_t (&start)[N], const int32_t (&stop)[N], const bool (&in)[N], bool (&skip)[N]) {
  bool cand[N];
  bool any = false;
#pragma unroll
  for (int j = 0; j < N; ++j) {
    // one unsigned compare for 0 <= t < n_tid, and no short circuit: a branch per read put a wait for every load in flight
    // (the next turn's prefetch included) in front of each of the N tests
    cand[j] = (ALL_IN | in[j]) & ((cg[j] & STRL_CIG_SINGLE_M) != 0) & ((uint32_t)t[j] < n_tid);
    any |= cand[j];
  }
  // lapper.find(start, stop) <=> any interval with iv.start < stop and iv.stop > start.
  // With idx = number of intervals with iv.start < stop, that is: (max stop of intervals 0 .. idx-1) > start = g_iv[idx].y.
  //
  // Merge join.  The reads of a wave iteration are consecutive records of a coordinate-sorted file: they sit on ONE
  // contig within a few kilobases, and only a handful of intervals START inside that span.  So the wave looks the span
  // up ONCE -- contig entry, bin directory, then a window of JOIN_WIN consecutive {start, running max stop} entries, all
  // at wave-uniform addresses -- and every read finds its idx by comparing its stop with the window's starts in
  // registers: no per-lane dependent global loads at all.
  int32_t t0 = 0;
#pragma unroll
  for (int j = N - 1; j >= 0; --j) if (cand[j]) t0 = t[j];
  t0 = __builtin_amdgcn_readfirstlane(any ? t0 : __builtin_amdgcn_readfirstlane(0));
  bool same = true;
#pragma unroll
  for (int j = 0; j < N; ++j) same = same && (!cand[j] || t[j] == t0);
  if (!__any(any)) {
#pragma unroll
    for (int j = 0; j < N; ++j) skip[j] = false;
    return;
  }
  constexpr int WIN = JOIN_WIN;
  if (__all(same)) {
    if (t0 != J.t) {
      J.tu = P.g_tid[__builtin_amdgcn_readfirstlane(t0 < 0 ? 0 : (t0 < P.n_tid ? t0 : 0))];
      J.t = t0;
      J.valid = 0;
    }
    const TidInfo &tu = J.tu;
    int32_t smin = INT32_MAX, smax = INT32_MIN;
#pragma unroll
    for (int j = 0; j < N; ++j) {
      cand[j] = cand[j] && tu.has;
      if (cand[j]) { smin = stop[j] < smin ? stop[j] : smin; smax = stop[j] > smax ? stop[j] : smax; }
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int32_t a = __shfl_xor(smin, d), b = __shfl_xor(smax, d);
      smin = a < smin ? a : smin;
      smax = b > smax ? b : smax;
    }
    smin = __builtin_amdgcn_readfirstlane(smin);
    smax = __builtin_amdgcn_readfirstlane(smax);
    if (smin > smax) {          // no candidate in the wave
#pragma unroll
      for (int j = 0; j < N; ++j) skip[j] = false;
      return;
    }
    if (!(J.valid && smin >= J.lo && J.e[WIN - 1].x >= smax)) {          // (re)load the window at the bin of the smallest stop
      const int32_t b0 = smin > 0 ? (smin >> BIN_SHIFT) : 0;
      int32_t i0 = tu.n_iv;
      if (b0 < tu.n_bins) i0 = (int32_t)P.g_bins[tu.bin_off + b0].x;    // # starts below the bin: <= idx(smin)
      i0 = __builtin_amdgcn_readfirstlane(i0);
      const int2 *w = P.g_iv + tu.iv_off + i0;
      const int32_t rem = tu.n_iv - i0;                                  // entries i0 .. n_iv exist (n_iv = the sentinel)
#pragma unroll
      for (int q = 0; q < WIN; ++q) {
        const int2 v = w[q < rem ? q : rem];
        J.e[q].x = __builtin_amdgcn_readfirstlane(v.x);
        J.e[q].y = __builtin_amdgcn_readfirstlane(v.y);
      }
      J.lo = b0 << BIN_SHIFT;                                            // (past the last bin every start lies below it, too)
      J.valid = 1;
    }
    if (J.e[WIN - 1].x >= smax) {                                        // the window holds every start below the largest stop
#pragma unroll
      for (int j = 0; j < N; ++j) {
        int32_t pm = J.e[0].y;
#pragma unroll
        for (int q = 0; q + 1 < WIN; ++q) pm = J.e[q].x < stop[j] ? J.e[q + 1].y : pm;   // starts ascend: the last true one decides
        skip[j] = cand[j] & !(pm > start[j]);
      }
      return;
    }
  }
#pragma unroll
  for (int j = 0; j < N; ++j) skip[j] = cand[j] && skip_one(P.g_tid, P.g_bins, P.g_iv, t[j], start[j], stop[j]);
}

// VEC: a lane owns 4 consecutive reads per group and fetches their coordinates with 16-byte loads (needs 16-byte aligned
// arrays; the host picks the scalar variant otherwise).
template <bool VEC>
__global__ __launch_bounds__(256, 4) void classify_kernel(ScoreParams P) {
  // Each wave owns one contiguous range of reads.  Kept read indices are staged in LDS; a flush reserves queue
  // space with ONE global atomic (one same-address atomic per wave-iteration ran into the ~88 ops/us limit of
  // the L2 atomic unit: 12 ms per 2^25 reads) and gathers the reads' metadata into self-contained 16-byte items.
  __shared__ uint32_t stage[4][CL_STAGE + 64 * CL_ILP];
  static_assert(CL_ILP == (int)CT_ILP, "classify_turn.h restates the turn");
  // the wave index in a scalar register: the range and every test on it (a full turn?) are scalar arithmetic
  const int lane0 = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  uint32_t *buf = stage[wave];
  const uint64_t n_waves = (uint64_t)gridDim.x * 4u;
  const uint64_t gw = (uint64_t)blockIdx.x * 4u + wave;
  const uint64_t per = (((P.n + n_waves - 1) / n_waves) + 255ull) & ~255ull;
  const ClassifyRange R = classify_range(P.n, per, gw);
  if (!classify_owns(R)) return;            // a wave without a read: before its first load (the kernel has no block-wide barrier)
  const uint64_t r0 = R.r0, r1 = R.r1;
  const uint32_t len = classify_len(R);
  uint32_t cnt = 0, nskip = 0;
  // read handled by this lane as sub-item j of the iteration starting at `base`
  auto ridx = [&](uint64_t base, int j, int lane) -> uint64_t {
    return VEC ? base + 256ull * (uint64_t)(j >> 2) + 4ull * (uint64_t)lane + (uint64_t)(j & 3) : base + 64ull * (uint64_t)j + (uint64_t)lane;
  };
  auto flush = [&]() {
    if (cnt) {
      uint32_t b = 0;
      if (lane0 == 0) b = atomicAdd(&P.counters[CNT_QUEUE], cnt);
      b = __shfl(b, 0);
      __builtin_amdgcn_wave_barrier();
      // Only the ids leave this kernel: it is the one launch of the step that HBM bounds, and gathering the kept reads' rows
      // here (8.5 % of the reads: three quarters of every 64-byte line fetched for nothing) was 160 MB of its 800 MB.
      // Stage A of the scorer, which integer issue bounds, gathers them beside its arithmetic and writes the entries.
      for (uint32_t i = lane0; i < cnt; i += 64) P.queue_id[b + i] = buf[i];
      __builtin_amdgcn_wave_barrier();
      cnt = 0;
    }
  };
  // What a load leaves in registers is the RAW vector (for VEC: a group of 4 consecutive reads), unpacked only when the
  // iteration that consumes it starts: unpacking at load time (byte extraction of the cigar classes) put an s_waitcnt
  // right behind the loads and serialised every prefetch with its own latency.
  struct In { int4 t, s, e; uint32_t c; };                    // VEC: 4 reads; scalar variant: .x / low byte only
  constexpr int NIN = VEC ? CL_ILP / 4 : CL_ILP;
  auto load = [&](uint64_t base, int lane, In (&x)[NIN]) {
    if (VEC) {
#pragma unroll
      for (int gq = 0; gq < NIN; ++gq) {
        const uint64_t r = base + 256ull * gq + 4ull * lane;
        if (r + 3 < r1) {
          x[gq].t = reinterpret_cast<const int4 *>(P.tid)[r >> 2];
          x[gq].s = reinterpret_cast<const int4 *>(P.pos)[r >> 2];
          x[gq].e = reinterpret_cast<const int4 *>(P.end)[r >> 2];
          x[gq].c = reinterpret_cast<const uint32_t *>(P.cig)[r >> 2];
        } else {                                               // the ragged end of the wave's range
          int32_t t[4], st[4], en[4];
          uint32_t cg = 0;
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const bool in = r + q < r1;
            cg |= (in ? (uint32_t)P.cig[r + q] : 0u) << (8 * q);
            t[q] = in ? P.tid[r + q] : -1; st[q] = in ? P.pos[r + q] : 0; en[q] = in ? P.end[r + q] : 0;
          }
          x[gq].t = make_int4(t[0], t[1], t[2], t[3]); x[gq].s = make_int4(st[0], st[1], st[2], st[3]);
          x[gq].e = make_int4(en[0], en[1], en[2], en[3]); x[gq].c = cg;
        }
      }
    } else {
#pragma unroll
      for (int j = 0; j < NIN; ++j) {
        const uint64_t r = base + 64 * j + lane;
        const bool in = r < r1;
        x[j].c = in ? P.cig[r] : 0u;
        x[j].t.x = in ? P.tid[r] : -1;
        x[j].s.x = in ? P.pos[r] : 0;
        x[j].e.x = in ? P.end[r] : 0;
      }
    }
  };
  auto comp = [](const int4 &v, int q) -> int32_t { return q == 0 ? v.x : q == 1 ? v.y : q == 2 ? v.z : v.w; };
  // The vectors of a turn that lies wholly inside the range (classify_turn.h; vector variant only): no bounds test, no exec
  // mask, a scalar base + the lane's 32-bit byte offset + an immediate per group.
  // (the turn's offset goes into the scalar base, classify_group_off(0, lane, gq) is the lane's part: reads, i.e. bytes of the
  // cigar column and a quarter of the bytes of a 4-byte column)
  auto load_full = [&](uint32_t off, int lane, In (&x)[NIN]) {
    const char *pt = reinterpret_cast<const char *>(P.tid + r0 + off), *ps = reinterpret_cast<const char *>(P.pos + r0 + off);
    const char *pe = reinterpret_cast<const char *>(P.end + r0 + off), *pc = reinterpret_cast<const char *>(P.cig + r0 + off);
#pragma unroll
    for (int gq = 0; gq < NIN; ++gq) {
      const uint32_t g = classify_group_off(0u, (uint32_t)lane, (uint32_t)gq);
      x[gq].t = *reinterpret_cast<const int4 *>(pt + 4u * g);
      x[gq].s = *reinterpret_cast<const int4 *>(ps + 4u * g);
      x[gq].e = *reinterpret_cast<const int4 *>(pe + 4u * g);
      x[gq].c = *reinterpret_cast<const uint32_t *>(pc + g);
    }
  };
  JoinState join;
  join.t = -2; join.valid = 0; join.lo = 0;
  // One turn: the reads of `cur`, while `nxt` is requested.  FULL (std::true_type): this turn and the next lie wholly inside the
  // range, wave-uniformly; nothing in it is loaded, tested or stored under an exec mask, and the next turn's eight loads, issued
  // first, stay in flight through the predicate, the ballots, the staging and the stores: what waits for `cur` is a counted
  // wait (vmcnt(8) in one copy of the turn, vmcnt(10) in the other) that leaves them outstanding.  The general turn is the loop body as it always was.
  auto turn = [&](auto full_c, uint64_t base, In (&cur)[NIN], In (&nxt)[NIN]) {
    constexpr bool FULL = decltype(full_c)::value;
    const uint32_t off = (uint32_t)(base - r0);
    // The lane index anew in every turn: what derives from it alone (byte offsets, the general turn's 64-bit addresses) is
    // invariant, was hoisted out of the loop for all four copies of the turn at once, and spilled.
    int lane = lane0;
    asm volatile("" : "+v"(lane));
    if constexpr (FULL) load_full(off + CT_TURN, lane, nxt);
    else load(base + 64 * CL_ILP, lane, nxt);   // next iteration's streaming loads fly while this one chases the interval table
    __builtin_amdgcn_sched_barrier(0);    // the loads stay in front of everything that waits for `cur`
    uint32_t n_tid_u = (uint32_t)(P.n_tid > 0 ? P.n_tid : 0);
    if constexpr (FULL) {
      // `cur` is first looked at HERE: without this, what the two kinds of turn do alike with it (the first compares, the cigar
      // bytes) is hoisted above their common branch, in front of the loads, with a wait for everything outstanding
      // (the cigar words themselves, and the table size the contig ids are compared with: enough to make the first uses differ)
#pragma unroll
      for (int gq = 0; gq < NIN; ++gq) asm volatile("" : "+v"(cur[gq].c));
      asm volatile("" : "+s"(n_tid_u));
      __builtin_amdgcn_sched_barrier(0);
    }
    bool need[CL_ILP], skipped[CL_ILP], inr[CL_ILP];
    uint32_t cgs[CL_ILP];
    int32_t ts[CL_ILP], sts[CL_ILP], ens[CL_ILP];
#pragma unroll
    for (int j = 0; j < CL_ILP; ++j) {
      inr[j] = FULL || ridx(base, j, lane) < r1;
      if (VEC) {
        const In &g4 = cur[j >> 2];
        cgs[j] = (g4.c >> (8 * (j & 3))) & 0xffu; ts[j] = comp(g4.t, j & 3); sts[j] = comp(g4.s, j & 3); ens[j] = comp(g4.e, j & 3);
      } else {
        cgs[j] = cur[j].c; ts[j] = cur[j].t.x; sts[j] = cur[j].s.x; ens[j] = cur[j].e.x;
      }
    }
    skip_predicate_n<CL_ILP, FULL>(P, join, n_tid_u, cgs, ts, sts, ens, inr, skipped);
#pragma unroll
    for (int j = 0; j < CL_ILP; ++j) {
      need[j] = inr[j] && !skipped[j];
      if (!VEC && skipped[j]) P.whole[ridx(base, j, lane)] = STRL_RES_SKIPPED;
    }
    if (VEC) {   // one 16-byte store per group; kept reads get 0 here and their real word from the scorer later
#pragma unroll
      for (int gq = 0; gq < CL_ILP / 4; ++gq) {
        const uint4 w4 = make_uint4(skipped[4 * gq] ? STRL_RES_SKIPPED : 0u, skipped[4 * gq + 1] ? STRL_RES_SKIPPED : 0u,
                                    skipped[4 * gq + 2] ? STRL_RES_SKIPPED : 0u, skipped[4 * gq + 3] ? STRL_RES_SKIPPED : 0u);
        if constexpr (FULL) {
          *reinterpret_cast<uint4 *>(reinterpret_cast<char *>(P.whole + r0 + off) + 4u * classify_group_off(0u, (uint32_t)lane, (uint32_t)gq)) = w4;
        } else {
          const uint64_t r = base + 256ull * gq + 4ull * lane;
          if (r + 3 < r1) {
            reinterpret_cast<uint4 *>(P.whole)[r >> 2] = w4;
          } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) if (skipped[4 * gq + q]) P.whole[r + q] = STRL_RES_SKIPPED;
          }
        }
      }
    }
#pragma unroll
    for (int j = 0; j < CL_ILP; ++j) {
      const unsigned long long m = __ballot(need[j]);
      nskip += (uint32_t)__popcll(__ballot(skipped[j]));
      // (the lanes below this one that keep their read: mbcnt, two instructions)
      const uint32_t slot = cnt + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
      if (need[j]) buf[slot] = FULL ? (uint32_t)r0 + classify_read_off(off, (uint32_t)lane, (uint32_t)j) : (uint32_t)ridx(base, j, lane);
      cnt += (uint32_t)__popcll(m);
    }
    if (cnt >= CL_STAGE) flush();
  };
  auto step = [&](uint64_t base, In (&cur)[NIN], In (&nxt)[NIN]) {
    if constexpr (VEC) {
      if (classify_full((uint32_t)(base - r0), len)) { turn(std::true_type{}, base, cur, nxt); return; }
    }
    turn(std::false_type{}, base, cur, nxt);
  };
  // Two register sets that swap roles from turn to turn: handing `nxt` over by copying it is a use of the loads just issued, and
  // a wait for them (and for the stores behind them, which the same counter counts) in the turn that issued them.
  In va[NIN], vb[NIN];
  bool first_full = false;
  if constexpr (VEC) first_full = classify_full(0u, len);
  if (first_full) { if constexpr (VEC) load_full(0u, lane0, va); }
  else load(r0, lane0, va);
  // ONE ITERATION IS A PAIR OF TURNS: the turn at `base` (va -> vb), then, if the range goes on, the turn 64 * CL_ILP reads
  // further (vb -> va), which advances `base` itself.  Every turn still starts at r0 + k * 64 * CL_ILP.
  for (uint64_t base = r0; base < r1; base += 64 * CL_ILP) {
    step(base, va, vb);
    base += 64 * CL_ILP;          // the second turn of the pair: the sets the other way round
    if (!(base < r1)) break;
    step(base, vb, va);
  }
  flush();
  if (lane0 == 0 && nskip) atomicAdd(&P.counters[CNT_SKIP], nskip);
}

// Order-preserving-within-block compaction of a dense array with EMPTY holes into a queue: one global atomic
// per 8192 slots, issued by a kernel that has nothing else to wait for (the scorers themselves never wait on
// an atomic).  KIND 0: soft-clip slots -> soft queue.  KIND 1: stage-A survivors -> 32-byte stage-B items.
template <int KIND, int MODE>
__global__ __launch_bounds__(1024) void compact_kernel(ScoreParams P) {
  __shared__ uint32_t wcnt[128];
  __shared__ uint32_t base_sh;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long below = (1ull << lane) - 1ull;
  uint32_t n_src, cap, cnt_idx;
  const uint4 *src;
  const uint4 *ent = nullptr;
  uint4 *dst;
  static_assert(KIND == 1, "soft items have their own compaction kernel");
  {
    n_src = MODE == 0 ? P.counters[CNT_QUEUE] : min(P.counters[CNT_SOFT], P.scap);
    src = P.sb_state[MODE]; ent = MODE == 0 ? P.queue : P.soft_queue; dst = P.sb_queue[MODE];
    cap = 0xffffffffu; cnt_idx = MODE == 0 ? CNT_SBW : CNT_SBS;
  }
  // U slots per thread and round: the same-address atomic that reserves queue space is what bounds this kernel
  // (~88 per microsecond on the L2 atomic unit), so a round covers 8192 slots, not 1024.
  constexpr int U = 8;
  for (uint32_t b0 = blockIdx.x * (1024u * U); b0 < n_src; b0 += gridDim.x * (1024u * U)) {
    uint4 v[U];
    unsigned long long m[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint32_t i = b0 + 1024u * u + threadIdx.x;
      v[u] = make_uint4(EMPTY, 0, 0, 0);
      if (i < n_src) v[u] = src[i];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      m[u] = __ballot(v[u].x != EMPTY);
      if (lane == 0) wcnt[u * 16 + wave] = (uint32_t)__popcll(m[u]);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      uint32_t tot = 0;
      for (int w = 0; w < 16 * U; ++w) { const uint32_t c = wcnt[w]; wcnt[w] = tot; tot += c; }
      base_sh = tot ? atomicAdd(&P.counters[cnt_idx], tot) : 0u;
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (v[u].x != EMPTY) {
        const uint32_t i = b0 + 1024u * u + threadIdx.x;
        const uint32_t d = base_sh + wcnt[u * 16 + wave] + (uint32_t)__popcll(m[u] & below);
        if (KIND == 0) { if (d < cap) dst[d] = v[u]; }
        else {
          dst[2 * (uint64_t)d] = ent[i];
          dst[2 * (uint64_t)d + 1] = make_uint4(i, v[u].x, v[u].y, v[u].z);   // slot, best, res0, res1
        }
      }
    }
    __syncthreads();
  }
}

// Soft-clip items of the scored reads: flag byte + the read's queue entry -> segment items {id << 1 | side, seq_off, first
// base, length} in the soft queue.  One queue-space atomic per 8192 reads.
//
// Inside the range [base, base + tot) a block round reserves, the items lie BY LENGTH CLASS, shortest class first (eight
// bases per class up to 160 bases, one class for everything longer), in no particular order inside a class: the segment
// scorer's work follows the longest segment of a wave (its square, for the k = 5, 6 counts), and a wave takes 64 consecutive
// items, so neighbours should be alike.  A lane-private rank from an LDS counter per class places an item; the round's range
// is filled as a permutation of what queue order would have put there, so every reader that identifies a record by its
// read_side (all of them: the entry point's host sort, the pair logic's hash keys and replay, the chunk append and the
// multi-GPU rebase) sees the same set of records.  A round that would run past `scap` keeps queue order (left clip before
// right clip, reads in queue order): the batch ends in STRL_ERR_CAPACITY and what is dropped there stays what it was.
constexpr int SOFT_NCLS = 22;
__device__ __forceinline__ uint32_t soft_len_class(uint32_t len) { return len <= 160u ? (len + 7u) >> 3 : (uint32_t)SOFT_NCLS - 1u; }
__global__ __launch_bounds__(1024) void soft_compact_kernel(ScoreParams P) {
  __shared__ uint32_t wcnt[128];
  __shared__ uint32_t ccnt[SOFT_NCLS];
  __shared__ uint32_t base_sh, tot_sh;
  constexpr int U = 8;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long below = (1ull << lane) - 1ull;
  const uint32_t n_src = P.counters[CNT_QUEUE];
  for (uint32_t b0 = blockIdx.x * (1024u * U); b0 < n_src; b0 += gridDim.x * (1024u * U)) {
    uint32_t f[U], rank[U];
    uint4 e[U];
    unsigned long long m0[U], m1[U];
    if (threadIdx.x < SOFT_NCLS) ccnt[threadIdx.x] = 0;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint32_t i = b0 + 1024u * u + threadIdx.x;
      f[u] = i < n_src ? (uint32_t)P.soft_flag[i] : 0u;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      e[u] = make_uint4(0, 0, 0, 0);
      if (f[u]) e[u] = P.queue[b0 + 1024u * u + threadIdx.x];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      m0[u] = __ballot((f[u] & 1u) != 0);
      m1[u] = __ballot((f[u] & 2u) != 0);
      if (lane == 0) wcnt[u * 16 + wave] = (uint32_t)(__popcll(m0[u]) + __popcll(m1[u]));
    }
    __syncthreads();
    // the clipped lengths, and each item's rank in its class (left | right << 16: a round has at most 16 384 items)
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint32_t L = e[u].z & 0xffffu, cl = min(e[u].z >> 16, L), cr = min(e[u].w & 0xffffu, L);
      rank[u] = 0;
      if (f[u] & 1u) rank[u] = atomicAdd(&ccnt[soft_len_class(cl)], 1u);
      if (f[u] & 2u) rank[u] |= atomicAdd(&ccnt[soft_len_class(cr)], 1u) << 16;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      uint32_t tot = 0;
      for (int w = 0; w < 16 * U; ++w) { const uint32_t c = wcnt[w]; wcnt[w] = tot; tot += c; }
      uint32_t at = 0;
      for (int c = 0; c < SOFT_NCLS; ++c) { const uint32_t k = ccnt[c]; ccnt[c] = at; at += k; }   // (at == tot)
      base_sh = tot ? atomicAdd(&P.counters[CNT_SOFT], tot) : 0u;
      tot_sh = tot;
    }
    __syncthreads();
    const uint32_t base = base_sh;
    const bool binned = (uint64_t)base + tot_sh <= P.scap;   // block-uniform
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (f[u]) {
        const uint32_t L = e[u].z & 0xffffu, cl = min(e[u].z >> 16, L), cr = min(e[u].w & 0xffffu, L);
        uint32_t d = base + wcnt[u * 16 + wave] + (uint32_t)(__popcll(m0[u] & below) + __popcll(m1[u] & below));
        if (f[u] & 1u) {
          const uint32_t at = binned ? base + ccnt[soft_len_class(cl)] + (rank[u] & 0xffffu) : d;
          if (at < P.scap) P.soft_queue[at] = make_uint4(e[u].x << 1, e[u].y, 0u, cl);
          ++d;
        }
        if (f[u] & 2u) {
          const uint32_t at = binned ? base + ccnt[soft_len_class(cr)] + (rank[u] >> 16) : d;
          if (at < P.scap) P.soft_queue[at] = make_uint4((e[u].x << 1) | 1u, e[u].y, L - cr, cr);
        }
      }
    }
    __syncthreads();
  }
}

// rows ([row][lane] dwords) of a wave's LDS region: raw SEQ staging, the class bins of k <= 4 (24 for k = 3), long-read hash slots
template <int NW, int SLOTS, int STAGE> constexpr int table_rows() {
  constexpr int raw = 4 * ((16 * NW + 62) / 32);
  constexpr int need = STAGE == 0 ? 24 : (NW <= 10 ? 0 : SLOTS);
  return raw > need ? raw : need;
}

// `strling index`: the scorer over fixed windows of a chromosome (genome_strs.nim:61-92: window 100, step 60)
__global__ void window_items_kernel(ScoreParams P, uint32_t n_win, uint32_t window, uint32_t step, uint64_t n_bases) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) P.counters[CNT_SOFT] = n_win;
  if (i >= n_win) return;
  const uint64_t s0 = (uint64_t)i * step;
  const uint64_t len = s0 + window <= n_bases ? window : n_bases - s0;
  P.soft_queue[i] = make_uint4(i, 0u, (uint32_t)s0, (uint32_t)len);
}

// chromosome text -> BAM nibble packing (what the scorer reads), 8 bases per lane per round.  Letters are folded to
// upper case (genome_strs.nim:71 toUpperAscii); anything that is not an IUPAC letter becomes '=' (code 0): not 'N',
// never a match -- the same thing the kmer table makes of it.
__device__ inline uint32_t nt16_code(uint32_t ch) {
  switch (ch & ~0x20u) {
    case 'A': return 1; case 'C': return 2; case 'M': return 3; case 'G': return 4; case 'R': return 5; case 'S': return 6;
    case 'V': return 7; case 'T': return 8; case 'W': return 9; case 'Y': return 10; case 'H': return 11; case 'K': return 12;
    case 'D': return 13; case 'B': return 14; case 'N': return 15; default: return 0;
  }
}
__global__ __launch_bounds__(256) void pack_text_kernel(const uint8_t *__restrict__ text, uint32_t *__restrict__ seq4, uint64_t n_bases, uint64_t n_dwords) {
  __shared__ uint8_t tbl[256];
  tbl[threadIdx.x] = (uint8_t)nt16_code(threadIdx.x);
  __syncthreads();
  for (uint64_t d = (uint64_t)blockIdx.x * 256 + threadIdx.x; d < n_dwords; d += (uint64_t)gridDim.x * 256) {
    uint32_t out = 0;
    if (8 * d + 8 <= n_bases) {
      const uint2 t = *reinterpret_cast<const uint2 *>(text + 8 * d);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint32_t w = j < 2 ? t.x >> (16 * j) : t.y >> (16 * (j - 2));
        out |= (((uint32_t)tbl[w & 0xffu] << 4) | tbl[(w >> 8) & 0xffu]) << (8 * j);
      }
    } else {
      for (int b = 0; b < 8; ++b) {
        const uint64_t i = 8 * d + b;
        const uint32_t cde = i < n_bases ? tbl[text[i]] : 0u;
        out |= cde << (8 * (b >> 1) + ((b & 1) ? 0 : 4));
      }
    }
    seq4[d] = out;
  }
}

template <int MODE, int STAGE> struct Item {
  uint32_t id, seq_off, slot;
  int L, len, s0;
  uint32_t cl, cr, cg, mq;
  int best;
  uint32_t res0, res1;
  bool act;
};

// STAGE 2 (segments of the short-read class): both stages in one launch -- 98 % of the clipped ends reach k = 5 anyway, so the
//          hand-over, the compaction and the second fetch + conversion of the segment buy nothing there.
// STAGE 0: k = 2..4 on queued items; a lane whose ladder goes on leaves (best, res0, res1) in the dense
//          hand-over array.  STAGE 1: k = 5, 6 on the compacted survivors.  Whoever finishes an item writes its
//          result and the item's two soft-clip slots.  The loop is software-pipelined: while item i runs
//          the ladder, the SEQ chunks and thresholds of item i+1 and the queue entry of item i+2 are in flight.
#ifndef STRL_SCORE_OCC
#define STRL_SCORE_OCC 5     // resident 256-thread blocks per CU stage A of the short-read class is compiled for (five waves per SIMD: 96 registers;
                             // stage B carries the k = 5, 6 tables in LDS: four blocks fit)
#endif
template <int NW, int SLOTS, int MODE, int STAGE, int BLOCK>
__global__ __launch_bounds__(BLOCK, (BLOCK == 256 && NW <= 10) ? (STAGE == 0 ? STRL_SCORE_OCC : 4) : 1) void score_kernel(ScoreParams P) {
  constexpr int L56 = (LUT_ENTRIES - LUT_OFF5) / 2;                                                // dwords of the k = 5, 6 code tables
  constexpr int LUTK = STAGE == 0 ? LUT_A_DWORDS : STAGE == 1 ? LUT_DWORDS : LUT_A_DWORDS + L56;   // k-mer tables this stage looks up
  constexpr int LUTW = LUTK + 256;                                  // + the byte -> 2-bit conversion table
  constexpr int NSLOT = STAGE == 2 ? INV_SLOTS / 2 : INV_SLOTS;     // (the fused kernel's four blocks must fit a CU's LDS)
  // Statically sized LDS where it fits the 64 KB a static allocation may have: the tables then sit at compile-time
  // addresses that fold into the ds_* offset fields (with a dynamic allocation every table access paid a `v_add 0` for
  // the unknown base: ~100 VALU instructions per read in a kernel that is bound by exactly those).
  constexpr int INV_AT = LUTW + (BLOCK / 64) * table_rows<NW, SLOTS, STAGE>() * 64;   // Seg::inv_lds of the block's waves
  constexpr int LDS_WORDS = INV_AT + (BLOCK / 64) * NSLOT * NW;
  constexpr bool STATIC_LDS = (size_t)LDS_WORDS * 4 <= 65536;
  extern __shared__ __attribute__((aligned(16))) uint32_t lds_dyn[];
  __shared__ __attribute__((aligned(16))) uint32_t lds_st[STATIC_LDS ? LDS_WORDS : 4];
  uint32_t *const lds = STATIC_LDS ? lds_st : lds_dyn;
  if (STAGE == 2) {
    for (int i = threadIdx.x; i < LUT_A_DWORDS; i += BLOCK) lds[i] = P.ta[i];
    for (int i = threadIdx.x; i < L56; i += BLOCK) lds[LUT_A_DWORDS + i] = reinterpret_cast<const uint32_t *>(P.lut)[LUT_OFF5 / 2 + i];
  } else {
    for (int i = threadIdx.x; i < LUTK; i += BLOCK) lds[i] = STAGE == 0 ? P.ta[i] : reinterpret_cast<const uint32_t *>(P.lut)[i];
  }
  for (int i = threadIdx.x; i < 256; i += BLOCK) lds[LUTK + i] = reinterpret_cast<const uint32_t *>(P.lut)[LUT_DWORDS + i];
  __syncthreads();
  // (stage B indexes `lut + LutOff<5 | 6>`: in the fused kernel only those two tables are resident, behind stage A's)
  const uint16_t *lut = STAGE == 2 ? reinterpret_cast<const uint16_t *>(lds + LUT_A_DWORDS) - LUT_OFF5 : reinterpret_cast<const uint16_t *>(lds);
  const uint32_t *clut = lds + LUTK;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  uint32_t *wave_tab = lds + LUTW + wave * (table_rows<NW, SLOTS, STAGE>() * 64);
  uint32_t *col = wave_tab + lane;
  constexpr int MAXCH = (16 * NW + 62) / 32;
  const int ROW0 = MODE == 0 ? 1 : P.seg_row0, ROW1 = MODE == 0 ? 1 : P.seg_row1;
  uint32_t n_items;
  const uint4 *q;
  if (STAGE == 1) { n_items = P.counters[MODE == 0 ? CNT_SBW : CNT_SBS]; q = P.sb_queue[MODE]; }
  else if (MODE == 0) { n_items = P.counters[CNT_QUEUE]; q = nullptr; }
  else { n_items = min(P.counters[CNT_SOFT], P.scap); q = P.soft_queue; }
  const uint32_t stride = gridDim.x * BLOCK;

  // Whole reads, stage A: the queue holds read ids; the lane gathers its read's row (or the six columns) and leaves the
  // 16-byte entry in P.queue for the two compaction kernels behind this launch.  The id is loaded one item further ahead.
  constexpr bool BY_ID = MODE == 0 && STAGE == 0;
  auto load_id = [&](uint32_t item) -> uint32_t { return (BY_ID && item < n_items) ? P.queue_id[item] : 0u; };
  // What a fetch leaves in registers is the RAW loaded words; they are unpacked when the item's own iteration starts.
  // (Unpacking at load time puts an s_waitcnt right behind the load: a gather's full latency at the top of every iteration.)
  struct Raw { uint4 e, x; };
  auto fetch = [&](uint32_t item, uint32_t rid) -> Raw {
    Raw r;
    r.e = make_uint4(0, 0, 0, 0);
    r.x = make_uint4(0, 0, 0, 0);
    if (BY_ID) {       // unconditional (an idle lane reads row 0): a conditional load's result is copied at the join -- a use, a wait
      const uint4 m = P.meta[rid];
      r.e = make_uint4(rid, m.x, m.y, m.z);
      return r;
    }
    if (item < n_items) {
      if (BY_ID) { }
      else if (STAGE != 1) r.e = q[item];
      else { r.e = q[2 * (uint64_t)item]; r.x = q[2 * (uint64_t)item + 1]; }
    }
    return r;
  };
  auto unpack = [&](const Raw &r, uint32_t item) {
    Item<MODE, STAGE> it;
    const uint4 e = r.e, x = r.x;
    it.act = item < n_items;
    it.id = e.x; it.seq_off = e.y;
    it.L = (int)(e.z & 0xffffu);
    it.slot = STAGE != 1 ? item : x.x;
    it.best = STAGE != 1 ? -1 : (int)x.y;
    it.res0 = x.z; it.res1 = x.w;
    if (MODE == 0) {
      it.cl = e.z >> 16; it.cr = e.w & 0xffffu; it.cg = (e.w >> 16) & 0xffu; it.mq = e.w >> 24;
      // a read of more bases than a lane's byte counters are exact for is the host twin's (long_reads_pass below): here it
      // is an empty read without clipped ends -- no word that counts, no soft-clip items -- whose entry keeps the device busy
      // for one turn of the ladder
      if (it.L > STRL_DEVICE_READ_LEN) { it.L = 0; it.cl = 0; it.cr = 0; }
      it.len = it.L; it.s0 = 0;
    } else {
      it.cl = it.cr = it.cg = it.mq = 0;
      it.s0 = (int)e.z;
      it.len = (int)e.w;
      it.L = it.len;
    }
    if (it.len > 16 * NW) it.len = 16 * NW;  // host picks NW from max_l_seq; never taken
    if (!it.act) { it.len = 0; it.s0 = 0; }
    return it;
  };
  struct Pre { uint4 s[MAXCH]; LaneThr t; };
  auto prefetch = [&](const Item<MODE, STAGE> &it, Pre &p) {
    const int nch = it.act ? ((it.s0 & 31) + it.len + 31) >> 5 : 0;
    const uint4 *src = reinterpret_cast<const uint4 *>(P.seq4 + (uint64_t)it.seq_off * 16u) + (it.s0 >> 5);
#pragma unroll
    for (int c = 0; c < MAXCH; ++c) p.s[c] = (c < nch) ? src[c] : make_uint4(0, 0, 0, 0);
    load_thr(P.thr, ROW0, ROW1, it.len, p.t);
  };

  uint32_t base = blockIdx.x * BLOCK + wave * 64;
  Raw cur_r = fetch(base + lane, load_id(base + lane)), nxt_r = fetch(base + stride + lane, load_id(base + stride + lane));
  uint32_t id2 = load_id(base + 2 * stride + lane);
  Pre pc;
  for (; base < n_items; base += stride) {  // wave-uniform
    const Raw nn_r = fetch(base + 2 * stride + lane, id2);
    id2 = load_id(base + 3 * stride + lane);
    const Item<MODE, STAGE> cur = unpack(cur_r, base + lane);
    // The SEQ chunks and thresholds of the item are loaded here, not one item ahead: the 30 registers a prefetched item
    // occupies through the whole ladder cost a wave per SIMD (96 registers: five waves), and five waves hide this
    // latency better than a prefetch under four did (measured: 0.213 -> 0.191 ms for stage A of the whole reads).
    prefetch(cur, pc);
    // ---- run item `cur` ----
    ScoreState st;
    st.best = cur.best; st.alive = STAGE == 1 && cur.act; st.res0 = cur.res0; st.res1 = cur.res1;
    st.ph_t = __builtin_readcyclecounter();
    Seg<NW> sg;
    sg.inv_lds = lds + INV_AT + wave * (NSLOT * NW);
    sg.inv_nslots = NSLOT;
    sg.inv = P.inv_spill;
    sg.inv_stride = gridDim.x * BLOCK;
    const LenBounds lb = len_bounds(cur.act, cur.len);
    if (MODE == 0 && STAGE == 0) {
      // whole reads start on a 16-byte boundary of the SEQ array: converted straight from the prefetched registers
      uint32_t raw[4 * MAXCH];
#pragma unroll
      for (int c = 0; c < MAXCH; ++c) { raw[4 * c] = pc.s[c].x; raw[4 * c + 1] = pc.s[c].y; raw[4 * c + 2] = pc.s[c].z; raw[4 * c + 3] = pc.s[c].w; }
      STRL_PH(st, 0);
      seg_from_words<NW>(raw, clut, cur.len, lb, sg);
    } else {
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int c = 0; c < MAXCH; ++c) {   // rows a lane does not need just receive zeros
        col[(4 * c + 0) * 64] = pc.s[c].x;
        col[(4 * c + 1) * 64] = pc.s[c].y;
        col[(4 * c + 2) * 64] = pc.s[c].z;
        col[(4 * c + 3) * 64] = pc.s[c].w;
      }
      __builtin_amdgcn_wave_barrier();
      STRL_PH(st, 0);
      seg_from_raw<NW>(col, clut, cur.s0 & 31, cur.len, sg);
    }
    STRL_PH(st, 1);
    if (STAGE != 1) score_stage_a<NW, SLOTS>(sg, cur.act, wave_tab, lds + LUTW, lane, lds, pc.t, lb, st);
    if (STAGE != 0) score_stage_b<NW, SLOTS>(sg, wave_tab, lane, lut, pc.t, lb, st);

    if (BY_ID && cur.act)    // the entry the compaction kernels read (stored here with the item's other results: a store beside the
                             // gather would wait out its latency, one in front of the SEQ loads would make them wait for it)
      P.queue[base + lane] = make_uint4(cur.id, cur.seq_off, (uint32_t)cur.L | (cur.cl << 16), cur.cr | (cur.cg << 16) | (cur.mq << 24));
    const bool fwd = STAGE == 0 && cur.act && st.alive;
    const bool fin = cur.act && !fwd;
    const uint32_t o0 = reduce_packed(st.res0), o1 = reduce_packed(st.res1);
    if (STAGE == 0 && cur.act)
      P.sb_state[MODE][cur.slot] = fwd ? make_uint4((uint32_t)st.best, st.res0, st.res1, 0u) : make_uint4(EMPTY, 0u, 0u, 0u);
    if (MODE == 0) {
      if (cur.act) {
        uint32_t flag = 0;
        if (fin) {
          P.whole[cur.id] = o0;
          if (P.bloom && STRL_RES_COUNT(o0)) bloom_set(P.bloom, P.bloom_mask, fmix64(P.qhash[cur.id]));
          // add_soft gates, extract.nim:97-106
          if (cur.mq >= P.min_mapq && (cur.cg & (STRL_CIG_FIRST_S | STRL_CIG_LAST_S))) {
            const bool has_unit = STRL_RES_K(o0) != 0;
            if ((cur.cg & STRL_CIG_FIRST_S) && (has_unit || cur.cl > 16)) flag |= 1u;
            // with a single cigar op both loop iterations are cig_index == 0 (the host replays the duplicate)
            if ((cur.cg & STRL_CIG_LAST_S) && !(cur.cg & STRL_CIG_ONE_OP) && (has_unit || cur.cr > 16)) flag |= 2u;
          }
        }
        P.soft_flag[cur.slot] = (uint8_t)flag;           // forwarded items leave 0; stage B overwrites
      }
    } else {
      if (fin && cur.slot < P.soft_cap) {
        strl_soft_rec o;
        o.read_side = cur.id;
        o.res_first = o0;
        o.res_after = o1;
        o.seg_len = (uint32_t)cur.len;
        P.soft_out[cur.slot] = o;
      }
    }
    STRL_PH(st, 12);
    cur_r = nxt_r; nxt_r = nn_r;
  }
}

// ---- host side of this translation unit -------------------------------------------------------
template <int NW, int SLOTS, int MODE, int STAGE, int BLOCK> static int launch_score(strl_ctx *ctx, const ScoreParams &P, int blocks) {
  auto kfn = score_kernel<NW, SLOTS, MODE, STAGE, BLOCK>;
  size_t shmem = (size_t)((STAGE == 0 ? LUT_A_DWORDS : STAGE == 1 ? LUT_DWORDS : LUT_A_DWORDS + (LUT_ENTRIES - LUT_OFF5) / 2) + 256) * 4 +
                 (size_t)(BLOCK / 64) * (table_rows<NW, SLOTS, STAGE>() * 64 + (STAGE == 2 ? INV_SLOTS / 2 : INV_SLOTS) * NW) * 4;
  if (shmem <= 65536) shmem = 0;      // the kernel allocates it statically (see STATIC_LDS there)
  // (only the long-read classes allocate dynamically; set on every such launch: the attribute belongs to the current DEVICE,
  // and contexts of one process may sit on different ones)
  if (shmem) STRL_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kfn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem));
  ScoreParams Q = P;
  // sized for the largest grid this class is ever launched with, so that it is allocated once per context and class (an
  // allocation synchronises the device: in the chunked extract every growing chunk would have paid for it)
  const size_t spill = (size_t)std::max(blocks, 8192) * BLOCK * NW * 4;
  if (ctx->inv_spill.cap < spill) {
    STRL_HIP(hipStreamSynchronize(ctx->stream));
    int rc = ctx->inv_spill.reserve(spill);
    if (rc) return rc;
  }
  Q.inv_spill = ctx->inv_spill.as<uint32_t>();
  hipLaunchKernelGGL(kfn, dim3(blocks), dim3(BLOCK), shmem, ctx->stream, Q);
  STRL_HIP(hipGetLastError());
  return STRL_OK;
}

// stage A -> compaction of the survivors -> stage B of one MODE, kernel class picked by the longest read
// ev (optional): two events, recorded behind stage A and behind the compaction
template <int MODE> static int launch_score_class(strl_ctx *ctx, const ScoreParams &P, uint32_t max_l, hipEvent_t *ev = nullptr) {
  int rc;
  // Grid: the kernels stride over the queue, so any grid works; measured on 2^25-read batches the time keeps falling
  // until ~8192 blocks for stage A and ~4096 for stage B (1.51 -> 1.29 ms per step against 512 blocks = two resident
  // blocks per CU): surplus blocks are what lets the hardware even out the very uneven cost of the items.  The queue
  // length lives on the device; the host knows an upper bound (reads of the batch / capacity of the segment queue).
  const uint64_t upper = MODE == 0 ? P.n : (uint64_t)P.scap;
  static const int env_a = getenv("STRL_GRID_A") ? atoi(getenv("STRL_GRID_A")) : 0, env_b = getenv("STRL_GRID_B") ? atoi(getenv("STRL_GRID_B")) : 0;
  const int ga = env_a > 0 ? env_a : (int)std::min<uint64_t>(8192, std::max<uint64_t>(256, (upper + 255) / 256));
  const int gb = env_b > 0 ? env_b : std::max(256, ga / 2);
  static const bool split_segments = getenv("STRL_SPLIT_SEGMENTS") != nullptr;
  if constexpr (MODE == 1) {
    if (max_l <= 160 && !split_segments) {        // segments of the short-read class: one fused launch
      if ((rc = launch_score<10, 64, MODE, 2, 256>(ctx, P, ga))) return rc;
      if (ev) { STRL_HIP(hipEventRecord(ev[0], ctx->stream)); STRL_HIP(hipEventRecord(ev[1], ctx->stream)); }
      return STRL_OK;
    }
  }
  // (a grid given by the environment is the grid of every length class: tests and sweeps put a lane through many turns of its loop)
  if (max_l <= 160) rc = launch_score<10, 64, MODE, 0, 256>(ctx, P, ga);
  else if (max_l <= 256) rc = launch_score<16, 128, MODE, 0, 256>(ctx, P, env_a > 0 ? env_a : std::max(256, ga / 4));
  else rc = launch_score<32, 256, MODE, 0, 64>(ctx, P, env_a > 0 ? env_a : std::max(512, ga / 2));
  if (rc) return rc;
  if (ev) STRL_HIP(hipEventRecord(ev[0], ctx->stream));
  hipLaunchKernelGGL((compact_kernel<1, MODE>), dim3(compact_grid(512)), dim3(1024), 0, ctx->stream, P);
  STRL_HIP(hipGetLastError());
  if (ev) STRL_HIP(hipEventRecord(ev[1], ctx->stream));
  if (max_l <= 160) return launch_score<10, 64, MODE, 1, 256>(ctx, P, gb);
  if (max_l <= 256) return launch_score<16, 128, MODE, 1, 256>(ctx, P, env_b > 0 ? env_b : std::max(256, gb / 4));
  return launch_score<32, 256, MODE, 1, 64>(ctx, P, env_b > 0 ? env_b : std::max(512, gb / 2));
}

// STRL_GRID_K (tests, grid sweeps): the grid of the three compaction kernels, whose fixed grids cover millions of slots per round
int compact_grid(int dflt) {
  static const int env_k = getenv("STRL_GRID_K") ? atoi(getenv("STRL_GRID_K")) : 0;
  return env_k > 0 ? env_k : dflt;
}

}  // namespace strl

using namespace strl;

// Bloom bitmap of the hot qname groups: ~n/2 bits (2 MB for 2^25 reads: L2 resident), four bits per key in one 64-bit word
// (bloom_layout.h; the size rule does not depend on the layout)
int bloom_reset(strl_ctx *c, uint64_t n) {
  uint64_t bits = 1ull << 16;
  while (bits < n / 2 && bits < (1ull << 27)) bits <<= 1;
  int rc;
  if ((rc = c->bloom.reserve((size_t)(bits / 8)))) return rc;
  STRL_HIP(zero_words(c->bloom.p, (size_t)(bits / 8), c->stream));
  c->bloom_mask = (uint32_t)(bits - 1);
  return STRL_OK;
}

extern "C" {      // (C linkage: the kernels keep the plain names the records under profiles/ have them by)
namespace strl {
// the strl_read_meta rows of a batch from its columns
__global__ void meta_rows_kernel(const uint32_t *seq_off, const uint16_t *l_seq, const uint16_t *clip_l, const uint16_t *clip_r, const uint8_t *cig, const uint8_t *mapq,
                                 uint32_t n, uint4 *out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = make_uint4(seq_off[i], (uint32_t)l_seq[i] | ((uint32_t)clip_l[i] << 16), (uint32_t)clip_r[i] | ((uint32_t)cig[i] << 16) | ((uint32_t)mapq[i] << 24), 0u);
}
// Reads of more than STRL_DEVICE_READ_LEN bases (extract.nim:36-40 scores any length; the reference's uint8 histograms wrap,
// utils.nim:192-195): behind the batch's launches the device lists them (index, row, skipped or not), packs their SEQ bytes,
// the host twin of the scorer (host_score.cpp) scores them on a few threads, and two small launches put the words where the
// kernels would have put them -- whole[], the Bloom mark, soft-clip records behind the device's own.  Synchronises the stream:
// only batches that hold such a read pay for it.
__global__ void long_scan_kernel(const uint4 *meta, const uint32_t *whole, uint32_t n, uint4 *out, uint32_t *cnt) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint4 m = meta[i];
  if ((m.y & 0xffffu) <= (uint32_t)STRL_DEVICE_READ_LEN) return;
  const uint32_t k = atomicAdd(cnt, 1u);
  out[k] = make_uint4(i | ((whole[i] & STRL_RES_SKIPPED) ? 0x80000000u : 0u), m.x, m.y, m.z);
}
// one wave per listed read: its SEQ bytes to off[k] of a dense buffer, as dwords (slots and offsets are 16-byte aligned)
__global__ __launch_bounds__(64) void long_gather_kernel(const uint8_t *seq4, const uint4 *list, const uint64_t *off, uint8_t *out) {
  const uint4 e = list[blockIdx.x];
  const uint32_t nb = ((e.z & 0xffffu) + 1u) / 2u, nd = (nb + 3u) / 4u;
  const uint32_t *src = reinterpret_cast<const uint32_t *>(seq4 + (uint64_t)e.y * 16u);
  uint32_t *dst = reinterpret_cast<uint32_t *>(out + off[blockIdx.x]);
  for (uint32_t j = threadIdx.x; j < nd; j += 64u) dst[j] = src[j];
}
__global__ void long_patch_kernel(const uint32_t *ids, const uint32_t *words, uint32_t n, uint32_t *whole, const uint64_t *qhash, uint32_t *bloom, uint32_t bloom_mask) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const uint32_t id = ids[k], w = words[k];
  whole[id] = w;
  if (bloom && STRL_RES_COUNT(w)) bloom_set(bloom, bloom_mask, fmix64(qhash[id]));
}
__global__ __launch_bounds__(1024) void long_soft_kernel(const strl_soft_rec *src, uint32_t n, strl_soft_rec *dst, uint32_t cap, uint32_t *counters) {
  __shared__ uint32_t base_sh;
  if (threadIdx.x == 0) base_sh = atomicAdd(&counters[CNT_SOFT], n);     // (one block, behind the segment scorer: the only writer now)
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < n; i += blockDim.x)
    if (base_sh + i < cap) dst[base_sh + i] = src[i];
}
}  // namespace strl
}  // extern "C"

// the packed rows of a device-resident batch's columns, into st_meta
static int meta_rows(strl_ctx *c, const strl_read_soa *d) {
  const uint64_t n = d->n;
  const int rc = c->st_meta.reserve(std::max<size_t>((size_t)n * 16, 64));
  if (rc) return rc;
  if (n) {
    hipLaunchKernelGGL(strl::meta_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, d->seq_off, d->l_seq, d->clip_l, d->clip_r, d->cig, d->mapq,
                       (uint32_t)n, c->st_meta.as<uint4>());
    STRL_HIP(hipGetLastError());
  }
  return STRL_OK;
}

static int long_reads_pass(strl_ctx *c, const ScoreParams &P, uint64_t scap) {
  const uint32_t n = (uint32_t)P.n;
  int rc;
  if ((rc = c->long_list.reserve((size_t)n * 16 + 64))) return rc;
  uint32_t *cnt = c->long_list.as<uint32_t>() + (size_t)n * 4;            // the counter behind the list
  STRL_HIP(hipMemsetAsync(cnt, 0, 4, c->stream));
  hipLaunchKernelGGL(strl::long_scan_kernel, dim3((n + 255u) / 256u), dim3(256), 0, c->stream, P.meta, P.whole, n, c->long_list.as<uint4>(), cnt);
  STRL_HIP(hipGetLastError());
  uint32_t n_long = 0;
  STRL_HIP(hipMemcpyAsync(&n_long, cnt, 4, hipMemcpyDeviceToHost, c->stream));
  STRL_HIP(hipStreamSynchronize(c->stream));
  if (!n_long) return STRL_OK;
  std::vector<uint4> list(n_long);
  STRL_HIP(hipMemcpy(list.data(), c->long_list.p, (size_t)n_long * 16, hipMemcpyDeviceToHost));
  std::vector<uint64_t> off((size_t)n_long + 1);
  uint64_t total = 0;
  for (uint32_t k = 0; k < n_long; ++k) { off[k] = total; total += ((((list[k].z & 0xffffu) + 1u) / 2u) + 15u) & ~15ull; }
  off[n_long] = total;
  if ((rc = c->long_seq.reserve((size_t)total + (size_t)(n_long + 1) * 8 + 64))) return rc;
  uint64_t *d_off = reinterpret_cast<uint64_t *>(c->long_seq.as<uint8_t>() + total);      // (total is a multiple of 16)
  STRL_HIP(hipMemcpyAsync(d_off, off.data(), (size_t)(n_long + 1) * 8, hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(strl::long_gather_kernel, dim3(n_long), dim3(64), 0, c->stream, P.seq4, c->long_list.as<uint4>(), d_off, c->long_seq.as<uint8_t>());
  STRL_HIP(hipGetLastError());
  std::vector<uint8_t> seq((size_t)total + 16);
  STRL_HIP(hipMemcpyAsync(seq.data(), c->long_seq.p, (size_t)total, hipMemcpyDeviceToHost, c->stream));
  STRL_HIP(hipStreamSynchronize(c->stream));
  std::vector<uint32_t> ids(n_long), words(n_long);
  std::vector<strl_soft_rec> soft((size_t)n_long * 2);
  std::vector<uint8_t> n_soft(n_long, 0);
  const strl_opts o = c->opts;
  auto run = [&](uint32_t k0, uint32_t k1) {
    for (uint32_t k = k0; k < k1; ++k) {
      const uint4 e = list[k];
      const uint32_t id = e.x & 0x7fffffffu;
      int ns = 0;
      uint32_t w = 0;
      strl::host_score_long_read(seq.data() + off[k], e.z & 0xffffu, e.z >> 16, e.w & 0xffffu, (e.w >> 16) & 0xffu, e.w >> 24, o, (e.x >> 31) != 0, id, w, &soft[(size_t)k * 2], ns);
      ids[k] = id;
      words[k] = (e.x >> 31) ? (uint32_t)STRL_RES_SKIPPED : w;
      n_soft[k] = (uint8_t)ns;
    }
  };
  const uint32_t workers = (uint32_t)std::min<uint64_t>(std::min<unsigned>(16u, std::max(1u, std::thread::hardware_concurrency())), n_long / 64 + 1);
  if (workers <= 1) run(0, n_long);
  else {
    std::vector<std::thread> th;
    for (uint32_t t = 0; t < workers; ++t) th.emplace_back(run, (uint32_t)((uint64_t)n_long * t / workers), (uint32_t)((uint64_t)n_long * (t + 1) / workers));
    for (auto &t : th) t.join();
  }
  std::vector<strl_soft_rec> dense;
  for (uint32_t k = 0; k < n_long; ++k)
    for (int q = 0; q < n_soft[k]; ++q) dense.push_back(soft[(size_t)k * 2 + q]);
  const size_t b_ids = ((size_t)n_long * 4 + 15) & ~(size_t)15, b_soft = dense.size() * sizeof(strl_soft_rec);
  if ((rc = c->long_seq.reserve(2 * b_ids + b_soft + 64))) return rc;
  uint8_t *base = c->long_seq.as<uint8_t>();
  STRL_HIP(hipMemcpyAsync(base, ids.data(), (size_t)n_long * 4, hipMemcpyHostToDevice, c->stream));
  STRL_HIP(hipMemcpyAsync(base + b_ids, words.data(), (size_t)n_long * 4, hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(strl::long_patch_kernel, dim3((n_long + 255u) / 256u), dim3(256), 0, c->stream, reinterpret_cast<const uint32_t *>(base),
                     reinterpret_cast<const uint32_t *>(base + b_ids), n_long, P.whole, P.qhash, P.bloom, P.bloom_mask);
  STRL_HIP(hipGetLastError());
  if (!dense.empty() && scap && P.soft_out) {
    STRL_HIP(hipMemcpyAsync(base + 2 * b_ids, dense.data(), b_soft, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(strl::long_soft_kernel, dim3(1), dim3(1024), 0, c->stream, reinterpret_cast<const strl_soft_rec *>(base + 2 * b_ids), (uint32_t)dense.size(), P.soft_out,
                       (uint32_t)std::min<uint64_t>(scap, P.soft_cap), P.counters);
    STRL_HIP(hipGetLastError());
  }
  STRL_HIP(hipStreamSynchronize(c->stream));       // (the host vectors above are the copies' sources)
  return STRL_OK;
}

int score_device(strl_ctx *c, const strl_read_soa *s, uint32_t *whole, strl_soft_rec *soft, uint64_t soft_cap, uint64_t *n_soft,
                 strl_score_stats *stats, bool sync_counts, const strl_pair_soa *pp, bool fresh_bloom, bool side_busy_ok) {
  const uint64_t n = s->n;
  // the side stream may still read this context's counters / Bloom bitmap / results (pair logic of the previous batch):
  // every scoring pass waits for it, except the overlapped strl_extract_device, which works on the other set of buffers
  if (!side_busy_ok) { const int rcj = side_join(c); if (rcj) return rcj; }
  if (n > 0x3fffffffull) { set_error("batch too large (%llu reads; limit 2^30-1)", (unsigned long long)n); return STRL_ERR_ARG; }
  if (s->max_l_seq > STRL_MAX_READ_LEN) { set_error("read of %u bases exceeds STRL_MAX_READ_LEN=%d", s->max_l_seq, STRL_MAX_READ_LEN); return STRL_ERR_ARG; }
  // reads of more than STRL_DEVICE_READ_LEN bases: the kernels pass them by, the host twin scores them behind the launches
  const bool long_reads = s->max_l_seq > (uint32_t)STRL_DEVICE_READ_LEN;
  const uint32_t class_l = std::min<uint32_t>(s->max_l_seq, STRL_DEVICE_READ_LEN);
  int rc;
  const uint64_t n1 = std::max<uint64_t>(n, 1);
  const uint64_t scap = std::max<uint64_t>(std::min<uint64_t>(soft_cap, 2 * n), 1);
  if ((rc = c->queue.reserve((size_t)n1 * 16))) return rc;
  if ((rc = c->queue_r.reserve((size_t)n1 * 4))) return rc;
  if ((rc = c->soft_dense.reserve((size_t)n1 + 64))) return rc;
  if ((rc = c->soft_queue.reserve((size_t)scap * 16))) return rc;
  if ((rc = c->sb_state_w.reserve((size_t)n1 * 16))) return rc;
  if ((rc = c->sb_state_s.reserve((size_t)scap * 16))) return rc;
  if ((rc = c->sb_whole.reserve((size_t)n1 * 32))) return rc;
  if ((rc = c->sb_soft.reserve((size_t)scap * 32))) return rc;
  STRL_HIP(zero_words(c->counters.p, CNT_WORDS * 4, c->stream));
  ScoreParams P{};
  P.n = n;
  P.tid = s->tid; P.pos = s->pos; P.end = s->end; P.seq_off = s->seq_off; P.l_seq = s->l_seq;
  P.clip_l = s->clip_l; P.clip_r = s->clip_r; P.mapq = s->mapq; P.cig = s->cig; P.seq4 = s->seq4;
  P.meta = reinterpret_cast<const uint4 *>(s->meta);
  if (!P.meta) {   // device-resident columns without the packed rows: stage A gathers rows, so they are built here (a pass over the batch:
                   // callers that care hand over strl_read_soa.meta)
    if ((rc = meta_rows(c, s))) return rc;
    P.meta = c->st_meta.as<uint4>();
  }
  if (!c->g_tid.p && (rc = strl_ctx_set_genome(c, nullptr))) return rc;   // never set: the empty table
  P.g_tid = c->g_tid.as<TidInfo>(); P.g_bins = c->g_bins.as<uint2>(); P.g_iv = c->g_start.as<int2>();
  P.n_tid = c->n_tid;
  P.lut = c->lut.as<uint16_t>(); P.thr = c->thr.as<uint64_t>();
  P.ta = c->lut.as<uint32_t>() + LUT_DWORDS + 256;
  P.whole = whole; P.queue = c->queue.as<uint4>(); P.queue_id = c->queue_r.as<uint32_t>(); P.soft_flag = c->soft_dense.as<uint8_t>();
  P.soft_queue = c->soft_queue.as<uint4>();
  P.sb_state[0] = c->sb_state_w.as<uint4>(); P.sb_state[1] = c->sb_state_s.as<uint4>();
  P.sb_queue[0] = c->sb_whole.as<uint4>(); P.sb_queue[1] = c->sb_soft.as<uint4>();
  P.scap = (uint32_t)scap;
  P.counters = c->counters.as<uint32_t>(); P.soft_out = soft;
  P.soft_cap = (uint32_t)std::min<uint64_t>(soft_cap, 0xffffffffull);
  P.min_mapq = c->opts.min_mapq;
  P.seg_row0 = 2; P.seg_row1 = 3;
  if (pp) {
    if (fresh_bloom && (rc = bloom_reset(c, n))) return rc;
    P.qhash = pp->qhash; P.bloom = c->bloom.as<uint32_t>(); P.bloom_mask = c->bloom_mask;
  }
  hipEvent_t *tev = c->timing ? &c->ring[(c->ring_pos % RING) * EV_PER] : nullptr;
  if (c->timing) ++c->ring_pos;
  if (tev) STRL_HIP(hipEventRecord(tev[0], c->stream));
  if (n) {
    static const int env_c = getenv("STRL_GRID_C") ? atoi(getenv("STRL_GRID_C")) : 0;
    const int cblocks = (int)std::min<uint64_t>((n + 255) / 256, env_c > 0 ? (uint64_t)env_c : 1024);   // one round: 256 CUs x 4 resident blocks (124 VGPRs, 16 KB of LDS); measured 768..10240
    const bool vec = (((uintptr_t)P.tid | (uintptr_t)P.pos | (uintptr_t)P.end | (uintptr_t)P.whole) & 15u) == 0 && ((uintptr_t)P.cig & 3u) == 0;
    if (vec) hipLaunchKernelGGL(classify_kernel<true>, dim3(cblocks), dim3(256), 0, c->stream, P);
    else hipLaunchKernelGGL(classify_kernel<false>, dim3(cblocks), dim3(256), 0, c->stream, P);
    STRL_HIP(hipGetLastError());
  }
  if (tev) STRL_HIP(hipEventRecord(tev[1], c->stream));
  if (n) { if ((rc = launch_score_class<0>(c, P, class_l, tev ? tev + 2 : nullptr))) return rc; }
  else if (tev) { STRL_HIP(hipEventRecord(tev[2], c->stream)); STRL_HIP(hipEventRecord(tev[3], c->stream)); }
  if (tev) STRL_HIP(hipEventRecord(tev[4], c->stream));
  if (n && soft_cap) {
    hipLaunchKernelGGL(soft_compact_kernel, dim3(strl::compact_grid(1024)), dim3(1024), 0, c->stream, P);
    STRL_HIP(hipGetLastError());
    if (tev) STRL_HIP(hipEventRecord(tev[5], c->stream));
    if ((rc = launch_score_class<1>(c, P, class_l, tev ? tev + 6 : nullptr))) return rc;
  } else if (tev) { for (int k = 5; k <= 7; ++k) STRL_HIP(hipEventRecord(tev[k], c->stream)); }
  if (tev) STRL_HIP(hipEventRecord(tev[8], c->stream));
  if (n && long_reads && (rc = long_reads_pass(c, P, soft_cap ? scap : 0))) return rc;
  if (sync_counts) {
    uint32_t raw[CNT_WORDS];
    STRL_HIP(hipMemcpyAsync(raw, c->counters.p, CNT_WORDS * 4, hipMemcpyDeviceToHost, c->stream));
    STRL_HIP(hipStreamSynchronize(c->stream));
    const uint64_t softs = soft_cap ? raw[CNT_SOFT] : 0;
    if (softs > scap || softs > soft_cap) { set_error("soft-clip queue overflow: %llu items, capacity %llu", (unsigned long long)softs, (unsigned long long)std::min(scap, soft_cap)); return STRL_ERR_CAPACITY; }
    if (n_soft) *n_soft = softs;
    if (stats) {
      memset(stats, 0, sizeof *stats);
      stats->n_reads = n; stats->n_skipped = raw[CNT_SKIP]; stats->n_scored = raw[CNT_QUEUE]; stats->n_soft_items = softs;
      stats->n_stage_b_whole = raw[CNT_SBW]; stats->n_stage_b_soft = soft_cap ? raw[CNT_SBS] : 0;
      if (tev) {
        (void)hipEventElapsedTime(&stats->ms_classify, tev[0], tev[1]);
        (void)hipEventElapsedTime(&stats->ms_score, tev[1], tev[4]);
        (void)hipEventElapsedTime(&stats->ms_soft, tev[4], tev[8]);
      }
    }
  }
  return STRL_OK;
}

// host-memory batch -> staging buffers in HBM (asynchronous copies on the context stream)
int stage_batch(strl_ctx *c, const strl_read_soa *s, const strl_pair_soa *pp, strl_read_soa *d, strl_pair_soa *dpp) {
  const uint64_t n = s->n;
  *d = *s;
  int rc;
  struct { strl::DevBuf *b; const void *src; size_t bytes; const void **dst; } cp[] = {
      {&c->st_tid, s->tid, (size_t)n * 4, (const void **)&d->tid},         {&c->st_pos, s->pos, (size_t)n * 4, (const void **)&d->pos},
      {&c->st_end, s->end, (size_t)n * 4, (const void **)&d->end},         {&c->st_seqoff, s->seq_off, (size_t)n * 4, (const void **)&d->seq_off},
      {&c->st_lseq, s->l_seq, (size_t)n * 2, (const void **)&d->l_seq},    {&c->st_clipl, s->clip_l, (size_t)n * 2, (const void **)&d->clip_l},
      {&c->st_clipr, s->clip_r, (size_t)n * 2, (const void **)&d->clip_r}, {&c->st_mapq, s->mapq, (size_t)n, (const void **)&d->mapq},
      {&c->st_cig, s->cig, (size_t)n, (const void **)&d->cig},             {&c->st_seq4, s->seq4, (size_t)s->seq4_bytes, (const void **)&d->seq4}};
  for (auto &x : cp) {
    if ((rc = x.b->reserve(std::max<size_t>(x.bytes, 64)))) return rc;
    if (x.bytes) STRL_HIP(hipMemcpyAsync(x.b->p, x.src, x.bytes, hipMemcpyHostToDevice, c->stream));
    *x.dst = x.b->p;
  }
  d->mem = STRL_MEM_DEVICE;
  if ((rc = meta_rows(c, d))) return rc;
  d->meta = c->st_meta.as<strl_read_meta>();
  if (pp) {
    struct { strl::DevBuf *b; const void *src; size_t bytes; const void **dst; } cq[] = {
        {&c->st_mtid, pp->rec, (size_t)n * sizeof(strl_pair_rec), (const void **)&dpp->rec},
        {&c->st_qhash, pp->qhash, (size_t)n * 8, (const void **)&dpp->qhash}};
    for (auto &x : cq) {
      if ((rc = x.b->reserve(std::max<size_t>(x.bytes, 64)))) return rc;
      if (x.bytes) STRL_HIP(hipMemcpyAsync(x.b->p, x.src, x.bytes, hipMemcpyHostToDevice, c->stream));
      *x.dst = x.b->p;
    }
  }
  return STRL_OK;
}

extern "C" {

#ifdef STRL_PHASE_TIMING
int strl_debug_phase(unsigned long long *out, int reset) {   // debug builds only (not part of the ABI)
  if (out) { if (hipMemcpyFromSymbol(out, HIP_SYMBOL(strl::g_phase), 32 * 8) != hipSuccess) return -1; }
  if (reset) { unsigned long long z[32] = {0}; if (hipMemcpyToSymbol(HIP_SYMBOL(strl::g_phase), z, 32 * 8) != hipSuccess) return -1; }
  return 0;
}
#endif

int strl_index_chrom(strl_ctx *c, const char *seq, uint64_t n_bases, uint32_t window, uint32_t step, uint32_t *words, uint64_t *n_windows) {
  if (!c || (!seq && n_bases) || !window || !step) { set_error("bad argument"); return STRL_ERR_ARG; }
  if (!c->have_opts) { set_error("strl_ctx_set_opts must be called before scoring"); return STRL_ERR_ARG; }
  if (window > 160) { set_error("window %u too long (<= 160)", window); return STRL_ERR_ARG; }
  if (n_bases >= (1ull << 31)) { set_error("sequence too long (< 2^31 bases)"); return STRL_ERR_ARG; }
  STRL_HIP(hipSetDevice(c->device));
  const uint64_t nw = n_bases ? (n_bases + step - 1) / step : 0;
  if (n_windows) *n_windows = nw;
  if (!nw || !words) return STRL_OK;
  const uint64_t n_dwords = (n_bases + 7) / 8 + 16;       // 64 bytes of zero slack behind the last base
  int rc;
  if ((rc = c->st_text.reserve((size_t)n_bases + 8))) return rc;
  if ((rc = c->st_seq4.reserve((size_t)n_dwords * 4))) return rc;
  if ((rc = c->soft_queue.reserve((size_t)nw * 16))) return rc;
  if ((rc = c->sb_state_s.reserve((size_t)nw * 16))) return rc;
  if ((rc = c->sb_soft.reserve((size_t)nw * 32))) return rc;
  if ((rc = c->st_soft.reserve((size_t)nw * sizeof(strl_soft_rec)))) return rc;
  STRL_HIP(hipMemcpyAsync(c->st_text.p, seq, (size_t)n_bases, hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(pack_text_kernel, dim3((unsigned)std::min<uint64_t>((n_dwords + 255) / 256, 4096)), dim3(256), 0, c->stream,
                     c->st_text.as<uint8_t>(), c->st_seq4.as<uint32_t>(), n_bases, n_dwords);
  STRL_HIP(hipGetLastError());
  STRL_HIP(hipMemsetAsync(c->counters.p, 0, CNT_WORDS * 4, c->stream));
  ScoreParams P{};
  P.n = nw; P.seq4 = c->st_seq4.as<uint8_t>();
  P.lut = c->lut.as<uint16_t>(); P.thr = c->thr.as<uint64_t>();
  P.ta = c->lut.as<uint32_t>() + LUT_DWORDS + 256;
  P.soft_queue = c->soft_queue.as<uint4>(); P.scap = (uint32_t)nw;
  P.sb_state[1] = c->sb_state_s.as<uint4>(); P.sb_queue[1] = c->sb_soft.as<uint4>();
  P.counters = c->counters.as<uint32_t>(); P.soft_out = c->st_soft.as<strl_soft_rec>(); P.soft_cap = (uint32_t)nw;
  P.seg_row0 = 1; P.seg_row1 = 1;                       // genome windows are scored with the plain -p threshold (genome_strs.nim:74)
  hipLaunchKernelGGL(window_items_kernel, dim3((unsigned)((nw + 255) / 256)), dim3(256), 0, c->stream, P, (uint32_t)nw, window, step, n_bases);
  STRL_HIP(hipGetLastError());
  if ((rc = launch_score_class<1>(c, P, window))) return rc;
  std::vector<strl_soft_rec> out((size_t)nw);
  STRL_HIP(hipMemcpyAsync(out.data(), c->st_soft.p, (size_t)nw * sizeof(strl_soft_rec), hipMemcpyDeviceToHost, c->stream));
  STRL_HIP(hipStreamSynchronize(c->stream));
  for (uint64_t i = 0; i < nw; ++i) words[out[(size_t)i].read_side] = out[(size_t)i].res_first;
  return STRL_OK;
}

int strl_score_reads(strl_ctx *c, const strl_read_soa *s, uint32_t *whole, strl_soft_rec *soft, uint64_t soft_cap,
                     uint64_t *n_soft, strl_score_stats *stats) {
  if (!c || !s || (!whole && s->n)) { set_error("null argument"); return STRL_ERR_ARG; }
  if (!c->have_opts) { set_error("strl_ctx_set_opts must be called before scoring"); return STRL_ERR_ARG; }
  STRL_HIP(hipSetDevice(c->device));
  if (s->mem == STRL_MEM_DEVICE) {
    // n_soft == NULL and stats == NULL: fully asynchronous (bench / pipelines read counters later)
    return score_device(c, s, whole, soft, soft_cap, n_soft, stats, n_soft != nullptr || stats != nullptr);
  }
  // host batch: stage to HBM, run, copy results back
  const uint64_t n = s->n;
  strl_read_soa d;
  int rc;
  if ((rc = stage_batch(c, s, nullptr, &d, nullptr))) return rc;
  if ((rc = c->st_whole.reserve((size_t)std::max<uint64_t>(n, 1) * 4))) return rc;
  const uint64_t dcap = 2 * n + 2;   // at most two clipped ends per read
  if ((rc = c->st_soft.reserve((size_t)std::max<uint64_t>(dcap, 1) * sizeof(strl_soft_rec)))) return rc;
  uint64_t ns = 0;
  strl_score_stats st{};
  rc = score_device(c, &d, c->st_whole.as<uint32_t>(), c->st_soft.as<strl_soft_rec>(), dcap, &ns, &st, true);
  if (rc) return rc;
  if (ns > soft_cap) { set_error("soft capacity %llu too small, need %llu", (unsigned long long)soft_cap, (unsigned long long)ns); return STRL_ERR_CAPACITY; }
  if (n) STRL_HIP(hipMemcpyAsync(whole, c->st_whole.p, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
  if (ns && soft) STRL_HIP(hipMemcpyAsync(soft, c->st_soft.p, (size_t)ns * sizeof(strl_soft_rec), hipMemcpyDeviceToHost, c->stream));
  STRL_HIP(hipStreamSynchronize(c->stream));
  if (soft && ns) std::sort(soft, soft + ns, [](const strl_soft_rec &a, const strl_soft_rec &b) { return a.read_side < b.read_side; });
  if (n_soft) *n_soft = ns;
  if (stats) *stats = st;
  return STRL_OK;
}

// test-only, undeclared (the strl_sort_probe precedent): the read ids classify_kernel queued in the context's last scoring pass,
// in queue order, after a sync -> their number (all of them are counted, at most `cap` are copied)
int strl_score_queue_probe(strl_ctx *c, uint32_t *ids, uint64_t cap, uint64_t *n_ids) {
  if (!c || !n_ids || (cap && !ids)) { set_error("strl_score_queue_probe: bad argument"); return STRL_ERR_ARG; }
  if (!c->counters.p || !c->queue_r.p) { set_error("strl_score_queue_probe: no scoring pass on this context"); return STRL_ERR_ARG; }
  STRL_HIP(hipSetDevice(c->device));
  uint32_t v = 0;
  STRL_HIP(hipMemcpyAsync(&v, c->counters.as<uint32_t>() + CNT_QUEUE, 4, hipMemcpyDeviceToHost, c->stream));
  STRL_HIP(hipStreamSynchronize(c->stream));
  *n_ids = v;
  const uint64_t m = std::min<uint64_t>(v, cap);
  if (m) {
    STRL_HIP(hipMemcpyAsync(ids, c->queue_r.p, m * 4, hipMemcpyDeviceToHost, c->stream));
    STRL_HIP(hipStreamSynchronize(c->stream));
  }
  return STRL_OK;
}

}  // extern "C"
