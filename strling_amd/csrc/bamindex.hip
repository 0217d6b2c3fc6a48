// bamindex.hip -- `strling bamindex`: the BAM index (.bai, SAM spec 5.2) built on the GPU (gfx950) behind the front end's record
// scan.  What `samtools index` does on one thread through htslib (sam_index_build: inflate, bam_read1, hts_idx_push per record,
// hts_idx_finish); the reference only consumes an index (call.nim:101-102).  A chunk of BGZF blocks goes through
//   front_stage_a        (front.hip)   copy + inflate + CRC + rec_guess / rec_walk / rec_link / rec_emit: recoff[] of the chunk
//   bai_record_kernel                  one lane per record: refID, pos, flag, CIGAR -> end, bin (reg2bin), virtual offsets of its
//                                      first byte and of the byte behind it, sortedness, the linear index's windows (a 64-bit
//                                      atomicMin only from the first record that reaches a window), the per-reference span and
//                                      counts (one set of atomics per wave), and a flag where (tid, bin) changes: a run starts
//   bai_scan_kernel                    one block: exclusive sums of the flags per 256 records
//   bai_emit_kernel                    the flagged records write their run into the resident table, in file order, and close
//                                      the run in front of them (records lie back to back: a run ends where the next begins)
// and nothing of a chunk but its runs stays: the table grows with the number of (tid, bin) changes, not with the records.
// At the end one stable radix sort (sort.hip) of the runs by (tid, bin), a second merge of runs that have become neighbours
// (prev.end == cur.beg in the inflated stream), and the host packs the bytes from the sorted chunks.
// rec_parse_kernel, the scorer and strl_front_begin's per-read state are not involved.
//
// The same builder also hangs off `strling extract`'s own pass (strl_front_index_*): behind rec_parse_kernel the
// per-record step reads the dense columns the parse has just written instead of the records, the run base is a running total in
// the device's state words, and the host learns of counts and refusals one chunk late, from a copy it never waits for.
//
// And off a finished `strling sort` (strl_bamsort_index): the records are those of the sort's arena in sorted
// order, a launch of the per-record step takes a tile of them, and a virtual offset is arithmetic on the record's offset in the
// output stream plus one load from the table of the members the host wrote (bamsort_core.h bsort_voff).
#include <string.h>
#include <algorithm>
#include <deque>
#include "front.h"
#include "sort.h"
#include "device_util.h"
#include "bam_rec.h"
#include "bamindex_core.h"
#include "bamsort_core.h"

namespace strl {

struct BaiRun { uint64_t key, beg_v, end_v, beg_abs, end_abs; };   // key = tid << key_shift | bin; virtual offsets; offsets in the inflated stream
struct BaiLast {          // the last record so far
  uint64_t key, end_v, end_abs;
  int32_t tid, pos, end_win, pad;
};
struct BaiState {         // device words of the builder; the host reads them back behind every chunk
  uint64_t err_ord[BAI_ERR_KINDS];   // ordinal of the first record of each kind of refusal, ~0 = none
  uint64_t n_no_coor;
  uint32_t n_heads, pad;             // runs that start in the chunk just scanned / chunks after the merge
  BaiLast last[2];                   // [parity of the chunk]: read from one, written to the other
  uint64_t run_base, run_total;      // (builder behind extract) runs in front of the chunk just scanned / runs so far: kept by the scan
  uint32_t overflow, pad2;           // (builder behind extract) a run did not fit the table: never written, reported at the end
};

struct BaiCols {           // the parse kernel's dense columns of the chunk's records (front.hip rec_parse_kernel)
  const int32_t *tid, *pos, *end;
  const uint32_t *fragw;   // flag in the low 16 bits
  uint32_t rec_end;        // buffer offset behind the chunk's last complete record
};
struct BaiSorted {         // the records of a finished sort (bamsort.hip): record i of the launch is the record of rank j0 + i
  BsortView V;
  uint64_t j0;
  const uint64_t *member_off;      // [n_members + 1] file offset of every member of the output, the EOF block's last
  uint64_t n_members;
};
constexpr int BAI_SRC_BYTES = 0, BAI_SRC_COLS = 1, BAI_SRC_SORTED = 2;      // where the per-record step takes its records from
struct BaiPush {
  const uint8_t *U;
  const uint32_t *recoff;
  uint32_t n;
  const int64_t *vrel;      // [vm + 1] offset in the chunk's buffer of each block's first inflated byte (blocks of the previous
  const uint64_t *vfoff;    //          chunks that the carried record may start in come first); file offset of the block.  [vm]: the end
  uint32_t vm;
  int64_t abs0;             // offset in the file's inflated stream of the buffer's byte 0
  uint64_t ord0;            // ordinal of the chunk's first record
  int32_t n_ref;
  const uint64_t *win_off;  // [n_ref + 1] first window of each reference in lin[]
  uint64_t *lin, *ref_beg, *ref_end, *ref_cnt;
  BaiState *S;
  uint32_t par;
  uint8_t *flag;
  uint32_t *blk_cnt;
  BaiRun *runs;
  uint64_t run_base;        // first slot of the chunk's runs, when the host knows it (run_acc == nullptr)
  const uint64_t *run_acc;  // ... else &BaiState::run_base on the device
  uint64_t run_cap;         // slots of runs[]
  BaiCols C;
  BaiSorted Z;
  BaiScheme sch;            // read by the kernels only where the scheme is not a .bai's (template parameter BAI)
};

__device__ __forceinline__ void bai_read(const uint8_t *U, uint32_t q, BaiRec &r) {
  const uint8_t *R = U + q;
  r.bs = ld32u(R);
  r.tid = (int32_t)ld32u(R + 4); r.pos = (int32_t)ld32u(R + 8);
  r.flag = ld16u(R + 18);
  const int64_t e = bam_rec_end(R);             // (the CIGAR lies inside the record: rec_header's rule, checked by the scan's walk)
  r.end = e > 0x7fffffffll ? 0x7fffffff : (int32_t)e;
}
// the record's five numbers: from its bytes, or (COLS) from the parse's columns -- the byte length is the distance to the next
// record (records lie back to back), end is bam_endpos as rec_parse_kernel computed it --, or (SORTED) from the sort's arena:
// slab, offset and length are held against the slab's used bytes as bsort_gather_kernel holds them, the CIGAR walk against the
// length; a record that fails either is refused as one without a valid refID (the sort's own checks leave none)
template <int SRC> __device__ __forceinline__ void bai_fetch(const BaiPush &P, uint32_t i, BaiRec &r) {
  if constexpr (SRC == BAI_SRC_SORTED) {
    const BsortView &V = P.Z.V;
    r = BaiRec{-2, -1, 0, 0, 0};
    const uint32_t p = V.perm[P.Z.j0 + i];
    if (p >= V.n_records) return;
    const uint64_t s = V.src[p], sl = s >> BSORT_SLAB_SHIFT, so = s & BSORT_SLAB_MASK;
    const uint32_t len = V.len[p];
    if (sl >= V.n_slabs || so > V.slab_used[sl] || len > V.slab_used[sl] - so) return;
    if (!bai_read_bounded(V.slab[sl] + so, len, r)) r = BaiRec{-2, -1, 0, 0, 0};
  } else if constexpr (SRC == BAI_SRC_COLS) {
    r.tid = P.C.tid[i]; r.pos = P.C.pos[i]; r.end = P.C.end[i]; r.flag = P.C.fragw[i] & 0xffffu;
    if (r.end <= r.pos) r.end = 0x7fffffff;     // (a reference span that left 31 bits: bai_read's clamp)
    r.bs = (i + 1u < P.n ? P.recoff[i + 1u] : P.C.rec_end) - P.recoff[i] - 4u;
  } else {
    bai_read(P.U, P.recoff[i], r);
  }
}
template <bool BAI> __device__ __forceinline__ int32_t bai_shift(const BaiPush &P) { return BAI ? 14 : P.sch.min_shift; }
// a record the index can hold: a reference of the header, 0 <= pos, end <= what the scheme addresses (2^29 for a .bai), its last
// window one of the reference's (l_ref and 1 Mbase behind it: aligners do leave reads that hang over the end of a contig).  else the kind of refusal
template <bool BAI> __device__ __forceinline__ int bai_refusal(const BaiRec &r, const BaiPush &P) {
  return bai_refusal_rule(r.tid, r.pos, r.end, P.n_ref, BAI ? BAI_MAX_POS : P.sch.max_end, bai_shift<BAI>(P), [&](int32_t t) { return P.win_off[t + 1] - P.win_off[t]; });
}
template <bool BAI> __device__ __forceinline__ uint64_t bai_key(const BaiRec &r, const BaiPush &P, bool indexable) {
  const int32_t ks = BAI ? 16 : P.sch.key_shift;
  if (r.tid < 0 || !indexable) return (uint64_t)(uint32_t)P.n_ref << ks;
  return ((uint64_t)(uint32_t)r.tid << ks) | (BAI ? bai_reg2bin(r.pos, r.end) : csi_reg2bin(r.pos, r.end, P.sch.min_shift, P.sch.depth));
}
// virtual offset of the byte at buffer offset q: the last block that starts at or in front of it (vrel[0] <= q <= vrel[m])
__device__ __forceinline__ uint64_t bai_voff(const int64_t *vrel, const uint64_t *vfoff, uint32_t m, int64_t q) {
  uint32_t lo = 0, hi = m;
  while (lo < hi) {
    const uint32_t mid = (lo + hi + 1u) >> 1;
    if (vrel[mid] <= q) lo = mid; else hi = mid - 1u;
  }
  return (vfoff[lo] << 16) | (uint64_t)(q - vrel[lo]);
}

// where record i begins / the byte behind it: virtual offset, offset in the inflated stream
template <int SRC> __device__ __forceinline__ void bai_beg(const BaiPush &P, uint32_t i, uint64_t &v, uint64_t &abs) {
  if constexpr (SRC == BAI_SRC_SORTED) { abs = P.Z.V.off[P.Z.j0 + i]; v = bsort_voff(P.Z.member_off, P.Z.n_members, P.Z.V.stream_bytes, abs); }
  else { const uint32_t q = P.recoff[i]; v = bai_voff(P.vrel, P.vfoff, P.vm, (int64_t)q); abs = (uint64_t)(P.abs0 + (int64_t)q); }
}
template <int SRC> __device__ __forceinline__ void bai_end(const BaiPush &P, uint32_t i, const BaiRec &r, uint64_t &v, uint64_t &abs) {
  if constexpr (SRC == BAI_SRC_SORTED) { abs = P.Z.V.off[P.Z.j0 + i + 1]; v = bsort_voff(P.Z.member_off, P.Z.n_members, P.Z.V.stream_bytes, abs); }
  else { const int64_t e = (int64_t)P.recoff[i] + 4 + (int64_t)r.bs; v = bai_voff(P.vrel, P.vfoff, P.vm, e); abs = (uint64_t)(P.abs0 + e); }
}

// the per-record step; the rules (refusals, bin, windows, virtual offsets, run heads) are this one body for every source
template <int SRC, bool BAI> __device__ __forceinline__ void bai_record_body(const BaiPush &P) {
  const int32_t m = bai_shift<BAI>(P);
  const uint32_t i = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u;
  const bool act = i < P.n;
  BaiRec r{-1, -1, 0, 0, 0};
  int bad = -1;
  if (act) { bai_fetch<SRC>(P, i, r); bad = bai_refusal<BAI>(r, P); }
  const bool placed = act && r.tid >= 0 && bad < 0;
  const uint64_t key = act ? bai_key<BAI>(r, P, bad < 0) : BAI_KEY_NONE;
  const int32_t end_win = placed ? (r.end - 1) >> m : -1;
  // the record in front: the lane below, or (first lane of a wave) read again / the previous chunk's last
  int32_t ptid = __shfl_up(r.tid, 1), ppos = __shfl_up(r.pos, 1), pwin = __shfl_up(end_win, 1);
  uint64_t pkey = __shfl_up(key, 1);
  if (act && lane == 0) {
    if (i == 0) { const BaiLast &L = P.S->last[P.par]; ptid = L.tid; ppos = L.pos; pwin = L.end_win; pkey = L.key; }
    else {
      BaiRec p;
      bai_fetch<SRC>(P, i - 1u, p);
      const bool pok = bai_refusal<BAI>(p, P) < 0;
      ptid = p.tid; ppos = p.pos; pkey = bai_key<BAI>(p, P, pok);
      pwin = (p.tid >= 0 && pok) ? (p.end - 1) >> m : -1;
    }
  }
  uint64_t beg_v = 0, end_v = 0, beg_abs = 0, end_abs = 0;
  if (act) {
    const uint64_t ord = P.ord0 + i;
    if (bad >= 0) atomicMin(reinterpret_cast<unsigned long long *>(&P.S->err_ord[bad]), (unsigned long long)ord);
    // coordinate order: (tid, pos) does not decrease, tid = -1 only at the end
    const uint32_t uc = (uint32_t)r.tid, up = (uint32_t)ptid;
    if (pkey != BAI_KEY_NONE && (uc < up || (uc == up && r.tid >= 0 && r.pos < ppos)))
      atomicMin(reinterpret_cast<unsigned long long *>(&P.S->err_ord[BAI_E_UNSORTED]), (unsigned long long)ord);
    bai_beg<SRC>(P, i, beg_v, beg_abs);
    bai_end<SRC>(P, i, r, end_v, end_abs);
  }
  // linear index: the windows no record in front of this one has reached (in a sorted stream the lane below covers all
  // but the window a record is the first to enter; an N skip of hundreds of kilobases enters many)
  if (placed) {
    const int32_t w0 = r.pos >> m, from = (ptid == r.tid && pwin >= w0) ? pwin + 1 : w0;
    uint64_t *lin = P.lin + P.win_off[r.tid];
    for (int32_t w = from; w <= end_win; ++w) atomicMin(reinterpret_cast<unsigned long long *>(&lin[w]), (unsigned long long)beg_v);
  }
  // per reference: span, mapped / placed-unmapped counts -- one lane of a wave whose records share a reference
  const unsigned long long pm = __ballot(placed);
  if (pm) {
    const int first = __ffsll((long long)pm) - 1, last = 63 - __clzll((long long)pm);
    const int32_t t0 = __shfl(r.tid, first);
    const unsigned long long same = __ballot(placed && r.tid == t0), un = __ballot(placed && (r.flag & 4u));
    const uint64_t last_end = __shfl(end_v, last);
    if (same == pm) {
      if ((int)lane == first) {
        atomicMin(reinterpret_cast<unsigned long long *>(&P.ref_beg[t0]), (unsigned long long)beg_v);
        atomicMax(reinterpret_cast<unsigned long long *>(&P.ref_end[t0]), (unsigned long long)last_end);
        const unsigned n_un = (unsigned)__popcll(un), n_map = (unsigned)__popcll(pm) - n_un;
        if (n_map) atomicAdd(reinterpret_cast<unsigned long long *>(&P.ref_cnt[2 * t0]), (unsigned long long)n_map);
        if (n_un) atomicAdd(reinterpret_cast<unsigned long long *>(&P.ref_cnt[2 * t0 + 1]), (unsigned long long)n_un);
      }
    } else if (placed) {
      atomicMin(reinterpret_cast<unsigned long long *>(&P.ref_beg[r.tid]), (unsigned long long)beg_v);
      atomicMax(reinterpret_cast<unsigned long long *>(&P.ref_end[r.tid]), (unsigned long long)end_v);
      atomicAdd(reinterpret_cast<unsigned long long *>(&P.ref_cnt[2 * r.tid + ((r.flag & 4u) ? 1 : 0)]), 1ull);
    }
  }
  const unsigned long long nc = __ballot(act && r.tid < 0);
  if (nc && lane == 0) atomicAdd(reinterpret_cast<unsigned long long *>(&P.S->n_no_coor), (unsigned long long)__popcll(nc));
  const bool head = act && key != pkey;
  if (act) P.flag[i] = head ? 1 : 0;
  const int heads = __syncthreads_count(head);
  if (threadIdx.x == 0) P.blk_cnt[blockIdx.x] = (uint32_t)heads;
  if (act && i == P.n - 1) {
    BaiLast L;
    L.key = key; L.end_v = end_v; L.end_abs = end_abs;
    L.tid = r.tid; L.pos = r.pos; L.end_win = end_win; L.pad = 0;
    P.S->last[P.par ^ 1u] = L;
  }
}
// <BAI>: the scheme is a .bai's (14, 5), compiled in -- the code of that path is what it was before schemes; else read from P.sch
template <bool BAI> __global__ __launch_bounds__(256) void bai_record_kernel(BaiPush P) { bai_record_body<BAI_SRC_BYTES, BAI>(P); }
template <bool BAI> __global__ __launch_bounds__(256) void bai_record_cols_kernel(BaiPush P) { bai_record_body<BAI_SRC_COLS, BAI>(P); }
template <bool BAI> __global__ __launch_bounds__(256) void bai_record_sorted_kernel(BaiPush P) { bai_record_body<BAI_SRC_SORTED, BAI>(P); }

// One block: cnt[0, n) -> exclusive sums in place, the total to *total; acc (if given): acc[0] = the running total so far (the
// base of this chunk's runs), acc[1] += total -- the host is not asked
__global__ __launch_bounds__(1024) void bai_scan_kernel(uint32_t *cnt, uint32_t n, uint32_t *total, uint64_t *acc) {
  __shared__ uint32_t part[1024];
  const uint32_t t = threadIdx.x, per = (n + 1023u) / 1024u, a = min(n, t * per), b = min(n, a + per);
  uint32_t s = 0;
  for (uint32_t k = a; k < b; ++k) s += cnt[k];
  part[t] = s;
  __syncthreads();
  if (t == 0) { uint32_t run = 0; for (int k = 0; k < 1024; ++k) { const uint32_t v = part[k]; part[k] = run; run += v; } *total = run; if (acc) { acc[0] = acc[1]; acc[1] += run; } }
  __syncthreads();
  uint32_t run = part[t];
  for (uint32_t k = a; k < b; ++k) { const uint32_t v = cnt[k]; cnt[k] = run; run += v; }
}

// rank of a flagged thread among the flagged threads of its 256-thread block
__device__ __forceinline__ uint32_t bai_block_rank(bool f) {
  __shared__ uint32_t wsum[4];
  const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  const unsigned long long m = __ballot(f);
  if (lane == 0) wsum[w] = (uint32_t)__popcll(m);
  __syncthreads();
  uint32_t r = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
  for (uint32_t k = 0; k < w; ++k) r += wsum[k];
  return r;
}

template <int SRC, bool BAI> __device__ __forceinline__ void bai_emit_body(const BaiPush &P) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  const bool head = i < P.n && P.flag[i];
  const uint32_t rank = bai_block_rank(head);
  if (!head) return;
  const uint64_t slot = (P.run_acc ? *P.run_acc : P.run_base) + P.blk_cnt[blockIdx.x] + rank;
  if (slot >= P.run_cap) { P.S->overflow = 1u; return; }       // (the host sizes the table for every record of the chunk: not reached)
  BaiRec r;
  bai_fetch<SRC>(P, i, r);
  uint64_t beg_v, beg_abs;
  bai_beg<SRC>(P, i, beg_v, beg_abs);
  BaiRun &R = P.runs[slot];
  R.key = bai_key<BAI>(r, P, bai_refusal<BAI>(r, P) < 0); R.beg_v = beg_v; R.beg_abs = beg_abs;
  if (slot) { BaiRun &B = P.runs[slot - 1]; B.end_v = beg_v; B.end_abs = beg_abs; }
}
template <bool BAI> __global__ __launch_bounds__(256) void bai_emit_kernel(BaiPush P) { bai_emit_body<BAI_SRC_BYTES, BAI>(P); }
template <bool BAI> __global__ __launch_bounds__(256) void bai_emit_cols_kernel(BaiPush P) { bai_emit_body<BAI_SRC_COLS, BAI>(P); }
template <bool BAI> __global__ __launch_bounds__(256) void bai_emit_sorted_kernel(BaiPush P) { bai_emit_body<BAI_SRC_SORTED, BAI>(P); }

// finish: the open run ends behind the last record; sort keys of the runs
__global__ void bai_keys_kernel(BaiRun *runs, uint32_t n, const BaiState *S, uint32_t par, uint64_t *keys, uint32_t *vals) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (i == n - 1) { runs[i].end_v = S->last[par].end_v; runs[i].end_abs = S->last[par].end_abs; }
  keys[i] = runs[i].key; vals[i] = i;
}
// sorted by (tid, bin), file order kept inside a key: a chunk starts where the key changes or the run in front does not end here
__global__ __launch_bounds__(256) void bai_merge_flag_kernel(const BaiRun *runs, const uint64_t *keys, const uint32_t *vals, uint32_t n, uint8_t *flag, uint32_t *blk_cnt) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  bool head = false;
  if (j < n) {
    head = j == 0 || keys[j] != keys[j - 1] || runs[vals[j - 1]].end_abs != runs[vals[j]].beg_abs;
    flag[j] = head ? 1 : 0;
  }
  const int heads = __syncthreads_count(head);
  if (threadIdx.x == 0) blk_cnt[blockIdx.x] = (uint32_t)heads;
}
__global__ __launch_bounds__(256) void bai_merge_emit_kernel(const BaiRun *runs, const uint64_t *keys, const uint32_t *vals, uint32_t n, const uint8_t *flag,
                                                             const uint32_t *blk_cnt, const uint32_t *total, BaiChunk *out) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  const bool head = j < n && flag[j];
  const uint32_t rank = bai_block_rank(head);
  if (j < n && j == n - 1) out[*total - 1].end_v = runs[vals[j]].end_v;
  if (!head) return;
  const uint32_t slot = blk_cnt[blockIdx.x] + rank;
  out[slot].key = keys[j]; out[slot].beg_v = runs[vals[j]].beg_v;
  if (j) out[slot - 1].end_v = runs[vals[j - 1]].end_v;
}
__global__ void bai_fill_kernel(uint64_t *p, size_t n, uint64_t v) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) p[i] = v;
}

struct BaiBlock { int64_t abs; uint64_t foff; };       // a pushed block: offset of its first byte in the inflated stream, file offset
struct strl_bai {
  int32_t n_ref = 0;
  BaiScheme sch{14, 5, 16, BAI_MAX_POS};
  bool auto_depth = false;                            // the depth follows from the header's longest reference (samtools' rule)
  bool csi = false;                                   // the bytes are a CSI payload (uncompressed), not a .bai -- whatever the scheme
  bool bai_scheme() const { return sch.min_shift == 14 && sch.depth == 5; }      // the kernels with the scheme compiled in
  std::vector<int32_t> l_ref;
  std::vector<uint64_t> win_off;                      // [n_ref + 1]
  DevBuf d_winoff, lin, ref_beg, ref_end, ref_cnt, state, runs, flag, blk_cnt;
  DevBuf vt[2];                                       // [slot] block table of the chunk: vrel[m + 1] | vfoff[m + 1]
  uint8_t *h_vt[2] = {nullptr, nullptr};              // pinned source of it
  size_t h_vt_cap[2] = {0, 0};
  uint32_t vm[2] = {0, 0};
  int64_t abs0[2] = {0, 0};
  BaiState *h_state = nullptr;                        // pinned
  std::vector<BaiBlock> tail;                         // blocks that hold the last FRONT_CARRY_MAX inflated bytes pushed so far
  int64_t abs_total = 0;                              // inflated bytes pushed so far
  uint64_t end_off = 0;                               // file offset behind the last block pushed
  uint64_t chunks = 0, done = 0;                      // pushed / indexed
  uint64_t n_records = 0, n_runs = 0, n_chunks = 0;
  uint32_t par = 0;
  bool finished = false;
  std::vector<uint8_t> bytes;                         // the serialized index
  // ---- behind `strling extract`'s own pass (strl_front_index_*): nothing here is waited for inside the chunk loop
  bool attached = false;
  int fail_rc = 0;                                    // the index ended early (the extraction goes on): reported by strl_front_index_finish
  std::string fail;
  struct Offsets { std::vector<uint64_t> block_off; uint64_t end_off; };
  std::deque<Offsets> want;                           // strl_front_index_blocks: file offsets of the chunks handed over next, in file order
  uint64_t want_end = 0;                              // file offset behind the last block announced
  bool have_table[2] = {false, false};                // [slot] the chunk in the slot came with its offsets
  uint64_t run_cap = 0;                               // slots of runs
  uint64_t known_runs = 0, known_at = 0;              // the device's running total as last seen, and the records indexed up to that look
  BaiState *h_snap = nullptr;                         // pinned: a copy of the state words made behind a chunk, looked at a chunk later
  hipEvent_t ev_snap = nullptr;
  bool snap_flying = false, refusal_seen = false;
  uint64_t snap_at = 0;
  std::vector<DevBuf> trash;                          // outgrown tables (kernels in flight may still use them): freed with the builder
};

void bai_destroy(strl_bai *B) {
  if (!B) return;
  for (uint8_t *p : B->h_vt) if (p) (void)hipHostFree(p);
  if (B->h_state) (void)hipHostFree(B->h_state);
  if (B->h_snap) (void)hipHostFree(B->h_snap);
  if (B->ev_snap) (void)hipEventDestroy(B->ev_snap);
  delete B;
}

static int bai_refuse(const strl_bai *B, const BaiState &S) {
  const uint32_t kind = bai_first_refusal(S.err_ord);
  if (kind == BAI_ERR_KINDS) return STRL_OK;
  std::string msg;
  const int rc = bai_refusal_text(kind, S.err_ord[kind], B->csi, B->auto_depth, B->sch, B->n_ref, msg);
  set_error("%s", msg.c_str());
  return rc;
}

// the runs of the chunk in slot si (its record scan was enqueued by the push before): waits on the host for the scan's counts
static int bai_index_chunk(strl_ctx *c, strl_front *F, strl_bai *B, int si) {
  FrontSlot &S = F->slot[si];
  STRL_HIP(hipEventSynchronize(S.ev_a));
  const FrontInfo I = S.h_info[0];
  if (I.err & FRONT_ERR_INFLATE) { set_error("invalid BGZF block (DEFLATE data or ISIZE)"); return STRL_ERR_FORMAT; }
  if (I.err & FRONT_ERR_CRC) { set_error("CRC32 checksum mismatch in a BGZF block"); return STRL_ERR_CRC; }
  if (I.err & FRONT_ERR_RECORD) { set_error("malformed BAM record"); return STRL_ERR_FORMAT; }
  if (I.err & FRONT_ERR_CARRY) { set_error("BAM record of more than %u bytes", FRONT_CARRY_MAX); return STRL_ERR_FORMAT; }
  const uint32_t n = I.n_records;
  hipStream_t st = c->stream;
  int rc;
  if (n) {
    const uint32_t nblk = (n + 255u) / 256u, m = B->vm[si];
    if ((rc = B->flag.reserve((size_t)n + 64)) || (rc = B->blk_cnt.reserve((size_t)nblk * 4 + 64)) || (rc = B->vt[si].reserve((size_t)(m + 1) * 16))) return rc;
    STRL_HIP(hipMemcpyAsync(B->vt[si].p, B->h_vt[si], (size_t)(m + 1) * 16, hipMemcpyHostToDevice, st));
    BaiPush P{};
    P.U = S.infl.as<uint8_t>(); P.recoff = S.recoff.as<uint32_t>(); P.n = n;
    P.vrel = B->vt[si].as<int64_t>(); P.vfoff = B->vt[si].as<uint64_t>() + (m + 1); P.vm = m;
    P.abs0 = B->abs0[si]; P.ord0 = B->n_records;
    P.n_ref = B->n_ref; P.win_off = B->d_winoff.as<uint64_t>();
    P.lin = B->lin.as<uint64_t>(); P.ref_beg = B->ref_beg.as<uint64_t>(); P.ref_end = B->ref_end.as<uint64_t>(); P.ref_cnt = B->ref_cnt.as<uint64_t>();
    P.S = B->state.as<BaiState>(); P.par = B->par; P.flag = B->flag.as<uint8_t>(); P.blk_cnt = B->blk_cnt.as<uint32_t>();
    P.sch = B->sch;
    const bool bai = B->bai_scheme();
    hipLaunchKernelGGL(bai ? bai_record_kernel<true> : bai_record_kernel<false>, dim3(nblk), dim3(256), 0, st, P);
    STRL_HIP(hipGetLastError());
    hipLaunchKernelGGL(bai_scan_kernel, dim3(1), dim3(1024), 0, st, P.blk_cnt, nblk, &P.S->n_heads, (uint64_t *)nullptr);
    STRL_HIP(hipGetLastError());
    STRL_HIP(hipMemcpyAsync(B->h_state, B->state.p, sizeof(BaiState), hipMemcpyDeviceToHost, st));
    STRL_HIP(hipStreamSynchronize(st));                 // the number of runs that start in the chunk: the table grows by exactly that
    if ((rc = bai_refuse(B, *B->h_state))) return rc;
    const uint64_t heads = B->h_state->n_heads;
    if (B->n_runs + heads > 0x7ffffff0ull) { set_error("more than 2^31 runs of equal (reference, bin): beyond one device sort"); return STRL_ERR_LIMIT; }
    if (heads) {
      if ((rc = B->runs.grow((size_t)(B->n_runs + heads) * sizeof(BaiRun), (size_t)B->n_runs * sizeof(BaiRun), st))) return rc;
      P.runs = B->runs.as<BaiRun>(); P.run_base = B->n_runs; P.run_acc = nullptr; P.run_cap = B->runs.cap / sizeof(BaiRun);
      hipLaunchKernelGGL(bai ? bai_emit_kernel<true> : bai_emit_kernel<false>, dim3(nblk), dim3(256), 0, st, P);
      STRL_HIP(hipGetLastError());
      B->n_runs += heads;
    }
    B->n_records += n;
    B->par ^= 1u;
  }
  STRL_HIP(hipEventRecord(S.ev_b, st));      // the slot's inflated bytes and record table may be overwritten behind this
  S.b_pending = true;
  return STRL_OK;
}

}  // namespace strl

using namespace strl;

// the schemes the builder takes (depth < 0: the rule, see bai_scheme_make)
static int csi_check(int32_t m, int32_t d) {
  std::string err;
  if (csi_scheme_ok(m, d, err)) return STRL_OK;
  set_error("%s", err.c_str());
  return STRL_ERR_ARG;
}
// the resident tables of a new builder B (linear index, per-reference words, state words), which its owner already holds.
// csi: null = a .bai; else {min_shift, depth}, depth < 0 = samtools' rule (the smallest depth whose scheme reaches max(l_ref) + 256)
static int bai_tables(strl_ctx *c, strl_bai *B, int32_t n_ref, const int32_t *l_ref, const int32_t *csi) {
  int rc;
  std::string err;
  if (!bai_scheme_make(csi, n_ref, l_ref, B->sch, err)) { set_error("%s", err.c_str()); return STRL_ERR_ARG; }
  B->n_ref = n_ref;
  B->csi = csi != nullptr;
  B->auto_depth = csi && csi[1] < 0;
  B->l_ref.assign(l_ref, l_ref + n_ref);
  bai_windows(B->sch, n_ref, l_ref, B->win_off);
  const size_t nw = (size_t)B->win_off[(size_t)n_ref], nr = (size_t)n_ref;
  if ((rc = B->d_winoff.reserve((nr + 1) * 8)) || (rc = B->lin.reserve(nw * 8 + 16)) || (rc = B->ref_beg.reserve(nr * 8 + 16)) ||
      (rc = B->ref_end.reserve(nr * 8 + 16)) || (rc = B->ref_cnt.reserve(nr * 16 + 16)) || (rc = B->state.reserve(sizeof(BaiState))))
    return rc;
  STRL_HIP(hipHostMalloc(reinterpret_cast<void **>(&B->h_state), sizeof(BaiState), hipHostMallocDefault));
  hipStream_t st = c->stream;
  STRL_HIP(hipMemcpyAsync(B->d_winoff.p, B->win_off.data(), (nr + 1) * 8, hipMemcpyHostToDevice, st));
  if (nw) hipLaunchKernelGGL(bai_fill_kernel, dim3((unsigned)std::min<size_t>((nw + 255) / 256, 1024)), dim3(256), 0, st, B->lin.as<uint64_t>(), nw, ~0ull);
  if (nr) hipLaunchKernelGGL(bai_fill_kernel, dim3((unsigned)std::min<size_t>((nr + 255) / 256, 1024)), dim3(256), 0, st, B->ref_beg.as<uint64_t>(), nr, ~0ull);
  STRL_HIP(hipGetLastError());
  if (nr) { STRL_HIP(hipMemsetAsync(B->ref_end.p, 0, nr * 8, st)); STRL_HIP(hipMemsetAsync(B->ref_cnt.p, 0, nr * 16, st)); }
  BaiState &H = *B->h_state;
  memset(&H, 0, sizeof H);
  for (uint64_t &e : H.err_ord) e = ~0ull;
  for (BaiLast &L : H.last) { L.key = BAI_KEY_NONE; L.tid = 0; L.pos = -1; L.end_win = -1; }
  STRL_HIP(hipMemcpyAsync(B->state.p, &H, sizeof H, hipMemcpyHostToDevice, st));
  STRL_HIP(hipStreamSynchronize(st));
  return STRL_OK;
}
// ... of a new builder on the context; replaces c->bai
static int bai_setup(strl_ctx *c, int32_t n_ref, const int32_t *l_ref, const int32_t *csi) {
  int rc;
  if (csi && (rc = csi_check(csi[0], csi[1]))) return rc;
  if (c->bai) { bai_destroy(c->bai); c->bai = nullptr; }
  c->bai = new strl_bai();
  return bai_tables(c, c->bai, n_ref, l_ref, csi);
}

// what a chunk's block offsets must be: ascending, behind `floor` (the end of what came before), 48 bits; ISIZE (where known) in [1, 65536]
static int bai_check_blocks(const char *who, uint64_t floor, const uint64_t *block_off, uint64_t end_off, const uint32_t *isize, uint32_t n_blocks) {
  for (uint32_t i = 0; i < n_blocks; ++i)
    if (block_off[i] >= (1ull << 48) || (i && block_off[i] <= block_off[i - 1]) || block_off[i] < floor || (isize && (isize[i] > 65536u || !isize[i]))) {
      set_error("%s: block %u: file offsets must ascend and fit 48 bits, ISIZE must be in [1, 65536]", who, i);
      return STRL_ERR_ARG;
    }
  if (end_off <= block_off[n_blocks - 1] || end_off >= (1ull << 48)) { set_error("%s: end_off is not behind the last block", who); return STRL_ERR_ARG; }
  return STRL_OK;
}

// block table of the chunk that goes to slot si, in the slot's pinned source (the previous chunk of the slot has left it): where
// each block's first inflated byte lies in the chunk's buffer and the block's file offset, the blocks of the previous chunks
// that the carried record may start in first (`tail`), the end last
static int bai_block_table(strl_bai *B, int si, const uint64_t *block_off, uint64_t end_off, const uint32_t *isize, uint32_t n_blocks) {
  const size_t m = B->tail.size() + n_blocks;
  if (B->h_vt_cap[si] < (m + 1) * 16) {
    if (B->h_vt[si]) { (void)hipHostFree(B->h_vt[si]); B->h_vt[si] = nullptr; }
    B->h_vt_cap[si] = (m + 1) * 16 + (m + 1) * 4 + 4096;
    STRL_HIP(hipHostMalloc(reinterpret_cast<void **>(&B->h_vt[si]), B->h_vt_cap[si], hipHostMallocDefault));
  }
  int64_t *vrel = reinterpret_cast<int64_t *>(B->h_vt[si]);
  uint64_t *vfoff = reinterpret_cast<uint64_t *>(B->h_vt[si]) + (m + 1);
  const int64_t base = (int64_t)FRONT_CARRY_MAX - B->abs_total;      // buffer offset of the inflated stream's byte 0
  size_t k = 0;
  for (const BaiBlock &t : B->tail) { vrel[k] = base + t.abs; vfoff[k] = t.foff; ++k; }
  int64_t at = B->abs_total;
  for (uint32_t i = 0; i < n_blocks; ++i) {
    vrel[k] = base + at; vfoff[k] = block_off[i]; ++k;
    B->tail.push_back(BaiBlock{at, block_off[i]});
    at += isize[i];
  }
  vrel[m] = base + at; vfoff[m] = end_off;
  B->vm[si] = (uint32_t)m;
  B->abs0[si] = -base;
  B->abs_total = at;
  B->end_off = end_off;
  size_t drop = 0;                                                    // keep the blocks that hold the last FRONT_CARRY_MAX bytes
  while (drop + 1 < B->tail.size() && B->tail[drop + 1].abs <= at - (int64_t)FRONT_CARRY_MAX) ++drop;
  B->tail.erase(B->tail.begin(), B->tail.begin() + (ptrdiff_t)drop);
  return STRL_OK;
}

extern "C" int strl_bamindex_begin(strl_ctx *c, int32_t n_ref, const int32_t *l_ref, uint64_t first_record_offset) {
  if (!c || n_ref < 0 || (n_ref && !l_ref)) { set_error("strl_bamindex_begin: bad argument"); return STRL_ERR_ARG; }
  int rc;
  if ((rc = front_begin_scan(c, n_ref, first_record_offset))) return rc;
  return bai_setup(c, n_ref, l_ref, nullptr);
}

extern "C" int strl_bamindex_begin_csi(strl_ctx *c, int32_t n_ref, const int32_t *l_ref, uint64_t first_record_offset, int32_t min_shift, int32_t depth) {
  if (!c || n_ref < 0 || (n_ref && !l_ref)) { set_error("strl_bamindex_begin_csi: bad argument"); return STRL_ERR_ARG; }
  int rc;
  if ((rc = csi_check(min_shift, depth)) || (rc = front_begin_scan(c, n_ref, first_record_offset))) return rc;
  const int32_t csi[2] = {min_shift, depth};
  return bai_setup(c, n_ref, l_ref, csi);
}

extern "C" int strl_bamindex_reserve(strl_ctx *c, uint32_t max_blocks, uint64_t max_comp_bytes) {
  if (!c || !c->bai || !c->front || !max_blocks) { set_error("strl_bamindex_reserve: bad argument / no strl_bamindex_begin"); return STRL_ERR_ARG; }
  STRL_HIP(hipSetDevice(c->device));
  int rc;
  const uint64_t rec_cap = (uint64_t)max_blocks * 65280u / 36 + 16;      // no record is shorter than 36 bytes (front_reserve's bound)
  if ((rc = c->bai->flag.reserve((size_t)rec_cap + 64)) || (rc = c->bai->blk_cnt.reserve((size_t)(rec_cap / 256 + 2) * 4 + 64))) return rc;
  return front_reserve(c, c->front, max_blocks, max_comp_bytes);
}

extern "C" int strl_bamindex_push(strl_ctx *c, const uint8_t *comp, uint64_t comp_bytes, const uint64_t *coff, const uint32_t *clen, const uint32_t *isize,
                                  const uint32_t *crc32, const uint64_t *block_off, uint64_t end_off, uint32_t n_blocks) {
  if (!c || !c->bai || !c->front || c->bai->finished || c->bai->attached || (n_blocks && (!comp || !coff || !clen || !isize || !block_off))) {
    set_error("strl_bamindex_push: bad argument / no strl_bamindex_begin");
    return STRL_ERR_ARG;
  }
  if (!n_blocks) return STRL_OK;
  STRL_HIP(hipSetDevice(c->device));
  strl_front *F = c->front;
  strl_bai *B = c->bai;
  const int si = (int)(B->chunks & 1);
  FrontSlot &S = F->slot[si];
  int rc;
  if ((rc = bai_check_blocks("strl_bamindex_push", B->end_off, block_off, end_off, isize, n_blocks))) return rc;
  // the chunk two back has left the slot (its table in h_vt was copied in front of its kernels)
  if (S.b_pending) { STRL_HIP(hipEventSynchronize(S.ev_b)); S.b_pending = false; }
  if ((rc = bai_block_table(B, si, block_off, end_off, isize, n_blocks))) return rc;
  const FrontChunkDesc d{comp, comp_bytes, coff, clen, isize, crc32, n_blocks};
  if ((rc = front_stage_a(c, F, si, d, B->chunks == 0))) return rc;
  ++B->chunks;
  // ... and beside this chunk's inflate, the runs of the previous one
  while (B->done + 1 < B->chunks) {
    if ((rc = bai_index_chunk(c, F, B, (int)(B->done & 1)))) return rc;
    ++B->done;
  }
  return STRL_OK;
}

// the finish step of both builders: every chunk's runs are in the table and the stream has been waited for
static int bai_sort_and_pack(strl_ctx *c, strl_bai *B) {
  hipStream_t st = c->stream;
  int rc;
  // one stable sort of the runs by (tid, bin), the second merge, the chunks to the host
  const uint32_t n = (uint32_t)B->n_runs;
  std::vector<BaiChunk> ch;
  if (n) {
    const int ks = B->sch.key_shift;                      // bits of the bin field (16 for a .bai); the reference field up to n_ref, the key of the unplaced
    int bits = ks + 1;
    while (bits < ks + 32 && ((uint64_t)B->n_ref >> (bits - ks))) ++bits;
    const size_t sb = radix_sort_scratch_bytes(n, bits);
    const uint32_t nblk = (n + 255u) / 256u;
    DevBuf k0, k1, v0, v1, sc, out;
    if ((rc = k0.reserve((size_t)n * 8)) || (rc = k1.reserve((size_t)n * 8)) || (rc = v0.reserve((size_t)n * 4)) || (rc = v1.reserve((size_t)n * 4)) || (rc = sc.reserve(sb)) ||
        (rc = out.reserve((size_t)n * sizeof(BaiChunk))) || (rc = B->flag.reserve((size_t)n + 64)) || (rc = B->blk_cnt.reserve((size_t)nblk * 4 + 64)))
      return rc;
    BaiState *S = B->state.as<BaiState>();
    hipLaunchKernelGGL(bai_keys_kernel, dim3(nblk), dim3(256), 0, st, B->runs.as<BaiRun>(), n, S, B->par, k0.as<uint64_t>(), v0.as<uint32_t>());
    uint32_t *d_n = &S->n_heads;                         // (the device-side count the sort reads)
    hipError_t e = hipMemcpyAsync(d_n, &n, 4, hipMemcpyHostToDevice, st);
    uint64_t *ok = nullptr;
    uint32_t *ov = nullptr;
    int se = 0;
    if (e == hipSuccess) se = radix_sort_pairs(st, d_n, n, k0.as<uint64_t>(), v0.as<uint32_t>(), k1.as<uint64_t>(), v1.as<uint32_t>(), sc.p, sb, 0, bits, &ok, &ov);
    if (e == hipSuccess && !se) {
      hipLaunchKernelGGL(bai_merge_flag_kernel, dim3(nblk), dim3(256), 0, st, B->runs.as<BaiRun>(), ok, ov, n, B->flag.as<uint8_t>(), B->blk_cnt.as<uint32_t>());
      hipLaunchKernelGGL(bai_scan_kernel, dim3(1), dim3(1024), 0, st, B->blk_cnt.as<uint32_t>(), nblk, d_n, (uint64_t *)nullptr);
      hipLaunchKernelGGL(bai_merge_emit_kernel, dim3(nblk), dim3(256), 0, st, B->runs.as<BaiRun>(), ok, ov, n, B->flag.as<uint8_t>(), B->blk_cnt.as<uint32_t>(), d_n, out.as<BaiChunk>());
      e = hipGetLastError();
      if (e == hipSuccess) e = hipMemcpyAsync(B->h_state, B->state.p, sizeof(BaiState), hipMemcpyDeviceToHost, st);
      if (e == hipSuccess) e = hipStreamSynchronize(st);
      if (e == hipSuccess) {
        ch.resize(B->h_state->n_heads);
        if (!ch.empty()) e = hipMemcpy(ch.data(), out.p, ch.size() * sizeof(BaiChunk), hipMemcpyDeviceToHost);
      }
    }
    if (se) { set_error("radix_sort_pairs failed: %s", hipGetErrorString((hipError_t)se)); return STRL_ERR_HIP; }
    if (e != hipSuccess) { set_error("strl_bamindex_finish: %s", hipGetErrorString(e)); return STRL_ERR_HIP; }
  } else {
    STRL_HIP(hipMemcpy(B->h_state, B->state.p, sizeof(BaiState), hipMemcpyDeviceToHost));
  }
  const size_t nr = (size_t)B->n_ref, nw = (size_t)B->win_off[nr];
  std::vector<uint64_t> lin(nw), rb(nr), re(nr), cnt(2 * nr);
  if (nw) STRL_HIP(hipMemcpy(lin.data(), B->lin.p, nw * 8, hipMemcpyDeviceToHost));
  if (nr) {
    STRL_HIP(hipMemcpy(rb.data(), B->ref_beg.p, nr * 8, hipMemcpyDeviceToHost));
    STRL_HIP(hipMemcpy(re.data(), B->ref_end.p, nr * 8, hipMemcpyDeviceToHost));
    STRL_HIP(hipMemcpy(cnt.data(), B->ref_cnt.p, nr * 16, hipMemcpyDeviceToHost));
  }
  B->n_chunks = bai_pack(B->sch, B->csi, B->n_ref, B->win_off, ch, lin, rb, re, cnt, B->h_state->n_no_coor, B->bytes);      // (bamindex_core.h)
  B->finished = true;
  return STRL_OK;
}

extern "C" int strl_bamindex_finish(strl_ctx *c, uint64_t *bai_bytes, strl_bamindex_info *info) {
  if (!c || !c->bai || !c->front || c->bai->attached) { set_error("strl_bamindex_finish without strl_bamindex_begin"); return STRL_ERR_ARG; }
  STRL_HIP(hipSetDevice(c->device));
  strl_front *F = c->front;
  strl_bai *B = c->bai;
  hipStream_t st = c->stream;
  int rc;
  if (!B->finished) {
    for (; B->done < B->chunks; ++B->done)
      if ((rc = bai_index_chunk(c, F, B, (int)(B->done & 1)))) return rc;
    STRL_HIP(hipStreamSynchronize(st));
    if (F->last_slot >= 0 && F->slot[F->last_slot].h_info[0].carry_len) { set_error("the BAM ends inside a record (truncated file)"); return STRL_ERR_FORMAT; }
    if ((rc = bai_sort_and_pack(c, B))) return rc;
  }
  if (bai_bytes) *bai_bytes = B->bytes.size();
  if (info) { info->n_records = B->n_records; info->n_no_coor = B->h_state->n_no_coor; info->n_runs = B->n_runs; info->n_chunks = B->n_chunks; }
  return STRL_OK;
}

// ---- the index as a by-product of `strling extract`'s own pass ----
// The builder hangs off a context whose front end strl_front_begin started.  Per chunk the front end calls bai_front_chunk where
// the chunk is handed over (the block table) and bai_front_index behind its parse (the kernels).  Neither waits for the device
// and neither can fail the extraction: what goes wrong ends the index and is reported by strl_front_index_finish.
static void bai_fail(strl_bai *B, int rc, const char *msg) {
  if (B->fail.empty()) { B->fail_rc = rc; B->fail = msg; }
}
// room for `bytes` in a chunk-temporary table without freeing what kernels in flight may still read (a free waits for the device)
static int bai_room(strl_bai *B, DevBuf &b, size_t bytes) {
  if (b.p && b.cap >= bytes) return STRL_OK;
  DevBuf nb;
  const int rc = nb.reserve(bytes + bytes / 4 + 4096);
  if (rc) return rc;
  if (b.p) B->trash.push_back(std::move(b));
  b = std::move(nb);
  return STRL_OK;
}

static int front_index_begin(strl_ctx *c, const int32_t *l_ref, uint64_t runs0, const int32_t *csi) {
  if (!c || !c->front || !c->x_open || !c->x_front) { set_error("strl_front_index_begin without strl_front_begin"); return STRL_ERR_ARG; }
  strl_front *F = c->front;
  if (F->n_ref && !l_ref) { set_error("strl_front_index_begin: bad argument"); return STRL_ERR_ARG; }
  if (F->chunks || F->not_first || F->next_trim || F->slot[0].staged || F->slot[1].staged) {
    set_error("strl_front_index_begin: the context must get the whole file from its first block (no chunk handed over yet, no share)");
    return STRL_ERR_ARG;
  }
  STRL_HIP(hipSetDevice(c->device));
  int rc;
  if ((rc = bai_setup(c, (int32_t)F->n_ref, l_ref, csi))) return rc;
  strl_bai *B = c->bai;
  B->attached = true;
  B->run_cap = std::max<uint64_t>(runs0 ? runs0 : (1ull << 20), 16);
  if ((rc = B->runs.reserve((size_t)B->run_cap * sizeof(BaiRun)))) return rc;
  STRL_HIP(hipHostMalloc(reinterpret_cast<void **>(&B->h_snap), sizeof(BaiState), hipHostMallocDefault));
  STRL_HIP(hipEventCreateWithFlags(&B->ev_snap, hipEventDisableTiming));
  return STRL_OK;
}
extern "C" int strl_front_index_begin(strl_ctx *c, const int32_t *l_ref, uint64_t runs0) { return front_index_begin(c, l_ref, runs0, nullptr); }
extern "C" int strl_front_index_begin_csi(strl_ctx *c, const int32_t *l_ref, uint64_t runs0, int32_t min_shift, int32_t depth) {
  const int32_t csi[2] = {min_shift, depth};
  return front_index_begin(c, l_ref, runs0, csi);
}

extern "C" int strl_front_index_blocks(strl_ctx *c, const uint64_t *block_off, uint64_t end_off, uint32_t n_blocks) {
  if (!c || !c->bai || !c->bai->attached || !c->front || c->bai->finished || !n_blocks || !block_off) {
    set_error("strl_front_index_blocks: bad argument / no strl_front_index_begin");
    return STRL_ERR_ARG;
  }
  strl_bai *B = c->bai;
  int rc;
  if (!B->fail.empty()) return STRL_OK;          // (the index has ended; strl_front_index_finish says why)
  if ((rc = bai_check_blocks("strl_front_index_blocks", B->want_end, block_off, end_off, nullptr, n_blocks))) return rc;
  if (B->want.size() >= 4) { set_error("strl_front_index_blocks: the offsets of four chunks are waiting for their chunks"); return STRL_ERR_ARG; }
  B->want.push_back(strl_bai::Offsets{std::vector<uint64_t>(block_off, block_off + n_blocks), end_off});
  B->want_end = end_off;
  return STRL_OK;
}

// a chunk has been handed over to slot si (its record scan is queued; the slot's previous chunk has completed): its block table
void strl::bai_front_chunk(strl_ctx *c, int si, const uint32_t *isize, uint32_t n_blocks, bool whole_file) {
  strl_bai *B = c->bai;
  if (!B || !B->attached || B->finished || !B->fail.empty()) return;
  B->have_table[si] = false;
  if (!whole_file) return bai_fail(B, STRL_ERR_ARG, "the context does not get the whole file (a share, or chunks in turn over several contexts): no index");
  if (B->want.empty()) return bai_fail(B, STRL_ERR_ARG, "a chunk was handed over without its block offsets (strl_front_index_blocks)");
  const strl_bai::Offsets W = std::move(B->want.front());
  B->want.pop_front();
  if (W.block_off.size() != n_blocks) return bai_fail(B, STRL_ERR_ARG, "strl_front_index_blocks named another number of blocks than the chunk handed over has");
  for (uint32_t i = 0; i < n_blocks; ++i)
    if (isize[i] > 65536u || !isize[i]) return bai_fail(B, STRL_ERR_ARG, "a block's ISIZE is outside [1, 65536]");
  if (bai_block_table(B, si, W.block_off.data(), W.end_off, isize, n_blocks)) return bai_fail(B, STRL_ERR_HIP, strl_last_error());
  B->have_table[si] = true;
}

// behind the parse of the chunk in slot si, on the context's stream: per-record step over the parse's columns, scan, emit, and a
// copy of the state words that is looked at when a later chunk comes by.  The table holds every run the chunks not yet
// accounted for can start (a chunk of n records starts at most n), so the emit kernel stays inside it whatever the counts are.
void strl::bai_front_index(strl_ctx *c, strl_front *F, int si, const FrontInfo &I, const int32_t *tid, const int32_t *pos, const int32_t *end, const uint32_t *fragw) {
  strl_bai *B = c->bai;
  if (!B || !B->attached || B->finished || !B->fail.empty()) return;
  hipStream_t st = c->stream;
  if (B->snap_flying) {                          // a look, not a wait
    if (hipEventQuery(B->ev_snap) != hipSuccess) (void)hipGetLastError();        // (not ready: not an error to find behind the next launch)
    else B->snap_flying = false;
  }
  if (!B->snap_flying && B->snap_at > B->known_at) {
    B->known_runs = B->h_snap->run_total; B->known_at = B->snap_at;
    for (uint64_t eo : B->h_snap->err_ord) if (eo != ~0ull) B->refusal_seen = true;
  }
  if (B->refusal_seen) return;                   // (what it is: strl_front_index_finish, from the state words)
  if (!B->have_table[si]) return bai_fail(B, STRL_ERR_ARG, "a chunk was handed over without its block offsets (strl_front_index_blocks)");
  B->have_table[si] = false;
  const uint32_t n = I.n_records;
  if (!n) return;
  FrontSlot &S = F->slot[si];
  const uint32_t nblk = (n + 255u) / 256u, m = B->vm[si];
  const uint64_t before = B->known_runs + (B->n_records - B->known_at), need = before + n;
  auto hip_fail = [&](hipError_t e) { bai_fail(B, STRL_ERR_HIP, hipGetErrorString(e)); };
  hipError_t e;
  if (need > B->run_cap) {
    const uint64_t cap = std::max<uint64_t>(need + need / 2, 2 * B->run_cap);
    DevBuf nb;
    if (nb.reserve((size_t)cap * sizeof(BaiRun))) return bai_fail(B, STRL_ERR_NOMEM, strl_last_error());
    const uint64_t keep = std::min(before, B->run_cap);
    if (keep && (e = hipMemcpyAsync(nb.p, B->runs.p, (size_t)keep * sizeof(BaiRun), hipMemcpyDeviceToDevice, st)) != hipSuccess) return hip_fail(e);
    B->trash.push_back(std::move(B->runs));
    B->runs = std::move(nb);
    B->run_cap = cap;
  }
  const size_t rec_room = std::max<size_t>(n, S.recoff.cap / 4);        // (what the slot's record table holds: later chunks do not reallocate)
  if (bai_room(B, B->flag, rec_room + 64) || bai_room(B, B->blk_cnt, (rec_room / 256 + 2) * 4 + 64) || bai_room(B, B->vt[si], (size_t)(m + 1) * 16))
    return bai_fail(B, STRL_ERR_NOMEM, strl_last_error());
  if ((e = hipMemcpyAsync(B->vt[si].p, B->h_vt[si], (size_t)(m + 1) * 16, hipMemcpyHostToDevice, st)) != hipSuccess) return hip_fail(e);
  BaiPush P{};
  P.U = S.infl.as<uint8_t>(); P.recoff = S.recoff.as<uint32_t>(); P.n = n;
  P.vrel = B->vt[si].as<int64_t>(); P.vfoff = B->vt[si].as<uint64_t>() + (m + 1); P.vm = m;
  P.abs0 = B->abs0[si]; P.ord0 = B->n_records;
  P.n_ref = B->n_ref; P.win_off = B->d_winoff.as<uint64_t>();
  P.lin = B->lin.as<uint64_t>(); P.ref_beg = B->ref_beg.as<uint64_t>(); P.ref_end = B->ref_end.as<uint64_t>(); P.ref_cnt = B->ref_cnt.as<uint64_t>();
  P.S = B->state.as<BaiState>(); P.par = B->par; P.flag = B->flag.as<uint8_t>(); P.blk_cnt = B->blk_cnt.as<uint32_t>();
  P.runs = B->runs.as<BaiRun>(); P.run_base = 0; P.run_acc = &P.S->run_base; P.run_cap = B->run_cap;
  P.C = BaiCols{tid, pos, end, fragw, I.carry_off};
  P.sch = B->sch;
  const bool bai = B->bai_scheme();
  // STRL_BAI_RECORDS=1 (measurements): the record-reading form of the per-record step, as `strling bamindex` runs it
  static const bool from_records = getenv("STRL_BAI_RECORDS") != nullptr;
  if (from_records) hipLaunchKernelGGL(bai ? bai_record_kernel<true> : bai_record_kernel<false>, dim3(nblk), dim3(256), 0, st, P);
  else hipLaunchKernelGGL(bai ? bai_record_cols_kernel<true> : bai_record_cols_kernel<false>, dim3(nblk), dim3(256), 0, st, P);
  hipLaunchKernelGGL(bai_scan_kernel, dim3(1), dim3(1024), 0, st, P.blk_cnt, nblk, &P.S->n_heads, &P.S->run_base);
  if (from_records) hipLaunchKernelGGL(bai ? bai_emit_kernel<true> : bai_emit_kernel<false>, dim3(nblk), dim3(256), 0, st, P);
  else hipLaunchKernelGGL(bai ? bai_emit_cols_kernel<true> : bai_emit_cols_kernel<false>, dim3(nblk), dim3(256), 0, st, P);
  if ((e = hipGetLastError()) != hipSuccess) return hip_fail(e);
  B->n_records += n;
  B->par ^= 1u;
  if (!B->snap_flying) {
    if ((e = hipMemcpyAsync(B->h_snap, B->state.p, sizeof(BaiState), hipMemcpyDeviceToHost, st)) != hipSuccess || (e = hipEventRecord(B->ev_snap, st)) != hipSuccess) return hip_fail(e);
    B->snap_flying = true;
    B->snap_at = B->n_records;
  }
}

extern "C" int strl_front_index_finish(strl_ctx *c, uint64_t *bai_bytes, strl_bamindex_info *info) {
  if (!c || !c->bai || !c->bai->attached || !c->front) { set_error("strl_front_index_finish without strl_front_index_begin"); return STRL_ERR_ARG; }
  STRL_HIP(hipSetDevice(c->device));
  strl_front *F = c->front;
  strl_bai *B = c->bai;
  int rc;
  if (!B->finished) {
    if (F->b_issued < F->chunks) { set_error("strl_front_index_finish before strl_front_finish"); return STRL_ERR_ARG; }
    if (!B->fail.empty()) { set_error("%s", B->fail.c_str()); return B->fail_rc; }
    STRL_HIP(hipStreamSynchronize(c->stream));
    B->snap_flying = false;
    STRL_HIP(hipMemcpy(B->h_state, B->state.p, sizeof(BaiState), hipMemcpyDeviceToHost));
    if ((rc = bai_refuse(B, *B->h_state))) { bai_fail(B, rc, strl_last_error()); return rc; }
    if (B->h_state->overflow) { bai_fail(B, STRL_ERR_CAPACITY, "the run table was outgrown (internal error)"); set_error("%s", B->fail.c_str()); return B->fail_rc; }
    if (B->h_state->run_total > 0x7ffffff0ull) { set_error("more than 2^31 runs of equal (reference, bin): beyond one device sort"); bai_fail(B, STRL_ERR_LIMIT, strl_last_error()); return STRL_ERR_LIMIT; }
    if (F->last_slot >= 0 && F->slot[F->last_slot].h_info[0].carry_len) { set_error("the BAM ends inside a record (truncated file)"); bai_fail(B, STRL_ERR_FORMAT, strl_last_error()); return STRL_ERR_FORMAT; }
    B->n_runs = B->h_state->run_total;
    if ((rc = bai_sort_and_pack(c, B))) return rc;
  }
  if (bai_bytes) *bai_bytes = B->bytes.size();
  if (info) { info->n_records = B->n_records; info->n_no_coor = B->h_state->n_no_coor; info->n_runs = B->n_runs; info->n_chunks = B->n_chunks; }
  return STRL_OK;
}

extern "C" int strl_bamindex_fetch(strl_ctx *c, uint8_t *out, uint64_t cap) {
  if (!c || !c->bai || !c->bai->finished || !out) { set_error("strl_bamindex_fetch without strl_bamindex_finish"); return STRL_ERR_ARG; }
  const std::vector<uint8_t> &b = c->bai->bytes;
  if (cap < b.size()) { set_error("strl_bamindex_fetch: %llu bytes, room for %llu", (unsigned long long)b.size(), (unsigned long long)cap); return STRL_ERR_CAPACITY; }
  memcpy(out, b.data(), b.size());
  return STRL_OK;
}

extern "C" int strl_bamindex_end(strl_ctx *c) {
  if (!c) { set_error("null argument"); return STRL_ERR_ARG; }
  STRL_HIP(hipSetDevice(c->device));
  if (c->front) {
    for (hipStream_t q : c->front->st_i) if (q) (void)hipStreamSynchronize(q);
    if (c->front->st_a) (void)hipStreamSynchronize(c->front->st_a);
    if (c->front->st_c) (void)hipStreamSynchronize(c->front->st_c);
  }
  STRL_HIP(hipStreamSynchronize(c->stream));
  if (c->bai) { bai_destroy(c->bai); c->bai = nullptr; }
  return STRL_OK;
}

// ---- the index of a sort's output from the sort's own pass (`strling sort --write-index`) ----
// Between the last fetch and strl_bamsort_end everything an index is made of is on the device: the records (the arena), their
// order (perm) and where each lies in the output stream (off[]).  The builder hangs off the sort, not off c->bai: a context with a
// sort open has no index pass open.  The records go through the per-record step in launches of at most `tile` records (BaiPush::n,
// flag[] and blk_cnt[] are 32-bit and sized per launch; BaiLast carries from one launch to the next as it does from chunk to
// chunk), the run table grows by the per-launch read of n_heads as in bai_index_chunk, and the finish is bai_sort_and_pack.
static uint32_t bsort_index_tile() {
  const char *e = getenv("STRL_SORT_INDEX_TILE");             // tests: launches of a few records (wave, block and launch seams)
  const long v = e ? atol(e) : 0;
  return v > 0 ? (uint32_t)std::min<long>(v, 1l << 30) : 1u << 22;
}

extern "C" int strl_bamsort_index(strl_ctx *c, const int32_t *l_ref, int32_t csi_min_shift, int32_t csi_depth, const uint64_t *member_off, uint64_t n_members,
                                  uint64_t *index_bytes, strl_bamindex_info *info) {
  BsortView V;
  strl_bai **slot = nullptr;
  const int vr = c ? bsort_view(c, &V, &slot) : STRL_ERR_ARG;
  if (vr == 2) { set_error("strl_bamsort_index: not supported by a windowed sort, whose records are never resident in sorted order; index the file it wrote"); return STRL_ERR_ARG; }
  if (vr) { set_error("strl_bamsort_index without strl_bamsort_finish"); return STRL_ERR_ARG; }
  if (V.n_ref && !l_ref) { set_error("strl_bamsort_index: bad argument"); return STRL_ERR_ARG; }
  if (!bsort_member_table_ok(member_off, n_members, V.stream_bytes)) {
    set_error("strl_bamsort_index: the member table must hold ceil(%llu / 0xFF00) + 1 = %llu file offsets that ascend and fit 48 bits (n_members given: %llu)",
              (unsigned long long)V.stream_bytes, (unsigned long long)bsort_n_members(V.stream_bytes) + 1, (unsigned long long)n_members);
    return STRL_ERR_ARG;
  }
  int rc;
  const int32_t csi[2] = {csi_min_shift, csi_depth};
  if (csi_min_shift >= 0 && (rc = csi_check(csi_min_shift, csi_depth))) return rc;
  STRL_HIP(hipSetDevice(c->device));
  if (*slot) { bai_destroy(*slot); *slot = nullptr; }
  strl_bai *B = *slot = new strl_bai();
  if ((rc = bai_tables(c, B, V.n_ref, l_ref, csi_min_shift >= 0 ? csi : nullptr))) return rc;
  hipStream_t st = c->stream;
  const uint64_t n = V.n_records;
  const uint32_t tile = bsort_index_tile();
  const size_t room = (size_t)std::min<uint64_t>(n, tile);
  if ((rc = B->vt[0].reserve((size_t)(n_members + 1) * 8)) || (rc = B->flag.reserve(room + 64)) || (rc = B->blk_cnt.reserve((room / 256 + 2) * 4 + 64))) return rc;
  STRL_HIP(hipMemcpyAsync(B->vt[0].p, member_off, (size_t)(n_members + 1) * 8, hipMemcpyHostToDevice, st));
  const bool bai = B->bai_scheme();
  for (uint64_t j0 = 0; j0 < n; j0 += tile) {
    const uint32_t m = (uint32_t)std::min<uint64_t>(tile, n - j0), nblk = (m + 255u) / 256u;
    BaiPush P{};
    P.n = m; P.ord0 = j0;
    P.n_ref = B->n_ref; P.win_off = B->d_winoff.as<uint64_t>();
    P.lin = B->lin.as<uint64_t>(); P.ref_beg = B->ref_beg.as<uint64_t>(); P.ref_end = B->ref_end.as<uint64_t>(); P.ref_cnt = B->ref_cnt.as<uint64_t>();
    P.S = B->state.as<BaiState>(); P.par = B->par; P.flag = B->flag.as<uint8_t>(); P.blk_cnt = B->blk_cnt.as<uint32_t>();
    P.Z = BaiSorted{V, j0, B->vt[0].as<uint64_t>(), n_members};
    P.sch = B->sch;
    hipLaunchKernelGGL(bai ? bai_record_sorted_kernel<true> : bai_record_sorted_kernel<false>, dim3(nblk), dim3(256), 0, st, P);
    STRL_HIP(hipGetLastError());
    hipLaunchKernelGGL(bai_scan_kernel, dim3(1), dim3(1024), 0, st, P.blk_cnt, nblk, &P.S->n_heads, (uint64_t *)nullptr);
    STRL_HIP(hipGetLastError());
    STRL_HIP(hipMemcpyAsync(B->h_state, B->state.p, sizeof(BaiState), hipMemcpyDeviceToHost, st));
    STRL_HIP(hipStreamSynchronize(st));                 // the number of runs that start in the launch: the table grows by exactly that
    if ((rc = bai_refuse(B, *B->h_state))) return rc;
    const uint64_t heads = B->h_state->n_heads;
    if (B->n_runs + heads > 0x7ffffff0ull) { set_error("more than 2^31 runs of equal (reference, bin): beyond one device sort"); return STRL_ERR_LIMIT; }
    if (heads) {
      if ((rc = B->runs.grow((size_t)(B->n_runs + heads) * sizeof(BaiRun), (size_t)B->n_runs * sizeof(BaiRun), st))) return rc;
      P.runs = B->runs.as<BaiRun>(); P.run_base = B->n_runs; P.run_acc = nullptr; P.run_cap = B->runs.cap / sizeof(BaiRun);
      hipLaunchKernelGGL(bai ? bai_emit_sorted_kernel<true> : bai_emit_sorted_kernel<false>, dim3(nblk), dim3(256), 0, st, P);
      STRL_HIP(hipGetLastError());
      B->n_runs += heads;
    }
    B->n_records += m;
    B->par ^= 1u;
  }
  STRL_HIP(hipStreamSynchronize(st));
  if ((rc = bai_sort_and_pack(c, B))) return rc;
  if (index_bytes) *index_bytes = B->bytes.size();
  if (info) { info->n_records = B->n_records; info->n_no_coor = B->h_state->n_no_coor; info->n_runs = B->n_runs; info->n_chunks = B->n_chunks; }
  return STRL_OK;
}

extern "C" int strl_bamsort_index_fetch(strl_ctx *c, uint8_t *out, uint64_t cap) {
  BsortView V;
  strl_bai **slot = nullptr;
  if (!c || !out || bsort_view(c, &V, &slot) || !*slot || !(*slot)->finished) { set_error("strl_bamsort_index_fetch without strl_bamsort_index"); return STRL_ERR_ARG; }
  const std::vector<uint8_t> &b = (*slot)->bytes;
  if (cap < b.size()) { set_error("strl_bamsort_index_fetch: %llu bytes, room for %llu", (unsigned long long)b.size(), (unsigned long long)cap); return STRL_ERR_CAPACITY; }
  memcpy(out, b.data(), b.size());
  return STRL_OK;
}

// the rule of the virtual offsets through the library, without a device (the Python mirror, tests): bamsort_core.h's bsort_voff over
// a table checked by bsort_member_table_ok, and the member walk the CLI runs over the bytes it writes
extern "C" int strl_bamsort_voff(const uint64_t *member_off, uint64_t n_members, uint64_t stream_bytes, uint64_t s, uint64_t *voff) {
  if (!voff || s > stream_bytes || !bsort_member_table_ok(member_off, n_members, stream_bytes)) {
    set_error("strl_bamsort_voff: the table must hold ceil(stream_bytes / 0xFF00) + 1 file offsets that ascend and fit 48 bits, s <= stream_bytes");
    return STRL_ERR_ARG;
  }
  *voff = bsort_voff(member_off, n_members, stream_bytes, s);
  return STRL_OK;
}
extern "C" int strl_bamsort_members(const uint8_t *bytes, uint64_t n, uint64_t file_off, uint64_t *member_off, uint64_t cap, uint64_t *n_out) {
  if ((n && !bytes) || !n_out) { set_error("strl_bamsort_members: null argument"); return STRL_ERR_ARG; }
  std::vector<uint64_t> m;
  uint64_t at = file_off;
  if (!bsort_walk_members(bytes, (size_t)n, &at, m)) { set_error("strl_bamsort_members: the bytes are not whole BGZF members"); return STRL_ERR_FORMAT; }
  *n_out = m.size();
  if (cap < m.size() || (m.size() && !member_off)) { set_error("strl_bamsort_members: %zu members, room for %llu", m.size(), (unsigned long long)cap); return STRL_ERR_CAPACITY; }
  if (!m.empty()) memcpy(member_off, m.data(), m.size() * 8);
  return STRL_OK;
}
