// fastq.hip -- `strling fastq`: the reads of a resident sort (bamsort.hip) back to paired FASTQ on the device (gfx950), behind
// strl_bamsort_finish.  The rule is fastq_core.h's.  DESIGN section 24.4.
//   fastq_record_kernel    16 lanes a record of the arena: slab, offset and every inner length bounded before use; lane 0 the class
//                          and the entry length, lane 1 the FNV-1a hash of the name
//   radix_sort_pairs       (name hash, ordinal), records that are not kept behind a sentinel bit
//   fastq_runs_kernel      the head lane of a run of equal hashes compares the NAMES in the arena: mate[] and the pair bit
//   fastq_tile / _scan     every ordinal owns a size in each stream (the earlier record of a pair its pair's bytes, a single its own
//                          bytes in s, everything else 0); one tiled 64-bit exclusive prefix sum a stream, in ordinal order, gives
//                          every entry its first byte -- the order of first appearance, with no further sort
//   fastq_text_kernel      the hot path: for a piece [lo, hi) of a stream two binary searches find the owners that touch it; 16 lanes
//                          an owner, each lane produces whole aligned 16-byte words of the piece in registers and stores each with
//                          one 16-byte store; the words at the ends that the owner covers only in part are written bytewise
#include <stdlib.h>
#include <algorithm>
#include "front.h"
#include "sort.h"
#include "device_util.h"
#include "bamsort_core.h"
#include "fastq_core.h"

namespace strl {

namespace {

constexpr uint32_t FASTQ_G = 16;                           // lanes a record / an owner
constexpr uint32_t FASTQ_TILE = 2048;                      // ordinals per workgroup of the layout: 256 lanes x 8
constexpr uint32_t FASTQ_NONE = 0xffffffffu;
static_assert((uint64_t)FRONT_CARRY_MAX * 2u + 512u < 0xffffffffull, "an entry's length fits 32 bits");

struct FastqState {
  uint64_t err_ord;          // ordinal of the first record whose lengths do not fit; ~0 = none
  uint64_t counts[5];        // kept, filtered, empty, pairs, singles
  uint64_t total[3];         // bytes of the streams
  uint64_t range[2];         // the owners that touch the piece being written
  uint32_t run_max;          // the longest run of one hash, where one is longer than MDUP_RUN_MAX
  uint32_t n;                // the count of all records, for the join's sort
};

struct FastqView {
  const uint64_t *src;
  const uint32_t *len;
  uint8_t *const *slab;
  const uint64_t *slab_used;
  uint32_t n_slabs, n;
};

// the record of ordinal `ord` inside its slab's used bytes, or null
__device__ __forceinline__ const uint8_t *fastq_at(const FastqView &V, uint32_t ord, uint32_t *len) {
  const uint64_t s = V.src[ord], sl = s >> BSORT_SLAB_SHIFT, so = s & BSORT_SLAB_MASK;
  const uint32_t l = V.len[ord];
  if (sl >= V.n_slabs || l < MDUP_FIXED || so > V.slab_used[sl] || l > V.slab_used[sl] - so) return nullptr;
  *len = l;
  return V.slab[sl] + so;
}

struct FastqRecord {
  FastqView V;
  FastqOpts o;
  uint64_t *hash;
  uint32_t *elen;
  uint8_t *cls;
  uint64_t hash_mask, sentinel;
  FastqState *S;
};

__global__ __launch_bounds__(256) void fastq_record_kernel(FastqRecord P) {
  const uint32_t g = threadIdx.x % FASTQ_G;
  const uint64_t group = ((uint64_t)blockIdx.x * 256u + threadIdx.x) / FASTQ_G, n_groups = (uint64_t)gridDim.x * 256u / FASTQ_G;
  uint32_t kept = 0, filtered = 0, empty = 0;                 // lane 0's
  for (uint64_t ord = group; ord < P.V.n; ord += n_groups) {
    uint32_t len = 0;
    const uint8_t *rec = fastq_at(P.V, (uint32_t)ord, &len);
    FastqRec R;
    const bool ok = rec && fastq_rec(rec, len, P.o, &R);
    const uint8_t cls = ok ? R.cls : 0;
    if (g == 0) {
      if (!ok) atomicMin(reinterpret_cast<unsigned long long *>(&P.S->err_ord), (unsigned long long)ord);
      else if (cls) ++kept;
      else if (R.flag & P.o.filter) ++filtered;
      else ++empty;
      P.cls[ord] = cls;
      P.elen[ord] = cls ? (uint32_t)R.len : 0u;
    } else if (g == 1) {
      P.hash[ord] = cls ? (mdup_name_hash(rec + R.name_at, R.n_name) & P.hash_mask) : P.sentinel;
    }
  }
  uint32_t what[3] = {kept, filtered, empty};
  for (int k = 0; k < 3; ++k) {
    uint32_t v = what[k];
    for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d);
    if ((threadIdx.x & 63u) == 0 && v) atomicAdd(reinterpret_cast<unsigned long long *>(&P.S->counts[k]), (unsigned long long)v);
  }
}

__global__ void fastq_iota_kernel(uint32_t *v, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) v[i] = i;
}

// the name of a kept record (the record kernel has held its lengths against the record)
__device__ __forceinline__ const uint8_t *fastq_name(const FastqView &V, uint32_t ord, uint32_t *n_name) {
  uint32_t len = 0;
  const uint8_t *rec = fastq_at(V, ord, &len);
  if (!rec || MDUP_FIXED + (uint32_t)rec[12] > len) return nullptr;
  *n_name = fastq_name_bytes(rec[12]);
  return rec + MDUP_FIXED;
}

// key[0, n) ascending, val[] the ordinals: the lane of a run's first element decides the pairs among the run's records, by name
__global__ __launch_bounds__(256) void fastq_runs_kernel(const uint64_t *key, const uint32_t *val, FastqView V, uint64_t sentinel, uint8_t *cls, uint32_t *mate, FastqState *S) {
  const uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (j >= V.n) return;
  const uint64_t k = key[j];
  if (k == sentinel || (j && key[j - 1] == k)) return;
  uint64_t a = j + 1, b = V.n;                                // the run's end: the first element behind j with another key
  while (a < b) { const uint64_t m = a + (b - a) / 2; if (key[m] != k) b = m; else a = m + 1; }
  const uint64_t end = a;
  if (end - j > MDUP_RUN_MAX) { atomicMax(&S->run_max, (uint32_t)(end - j)); return; }      // (n < 2^32)
  if (end - j < 2) return;
  for (uint64_t x = j; x < end; ++x) {
    const uint32_t ox = val[x];
    if (ox >= V.n || (cls[ox] & FASTQ_C_SEEN)) continue;
    uint32_t lx = 0, count = 1, other = 0;
    const uint8_t *nx = fastq_name(V, ox, &lx);
    if (!nx) continue;
    for (uint64_t y = x + 1; y < end; ++y) {
      const uint32_t oy = val[y];
      if (oy >= V.n || (cls[oy] & FASTQ_C_SEEN)) continue;
      uint32_t ly = 0;
      const uint8_t *ny = fastq_name(V, oy, &ly);
      if (!ny || !mdup_same_name(nx, lx, ny, ly)) continue;
      cls[oy] |= FASTQ_C_SEEN;
      if (++count == 2) other = oy;
    }
    if (count == 2 && fastq_is_pair(cls[ox], cls[other])) {
      cls[ox] |= FASTQ_C_PAIRED; cls[other] |= FASTQ_C_PAIRED;
      mate[ox] = other; mate[other] = ox;
    }
  }
}

struct FastqOwn {
  const uint8_t *cls;
  const uint32_t *elen, *mate;
  uint32_t n, interleaved, singles;
};
// the records whose entries ordinal i owns in `stream`, in the order they are written (FASTQ_NONE: none)
__device__ __forceinline__ void fastq_owned(const FastqOwn &P, uint32_t i, int stream, uint32_t *r1, uint32_t *r2) {
  *r1 = *r2 = FASTQ_NONE;
  const uint8_t c = P.cls[i];
  if (!(c & FASTQ_C_KEPT)) return;
  if (!(c & FASTQ_C_PAIRED)) { if (stream == FASTQ_S && P.singles) *r1 = i; return; }
  const uint32_t m = P.mate[i];
  if (m >= P.n || m < i) return;                              // the pair stands where the earlier of its two records stood
  const uint32_t first = c & FASTQ_C_R1 ? i : m, second = c & FASTQ_C_R1 ? m : i;
  if (stream == FASTQ_P1) { *r1 = first; if (P.interleaved) *r2 = second; }
  else if (stream == FASTQ_P2 && !P.interleaved) *r1 = second;
}
__device__ __forceinline__ uint64_t fastq_own_bytes(const FastqOwn &P, uint32_t i, int stream) {
  uint32_t r1, r2;
  fastq_owned(P, i, stream, &r1, &r2);
  return (r1 != FASTQ_NONE ? (uint64_t)P.elen[r1] : 0ull) + (r2 != FASTQ_NONE ? (uint64_t)P.elen[r2] : 0ull);
}

// pairs and singles, once the join has decided
__global__ __launch_bounds__(256) void fastq_count_kernel(FastqOwn P, FastqState *S) {
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  const uint8_t c = i < P.n ? P.cls[i] : 0;
  const bool kept = (c & FASTQ_C_KEPT) != 0, paired = kept && (c & FASTQ_C_PAIRED);
  const bool what[2] = {paired && P.mate[i] < P.n && (uint32_t)i < P.mate[i], kept && !paired};
  for (int k = 0; k < 2; ++k) {
    const unsigned long long m = __ballot(what[k]);
    if (m && (threadIdx.x & 63u) == 0) atomicAdd(reinterpret_cast<unsigned long long *>(&S->counts[3 + k]), (unsigned long long)__popcll(m));
  }
}

// exclusive sum over the 256 lanes of a workgroup (sh: 4 words); *block_total = the sum of all
__device__ __forceinline__ uint64_t fastq_block_excl(uint64_t v, uint64_t *sh, uint64_t *block_total) {
  const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  uint64_t inc = v;
  for (int d = 1; d < 64; d <<= 1) { const uint64_t o = __shfl_up(inc, d); if ((int)lane >= d) inc += o; }
  if (lane == 63u) sh[w] = inc;
  __syncthreads();
  uint64_t base = 0, tot = 0;
  for (uint32_t k = 0; k < 4u; ++k) { if (k < w) base += sh[k]; tot += sh[k]; }
  *block_total = tot;
  return base + inc - v;
}
template <bool ADD> __global__ __launch_bounds__(256) void fastq_tile_kernel(FastqOwn P, int stream, uint64_t *tile, uint64_t *off) {
  __shared__ uint64_t sh[4];
  const uint64_t j0 = (uint64_t)blockIdx.x * FASTQ_TILE + (uint64_t)threadIdx.x * 8u;
  uint64_t l[8], mine = 0;
  for (uint32_t k = 0; k < 8u; ++k) {
    const uint64_t j = j0 + k;
    l[k] = j < P.n ? fastq_own_bytes(P, (uint32_t)j, stream) : 0ull;
    mine += l[k];
  }
  uint64_t tot;
  uint64_t at = fastq_block_excl(mine, sh, &tot);
  if constexpr (!ADD) {
    if (threadIdx.x == 0) tile[blockIdx.x] = tot;
  } else {
    at += tile[blockIdx.x];
    for (uint32_t k = 0; k < 8u; ++k) { const uint64_t j = j0 + k; if (j < P.n) off[j] = at; at += l[k]; }
  }
}
// one workgroup: tile[0, n_tiles) -> exclusive sums in place, the total to S->total[stream] and to off[n]
__global__ __launch_bounds__(1024) void fastq_scan_kernel(uint64_t *tile, uint32_t n_tiles, uint64_t *off, uint32_t n, int stream, FastqState *S) {
  __shared__ uint64_t part[1024];
  const uint32_t t = threadIdx.x, per = (n_tiles + 1023u) / 1024u, a = min(n_tiles, t * per), b = min(n_tiles, a + per);
  uint64_t s = 0;
  for (uint32_t k = a; k < b; ++k) s += tile[k];
  part[t] = s;
  __syncthreads();
  if (t == 0) {
    uint64_t run = 0;
    for (int k = 0; k < 1024; ++k) { const uint64_t v = part[k]; part[k] = run; run += v; }
    S->total[stream] = run; off[n] = run;
  }
  __syncthreads();
  uint64_t run = part[t];
  for (uint32_t k = a; k < b; ++k) { const uint64_t v = tile[k]; tile[k] = run; run += v; }
}

// ---- a piece of a stream -------------------------------------------------------------------------------------------------------------
__global__ void fastq_range_kernel(const uint64_t *off, uint64_t n, uint64_t lo, uint64_t hi, FastqState *S) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const uint64_t a = bsort_first_touch(off, n, lo), b = bsort_end_touch(off, n, hi);
    S->range[0] = a; S->range[1] = b > a ? b : a;
  }
}

struct FastqText {
  FastqView V;
  FastqOwn O;
  FastqOpts o;
  const uint64_t *off;       // [n + 1]
  int stream;
  uint64_t lo, hi;           // the piece of the stream; dst[0] is byte lo
  uint8_t *dst;              // 16-byte aligned
  const FastqState *S;
};

// bytes [t, t + c) of an owner's bytes: its first entry, then (interleaved) its second
template <typename Emit> __device__ __forceinline__ void fastq_owner_emit(const uint8_t *rec1, const FastqRec &R1, const uint8_t *rec2, const FastqRec &R2, uint64_t t, uint64_t c, Emit &&emit) {
  if (t < R1.len) fastq_entry_emit(rec1, R1, t, c, emit);      // (cut at the entry's end)
  if (rec2 && t + c > R1.len) {
    const uint64_t first = t > R1.len ? t - R1.len : 0ull, skip = t < R1.len ? R1.len - t : 0ull;
    fastq_entry_emit(rec2, R2, first, c - skip, [&](uint32_t at, uint8_t b) { emit(at + (uint32_t)skip, b); });
  }
}

__global__ __launch_bounds__(256) void fastq_text_kernel(FastqText P) {
  const uint32_t g = threadIdx.x % FASTQ_G;
  const uint64_t group = ((uint64_t)blockIdx.x * 256u + threadIdx.x) / FASTQ_G, n_groups = (uint64_t)gridDim.x * 256u / FASTQ_G;
  const uint64_t a = P.S->range[0], b = min(P.S->range[1], (uint64_t)P.V.n);
  for (uint64_t ord = a + group; ord < b; ord += n_groups) {
    const uint64_t A = P.off[ord], B = P.off[ord + 1];
    if (B <= A) continue;                                     // owns nothing in this stream
    uint32_t r1, r2, len1 = 0, len2 = 0;
    fastq_owned(P.O, (uint32_t)ord, P.stream, &r1, &r2);
    if (r1 == FASTQ_NONE) continue;
    const uint8_t *rec1 = fastq_at(P.V, r1, &len1), *rec2 = r2 != FASTQ_NONE ? fastq_at(P.V, r2, &len2) : nullptr;
    FastqRec R1, R2;
    R2.len = 0;
    if (!rec1 || !fastq_rec(rec1, len1, P.o, &R1) || (r2 != FASTQ_NONE && (!rec2 || !fastq_rec(rec2, len2, P.o, &R2)))) continue;
    if (R1.len + R2.len != B - A) continue;                   // (the layout's sizes are these entries' lengths)
    const uint64_t s0 = A > P.lo ? A : P.lo, s1 = B < P.hi ? B : P.hi;
    if (s1 <= s0) continue;
    // inside the piece: bytes [pa, pb) of dst; whole 16-byte words [w0, w1)
    const uint64_t pa = s0 - P.lo, pb = s1 - P.lo, w0 = (pa + 15u) & ~15ull, w1 = pb & ~15ull;      // (owner offset of dst byte k = k + lo - A)
    const bool words = w0 < w1;
    for (uint64_t w = w0 + 16u * g; words && w < w1; w += 16u * FASTQ_G) {
      uint64_t q0 = 0, q1 = 0;
      fastq_owner_emit(rec1, R1, rec2, R2, w + P.lo - A, 16u, [&](uint32_t at, uint8_t v) {
        if (at < 8u) q0 |= (uint64_t)v << (at * 8u); else q1 |= (uint64_t)v << ((at - 8u) * 8u);
      });
      *reinterpret_cast<uint4 *>(P.dst + w) = make_uint4((uint32_t)q0, (uint32_t)(q0 >> 32), (uint32_t)q1, (uint32_t)(q1 >> 32));
    }
    // the ends: [pa, w0) and [w1, pb), or all of [pa, pb) where it holds no whole word (fewer than 31 bytes)
    const uint64_t n_head = (words ? w0 : pb) - pa, tail_at = words ? w1 : pb, n_ends = n_head + (pb - tail_at);
    for (uint64_t x = g; x < n_ends; x += FASTQ_G) {
      const uint64_t k = x < n_head ? pa + x : tail_at + (x - n_head);
      uint8_t *d = P.dst + k;
      fastq_owner_emit(rec1, R1, rec2, R2, k + P.lo - A, 1u, [d](uint32_t, uint8_t v) { *d = v; });
    }
  }
}

int fastq_hash_bits() {
  static const int v = [] {
    const char *e = getenv("STRL_FASTQ_HASH_BITS");          // tests: different names under one hash as a rule
    const int x = e ? atoi(e) : 0;
    return x >= 1 && x <= 63 ? x : 63;
  }();
  return v;
}

}  // namespace

struct FastqPlan {
  FastqOpts o{};
  uint32_t n = 0;
  DevBuf cls, elen, mate, off[3], piece, state;
  strl_fastq_info info{};
  hipEvent_t e0 = nullptr, e1 = nullptr;
};

void fastq_destroy(FastqPlan *F) {
  if (!F) return;
  for (hipEvent_t e : {F->e0, F->e1}) if (e) (void)hipEventDestroy(e);
  delete F;
}
const strl_fastq_info *fastq_info(const FastqPlan *F) { return &F->info; }

static FastqView fastq_view(const BsortView &B) { return FastqView{B.src, B.len, B.slab, B.slab_used, B.n_slabs, (uint32_t)B.n_records}; }

int fastq_plan(strl_ctx *c, const BsortView &B, const strl_fastq_opts *opts, FastqPlan **slot, strl_fastq_info *out) {
  hipStream_t st = c->stream;
  if (B.n_records > BSORT_MAX_RECORDS) { set_error("fastq: more than 2^32 - 2 records"); return STRL_ERR_LIMIT; }
  FastqPlan *F = new FastqPlan();
  fastq_destroy(*slot);
  *slot = F;
  F->o = FastqOpts{opts->filter, opts->suffix ? 1u : 0u, opts->default_qual, opts->interleaved ? 1u : 0u, opts->singles ? 1u : 0u};
  const uint32_t n = F->n = (uint32_t)B.n_records;
  STRL_HIP(hipEventCreate(&F->e0));
  STRL_HIP(hipEventCreate(&F->e1));
  strl_fastq_info &I = F->info;
  if (!n) { if (out) *out = I; return STRL_OK; }
  const int hb = fastq_hash_bits();
  const uint64_t sentinel = 1ull << hb, hash_mask = sentinel - 1ull;
  const size_t sb = radix_sort_scratch_bytes(n, 64);
  const uint32_t n_tiles = (n + FASTQ_TILE - 1u) / FASTQ_TILE;
  const bool laid[3] = {true, !F->o.interleaved, F->o.singles != 0};
  DevBuf k0, k1, v0, v1, scratch, tile;
  int rc;
  if ((rc = F->cls.reserve((size_t)n + 64)) || (rc = F->elen.reserve((size_t)n * 4 + 64)) || (rc = F->mate.reserve((size_t)n * 4 + 64)) || (rc = F->state.reserve(sizeof(FastqState))) ||
      (rc = k0.reserve((size_t)n * 8 + 64)) || (rc = k1.reserve((size_t)n * 8 + 64)) || (rc = v0.reserve((size_t)n * 4 + 64)) || (rc = v1.reserve((size_t)n * 4 + 64)) ||
      (rc = scratch.reserve(sb + 64)) || (rc = tile.reserve((size_t)n_tiles * 8 + 64)))
    return rc;
  for (int s = 0; s < 3; ++s) if (laid[s] && (rc = F->off[s].reserve(((size_t)n + 1) * 8 + 64))) return rc;
  hipEvent_t ev[4] = {};
  struct Events { hipEvent_t *e; ~Events() { for (int k = 0; k < 4; ++k) if (e[k]) (void)hipEventDestroy(e[k]); } } guard{ev};
  for (hipEvent_t &e : ev) STRL_HIP(hipEventCreate(&e));
  FastqState H{};
  H.err_ord = ~0ull;
  H.n = n;
  FastqState *S = F->state.as<FastqState>();
  STRL_HIP(hipMemcpyAsync(S, &H, sizeof H, hipMemcpyHostToDevice, st));
  STRL_HIP(hipMemsetAsync(F->mate.p, 0xff, (size_t)n * 4, st));
  const FastqView V = fastq_view(B);
  const unsigned blocks = (n + 255u) / 256u;

  // ---- the records ----
  STRL_HIP(hipEventRecord(ev[0], st));
  const unsigned rgrid = (unsigned)std::min<uint64_t>(8192, ((uint64_t)n * FASTQ_G + 255u) / 256u);
  const FastqRecord RP{V, F->o, k0.as<uint64_t>(), F->elen.as<uint32_t>(), F->cls.as<uint8_t>(), hash_mask, sentinel, S};
  hipLaunchKernelGGL(fastq_record_kernel, dim3(rgrid), dim3(256), 0, st, RP);
  STRL_HIP(hipGetLastError());
  STRL_HIP(hipEventRecord(ev[1], st));
  STRL_HIP(hipMemcpyAsync(&H, S, sizeof H, hipMemcpyDeviceToHost, st));
  STRL_HIP(hipStreamSynchronize(st));
  if (H.err_ord != ~0ull) {
    set_error("malformed BAM record %llu: its name, CIGAR, bases and qualities do not fit its block_size", (unsigned long long)H.err_ord);
    return STRL_ERR_FORMAT;
  }

  // ---- the join by name ----
  uint64_t *key = k0.as<uint64_t>();
  uint32_t *val = v0.as<uint32_t>();
  hipLaunchKernelGGL(fastq_iota_kernel, dim3(blocks), dim3(256), 0, st, val, n);
  const int se = radix_sort_pairs(st, &S->n, n, k0.as<uint64_t>(), v0.as<uint32_t>(), k1.as<uint64_t>(), v1.as<uint32_t>(), scratch.p, sb, 0, hb + 1, &key, &val);
  if (se) { set_error("radix_sort_pairs failed: %s", hipGetErrorString((hipError_t)se)); return STRL_ERR_HIP; }
  hipLaunchKernelGGL(fastq_runs_kernel, dim3(blocks), dim3(256), 0, st, key, val, V, sentinel, F->cls.as<uint8_t>(), F->mate.as<uint32_t>(), S);
  STRL_HIP(hipGetLastError());
  STRL_HIP(hipEventRecord(ev[2], st));
  STRL_HIP(hipMemcpyAsync(&H, S, sizeof H, hipMemcpyDeviceToHost, st));
  STRL_HIP(hipStreamSynchronize(st));
  if (H.run_max) {
    set_error("fastq: %u kept records share one name hash, more than the %u a run of the device's join resolves; write this file on the host: STRL_FASTQ=host", H.run_max, MDUP_RUN_MAX);
    return STRL_ERR_LIMIT;
  }

  // ---- the layout ----
  const FastqOwn O{F->cls.as<uint8_t>(), F->elen.as<uint32_t>(), F->mate.as<uint32_t>(), n, F->o.interleaved, F->o.singles};
  hipLaunchKernelGGL(fastq_count_kernel, dim3(blocks), dim3(256), 0, st, O, S);
  for (int s = 0; s < 3; ++s) {
    if (!laid[s]) continue;
    hipLaunchKernelGGL(fastq_tile_kernel<false>, dim3(n_tiles), dim3(256), 0, st, O, s, tile.as<uint64_t>(), F->off[s].as<uint64_t>());
    hipLaunchKernelGGL(fastq_scan_kernel, dim3(1), dim3(1024), 0, st, tile.as<uint64_t>(), n_tiles, F->off[s].as<uint64_t>(), n, s, S);
    hipLaunchKernelGGL(fastq_tile_kernel<true>, dim3(n_tiles), dim3(256), 0, st, O, s, tile.as<uint64_t>(), F->off[s].as<uint64_t>());
  }
  STRL_HIP(hipGetLastError());
  STRL_HIP(hipEventRecord(ev[3], st));
  STRL_HIP(hipMemcpyAsync(&H, S, sizeof H, hipMemcpyDeviceToHost, st));
  STRL_HIP(hipStreamSynchronize(st));
  I.n_kept = H.counts[0]; I.n_filtered = H.counts[1]; I.n_empty = H.counts[2]; I.n_pairs = H.counts[3]; I.n_singles = H.counts[4];
  I.n_singles_unwritten = F->o.singles ? 0 : I.n_singles;
  for (int s = 0; s < 3; ++s) I.stream_bytes[s] = laid[s] ? H.total[s] : 0;
  double *ms[3] = {&I.record_ms, &I.join_ms, &I.layout_ms};
  for (int k = 0; k < 3; ++k) { float t = 0.f; if (hipEventElapsedTime(&t, ev[k], ev[k + 1]) == hipSuccess) *ms[k] = t; else (void)hipGetLastError(); }
  if (out) *out = I;
  return STRL_OK;
}

int fastq_fetch(strl_ctx *c, FastqPlan *F, const BsortView &B, int stream, uint64_t lo, uint64_t len, uint8_t *dst) {
  if (stream < 0 || stream > 2 || lo > F->info.stream_bytes[stream] || len > F->info.stream_bytes[stream] - lo || len > 0xffffffffull) {
    set_error("strl_bamsort_fastq_fetch: stream %d, [%llu, %llu + %llu) is not inside one of the three streams (a piece holds less than 4 GiB)", stream, (unsigned long long)lo,
              (unsigned long long)lo, (unsigned long long)len);
    return STRL_ERR_ARG;
  }
  if (!len) return STRL_OK;
  if (!dst) { set_error("null argument"); return STRL_ERR_ARG; }
  hipStream_t st = c->stream;
  int rc;
  if ((rc = F->piece.reserve((size_t)len + 64))) return rc;
  FastqState *S = F->state.as<FastqState>();
  const uint64_t *off = F->off[stream].as<uint64_t>();
  const FastqOwn O{F->cls.as<uint8_t>(), F->elen.as<uint32_t>(), F->mate.as<uint32_t>(), F->n, F->o.interleaved, F->o.singles};
  const FastqText T{fastq_view(B), O, F->o, off, stream, lo, lo + len, F->piece.as<uint8_t>(), S};
  hipLaunchKernelGGL(fastq_range_kernel, dim3(1), dim3(64), 0, st, off, (uint64_t)F->n, lo, lo + len, S);
  // a group an owner of a few hundred bytes; the groups stride over the owners that touch the piece
  const unsigned grid = (unsigned)std::min<uint64_t>(16384, len / (256u * FASTQ_G) + 1u);
  STRL_HIP(hipEventRecord(F->e0, st));
  hipLaunchKernelGGL(fastq_text_kernel, dim3(grid), dim3(256), 0, st, T);
  STRL_HIP(hipGetLastError());
  STRL_HIP(hipEventRecord(F->e1, st));
  STRL_HIP(hipMemcpyAsync(dst, F->piece.p, len, hipMemcpyDeviceToHost, st));
  STRL_HIP(hipStreamSynchronize(st));
  float t = 0.f;
  if (hipEventElapsedTime(&t, F->e0, F->e1) == hipSuccess) F->info.text_ms += t; else (void)hipGetLastError();
  F->info.text_bytes += len;
  return STRL_OK;
}

}  // namespace strl
