// markdup.hip -- `strling sort --markdup`: flag 0x400 on duplicate pairs and fragments, decided on the device (gfx950) over the
// records a resident sort holds (bamsort.hip), between strl_bamsort_finish and the first fetch.  The rule is markdup_core.h's; the
// reference drops the records that carry the flag (collect.nim:140).  DESIGN section 24.3.
//   mdup_record_kernel     16 lanes a record of the arena: lane 0 walks the CIGAR ends (the signature), lane 1 hashes the name, all
//                          sum the qualities with aligned 16-byte loads; slab, offset and every inner length bounded before use
//   radix_sort_pairs       (name hash, ordinal), records that are not eligible behind a sentinel
//   mdup_runs_kernel       the head lane of a run of equal hashes compares the NAMES in the arena and decides the pairs (<= 512 records)
//   pairs                  one element a pair, stable sorts chained in LSD order: (~template score, ordinal of the 0x40 record), e_hi,
//                          e_lo; every element that is not the first of its (e_lo, e_hi) run is marked.  No serial walk over a run
//   fragments              one element a fragment and one a pair end (their class ordered first): tiebreak, then signature; every
//                          fragment that is not the first of its signature run is marked -- a pair end, where there is one, is first
//   mdup_flag_kernel       the decided bit into the arena: one byte store a record whose flag changes, and the five counts
#include <stdlib.h>
#include <algorithm>
#include "front.h"
#include "sort.h"
#include "device_util.h"
#include "bamsort_core.h"
#include "markdup_core.h"

namespace strl {

namespace {

constexpr uint32_t MDUP_G = 16;                            // lanes a record, as the gather's
constexpr uint8_t MDUP_C_SEEN = 64;                        // the runs kernel's: the record's name has been counted
static_assert((uint64_t)FRONT_CARRY_MAX * 255u * 2u < 0x7fffffffull, "a template's score fits the tiebreak word's field");

struct MdupState {
  uint64_t err_ord[2];       // ordinal of the first record whose lengths do not fit / whose unclipped end is no position; ~0 = none
  uint64_t max_score;
  uint64_t counts[5];        // pairs, duplicate pairs, fragments, duplicate fragments, ineligible
  uint32_t run_max;          // the longest run of one hash, where one is longer than MDUP_RUN_MAX
  uint32_t n_elem;           // elements of the list being sorted
};

struct MdupView {
  const uint64_t *src;
  const uint32_t *len;
  uint8_t *const *slab;
  const uint64_t *slab_used;
  uint32_t n_slabs, n;
};

// the record of ordinal `ord` inside its slab's used bytes, or null
__device__ __forceinline__ uint8_t *mdup_rec(const MdupView &V, uint32_t ord, uint32_t *len) {
  const uint64_t s = V.src[ord], sl = s >> BSORT_SLAB_SHIFT, so = s & BSORT_SLAB_MASK;
  const uint32_t l = V.len[ord];
  if (sl >= V.n_slabs || l < MDUP_FIXED || so > V.slab_used[sl] || l > V.slab_used[sl] - so) return nullptr;
  *len = l;
  return V.slab[sl] + so;
}

struct MdupRecord {
  MdupView V;
  uint64_t *sig, *hash;
  uint32_t *score;
  uint8_t *cls;
  uint64_t hash_mask, sentinel;
  MdupState *S;
};

__global__ __launch_bounds__(256) void mdup_record_kernel(MdupRecord P) {
  const uint32_t g = threadIdx.x % MDUP_G;
  const uint64_t group = ((uint64_t)blockIdx.x * 256u + threadIdx.x) / MDUP_G, n_groups = (uint64_t)gridDim.x * 256u / MDUP_G;
  uint64_t top = 0;                                           // the largest score this lane has written
  for (uint64_t ord = group; ord < P.V.n; ord += n_groups) {
    uint32_t len = 0;
    const uint8_t *rec = mdup_rec(P.V, (uint32_t)ord, &len);
    MdupFields f;
    const bool ok = rec && mdup_fields(rec, len, &f);
    const uint8_t cls = ok ? mdup_class(f.flag) : 0;
    uint32_t sum = 0;
    if (cls) {
      // the qualities: bytes up to the first aligned address, aligned 16-byte words, the bytes behind them; all inside the record
      const uint8_t *q = rec + f.qual_at;
      const uint32_t n = f.l_seq, to16 = (16u - (uint32_t)(reinterpret_cast<uintptr_t>(q) & 15u)) & 15u, head = n < to16 ? n : to16;
      if (g < head) sum += mdup_qual(q[g]);                   // (head < 16 = MDUP_G)
      const uint32_t n_vec = (n - head) >> 4;
      const uint4 *v = reinterpret_cast<const uint4 *>(q + head);
      for (uint32_t k = g; k < n_vec; k += MDUP_G) { const uint4 w = v[k]; sum += mdup_qual4(w.x) + mdup_qual4(w.y) + mdup_qual4(w.z) + mdup_qual4(w.w); }
      const uint32_t done = head + (n_vec << 4);
      if (g < n - done) sum += mdup_qual(q[done + g]);        // (fewer than 16)
    }
    for (int d = MDUP_G / 2; d > 0; d >>= 1) sum += __shfl_xor(sum, d, MDUP_G);
    if (g == 0) {
      uint64_t sig = 0;
      uint8_t c = cls;
      if (!ok) atomicMin(reinterpret_cast<unsigned long long *>(&P.S->err_ord[0]), (unsigned long long)ord);
      else if (cls) {
        int32_t u = 0;
        if (mdup_unclipped(rec + f.cigar_at, f.n_cigar, f.pos, (f.flag & 0x10u) != 0, &u)) sig = mdup_sig(f.tid, u, f.flag >> 4 & 1u);
        else { atomicMin(reinterpret_cast<unsigned long long *>(&P.S->err_ord[1]), (unsigned long long)ord); c = 0; }
      }
      P.sig[ord] = sig; P.score[ord] = sum; P.cls[ord] = c;
      if (sum > top) top = sum;
    } else if (g == 1) {
      P.hash[ord] = cls ? (mdup_name_hash(rec + MDUP_FIXED, f.l_name) & P.hash_mask) : P.sentinel;
    }
  }
  for (int d = 32; d > 0; d >>= 1) { const uint64_t o = __shfl_down(top, d); if (o > top) top = o; }
  if ((threadIdx.x & 63u) == 0 && top) atomicMax(reinterpret_cast<unsigned long long *>(&P.S->max_score), (unsigned long long)top);
}

__global__ void mdup_iota_kernel(uint32_t *v, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) v[i] = i;
}

// the name of an eligible record (the record kernel has held its lengths against the record)
__device__ __forceinline__ const uint8_t *mdup_name(const MdupView &V, uint32_t ord, uint32_t *l_name) {
  uint32_t len = 0;
  const uint8_t *rec = mdup_rec(V, ord, &len);
  if (!rec || MDUP_FIXED + (uint32_t)rec[12] > len) return nullptr;
  *l_name = rec[12];
  return rec + MDUP_FIXED;
}

// key[0, n) ascending, val[] the ordinals: the lane of a run's first element decides the pairs among the run's records, by name
__global__ __launch_bounds__(256) void mdup_runs_kernel(const uint64_t *key, const uint32_t *val, MdupView V, uint64_t sentinel, uint8_t *cls, uint32_t *mate, MdupState *S) {
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
    if (ox >= V.n || (cls[ox] & MDUP_C_SEEN)) continue;
    uint32_t lx = 0, count = 1, other = 0;
    const uint8_t *nx = mdup_name(V, ox, &lx);
    if (!nx) continue;
    for (uint64_t y = x + 1; y < end; ++y) {
      const uint32_t oy = val[y];
      if (oy >= V.n || (cls[oy] & MDUP_C_SEEN)) continue;
      uint32_t ly = 0;
      const uint8_t *ny = mdup_name(V, oy, &ly);
      if (!ny || !mdup_same_name(nx, lx, ny, ly)) continue;
      cls[oy] |= MDUP_C_SEEN;
      if (++count == 2) other = oy;
    }
    if (count == 2 && mdup_is_pair(cls[ox], cls[other])) {
      cls[ox] |= MDUP_C_PAIRED; cls[other] |= MDUP_C_PAIRED;
      mate[ox] = other; mate[other] = ox;
    }
  }
}

// a slot of the element list for every lane that wants one: one atomic a wave
__device__ __forceinline__ uint32_t mdup_slot(bool want, uint32_t *counter) {
  const unsigned long long m = __ballot(want);
  const uint32_t lane = threadIdx.x & 63u;
  uint32_t base = 0;
  if (m && lane == (uint32_t)(__ffsll((long long)m) - 1)) base = atomicAdd(counter, (uint32_t)__popcll(m));
  base = __shfl(base, m ? __ffsll((long long)m) - 1 : 0);
  return base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
}

struct MdupLists {
  uint32_t n;
  int score_bits;            // of a record's score; a template's field has one more
  const uint64_t *sig;
  const uint32_t *score, *mate;
  uint8_t *cls;
  uint64_t *key;
  uint32_t *val;
  MdupState *S;
};

// one element a pair: the ordinal of its 0x40 record under the pairs' tiebreak word
__global__ __launch_bounds__(256) void mdup_pair_list_kernel(MdupLists P) {
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  uint8_t c = 0;
  uint32_t m = 0;
  if (i < P.n) { c = P.cls[i]; m = P.mate[i]; }
  const bool want = (c & MDUP_C_PAIRED) && (c & MDUP_C_FIRST) && m < P.n;
  const uint32_t at = mdup_slot(want, &P.S->n_elem);
  if (want && at < P.n) { P.val[at] = (uint32_t)i; P.key[at] = mdup_tiebreak((uint64_t)P.score[i] + P.score[m], P.score_bits + 1, (uint32_t)i); }
}
// one element a fragment and one a pair end, the pair ends' class first
__global__ __launch_bounds__(256) void mdup_frag_list_kernel(MdupLists P) {
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  const uint8_t c = i < P.n ? P.cls[i] : 0;
  const bool want = (c & MDUP_C_ELIGIBLE) != 0;
  const uint32_t at = mdup_slot(want, &P.S->n_elem);
  if (want && at < P.n) {
    P.val[at] = (uint32_t)i;
    P.key[at] = (c & MDUP_C_PAIRED) ? (uint64_t)(uint32_t)i : (1ull << (32 + P.score_bits) | mdup_tiebreak(P.score[i], P.score_bits, (uint32_t)i));
  }
}

__device__ __forceinline__ void mdup_pair_key(const MdupLists &P, uint32_t v, uint64_t *lo, uint64_t *hi) {
  const uint32_t m = P.mate[v];
  const uint64_t a = P.sig[v], b = m < P.n ? P.sig[m] : a;
  *lo = a < b ? a : b; *hi = a < b ? b : a;
}
// which: 0 = the signature of the element's record, 1 = its pair's e_lo, 2 = its pair's e_hi
__global__ __launch_bounds__(256) void mdup_key_kernel(MdupLists P, int which) {
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= P.S->n_elem || i >= P.n) return;
  const uint32_t v = P.val[i];
  if (v >= P.n) return;
  uint64_t lo = P.sig[v], hi = lo;
  if (which) mdup_pair_key(P, v, &lo, &hi);
  P.key[i] = which == 2 ? hi : lo;
}
__global__ __launch_bounds__(256) void mdup_pair_mark_kernel(MdupLists P) {
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i == 0 || i >= P.S->n_elem || i >= P.n) return;
  const uint32_t v = P.val[i], w = P.val[i - 1];
  if (v >= P.n || w >= P.n) return;
  uint64_t lo, hi, lo2, hi2;
  mdup_pair_key(P, v, &lo, &hi);
  mdup_pair_key(P, w, &lo2, &hi2);
  if (lo != lo2 || hi != hi2) return;
  const uint32_t m = P.mate[v];
  P.cls[v] |= MDUP_C_MARK;                                    // (a record belongs to one pair, a pair to one element: no other lane writes these bytes)
  if (m < P.n) P.cls[m] |= MDUP_C_MARK;
}
__global__ __launch_bounds__(256) void mdup_frag_mark_kernel(MdupLists P) {
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i == 0 || i >= P.S->n_elem || i >= P.n) return;
  const uint32_t v = P.val[i], w = P.val[i - 1];
  if (v >= P.n || w >= P.n || (P.cls[v] & MDUP_C_PAIRED)) return;
  if (P.sig[v] == P.sig[w]) P.cls[v] |= MDUP_C_MARK;
}

// the decided bit into the arena -- 0x400 is bit 2 of the flag word's high byte, which has an address of any parity: one byte store
// where the byte changes -- and the counts
__global__ __launch_bounds__(256) void mdup_flag_kernel(MdupView V, const uint8_t *cls, MdupState *S) {
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  const uint8_t c = i < V.n ? cls[i] : 0;
  if (c & MDUP_C_ELIGIBLE) {
    uint32_t len = 0;
    uint8_t *rec = mdup_rec(V, (uint32_t)i, &len);
    if (rec) {
      const uint8_t b = rec[MDUP_FLAG_AT + 1], nb = (uint8_t)((b & ~(MDUP_DUP >> 8)) | ((c & MDUP_C_MARK) ? (MDUP_DUP >> 8) : 0u));
      if (nb != b) rec[MDUP_FLAG_AT + 1] = nb;
    }
  }
  const bool el = (c & MDUP_C_ELIGIBLE) != 0, pr = el && (c & MDUP_C_PAIRED), first = pr && (c & MDUP_C_FIRST), mk = (c & MDUP_C_MARK) != 0;
  const bool what[5] = {first, first && mk, el && !pr, el && !pr && mk, i < V.n && !el};
  for (int k = 0; k < 5; ++k) {
    const unsigned long long m = __ballot(what[k]);
    if (m && (threadIdx.x & 63u) == 0) atomicAdd(reinterpret_cast<unsigned long long *>(&S->counts[k]), (unsigned long long)__popcll(m));
  }
}

int mdup_hash_bits() {
  static const int v = [] {
    const char *e = getenv("STRL_MARKDUP_HASH_BITS");        // tests: different names under one hash as a rule
    const int x = e ? atoi(e) : 0;
    return x >= 1 && x <= 63 ? x : 63;
  }();
  return v;
}

}  // namespace

int markdup_run(strl_ctx *c, const BsortView &B, strl_markdup_info *out) {
  hipStream_t st = c->stream;
  strl_markdup_info I{};
  const uint32_t n = (uint32_t)B.n_records;
  if (B.n_records > BSORT_MAX_RECORDS) { set_error("markdup: more than 2^32 - 2 records"); return STRL_ERR_LIMIT; }
  if (!n) { if (out) *out = I; return STRL_OK; }
  const int hb = mdup_hash_bits(), ord_bits = bsort_bits(n), sig_bits = mdup_sig_bits(B.n_ref);
  const uint64_t sentinel = 1ull << hb, hash_mask = sentinel - 1ull;
  const size_t sb = radix_sort_scratch_bytes(n, 64);
  DevBuf sig, score, mate, cls, k0, k1, v0, v1, scratch, state;
  int rc;
  if ((rc = sig.reserve((size_t)n * 8 + 64)) || (rc = score.reserve((size_t)n * 4 + 64)) || (rc = mate.reserve((size_t)n * 4 + 64)) || (rc = cls.reserve((size_t)n + 64)) ||
      (rc = k0.reserve((size_t)n * 8 + 64)) || (rc = k1.reserve((size_t)n * 8 + 64)) || (rc = v0.reserve((size_t)n * 4 + 64)) || (rc = v1.reserve((size_t)n * 4 + 64)) ||
      (rc = scratch.reserve(sb + 64)) || (rc = state.reserve(sizeof(MdupState))))
    return rc;
  hipEvent_t ev[6] = {};
  struct Events { hipEvent_t *e; ~Events() { for (int k = 0; k < 6; ++k) if (e[k]) (void)hipEventDestroy(e[k]); } } guard{ev};
  for (hipEvent_t &e : ev) STRL_HIP(hipEventCreate(&e));
  MdupState H{};
  H.err_ord[0] = H.err_ord[1] = ~0ull;
  MdupState *S = state.as<MdupState>();
  STRL_HIP(hipMemcpyAsync(S, &H, sizeof H, hipMemcpyHostToDevice, st));
  STRL_HIP(hipMemsetAsync(mate.p, 0xff, (size_t)n * 4, st));
  const MdupView V{B.src, B.len, B.slab, B.slab_used, B.n_slabs, n};
  const unsigned blocks = (n + 255u) / 256u;

  // ---- the records ----
  STRL_HIP(hipEventRecord(ev[0], st));
  const unsigned rgrid = (unsigned)std::min<uint64_t>(8192, ((uint64_t)n * MDUP_G + 255u) / 256u);
  const MdupRecord RP{V, sig.as<uint64_t>(), k0.as<uint64_t>(), score.as<uint32_t>(), cls.as<uint8_t>(), hash_mask, sentinel, S};
  hipLaunchKernelGGL(mdup_record_kernel, dim3(rgrid), dim3(256), 0, st, RP);
  STRL_HIP(hipGetLastError());
  STRL_HIP(hipEventRecord(ev[1], st));
  STRL_HIP(hipMemcpyAsync(&H, S, sizeof H, hipMemcpyDeviceToHost, st));
  STRL_HIP(hipStreamSynchronize(st));
  if (H.err_ord[0] != ~0ull && H.err_ord[0] <= H.err_ord[1]) {
    set_error("malformed BAM record %llu: its name, CIGAR, bases and qualities do not fit its block_size", (unsigned long long)H.err_ord[0]);
    return STRL_ERR_FORMAT;
  }
  if (H.err_ord[1] != ~0ull) { set_error("malformed BAM record %llu: its unclipped end is no 32-bit position", (unsigned long long)H.err_ord[1]); return STRL_ERR_FORMAT; }
  const int score_bits = std::max(1, bsort_bits((uint32_t)std::min<uint64_t>(H.max_score, 0x3fffffffull)));

  // a stable sort of the current (key, value) buffers over one bit window; the buffers that hold the result become the current ones
  uint64_t *key = k0.as<uint64_t>(), *key_alt = k1.as<uint64_t>();
  uint32_t *val = v0.as<uint32_t>(), *val_alt = v1.as<uint32_t>();
  auto sort = [&](const uint32_t *d_n, int bit_lo, int bits) -> int {
    uint64_t *ok = key;
    uint32_t *ov = val;
    const int se = radix_sort_pairs(st, d_n, n, key, val, key_alt, val_alt, scratch.p, sb, bit_lo, bits, &ok, &ov);
    if (se) { set_error("radix_sort_pairs failed: %s", hipGetErrorString((hipError_t)se)); return STRL_ERR_HIP; }
    if (ok != key) { std::swap(key, key_alt); std::swap(val, val_alt); }
    return STRL_OK;
  };
  // the count of all records, for the join's sort: on the device like the lists' counts
  STRL_HIP(hipMemcpyAsync(&S->n_elem, &n, 4, hipMemcpyHostToDevice, st));

  // ---- the join by name ----
  hipLaunchKernelGGL(mdup_iota_kernel, dim3(blocks), dim3(256), 0, st, val, n);
  if ((rc = sort(&S->n_elem, 0, hb + 1))) return rc;
  hipLaunchKernelGGL(mdup_runs_kernel, dim3(blocks), dim3(256), 0, st, key, val, V, sentinel, cls.as<uint8_t>(), mate.as<uint32_t>(), S);
  STRL_HIP(hipGetLastError());
  STRL_HIP(hipEventRecord(ev[2], st));
  STRL_HIP(hipMemcpyAsync(&H, S, sizeof H, hipMemcpyDeviceToHost, st));
  STRL_HIP(hipStreamSynchronize(st));
  if (H.run_max) {
    set_error("markdup: %u eligible records share one name hash, more than the %u a run of the device's join resolves; mark this file on the host: STRL_SORT=host", H.run_max, MDUP_RUN_MAX);
    return STRL_ERR_LIMIT;
  }

  // ---- the pairs ----
  MdupLists L{n, score_bits, sig.as<uint64_t>(), score.as<uint32_t>(), mate.as<uint32_t>(), cls.as<uint8_t>(), key, val, S};
  auto lists = [&]() { L.key = key; L.val = val; return L; };
  STRL_HIP(hipMemsetAsync(&S->n_elem, 0, 4, st));
  hipLaunchKernelGGL(mdup_pair_list_kernel, dim3(blocks), dim3(256), 0, st, lists());
  if ((rc = sort(&S->n_elem, 0, ord_bits)) || (rc = sort(&S->n_elem, 32, score_bits + 1))) return rc;
  hipLaunchKernelGGL(mdup_key_kernel, dim3(blocks), dim3(256), 0, st, lists(), 2);
  if ((rc = sort(&S->n_elem, 0, sig_bits))) return rc;
  hipLaunchKernelGGL(mdup_key_kernel, dim3(blocks), dim3(256), 0, st, lists(), 1);
  if ((rc = sort(&S->n_elem, 0, sig_bits))) return rc;
  hipLaunchKernelGGL(mdup_pair_mark_kernel, dim3(blocks), dim3(256), 0, st, lists());
  STRL_HIP(hipGetLastError());
  STRL_HIP(hipEventRecord(ev[3], st));

  // ---- the fragments ----
  STRL_HIP(hipMemsetAsync(&S->n_elem, 0, 4, st));
  hipLaunchKernelGGL(mdup_frag_list_kernel, dim3(blocks), dim3(256), 0, st, lists());
  if ((rc = sort(&S->n_elem, 0, ord_bits)) || (rc = sort(&S->n_elem, 32, score_bits + 1))) return rc;
  hipLaunchKernelGGL(mdup_key_kernel, dim3(blocks), dim3(256), 0, st, lists(), 0);
  if ((rc = sort(&S->n_elem, 0, sig_bits))) return rc;
  hipLaunchKernelGGL(mdup_frag_mark_kernel, dim3(blocks), dim3(256), 0, st, lists());
  STRL_HIP(hipGetLastError());
  STRL_HIP(hipEventRecord(ev[4], st));

  // ---- the flags ----
  hipLaunchKernelGGL(mdup_flag_kernel, dim3(blocks), dim3(256), 0, st, V, cls.as<uint8_t>(), S);
  STRL_HIP(hipGetLastError());
  STRL_HIP(hipEventRecord(ev[5], st));
  STRL_HIP(hipMemcpyAsync(&H, S, sizeof H, hipMemcpyDeviceToHost, st));
  STRL_HIP(hipStreamSynchronize(st));
  I.n_pairs = H.counts[0]; I.n_dup_pairs = H.counts[1]; I.n_fragments = H.counts[2]; I.n_dup_fragments = H.counts[3]; I.n_ineligible = H.counts[4];
  double *ms[5] = {&I.record_ms, &I.join_ms, &I.pairs_ms, &I.fragments_ms, &I.flag_ms};
  for (int k = 0; k < 5; ++k) { float t = 0.f; if (hipEventElapsedTime(&t, ev[k], ev[k + 1]) == hipSuccess) *ms[k] = t; else (void)hipGetLastError(); }
  if (out) *out = I;
  return STRL_OK;
}

}  // namespace strl
