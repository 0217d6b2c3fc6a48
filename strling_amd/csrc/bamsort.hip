// bamsort.hip -- `strling sort`: a BAM coordinate-sorted on the GPU (gfx950), the whole file resident.  What
// `samtools sort` does on the host (the reference's simulator shells out to it, simulate_reads.nim:178).  A chunk of BGZF blocks
// goes through
//   front_stage_a        (front.hip)   copy + inflate + CRC + record scan: recoff[] of the chunk
//   bsort_keys_kernel                  one lane per record: key (bamsort_core.h), len = 4 + block_size, src = where the record
//                                      lies in the arena; the first refused record through an integer atomicMin
//   a device-to-device copy            the chunk's complete records into the arena: fixed-size slabs allocated as the file is
//                                      read, a chunk wholly inside one slab, nothing ever copied again to grow
// and at the end
//   radix_sort_pairs     (sort.hip)    (key, ordinal), stable, over the 33 + bits(n_ref) key bits that can differ
//   bsort_tile_kernel<false> / bsort_scan_kernel / bsort_tile_kernel<true>
//                                      the layout: exclusive 64-bit sums of len in sorted order, based at the header's size, tiled;
//                                      and whether the permutation is the identity (the input was in order already)
// The output stream (header || records in sorted order) is never materialised whole: a piece [lo, hi) of it is gathered on request
//   bsort_range_kernel                 the two binary searches over the sums: the records that touch the piece
//   bsort_gather_kernel                a group of 16 lanes per record copies the part inside the piece with aligned 16-byte stores,
//                                      each assembled from two aligned loads (source and destination differ mod 16)
// and leaves as it is (strl_bamsort_fetch) or through the device BGZF compressor (deflate.hip; strl_bamsort_fetch_bgzf).
// A file larger than device memory (`sort --windowed`; strl_bamsort_begin_windowed) keeps no arena: pass 0 is
// the keys kernel alone (12 bytes a record stay), the finish adds
//   bsort_dest_kernel                  dest[perm[j]] = off[j]: where every record of the INPUT starts in the stream
// and every later pass reads the file again for one window [lo, hi) of the stream (strl_bamsort_window_begin / _push / _end)
//   bsort_scatter_kernel               a group of 16 lanes per record of the chunk copies the part inside the window to its place,
//                                      as the gather copies; a length that is not pass 0's is refused, the bytes placed are counted
// after which the window buffer is a finished piece of the stream and the fetches read it.
// SAM text (strl_bamsort_sam_begin / strl_bamsort_push_sam) is a second producer of "records back to back plus
// recoff[]": samparse.hip encodes a chunk of lines into a slot, and bsort_keys_kernel and the copy into the arena run over that slot
// as they run over an inflated chunk; everything behind the read phase is the same.
#include <string.h>
#include <algorithm>
#include <vector>
#include "front.h"
#include "sort.h"
#include "device_util.h"
#include "bamsort_core.h"
#include "samparse.h"
#include "markdup_core.h"
#include "fastq_core.h"

namespace strl {

constexpr uint32_t BSORT_TILE = 2048;                        // ranks per workgroup of the layout: 256 lanes x 8
constexpr uint32_t BSORT_E_TID = 0, BSORT_E_RECORD = 1;

struct BsortState {          // device words of a sort
  uint64_t err_ord[2];       // ordinal of the first record refused for its refID / that does not lie inside its chunk; ~0 = none
  uint64_t n_no_ref;
  uint64_t total;            // the layout's sum: bytes of all records
  uint64_t range[2];         // the records that touch the piece asked for last
  uint32_t not_identity, n;  // n: the device-side count the sort reads
};

struct BsortKeys {
  const uint8_t *U;
  const uint32_t *recoff;
  uint32_t n, start0, rec_end;
  int32_t n_ref;
  uint64_t ord0, cap;        // ordinal of the chunk's first record; slots of key / len / src
  uint64_t src0;             // slab << 40 | offset of the chunk's byte start0
  uint64_t *key, *src;
  uint32_t *len;
  BsortState *S;
};

__global__ __launch_bounds__(256) void bsort_keys_kernel(BsortKeys P) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  const bool act = i < P.n && P.ord0 + i < P.cap;
  bool no_ref = false;
  if (act) {
    const uint32_t q = P.recoff[i];
    uint64_t key = (uint64_t)(uint32_t)P.n_ref << 33, bad = ~0ull;
    uint32_t len = 0;
    uint32_t kind = BSORT_E_RECORD;
    if (q >= P.start0 && q <= P.rec_end && P.rec_end - q >= BSORT_MIN_REC) {
      const uint8_t *R = P.U + q;
      const uint32_t bs = ld32u(R);
      if (bs >= 32u && bs <= P.rec_end - q - 4u) {
        len = bs + 4u;
        if (bsort_key(R + 4, P.n_ref, &key)) no_ref = (int32_t)ld32u(R + 4) < 0;
        else { bad = P.ord0 + i; kind = BSORT_E_TID; }
      } else bad = P.ord0 + i;
    } else bad = P.ord0 + i;
    if (bad != ~0ull) atomicMin(reinterpret_cast<unsigned long long *>(&P.S->err_ord[kind]), (unsigned long long)bad);
    P.key[P.ord0 + i] = key;
    P.len[P.ord0 + i] = len;                                  // (0 for a refused record: nothing of it is ever copied)
    if (P.src) P.src[P.ord0 + i] = P.src0 + (uint64_t)(q - (len ? P.start0 : q));      // (null: a windowed sort keeps no arena)
  }
  const unsigned long long m = __ballot(no_ref);
  if (m && (threadIdx.x & 63u) == 0) atomicAdd(reinterpret_cast<unsigned long long *>(&P.S->n_no_ref), (unsigned long long)__popcll(m));
}

__global__ void bsort_iota_kernel(uint32_t *v, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) v[i] = i;
}

// ---- layout: off[j] = base + sum of len[perm[k]], k < j; off[n] = base + everything -------------------------------------------
// the sum of the 256 lanes' values in every lane's hand; sh: 4 words
__device__ __forceinline__ uint64_t bsort_block_excl(uint64_t v, uint64_t *sh, uint64_t *block_total) {
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
template <bool ADD> __global__ __launch_bounds__(256) void bsort_tile_kernel(const uint32_t *perm, const uint32_t *len, uint32_t n, uint64_t n_len, uint64_t base,
                                                                              uint64_t *tile, uint64_t *off, BsortState *S) {
  __shared__ uint64_t sh[4];
  const uint64_t j0 = (uint64_t)blockIdx.x * BSORT_TILE + (uint64_t)threadIdx.x * 8u;
  uint32_t l[8];
  uint64_t mine = 0;
  bool moved = false;
  for (uint32_t k = 0; k < 8u; ++k) {
    const uint64_t j = j0 + k;
    l[k] = 0;
    if (j < n) {
      const uint32_t p = perm[j];
      if (p < n_len) l[k] = len[p];
      moved = moved || p != (uint32_t)j;
    }
    mine += l[k];
  }
  uint64_t tot;
  uint64_t at = bsort_block_excl(mine, sh, &tot);
  if constexpr (!ADD) {
    if (threadIdx.x == 0) tile[blockIdx.x] = tot;
    if (moved) S->not_identity = 1u;                          // (plain stores of the same value)
  } else {
    at += base + tile[blockIdx.x];
    for (uint32_t k = 0; k < 8u; ++k) { const uint64_t j = j0 + k; if (j < n) off[j] = at; at += l[k]; }
  }
}
// one workgroup: tile[0, n_tiles) -> exclusive sums in place, the total to S->total and base + total to off[n]
__global__ __launch_bounds__(1024) void bsort_scan_kernel(uint64_t *tile, uint32_t n_tiles, uint64_t base, uint64_t *off, uint32_t n, BsortState *S) {
  __shared__ uint64_t part[1024];
  const uint32_t t = threadIdx.x, per = (n_tiles + 1023u) / 1024u, a = min(n_tiles, t * per), b = min(n_tiles, a + per);
  uint64_t s = 0;
  for (uint32_t k = a; k < b; ++k) s += tile[k];
  part[t] = s;
  __syncthreads();
  if (t == 0) {
    uint64_t run = 0;
    for (int k = 0; k < 1024; ++k) { const uint64_t v = part[k]; part[k] = run; run += v; }
    S->total = run; off[n] = base + run;
  }
  __syncthreads();
  uint64_t run = part[t];
  for (uint32_t k = a; k < b; ++k) { const uint64_t v = tile[k]; tile[k] = run; run += v; }
}

// ---- a piece of the stream -----------------------------------------------------------------------------------------------------
__global__ void bsort_range_kernel(const uint64_t *off, uint64_t n, uint64_t lo, uint64_t hi, BsortState *S) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const uint64_t a = bsort_first_touch(off, n, lo), b = bsort_end_touch(off, n, hi);
    S->range[0] = a; S->range[1] = b > a ? b : a;
  }
}
// test-only (strl_bamsort_probe): the parts of the touched records, as the gather computes them
__global__ void bsort_parts_kernel(const uint64_t *off, uint64_t n, uint64_t lo, uint64_t hi, const BsortState *S, uint64_t *parts, uint64_t cap) {
  const uint64_t a = S->range[0], b = S->range[1];
  for (uint64_t j = a + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < b && j < n; j += (uint64_t)gridDim.x * blockDim.x) {
    if (j - a >= cap) return;
    const BsortPart p = bsort_part(off[j], off[j + 1], lo, hi);
    parts[3 * (j - a)] = p.skip; parts[3 * (j - a) + 1] = p.dst; parts[3 * (j - a) + 2] = p.bytes;
  }
}

struct BsortGather {
  const uint64_t *off, *src;
  const uint32_t *perm;
  uint64_t n;
  uint8_t *const *slab;        // [n_slabs] bases (16-byte aligned; 64 readable bytes behind each slab's last byte)
  const uint64_t *slab_bytes;
  uint32_t n_slabs;
  const uint8_t *header;
  uint64_t header_bytes;
  uint64_t lo, hi;
  uint8_t *piece;              // 16-byte aligned, hi - lo bytes
  const BsortState *S;
};

// 16 bytes from an address that is `sh` bytes (1 .. 15) behind the aligned one `p` points to
__device__ __forceinline__ uint4 bsort_load_shifted(const uint4 *p, uint32_t sh) {
  const uint4 a = p[0], b = p[1];
  const uint32_t ws = sh >> 2, bs = (sh & 3u) * 8u;
  uint32_t x0, x1, x2, x3, x4;
  if (ws == 0) { x0 = a.x; x1 = a.y; x2 = a.z; x3 = a.w; x4 = b.x; }
  else if (ws == 1) { x0 = a.y; x1 = a.z; x2 = a.w; x3 = b.x; x4 = b.y; }
  else if (ws == 2) { x0 = a.z; x1 = a.w; x2 = b.x; x3 = b.y; x4 = b.z; }
  else { x0 = a.w; x1 = b.x; x2 = b.y; x3 = b.z; x4 = b.w; }
  if (!bs) return make_uint4(x0, x1, x2, x3);
  return make_uint4(x0 >> bs | x1 << (32u - bs), x1 >> bs | x2 << (32u - bs), x2 >> bs | x3 << (32u - bs), x3 >> bs | x4 << (32u - bs));
}

// G lanes per record (a wave holds 64 / G records at a time)
template <uint32_t G> __global__ __launch_bounds__(256) void bsort_gather_kernel(BsortGather P) {
  const uint64_t piece_bytes = P.hi - P.lo;
  // header bytes inside the piece
  if (P.lo < P.header_bytes) {
    const uint64_t e = (P.hi < P.header_bytes ? P.hi : P.header_bytes) - P.lo;
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < e; i += (uint64_t)gridDim.x * 256u) P.piece[i] = P.header[P.lo + i];
  }
  const uint64_t first = P.S->range[0], end = P.S->range[1] < P.n ? P.S->range[1] : P.n;
  const uint32_t g = threadIdx.x % G;
  const uint64_t group = ((uint64_t)blockIdx.x * 256u + threadIdx.x) / G, n_groups = (uint64_t)gridDim.x * 256u / G;
  for (uint64_t j = first + group; j < end; j += n_groups) {
    const BsortPart pt = bsort_part(P.off[j], P.off[j + 1], P.lo, P.hi);
    const uint64_t s = P.src[P.perm[j]];
    const uint64_t sl = s >> BSORT_SLAB_SHIFT, so = (s & BSORT_SLAB_MASK) + pt.skip;
    if (!pt.bytes || sl >= P.n_slabs || so > P.slab_bytes[sl] || pt.bytes > P.slab_bytes[sl] - so || pt.dst > piece_bytes || pt.bytes > piece_bytes - pt.dst) continue;
    const uint8_t *src = P.slab[sl] + so;
    uint8_t *dst = P.piece + pt.dst;
    const uint64_t to16 = (16u - (uint32_t)(pt.dst & 15u)) & 15u, head = pt.bytes < to16 ? pt.bytes : to16;
    if (g < head) dst[g] = src[g];                            // (head < 16 <= G)
    const uint64_t n_vec = (pt.bytes - head) >> 4;
    const uint8_t *sv = src + head;
    const uint32_t sh = (uint32_t)(reinterpret_cast<uintptr_t>(sv) & 15u);
    const uint4 *sa = reinterpret_cast<const uint4 *>(sv - sh);
    uint4 *da = reinterpret_cast<uint4 *>(dst + head);
    if (sh) for (uint64_t v = g; v < n_vec; v += G) da[v] = bsort_load_shifted(sa + v, sh);
    else for (uint64_t v = g; v < n_vec; v += G) da[v] = sa[v];
    const uint64_t done = head + (n_vec << 4), tail = pt.bytes - done;
    if (g < tail) dst[done + g] = src[done + g];              // (tail < 16)
  }
}

// ---- `sort --windowed`: the file read again for every window of the stream ---------------------------------------------------------
// dest[perm[j]] = off[j]: the permutation inverted once, so that a pass over the input reads dest[] and len[] in input order, coalesced
__global__ __launch_bounds__(256) void bsort_dest_kernel(const uint32_t *perm, const uint64_t *off, uint32_t n, uint64_t *dest) {
  const uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (j < n) { const uint32_t p = perm[j]; if (p < n) dest[p] = off[j]; }
}

struct BsortWinState {       // device words of a window's pass
  uint64_t err_ord;          // ordinal of the first record that is not pass 0's (length, count, or outside its chunk); ~0 = none
  uint64_t placed;           // bytes of records placed in the window
};

struct BsortScatter {
  const uint8_t *U;          // the chunk's inflated bytes (16-byte aligned; src_cap readable bytes)
  const uint32_t *recoff;
  uint32_t n, start0, rec_end;
  uint64_t src_cap;
  uint64_t ord0, n_records;  // ordinal of the chunk's first record; records of pass 0
  const uint64_t *dest;      // [n_records] by input ordinal
  const uint32_t *len;
  uint64_t lo, hi;
  uint8_t *window;           // 16-byte aligned, hi - lo bytes
  BsortWinState *S;
};

// G lanes per record of the chunk: the part of it inside the window goes to its place, copied as the gather copies
template <uint32_t G> __global__ __launch_bounds__(256) void bsort_scatter_kernel(BsortScatter P) {
  const uint64_t win_bytes = P.hi - P.lo;
  const uint32_t g = threadIdx.x % G;
  const uint64_t group = ((uint64_t)blockIdx.x * 256u + threadIdx.x) / G, n_groups = (uint64_t)gridDim.x * 256u / G;
  uint64_t placed = 0;                                        // (counted by lane 0 of a group)
  for (uint64_t i = group; i < P.n; i += n_groups) {
    const uint64_t ord = P.ord0 + i;
    const uint32_t q = P.recoff[i];
    BsortPart pt{0, 0, 0};
    bool ok = false;
    uint32_t len = 0;
    if (ord < P.n_records && q >= P.start0 && q <= P.rec_end && P.rec_end - q >= BSORT_MIN_REC) {      // (the chunk bounds of bsort_keys_kernel)
      const uint32_t bs = ld32u(P.U + q);
      len = P.len[ord];
      ok = bs >= 32u && bs <= P.rec_end - q - 4u && bsort_scatter_part(P.dest[ord], len, bs, P.lo, P.hi, &pt);
    }
    if (!ok) { if (g == 0) atomicMin(reinterpret_cast<unsigned long long *>(&P.S->err_ord), (unsigned long long)ord); continue; }
    // outside the window: nothing to do for the whole group.  Source inside the record (so inside [start0, rec_end): q + len <= rec_end
    // by the check above), destination inside the window
    if (!pt.bytes || pt.skip > len || pt.bytes > len - pt.skip || pt.dst > win_bytes || pt.bytes > win_bytes - pt.dst) continue;
    const uint64_t so = (uint64_t)q + pt.skip;
    const uint8_t *src = P.U + so;
    uint8_t *dst = P.window + pt.dst;
    if (g == 0) placed += pt.bytes;
    const uint64_t to16 = (16u - (uint32_t)(pt.dst & 15u)) & 15u, head = pt.bytes < to16 ? pt.bytes : to16;
    const uint64_t n_vec = (pt.bytes - head) >> 4;
    const uint32_t sh = (uint32_t)((so + head) & 15u);        // (U is 16-byte aligned)
    // the shifted copy's second aligned load reads up to 16 bytes behind the last one copied, so behind the record's end at most 16
    // bytes: the front end leaves 256 readable bytes behind a slot's inflated end (front.hip, S.infl.reserve(end + 256)), which is
    // what src_cap holds the loads against.  Where they do not fit the bytes go singly
    if (n_vec && so + head - sh + (n_vec + 1u) * 16u > P.src_cap) {
      for (uint64_t b = g; b < pt.bytes; b += G) dst[b] = src[b];
      continue;
    }
    if (g < head) dst[g] = src[g];                            // (head < 16 <= G)
    const uint4 *sa = reinterpret_cast<const uint4 *>(src + head - sh);
    uint4 *da = reinterpret_cast<uint4 *>(dst + head);
    if (sh) for (uint64_t v = g; v < n_vec; v += G) da[v] = bsort_load_shifted(sa + v, sh);
    else for (uint64_t v = g; v < n_vec; v += G) da[v] = sa[v];
    const uint64_t done = head + (n_vec << 4), tail = pt.bytes - done;
    if (g < tail) dst[done + g] = src[done + g];              // (tail < 16)
  }
  // the bytes placed: summed over the wave, one vector atomic a wave
  for (int d = 32; d > 0; d >>= 1) placed += __shfl_down(placed, d);
  if ((threadIdx.x & 63u) == 0 && placed) atomicAdd(reinterpret_cast<unsigned long long *>(&P.S->placed), (unsigned long long)placed);
}

// test-only (strl_bamsort_window_probe): the scatter's part of every record, by ordinal, with the block_size word pass 0 saw
__global__ void bsort_wparts_kernel(const uint64_t *dest, const uint32_t *len, uint32_t n, uint64_t lo, uint64_t hi, uint64_t *parts) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  BsortPart p{0, 0, 0};
  if (!bsort_scatter_part(dest[i], len[i], len[i] - 4u, lo, hi, &p)) p.skip = p.dst = p.bytes = ~0ull;
  parts[3 * i] = p.skip; parts[3 * i + 1] = p.dst; parts[3 * i + 2] = p.bytes;
}

struct BsortSlab { DevBuf buf; uint64_t bytes = 0, used = 0; };
struct strl_bsort {
  int32_t n_ref = 0;
  uint64_t slab_want = 0, arena_limit = 0;
  const strl_front *front = nullptr;          // the front end strl_bamsort_begin made: another pass' begin replaces it
  std::vector<BsortSlab> slabs;
  uint64_t arena_bytes = 0;
  DevBuf key, len, src, state;                 // resident, one entry per record
  DevBuf key_alt, val, val_alt, scratch, off, tile, d_header, d_slab, piece;      // the finish step's, and a fetch's
  BsortState *h_state = nullptr;               // pinned
  uint32_t *perm = nullptr;                    // device: inside val / val_alt
  uint64_t chunks = 0, done = 0, n_records = 0, rec_cap = 0;
  uint64_t header_bytes = 0, stream_bytes = 0;
  bool finished = false;
  int fail_rc = 0;
  std::string fail;
  hipEvent_t e0 = nullptr, e1 = nullptr, e2 = nullptr;
  strl_bamsort_info info{};
  strl_bai *index = nullptr;                   // `sort --write-index`: the index builder over the sorted records (bamindex.hip strl_bamsort_index)
  // `sort --windowed`: no arena, no src; behind the finish only dest[ordinal] and len[ordinal] stay
  bool windowed = false;
  int deflate_mode = STRL_DEFLATE_FAST;        // the rule of strl_bamsort_fetch_bgzf (strl_bamsort_deflate_mode)
  DevBuf dest, window, wstate;
  BsortWinState *h_wstate = nullptr;           // pinned
  std::vector<uint8_t> header;                 // the output's header bytes: every window that holds some gets them again
  uint64_t first_off = 0;                      // strl_bamsort_begin_windowed's: the front end is rewound with it
  uint32_t res_blocks = 0;                     // strl_bamsort_reserve's, repeated for every window's front end
  uint64_t res_comp = 0;
  uint64_t win_lo = 0, win_hi = 0;
  bool win_open = false, win_done = false;     // a window's pass is running | the window is complete and may be fetched from
  uint64_t w_chunks = 0, w_done = 0, w_ord = 0;   // chunks pushed / scattered in this pass; ordinal of the next chunk's first record
  SamParser *sam = nullptr;                    // the input is SAM text (strl_bamsort_sam_begin): no front end, samparse.hip's slots instead
  // `sort --markdup` (markdup.hip): asked for before the first push | ran | a piece has been gathered: the flags can no longer change
  bool markdup_on = false, markdup_done = false, fetched = false;
  // `strling fastq` (fastq.hip): asked for before the first push | the plan of the three streams, once strl_bamsort_fastq has run
  bool fastq_on = false;
  FastqPlan *fastq = nullptr;
};
static_assert(SAM_REC_MAX == FRONT_CARRY_MAX, "a record from SAM text is held to the front end's limit");

void bsort_destroy(strl_bsort *B) {
  if (!B) return;
  if (B->index) bai_destroy(B->index);
  fastq_destroy(B->fastq);
  if (B->sam) sam_parser_destroy(B->sam);
  if (B->h_state) (void)hipHostFree(B->h_state);
  if (B->h_wstate) (void)hipHostFree(B->h_wstate);
  for (hipEvent_t e : {B->e0, B->e1, B->e2}) if (e) (void)hipEventDestroy(e);
  delete B;
}

// the finished sort of the context, for the index step; *slot: where its builder hangs (bsort_destroy destroys it)
int bsort_view(strl_ctx *c, BsortView *v, strl_bai ***slot) {
  if (!c || !c->bsort || !c->bsort->finished) return STRL_ERR_ARG;
  strl_bsort *B = c->bsort;
  if (B->windowed) return 2;                   // (a windowed sort holds no records: strl_bamsort_index says so)
  const size_t ns = B->slabs.size();
  *v = BsortView{B->off.as<uint64_t>(), B->src.as<uint64_t>(), B->perm, B->len.as<uint32_t>(), B->d_slab.as<uint8_t *>(), B->d_slab.as<uint64_t>() + ns, (uint32_t)ns, B->n_ref,
                 B->n_records, B->stream_bytes};
  *slot = &B->index;
  return STRL_OK;
}

static int bsort_fail(strl_bsort *B, int rc) {
  if (rc && !B->fail_rc) { B->fail_rc = rc; B->fail = strl_last_error(); }
  return rc;
}

static uint64_t bsort_slab_want() {
  const char *e = getenv("STRL_SORT_SLAB_MB");               // tests: tiny slabs (fractions allowed)
  const double mb = e ? atof(e) : 0.0;
  return mb > 0 ? std::max<uint64_t>(4096, (uint64_t)(mb * 1048576.0)) : (uint64_t)4 << 30;
}

// room for `bytes` of a chunk's records, wholly inside one slab: *src0 = slab << 40 | offset, *dst = where they go
static int bsort_place(strl_bsort *B, uint64_t bytes, uint64_t n_more, uint64_t *src0, uint8_t **dst) {
  if (B->slabs.empty() || B->slabs.back().bytes - B->slabs.back().used < bytes) {
    const uint64_t want = std::max(B->slab_want, bytes);
    if (want > BSORT_SLAB_MASK || B->slabs.size() >= (1u << 20)) { set_error("bamsort: a chunk of %llu bytes / too many slabs", (unsigned long long)bytes); return STRL_ERR_LIMIT; }
    uint64_t limit = B->arena_limit;
    const char *what = "the arena's limit";
    if (!limit) {
      // what the device has free, minus the finish step's needs: 24 bytes a record (the sort's other buffers, the offsets), a quarter more
      // for the records still to come, and the sort's scratch, the piece and the compressor's buffers
      size_t fr = 0, tot = 0;
      if (hipMemGetInfo(&fr, &tot) != hipSuccess) { (void)hipGetLastError(); fr = ~(size_t)0 >> 1; }
      // (`sort --markdup`: MDUP_RECORD_BYTES more for the step between the finish and the first fetch)
      // (`strling fastq`: FASTQ_RECORD_BYTES more for its plan)
      const uint64_t keep = (B->n_records + n_more) * (30ull + (B->markdup_on ? MDUP_RECORD_BYTES : 0ull) + (B->fastq_on ? FASTQ_RECORD_BYTES : 0ull)) + ((uint64_t)768 << 20);
      limit = B->arena_bytes + (fr > keep ? (uint64_t)fr - keep : 0);
      what = "the device's free memory less the finish step's needs";
    }
    if (B->arena_bytes + want > limit) {
      set_error("bamsort: the arena holds %llu bytes in %zu slabs and needs %llu more, past %s (%llu bytes)", (unsigned long long)B->arena_bytes, B->slabs.size(),
                (unsigned long long)want, what, (unsigned long long)limit);
      return STRL_ERR_NOMEM;
    }
    BsortSlab s;
    const size_t ask = (size_t)((want + 64) / 9 * 8 + 64);    // (DevBuf::reserve adds an eighth: the slab comes out a little above `want`)
    if (s.buf.reserve(ask) || s.buf.cap < want + 64) {
      if (s.buf.p) s.buf.release();
      const std::string why = strl_last_error();
      set_error("bamsort: the arena holds %llu bytes in %zu slabs and needs %llu more: %s", (unsigned long long)B->arena_bytes, B->slabs.size(), (unsigned long long)want, why.c_str());
      return STRL_ERR_NOMEM;
    }
    s.bytes = ((uint64_t)s.buf.cap - 64) & ~(uint64_t)15;
    B->arena_bytes += s.bytes;
    B->slabs.push_back(std::move(s));
  }
  BsortSlab &s = B->slabs.back();
  *src0 = (uint64_t)(B->slabs.size() - 1) << BSORT_SLAB_SHIFT | s.used;
  *dst = s.buf.as<uint8_t>() + s.used;
  s.used += bytes;
  return STRL_OK;
}

// keys and arena copy of the chunk in slot si (its record scan was enqueued by the push before)
static int bsort_chunk(strl_ctx *c, strl_front *F, strl_bsort *B, int si) {
  FrontSlot &S = F->slot[si];
  STRL_HIP(hipEventSynchronize(S.ev_a));
  const FrontInfo I = S.h_info[0];
  if (I.err & FRONT_ERR_INFLATE) { set_error("invalid BGZF block (DEFLATE data or ISIZE)"); return STRL_ERR_FORMAT; }
  if (I.err & FRONT_ERR_CRC) { set_error("CRC32 checksum mismatch in a BGZF block"); return STRL_ERR_CRC; }
  if (I.err & FRONT_ERR_RECORD) { set_error("malformed BAM record"); return STRL_ERR_FORMAT; }
  if (I.err & FRONT_ERR_CARRY) { set_error("BAM record of more than %u bytes", FRONT_CARRY_MAX); return STRL_ERR_FORMAT; }
  const uint32_t n = I.n_records, rec_end = std::min(I.carry_off, I.end);
  hipStream_t st = c->stream;
  int rc;
  if (n && rec_end > I.start0 && (uint64_t)rec_end <= S.infl.cap) {
    if (B->n_records + n > BSORT_MAX_RECORDS) { set_error("more than 2^32 - 2 = %llu records: beyond one device sort", (unsigned long long)BSORT_MAX_RECORDS); return STRL_ERR_LIMIT; }
    const uint64_t need = B->n_records + n, bytes = rec_end - I.start0;
    if (need > B->rec_cap) {
      const uint64_t cap = std::max<uint64_t>(need + need / 2, 1u << 16);
      if ((rc = B->key.grow((size_t)cap * 8, (size_t)B->n_records * 8, st)) || (!B->windowed && (rc = B->src.grow((size_t)cap * 8, (size_t)B->n_records * 8, st))) ||
          (rc = B->len.grow((size_t)cap * 4, (size_t)B->n_records * 4, st)))
        return rc;
      B->rec_cap = cap;
    }
    uint64_t src0 = 0;
    uint8_t *dst = nullptr;
    if (!B->windowed && (rc = bsort_place(B, bytes, n, &src0, &dst))) return rc;
    BsortKeys P{S.infl.as<uint8_t>(), S.recoff.as<uint32_t>(), n, I.start0, rec_end, B->n_ref, B->n_records, B->rec_cap, src0,
                B->key.as<uint64_t>(), B->windowed ? nullptr : B->src.as<uint64_t>(), B->len.as<uint32_t>(), B->state.as<BsortState>()};
    hipLaunchKernelGGL(bsort_keys_kernel, dim3((n + 255u) / 256u), dim3(256), 0, st, P);
    STRL_HIP(hipGetLastError());
    if (!B->windowed) STRL_HIP(hipMemcpyAsync(dst, S.infl.as<uint8_t>() + I.start0, bytes, hipMemcpyDeviceToDevice, st));      // (windowed: 12 bytes a record stay, no more)
    B->n_records += n;
  }
  STRL_HIP(hipEventRecord(S.ev_b, st));        // the slot's inflated bytes and record table may be overwritten behind this
  S.b_pending = true;
  return STRL_OK;
}

// keys and arena copy of the chunk of SAM text in slot si: its records were encoded behind the push before
static int bsort_sam_chunk(strl_ctx *c, strl_bsort *B, int si) {
  hipStream_t st = c->stream;
  SamInfo I;
  int rc;
  if ((rc = sam_parser_collect(B->sam, si, st, &I))) return rc;
  SamSlot &S = B->sam->slot[si];
  const uint32_t n = I.n_lines;
  const uint64_t bytes = I.total;
  if (!n || !bytes) return STRL_OK;
  if (B->n_records + n > BSORT_MAX_RECORDS) { set_error("more than 2^32 - 2 = %llu records: beyond one device sort", (unsigned long long)BSORT_MAX_RECORDS); return STRL_ERR_LIMIT; }
  const uint64_t need = B->n_records + n;
  if (need > B->rec_cap) {
    const uint64_t cap = std::max<uint64_t>(need + need / 2, 1u << 16);
    if ((rc = B->key.grow((size_t)cap * 8, (size_t)B->n_records * 8, st)) || (rc = B->src.grow((size_t)cap * 8, (size_t)B->n_records * 8, st)) ||
        (rc = B->len.grow((size_t)cap * 4, (size_t)B->n_records * 4, st)))
      return rc;
    B->rec_cap = cap;
  }
  uint64_t src0 = 0;
  uint8_t *dst = nullptr;
  if ((rc = bsort_place(B, bytes, n, &src0, &dst))) return rc;
  BsortKeys P{S.rec.as<uint8_t>(), S.recoff.as<uint32_t>(), n, 0u, (uint32_t)bytes, B->n_ref, B->n_records, B->rec_cap, src0, B->key.as<uint64_t>(), B->src.as<uint64_t>(),
              B->len.as<uint32_t>(), B->state.as<BsortState>()};
  hipLaunchKernelGGL(bsort_keys_kernel, dim3((n + 255u) / 256u), dim3(256), 0, st, P);
  STRL_HIP(hipGetLastError());
  STRL_HIP(hipMemcpyAsync(dst, S.rec.p, bytes, hipMemcpyDeviceToDevice, st));
  B->n_records += n;
  return STRL_OK;
}

static int bsort_refuse(const strl_bsort *B, const BsortState &S) {
  if (S.err_ord[BSORT_E_TID] != ~0ull && S.err_ord[BSORT_E_TID] <= S.err_ord[BSORT_E_RECORD]) {
    set_error("malformed BAM record %llu: its refID is not one of the header's %d references", (unsigned long long)S.err_ord[BSORT_E_TID], B->n_ref);
    return STRL_ERR_FORMAT;
  }
  if (S.err_ord[BSORT_E_RECORD] != ~0ull) { set_error("malformed BAM record %llu: it does not lie inside its chunk's bytes", (unsigned long long)S.err_ord[BSORT_E_RECORD]); return STRL_ERR_FORMAT; }
  return STRL_OK;
}

// off[0 .. n] on the stream: the tiled sums of len[perm[j]] based at `base`
static int bsort_layout(hipStream_t st, const uint32_t *perm, const uint32_t *len, uint32_t n, uint64_t n_len, uint64_t base, uint64_t *tile, uint64_t *off, BsortState *S) {
  const uint32_t n_tiles = (n + BSORT_TILE - 1u) / BSORT_TILE;
  if (n_tiles) hipLaunchKernelGGL(bsort_tile_kernel<false>, dim3(n_tiles), dim3(256), 0, st, perm, len, n, n_len, base, tile, off, S);
  hipLaunchKernelGGL(bsort_scan_kernel, dim3(1), dim3(1024), 0, st, tile, n_tiles, base, off, n, S);
  if (n_tiles) hipLaunchKernelGGL(bsort_tile_kernel<true>, dim3(n_tiles), dim3(256), 0, st, perm, len, n, n_len, base, tile, off, S);
  STRL_HIP(hipGetLastError());
  return STRL_OK;
}

static uint32_t bsort_gather_lanes() {
  // 16 measured fastest on 150-base records with qualities and tags (~300 bytes: 19 words of 16 bytes), 1.18 TB/s of stream against
  // 0.94 with 32 lanes and 0.60 with a wave per record (profiles/sort/README.md); STRL_SORT_GATHER_LANES = 16 / 32 / 64 to measure again
  const char *e = getenv("STRL_SORT_GATHER_LANES");
  const int v = e ? atoi(e) : 16;
  return v == 32 || v == 64 ? (uint32_t)v : 16u;
}

// the piece [lo, hi) of the stream into B->piece, on the stream; nothing is waited for
static int bsort_gather(strl_ctx *c, strl_bsort *B, uint64_t lo, uint64_t hi) {
  int rc;
  if ((rc = B->piece.reserve((size_t)(hi - lo) + 64))) return rc;
  hipStream_t st = c->stream;
  const uint64_t n = B->n_records;
  BsortState *S = B->state.as<BsortState>();
  (void)hipEventRecord(B->e0, st);
  hipLaunchKernelGGL(bsort_range_kernel, dim3(1), dim3(64), 0, st, B->off.as<uint64_t>(), n, lo, hi, S);
  BsortGather P{B->off.as<uint64_t>(), B->src.as<uint64_t>(), B->perm, n, B->d_slab.as<uint8_t *>(), B->d_slab.as<uint64_t>() + B->slabs.size(), (uint32_t)B->slabs.size(),
                B->d_header.as<uint8_t>(), B->header_bytes, lo, hi, B->piece.as<uint8_t>(), S};
  const unsigned grid = (unsigned)std::min<uint64_t>(4096, std::max<uint64_t>(1, (hi - lo) / 4096));
  const uint32_t G = bsort_gather_lanes();
  if (G == 32) hipLaunchKernelGGL(bsort_gather_kernel<32>, dim3(grid), dim3(256), 0, st, P);
  else if (G == 64) hipLaunchKernelGGL(bsort_gather_kernel<64>, dim3(grid), dim3(256), 0, st, P);
  else hipLaunchKernelGGL(bsort_gather_kernel<16>, dim3(grid), dim3(256), 0, st, P);
  STRL_HIP(hipGetLastError());
  (void)hipEventRecord(B->e1, st);
  return STRL_OK;
}
static void bsort_gather_time(strl_bsort *B) {
  float ms = 0.f;
  if (hipEventElapsedTime(&ms, B->e0, B->e1) == hipSuccess) B->info.gather_ms += ms; else (void)hipGetLastError();
}

// ---- `sort --windowed` ---------------------------------------------------------------------------------------------------------------
// The finish of a windowed sort: the same radix sort and layout, then dest[perm[j]] = off[j]; everything but dest (8 B) and len
// (4 B) goes.  The buffers come and go in steps -- the key buffers and the scratch leave before off[] and dest[] arrive -- so the
// peak is the sort's own 28 B a record (two keys, two values, len) and its scratch.
static int bsort_finish_windowed(strl_ctx *c, strl_bsort *B, const uint8_t *header, uint64_t header_bytes) {
  hipStream_t st = c->stream;
  const uint32_t n = (uint32_t)B->n_records;
  const int bits = bsort_key_bits(B->n_ref);
  const size_t sb = radix_sort_scratch_bytes(std::max(n, 1u), bits);
  const uint32_t n_tiles = (n + BSORT_TILE - 1u) / BSORT_TILE;
  int rc;
  if ((rc = B->key.reserve(64)) || (rc = B->len.reserve(64)) || (rc = B->key_alt.reserve((size_t)n * 8 + 64)) || (rc = B->val.reserve((size_t)n * 4 + 64)) ||
      (rc = B->val_alt.reserve((size_t)n * 4 + 64)) || (rc = B->scratch.reserve(sb + 64)))
    return rc;
  BsortState *S = B->state.as<BsortState>();
  STRL_HIP(hipMemcpyAsync(&S->n, &n, 4, hipMemcpyHostToDevice, st));
  uint64_t *ok = B->key.as<uint64_t>();
  uint32_t *ov = B->val.as<uint32_t>();
  STRL_HIP(hipEventRecord(B->e0, st));
  if (n) {
    hipLaunchKernelGGL(bsort_iota_kernel, dim3((n + 255u) / 256u), dim3(256), 0, st, B->val.as<uint32_t>(), n);
    STRL_HIP(hipGetLastError());
    const int se = radix_sort_pairs(st, &S->n, n, B->key.as<uint64_t>(), B->val.as<uint32_t>(), B->key_alt.as<uint64_t>(), B->val_alt.as<uint32_t>(), B->scratch.p, sb, 0, bits, &ok, &ov);
    if (se) { set_error("radix_sort_pairs failed: %s", hipGetErrorString((hipError_t)se)); return STRL_ERR_HIP; }
  }
  B->perm = ov;
  STRL_HIP(hipEventRecord(B->e1, st));
  STRL_HIP(hipStreamSynchronize(st));
  float a = 0.f;
  (void)hipEventElapsedTime(&a, B->e0, B->e1);
  B->info.sort_ms = a;
  B->key.release(); B->key_alt.release(); B->scratch.release();
  if (ov == B->val.as<uint32_t>()) B->val_alt.release(); else B->val.release();
  if ((rc = B->off.reserve(((size_t)n + 1) * 8 + 64)) || (rc = B->tile.reserve((size_t)n_tiles * 8 + 64)) || (rc = B->dest.reserve((size_t)n * 8 + 64))) return rc;
  STRL_HIP(hipEventRecord(B->e1, st));
  if ((rc = bsort_layout(st, B->perm, B->len.as<uint32_t>(), n, B->n_records, header_bytes, B->tile.as<uint64_t>(), B->off.as<uint64_t>(), S))) return rc;
  if (n) hipLaunchKernelGGL(bsort_dest_kernel, dim3((n + 255u) / 256u), dim3(256), 0, st, B->perm, B->off.as<uint64_t>(), n, B->dest.as<uint64_t>());
  STRL_HIP(hipGetLastError());
  STRL_HIP(hipEventRecord(B->e2, st));
  STRL_HIP(hipMemcpyAsync(B->h_state, B->state.p, sizeof(BsortState), hipMemcpyDeviceToHost, st));
  STRL_HIP(hipStreamSynchronize(st));
  float b = 0.f;
  (void)hipEventElapsedTime(&b, B->e1, B->e2);
  B->perm = nullptr;
  B->val.release(); B->val_alt.release(); B->off.release(); B->tile.release();
  B->header.assign(header, header + header_bytes);
  B->header_bytes = header_bytes;
  B->stream_bytes = header_bytes + B->h_state->total;
  strl_bamsort_info &I = B->info;
  I.n_records = B->n_records; I.n_no_ref = B->h_state->n_no_ref; I.stream_bytes = B->stream_bytes;
  I.already_sorted = B->h_state->not_identity ? 0u : 1u;
  I.n_slabs = 0; I.arena_bytes = 0;
  I.layout_ms = b; I.gather_ms = 0;
  B->finished = true;
  return STRL_OK;
}

// the scatter of the chunk in slot si into the window (its record scan was enqueued by the push before)
static int bsort_window_chunk(strl_ctx *c, strl_front *F, strl_bsort *B, int si) {
  FrontSlot &S = F->slot[si];
  STRL_HIP(hipEventSynchronize(S.ev_a));
  const FrontInfo I = S.h_info[0];
  if (I.err & FRONT_ERR_INFLATE) { set_error("invalid BGZF block (DEFLATE data or ISIZE)"); return STRL_ERR_FORMAT; }
  if (I.err & FRONT_ERR_CRC) { set_error("CRC32 checksum mismatch in a BGZF block"); return STRL_ERR_CRC; }
  if (I.err & FRONT_ERR_RECORD) { set_error("malformed BAM record"); return STRL_ERR_FORMAT; }
  if (I.err & FRONT_ERR_CARRY) { set_error("BAM record of more than %u bytes", FRONT_CARRY_MAX); return STRL_ERR_FORMAT; }
  const uint32_t n = I.n_records, rec_end = std::min(I.carry_off, I.end);
  hipStream_t st = c->stream;
  if (n && rec_end > I.start0 && (uint64_t)rec_end <= S.infl.cap) {
    BsortScatter P{S.infl.as<uint8_t>(), S.recoff.as<uint32_t>(), n, I.start0, rec_end, (uint64_t)S.infl.cap, B->w_ord, B->n_records, B->dest.as<uint64_t>(), B->len.as<uint32_t>(),
                   B->win_lo, B->win_hi, B->window.as<uint8_t>(), B->wstate.as<BsortWinState>()};
    const uint32_t G = bsort_gather_lanes();
    const unsigned grid = (unsigned)std::min<uint64_t>(4096, std::max<uint64_t>(1, ((uint64_t)n * G + 255u) / 256u));
    if (G == 32) hipLaunchKernelGGL(bsort_scatter_kernel<32>, dim3(grid), dim3(256), 0, st, P);
    else if (G == 64) hipLaunchKernelGGL(bsort_scatter_kernel<64>, dim3(grid), dim3(256), 0, st, P);
    else hipLaunchKernelGGL(bsort_scatter_kernel<16>, dim3(grid), dim3(256), 0, st, P);
    STRL_HIP(hipGetLastError());
    B->w_ord += n;
  }
  STRL_HIP(hipEventRecord(S.ev_b, st));        // the slot's inflated bytes and record table may be overwritten behind this
  S.b_pending = true;
  return STRL_OK;
}

}  // namespace strl

using namespace strl;

// ---- the rule through the library, without a device (the Python mirror, tests) --------------------------------------------------
extern "C" int strl_bamsort_key(const uint8_t *rec20, int32_t n_ref, uint64_t *key) {
  if (!rec20 || !key || n_ref < 0) { set_error("strl_bamsort_key: bad argument"); return STRL_ERR_ARG; }
  if (!bsort_key(rec20, n_ref, key)) { set_error("the refID is not one of the header's %d references", n_ref); return STRL_ERR_FORMAT; }
  return STRL_OK;
}
extern "C" int strl_bamsort_key_bits(int32_t n_ref) { return n_ref < 0 ? 0 : bsort_key_bits(n_ref); }

extern "C" int strl_bamsort_header(const uint8_t *in, uint64_t in_bytes, uint8_t *out, uint64_t cap, uint64_t *out_bytes) {
  if (!in || !out_bytes) { set_error("strl_bamsort_header: null argument"); return STRL_ERR_ARG; }
  std::vector<uint8_t> h;
  std::string err;
  if (!bsort_header(in, (size_t)in_bytes, h, nullptr, nullptr, err)) { set_error("%s", err.c_str()); return STRL_ERR_FORMAT; }
  *out_bytes = h.size();
  if (cap < h.size() || !out) { set_error("strl_bamsort_header: %zu bytes, room for %llu", h.size(), (unsigned long long)cap); return STRL_ERR_CAPACITY; }
  memcpy(out, h.data(), h.size());
  return STRL_OK;
}

extern "C" int strl_sam_encode(const uint8_t *line, uint64_t len, const uint8_t *names, const uint32_t *name_off, int32_t n_ref, uint8_t *out, uint64_t cap, uint64_t *out_bytes) {
  if ((len && !line) || !out_bytes || n_ref < 0 || (n_ref && (!names || !name_off))) { set_error("strl_sam_encode: bad argument"); return STRL_ERR_ARG; }
  static const uint32_t zero = 0;
  if (!line) line = reinterpret_cast<const uint8_t *>("");
  SamRefTable T;
  int32_t dup = 0;
  if (!T.build(names, n_ref ? name_off : &zero, n_ref, &dup)) { set_error("strl_sam_encode: reference name %d occurs twice", dup); return STRL_ERR_FORMAT; }
  while (len && line[len - 1] == '\n') --len;
  if (len > (uint64_t)SAM_LINE_MAX + 1u) len = (uint64_t)SAM_LINE_MAX + 2u;      // (refused as too long, whatever it holds)
  std::vector<uint8_t> rec;
  std::string why;
  if (sam_encode_line(line, (uint32_t)len, T.view(), rec, why)) { set_error("%s", why.c_str()); return STRL_ERR_FORMAT; }
  *out_bytes = rec.size();
  if (cap < rec.size() || !out) { set_error("strl_sam_encode: %zu bytes, room for %llu", rec.size(), (unsigned long long)cap); return STRL_ERR_CAPACITY; }
  memcpy(out, rec.data(), rec.size());
  return STRL_OK;
}

extern "C" int strl_sam_header(const uint8_t *text, uint64_t len, uint8_t *out, uint64_t cap, uint64_t *out_bytes, int32_t *n_ref) {
  if ((len && !text) || !out_bytes) { set_error("strl_sam_header: null argument"); return STRL_ERR_ARG; }
  SamHeader H;
  std::string err;
  if (!sam_header(text, (size_t)len, H, err)) { set_error("%s", err.c_str()); return STRL_ERR_FORMAT; }
  *out_bytes = H.bam.size();
  if (n_ref) *n_ref = (int32_t)H.l_ref.size();
  if (cap < H.bam.size() || !out) { set_error("strl_sam_header: %zu bytes, room for %llu", H.bam.size(), (unsigned long long)cap); return STRL_ERR_CAPACITY; }
  memcpy(out, H.bam.data(), H.bam.size());
  return STRL_OK;
}

// ---- the device sort --------------------------------------------------------------------------------------------------------------
static int bsort_begin(strl_ctx *c, int32_t n_ref, uint64_t first_record_offset, uint64_t arena_limit_bytes, bool windowed, bool sam = false) {
  if (!c || n_ref < 0) { set_error("%s: bad argument", sam ? "strl_bamsort_sam_begin" : windowed ? "strl_bamsort_begin_windowed" : "strl_bamsort_begin"); return STRL_ERR_ARG; }
  int rc;
  if (sam) STRL_HIP(hipSetDevice(c->device));
  else if ((rc = front_begin_scan(c, n_ref, first_record_offset))) return rc;
  // one consumer of the record scan on a context: a builder or a sweep of an earlier pass ends here, as theirs end each other's
  if (c->bai) { bai_destroy(c->bai); c->bai = nullptr; }
  if (c->sweep) { sweep_destroy(c->sweep); c->sweep = nullptr; }
  if (c->bsort) { bsort_destroy(c->bsort); c->bsort = nullptr; }
  strl_bsort *B = new strl_bsort();
  c->bsort = B;
  B->n_ref = n_ref;
  B->front = sam ? nullptr : c->front;          // (SAM text does not go through the front end)
  B->slab_want = bsort_slab_want();
  B->arena_limit = arena_limit_bytes;
  STRL_HIP(hipHostMalloc(reinterpret_cast<void **>(&B->h_state), sizeof(BsortState), hipHostMallocDefault));
  STRL_HIP(hipEventCreate(&B->e0));
  STRL_HIP(hipEventCreate(&B->e1));
  STRL_HIP(hipEventCreate(&B->e2));
  if ((rc = B->state.reserve(sizeof(BsortState)))) return rc;
  BsortState &H = *B->h_state;
  memset(&H, 0, sizeof H);
  H.err_ord[0] = H.err_ord[1] = ~0ull;
  STRL_HIP(hipMemcpyAsync(B->state.p, &H, sizeof H, hipMemcpyHostToDevice, c->stream));
  STRL_HIP(hipStreamSynchronize(c->stream));
  if (windowed) {
    B->windowed = true;
    B->first_off = first_record_offset;
    STRL_HIP(hipHostMalloc(reinterpret_cast<void **>(&B->h_wstate), sizeof(BsortWinState), hipHostMallocDefault));
    if ((rc = B->wstate.reserve(sizeof(BsortWinState)))) return rc;
  }
  return STRL_OK;
}

extern "C" int strl_bamsort_begin(strl_ctx *c, int32_t n_ref, uint64_t first_record_offset, uint64_t arena_limit_bytes) {
  return bsort_begin(c, n_ref, first_record_offset, arena_limit_bytes, false);
}
extern "C" int strl_bamsort_begin_windowed(strl_ctx *c, int32_t n_ref, uint64_t first_record_offset) { return bsort_begin(c, n_ref, first_record_offset, 0, true); }

extern "C" int strl_bamsort_sam_begin(strl_ctx *c, const uint8_t *names, const uint32_t *name_off, int32_t n_ref, uint64_t arena_limit_bytes) {
  if (n_ref > 0 && (!names || !name_off)) { set_error("strl_bamsort_sam_begin: bad argument"); return STRL_ERR_ARG; }
  int rc;
  if ((rc = bsort_begin(c, n_ref, 0, arena_limit_bytes, false, true))) return rc;
  static const uint32_t zero = 0;
  return bsort_fail(c->bsort, sam_parser_create(&c->bsort->sam, names, n_ref > 0 ? name_off : &zero, n_ref, c->stream));
}

extern "C" int strl_bamsort_sam_reserve(strl_ctx *c, uint64_t max_text_bytes) {
  if (!c || !c->bsort || !c->bsort->sam) { set_error("strl_bamsort_sam_reserve: bad argument / no strl_bamsort_sam_begin"); return STRL_ERR_ARG; }
  strl_bsort *B = c->bsort;
  if (B->done < B->chunks) { set_error("strl_bamsort_sam_reserve: a chunk is in flight"); return STRL_ERR_ARG; }
  STRL_HIP(hipSetDevice(c->device));
  return sam_parser_reserve(B->sam, max_text_bytes);
}

extern "C" int strl_bamsort_push_sam(strl_ctx *c, const uint8_t *text, uint64_t bytes) {
  if (!c || !c->bsort || !c->bsort->sam || c->bai || c->sweep || c->x_open || c->bsort->finished || (bytes && !text)) {
    set_error("strl_bamsort_push_sam: bad argument / no strl_bamsort_sam_begin");
    return STRL_ERR_ARG;
  }
  if (!bytes) return STRL_OK;
  STRL_HIP(hipSetDevice(c->device));
  strl_bsort *B = c->bsort;
  if (B->fail_rc) { set_error("%s", B->fail.c_str()); return B->fail_rc; }
  if (text[bytes - 1] != '\n' || bytes > B->sam->max_text) {      // (the caller's mistake, not the file's: the sort goes on)
    set_error("strl_bamsort_push_sam: a chunk is whole lines, its last byte a newline, and at most strl_bamsort_sam_reserve's %llu bytes (got %llu)",
              (unsigned long long)B->sam->max_text, (unsigned long long)bytes);
    return STRL_ERR_ARG;
  }
  int rc;
  // keys and arena copy of the chunk before (its kernels ran beside the caller's read of this one), then this chunk's copy and kernels
  for (; B->done < B->chunks; ++B->done)
    if ((rc = bsort_sam_chunk(c, B, (int)(B->done & 1)))) return bsort_fail(B, rc);
  if ((rc = sam_parser_enqueue(B->sam, (int)(B->chunks & 1), text, bytes, B->sam->fig.lines, c->stream))) return bsort_fail(B, rc);
  ++B->chunks;
  return STRL_OK;
}

extern "C" int strl_bamsort_sam_info(strl_ctx *c, strl_bamsort_sam_figures *out) {
  if (!c || !c->bsort || !c->bsort->sam || !out) { set_error("strl_bamsort_sam_info: bad argument / no strl_bamsort_sam_begin"); return STRL_ERR_ARG; }
  *out = c->bsort->sam->fig;
  return STRL_OK;
}

extern "C" int strl_bamsort_reserve(strl_ctx *c, uint32_t max_blocks, uint64_t max_comp_bytes) {
  if (!c || !c->bsort || !c->front || c->bsort->sam || !max_blocks) { set_error("strl_bamsort_reserve: bad argument / no strl_bamsort_begin"); return STRL_ERR_ARG; }
  STRL_HIP(hipSetDevice(c->device));
  c->bsort->res_blocks = max_blocks; c->bsort->res_comp = max_comp_bytes;
  return front_reserve(c, c->front, max_blocks, max_comp_bytes);
}

extern "C" int strl_bamsort_push(strl_ctx *c, const uint8_t *comp, uint64_t comp_bytes, const uint64_t *coff, const uint32_t *clen, const uint32_t *isize,
                                 const uint32_t *crc32, uint32_t n_blocks) {
  if (!c || !c->bsort || c->bsort->sam || !c->front || c->front != c->bsort->front || c->bai || c->sweep || c->x_open || c->bsort->finished || (n_blocks && (!comp || !coff || !clen || !isize))) {
    set_error("strl_bamsort_push: bad argument / no strl_bamsort_begin / another pass has taken the context's front end");
    return STRL_ERR_ARG;
  }
  if (!n_blocks) return STRL_OK;
  STRL_HIP(hipSetDevice(c->device));
  strl_front *F = c->front;
  strl_bsort *B = c->bsort;
  if (B->fail_rc) { set_error("%s", B->fail.c_str()); return B->fail_rc; }
  const int si = (int)(B->chunks & 1);
  FrontSlot &S = F->slot[si];
  int rc;
  if (S.b_pending) { STRL_HIP(hipEventSynchronize(S.ev_b)); S.b_pending = false; }     // the chunk two back has left the slot
  const FrontChunkDesc d{comp, comp_bytes, coff, clen, isize, crc32, n_blocks};
  if ((rc = front_stage_a(c, F, si, d, B->chunks == 0))) return bsort_fail(B, rc);
  ++B->chunks;
  // ... and beside this chunk's inflate, the keys and the copy of the previous one
  while (B->done + 1 < B->chunks) {
    if ((rc = bsort_chunk(c, F, B, (int)(B->done & 1)))) return bsort_fail(B, rc);
    ++B->done;
  }
  return STRL_OK;
}

extern "C" int strl_bamsort_finish(strl_ctx *c, const uint8_t *header, uint64_t header_bytes, strl_bamsort_info *info) {
  const bool sam = c && c->bsort && c->bsort->sam;
  if (!c || !c->bsort || (!sam && (!c->front || c->front != c->bsort->front)) || c->bai || c->sweep || c->x_open || (header_bytes && !header)) { set_error("strl_bamsort_finish: bad argument / no strl_bamsort_begin"); return STRL_ERR_ARG; }
  STRL_HIP(hipSetDevice(c->device));
  strl_front *F = c->front;
  strl_bsort *B = c->bsort;
  if (B->fail_rc) { set_error("%s", B->fail.c_str()); return B->fail_rc; }
  hipStream_t st = c->stream;
  int rc;
  if (!B->finished) {
    for (; B->done < B->chunks; ++B->done)
      if ((rc = sam ? bsort_sam_chunk(c, B, (int)(B->done & 1)) : bsort_chunk(c, F, B, (int)(B->done & 1)))) return bsort_fail(B, rc);
    STRL_HIP(hipMemcpyAsync(B->h_state, B->state.p, sizeof(BsortState), hipMemcpyDeviceToHost, st));
    STRL_HIP(hipStreamSynchronize(st));
    if (!sam && F->last_slot >= 0 && F->slot[F->last_slot].h_info[0].carry_len) { set_error("the BAM ends inside a record (truncated file)"); return bsort_fail(B, STRL_ERR_FORMAT); }
    if ((rc = bsort_refuse(B, *B->h_state))) return bsort_fail(B, rc);
    if (B->windowed) {
      if ((rc = bsort_finish_windowed(c, B, header, header_bytes))) return bsort_fail(B, rc);
      if (info) *info = B->info;
      return STRL_OK;
    }
    const uint32_t n = (uint32_t)B->n_records;
    const int bits = bsort_key_bits(B->n_ref);
    const size_t sb = radix_sort_scratch_bytes(std::max(n, 1u), bits), ns = B->slabs.size();
    const uint32_t n_tiles = (n + BSORT_TILE - 1u) / BSORT_TILE;
    if ((rc = B->key.reserve(64)) || (rc = B->len.reserve(64)) || (rc = B->src.reserve(64)) ||      // (no record: the kernels still get pointers)
        (rc = B->key_alt.reserve((size_t)n * 8 + 64)) || (rc = B->val.reserve((size_t)n * 4 + 64)) || (rc = B->val_alt.reserve((size_t)n * 4 + 64)) ||
        (rc = B->scratch.reserve(sb + 64)) || (rc = B->off.reserve(((size_t)n + 1) * 8 + 64)) || (rc = B->tile.reserve((size_t)n_tiles * 8 + 64)) ||
        (rc = B->d_header.reserve((size_t)header_bytes + 64)) || (rc = B->d_slab.reserve(ns * 16 + 64)))
      return bsort_fail(B, rc);
    std::vector<uint64_t> tab(2 * ns + 1);
    for (size_t k = 0; k < ns; ++k) { tab[k] = (uint64_t)reinterpret_cast<uintptr_t>(B->slabs[k].buf.p); tab[ns + k] = B->slabs[k].used; }
    if (ns) STRL_HIP(hipMemcpyAsync(B->d_slab.p, tab.data(), ns * 16, hipMemcpyHostToDevice, st));
    if (header_bytes) STRL_HIP(hipMemcpyAsync(B->d_header.p, header, header_bytes, hipMemcpyHostToDevice, st));
    BsortState *S = B->state.as<BsortState>();
    STRL_HIP(hipMemcpyAsync(&S->n, &n, 4, hipMemcpyHostToDevice, st));
    uint64_t *ok = B->key.as<uint64_t>();
    uint32_t *ov = B->val.as<uint32_t>();
    STRL_HIP(hipEventRecord(B->e0, st));
    if (n) {
      hipLaunchKernelGGL(bsort_iota_kernel, dim3((n + 255u) / 256u), dim3(256), 0, st, B->val.as<uint32_t>(), n);
      STRL_HIP(hipGetLastError());
      const int se = radix_sort_pairs(st, &S->n, n, B->key.as<uint64_t>(), B->val.as<uint32_t>(), B->key_alt.as<uint64_t>(), B->val_alt.as<uint32_t>(), B->scratch.p, sb, 0, bits, &ok, &ov);
      if (se) { set_error("radix_sort_pairs failed: %s", hipGetErrorString((hipError_t)se)); return bsort_fail(B, STRL_ERR_HIP); }
    }
    B->perm = ov;
    STRL_HIP(hipEventRecord(B->e1, st));
    if ((rc = bsort_layout(st, B->perm, B->len.as<uint32_t>(), n, B->n_records, header_bytes, B->tile.as<uint64_t>(), B->off.as<uint64_t>(), S))) return bsort_fail(B, rc);
    STRL_HIP(hipEventRecord(B->e2, st));
    STRL_HIP(hipMemcpyAsync(B->h_state, B->state.p, sizeof(BsortState), hipMemcpyDeviceToHost, st));
    STRL_HIP(hipStreamSynchronize(st));
    float a = 0.f, b = 0.f;
    (void)hipEventElapsedTime(&a, B->e0, B->e1);
    (void)hipEventElapsedTime(&b, B->e1, B->e2);
    // the sort's ping-pong key buffers are done with: their memory goes to the pieces and the compressor
    B->key.release(); B->key_alt.release(); B->scratch.release();
    if (ov == B->val.as<uint32_t>()) B->val_alt.release(); else B->val.release();
    B->header_bytes = header_bytes;
    B->stream_bytes = header_bytes + B->h_state->total;
    strl_bamsort_info &I = B->info;
    I.n_records = B->n_records; I.n_no_ref = B->h_state->n_no_ref; I.stream_bytes = B->stream_bytes;
    I.already_sorted = B->h_state->not_identity ? 0u : 1u;
    I.n_slabs = (uint32_t)ns; I.arena_bytes = B->arena_bytes;
    I.sort_ms = a; I.layout_ms = b; I.gather_ms = 0;
    B->finished = true;
  }
  if (info) *info = B->info;
  return STRL_OK;
}

extern "C" int strl_bamsort_info_now(strl_ctx *c, strl_bamsort_info *info) {
  if (!c || !c->bsort || !c->bsort->finished || !info) { set_error("strl_bamsort_info_now without strl_bamsort_finish"); return STRL_ERR_ARG; }
  *info = c->bsort->info;
  return STRL_OK;
}

static int bsort_fetch_check(strl_ctx *c, const char *who, uint64_t off, uint64_t bytes) {
  if (!c || !c->bsort || !c->bsort->finished) { set_error("%s without strl_bamsort_finish", who); return STRL_ERR_ARG; }
  if (off > c->bsort->stream_bytes || bytes > c->bsort->stream_bytes - off || bytes > 0xffffffffull) {
    set_error("%s: [%llu, %llu + %llu) is not inside the stream's %llu bytes (a piece holds less than 4 GiB)", who, (unsigned long long)off, (unsigned long long)off,
              (unsigned long long)bytes, (unsigned long long)c->bsort->stream_bytes);
    return STRL_ERR_ARG;
  }
  const strl_bsort *B = c->bsort;
  if (B->windowed && bytes && (!B->win_done || off < B->win_lo || off + bytes > B->win_hi)) {
    if (!B->win_done) set_error("%s: a windowed sort has no finished window (strl_bamsort_window_begin / _push / _end)", who);
    else set_error("%s: [%llu, %llu + %llu) is not inside the current window [%llu, %llu) of a windowed sort", who, (unsigned long long)off, (unsigned long long)off,
                   (unsigned long long)bytes, (unsigned long long)B->win_lo, (unsigned long long)B->win_hi);
    return STRL_ERR_ARG;
  }
  return STRL_OK;
}

extern "C" int strl_bamsort_fetch(strl_ctx *c, uint64_t off, uint64_t bytes, uint8_t *out) {
  int rc;
  if ((rc = bsort_fetch_check(c, "strl_bamsort_fetch", off, bytes))) return rc;
  if (!bytes) return STRL_OK;
  if (!out) { set_error("null argument"); return STRL_ERR_ARG; }
  STRL_HIP(hipSetDevice(c->device));
  strl_bsort *B = c->bsort;
  if (B->windowed) {                                          // the window is a finished piece of the stream: the bytes lie there
    STRL_HIP(hipMemcpyAsync(out, B->window.as<uint8_t>() + (off - B->win_lo), bytes, hipMemcpyDeviceToHost, c->stream));
    STRL_HIP(hipStreamSynchronize(c->stream));
    return STRL_OK;
  }
  B->fetched = true;
  if ((rc = bsort_gather(c, B, off, off + bytes))) return rc;
  STRL_HIP(hipMemcpyAsync(out, B->piece.p, bytes, hipMemcpyDeviceToHost, c->stream));
  STRL_HIP(hipStreamSynchronize(c->stream));
  bsort_gather_time(B);
  return STRL_OK;
}

extern "C" int strl_bamsort_fetch_bgzf(strl_ctx *c, uint64_t off, uint64_t bytes, uint8_t *out, uint64_t out_cap, uint64_t *out_bytes, uint32_t *n_stored) {
  int rc;
  if ((rc = bsort_fetch_check(c, "strl_bamsort_fetch_bgzf", off, bytes))) return rc;
  if (off % BSORT_BLK || !out_bytes) { set_error("strl_bamsort_fetch_bgzf: off must be a multiple of 0xFF00, out_bytes not null"); return STRL_ERR_ARG; }
  *out_bytes = 0;
  if (n_stored) *n_stored = 0;
  if (!bytes) return STRL_OK;
  STRL_HIP(hipSetDevice(c->device));
  strl_bsort *B = c->bsort;
  if (B->windowed) return bgzf_deflate_device(c, B->deflate_mode, B->window.as<uint8_t>() + (off - B->win_lo), bytes, BSORT_BLK, out, out_cap, out_bytes, nullptr, n_stored);
  B->fetched = true;
  if ((rc = bsort_gather(c, B, off, off + bytes))) return rc;
  rc = bgzf_deflate_device(c, B->deflate_mode, B->piece.as<uint8_t>(), bytes, BSORT_BLK, out, out_cap, out_bytes, nullptr, n_stored);      // (waits for the stream)
  if (!rc) bsort_gather_time(B);
  return rc;
}

extern "C" int strl_bamsort_deflate_mode(strl_ctx *c, int mode) {
  if (!c || !c->bsort) { set_error("strl_bamsort_deflate_mode without strl_bamsort_begin"); return STRL_ERR_ARG; }
  if (mode != STRL_DEFLATE_FAST && mode != STRL_DEFLATE_DENSE) { set_error("strl_bamsort_deflate_mode: mode %d is neither STRL_DEFLATE_FAST nor STRL_DEFLATE_DENSE", mode); return STRL_ERR_ARG; }
  c->bsort->deflate_mode = mode;
  return STRL_OK;
}

// ---- `sort --markdup`: flag 0x400 decided on the resident records, between the finish and the first fetch (markdup.hip) -----------------
extern "C" int strl_bamsort_markdup_mode(strl_ctx *c, int on) {
  if (!c || !c->bsort || c->bsort->chunks || c->bsort->finished) { set_error("strl_bamsort_markdup_mode: behind strl_bamsort_begin / _sam_begin and before the first push"); return STRL_ERR_ARG; }
  if (c->bsort->windowed && on) { set_error("strl_bamsort_markdup_mode: a windowed sort holds no records to mark"); return STRL_ERR_ARG; }
  if (c->bsort->fastq_on && on) { set_error("strl_bamsort_markdup_mode: not together with strl_bamsort_fastq_mode"); return STRL_ERR_ARG; }
  c->bsort->markdup_on = on != 0;
  return STRL_OK;
}

extern "C" int strl_bamsort_markdup(strl_ctx *c, strl_markdup_info *out) {
  if (!c || !c->bsort || !c->bsort->finished) { set_error("strl_bamsort_markdup without strl_bamsort_finish"); return STRL_ERR_ARG; }
  strl_bsort *B = c->bsort;
  if (B->windowed) { set_error("strl_bamsort_markdup: a windowed sort holds no records to mark"); return STRL_ERR_ARG; }
  if (B->fail_rc) { set_error("%s", B->fail.c_str()); return B->fail_rc; }
  if (B->fetched) { set_error("strl_bamsort_markdup: a piece of the stream has been fetched already"); return STRL_ERR_ARG; }
  if (B->markdup_done) { set_error("strl_bamsort_markdup: the step has run on this sort already"); return STRL_ERR_ARG; }
  STRL_HIP(hipSetDevice(c->device));
  const size_t ns = B->slabs.size();
  const BsortView V{B->off.as<uint64_t>(), B->src.as<uint64_t>(), B->perm, B->len.as<uint32_t>(), B->d_slab.as<uint8_t *>(), B->d_slab.as<uint64_t>() + ns, (uint32_t)ns, B->n_ref,
                    B->n_records, B->stream_bytes};
  B->markdup_done = true;
  // (a refusal fails the sort: the arena may hold flags of a step that did not end)
  return bsort_fail(B, markdup_run(c, V, out));
}

// ---- `strling fastq`: the resident records as FASTQ text, behind the finish (fastq.hip) ---------------------------------------------------
extern "C" int strl_bamsort_fastq_mode(strl_ctx *c, int on) {
  if (!c || !c->bsort || c->bsort->chunks || c->bsort->finished) { set_error("strl_bamsort_fastq_mode: behind strl_bamsort_begin / _sam_begin and before the first push"); return STRL_ERR_ARG; }
  if (c->bsort->windowed && on) { set_error("strl_bamsort_fastq_mode: a windowed sort holds no records to write"); return STRL_ERR_ARG; }
  if (c->bsort->markdup_on && on) { set_error("strl_bamsort_fastq_mode: not together with strl_bamsort_markdup_mode"); return STRL_ERR_ARG; }
  c->bsort->fastq_on = on != 0;
  return STRL_OK;
}

static BsortView bsort_view_of(strl_bsort *B) {
  const size_t ns = B->slabs.size();
  return BsortView{B->off.as<uint64_t>(), B->src.as<uint64_t>(), B->perm, B->len.as<uint32_t>(), B->d_slab.as<uint8_t *>(), B->d_slab.as<uint64_t>() + ns, (uint32_t)ns, B->n_ref,
                   B->n_records, B->stream_bytes};
}

extern "C" int strl_bamsort_fastq(strl_ctx *c, const strl_fastq_opts *opts, strl_fastq_info *out) {
  if (!c || !c->bsort || !c->bsort->finished || !opts) { set_error("strl_bamsort_fastq without strl_bamsort_finish"); return STRL_ERR_ARG; }
  strl_bsort *B = c->bsort;
  if (B->windowed) { set_error("strl_bamsort_fastq: a windowed sort holds no records to write"); return STRL_ERR_ARG; }
  if (B->fail_rc) { set_error("%s", B->fail.c_str()); return B->fail_rc; }
  if (!B->fastq_on) { set_error("strl_bamsort_fastq without strl_bamsort_fastq_mode before the first push"); return STRL_ERR_ARG; }
  if (B->fastq) { set_error("strl_bamsort_fastq: the step has run on this sort already"); return STRL_ERR_ARG; }
  STRL_HIP(hipSetDevice(c->device));
  // (a refusal fails the sort: its plan is no plan)
  return bsort_fail(B, fastq_plan(c, bsort_view_of(B), opts, &B->fastq, out));
}

static int bsort_fastq_check(strl_ctx *c, const char *who) {
  if (!c || !c->bsort || !c->bsort->finished || !c->bsort->fastq) { set_error("%s without strl_bamsort_fastq", who); return STRL_ERR_ARG; }
  if (c->bsort->fail_rc) { set_error("%s", c->bsort->fail.c_str()); return c->bsort->fail_rc; }
  return STRL_OK;
}

extern "C" int strl_bamsort_fastq_fetch(strl_ctx *c, int stream, uint64_t lo, uint64_t len, uint8_t *dst) {
  int rc;
  if ((rc = bsort_fastq_check(c, "strl_bamsort_fastq_fetch"))) return rc;
  STRL_HIP(hipSetDevice(c->device));
  return fastq_fetch(c, c->bsort->fastq, bsort_view_of(c->bsort), stream, lo, len, dst);
}

extern "C" int strl_bamsort_fastq_info_now(strl_ctx *c, strl_fastq_info *info) {
  int rc;
  if ((rc = bsort_fastq_check(c, "strl_bamsort_fastq_info_now"))) return rc;
  if (!info) { set_error("null argument"); return STRL_ERR_ARG; }
  *info = *fastq_info(c->bsort->fastq);
  return STRL_OK;
}

extern "C" int strl_bamsort_order(strl_ctx *c, uint32_t *perm, uint64_t cap) {
  if (!c || !c->bsort || !c->bsort->finished) { set_error("strl_bamsort_order without strl_bamsort_finish"); return STRL_ERR_ARG; }
  strl_bsort *B = c->bsort;
  if (B->windowed) { set_error("strl_bamsort_order: not supported by a windowed sort, which gives the order up for the records' places in the stream"); return STRL_ERR_ARG; }
  if (cap < B->n_records || (B->n_records && !perm)) { set_error("strl_bamsort_order: %llu records, room for %llu", (unsigned long long)B->n_records, (unsigned long long)cap); return STRL_ERR_CAPACITY; }
  STRL_HIP(hipSetDevice(c->device));
  if (B->n_records) STRL_HIP(hipMemcpy(perm, B->perm, (size_t)B->n_records * 4, hipMemcpyDeviceToHost));
  return STRL_OK;
}

// ---- `sort --windowed`: one window of the stream per pass over the input ---------------------------------------------------------------
extern "C" int strl_bamsort_window_plan(uint64_t stream_bytes, uint64_t limit_bytes, uint64_t piece_bytes, uint64_t *window_bytes, uint64_t *n_windows) {
  if (!piece_bytes || !window_bytes || !n_windows) { set_error("strl_bamsort_window_plan: bad argument"); return STRL_ERR_ARG; }
  const BsortWindowPlan p = bsort_window_plan(stream_bytes, limit_bytes, piece_bytes);
  *window_bytes = p.window_bytes; *n_windows = p.n_windows;
  return STRL_OK;
}

static int bsort_windowed_check(strl_ctx *c, const char *who) {
  if (!c || !c->bsort || !c->bsort->windowed || !c->bsort->finished) { set_error("%s without strl_bamsort_begin_windowed and strl_bamsort_finish", who); return STRL_ERR_ARG; }
  if (c->bsort->fail_rc) { set_error("%s", c->bsort->fail.c_str()); return c->bsort->fail_rc; }
  return STRL_OK;
}

extern "C" int strl_bamsort_window_limit(strl_ctx *c, uint64_t *bytes) {
  int rc;
  if ((rc = bsort_windowed_check(c, "strl_bamsort_window_limit"))) return rc;
  if (!bytes) { set_error("null argument"); return STRL_ERR_ARG; }
  STRL_HIP(hipSetDevice(c->device));
  size_t fr = 0, tot = 0;
  STRL_HIP(hipMemGetInfo(&fr, &tot));
  // the front end's slots are allocated by now (pass 0 ran through them, and a window's front end asks for the same again), so they
  // are outside `fr` already; a window buffer of an earlier window is not, and is reused
  const uint64_t have = (uint64_t)fr + c->bsort->window.cap, keep = (uint64_t)768 << 20;
  *bytes = have > keep ? have - keep : 0;
  return STRL_OK;
}

extern "C" int strl_bamsort_window_begin(strl_ctx *c, uint64_t lo, uint64_t hi) {
  int rc;
  if ((rc = bsort_windowed_check(c, "strl_bamsort_window_begin"))) return rc;
  strl_bsort *B = c->bsort;
  if (c->bai || c->sweep || c->x_open || lo >= hi || hi > B->stream_bytes) {
    set_error("strl_bamsort_window_begin: [%llu, %llu) is not a window of the stream's %llu bytes / another pass has taken the context", (unsigned long long)lo, (unsigned long long)hi,
              (unsigned long long)B->stream_bytes);
    return STRL_ERR_ARG;
  }
  STRL_HIP(hipSetDevice(c->device));
  B->win_open = B->win_done = false;
  // the front end again from the start of the file (this waits for everything the last pass left in flight)
  if ((rc = front_begin_scan(c, B->n_ref, B->first_off))) { B->front = c->front; return bsort_fail(B, rc); }
  B->front = c->front;
  if (B->res_blocks && (rc = front_reserve(c, c->front, B->res_blocks, B->res_comp))) return bsort_fail(B, rc);
  if ((rc = B->window.reserve((size_t)(hi - lo) + 64))) return bsort_fail(B, rc);      // (reserve never shrinks; hipMalloc aligns far beyond 16 bytes)
  hipStream_t st = c->stream;
  const uint64_t hb = bsort_window_header(B->header_bytes, lo, hi);
  if (hb) STRL_HIP(hipMemcpyAsync(B->window.p, B->header.data() + lo, hb, hipMemcpyHostToDevice, st));
  BsortWinState &H = *B->h_wstate;
  H.err_ord = ~0ull; H.placed = 0;
  STRL_HIP(hipMemcpyAsync(B->wstate.p, &H, sizeof H, hipMemcpyHostToDevice, st));
  STRL_HIP(hipStreamSynchronize(st));
  B->win_lo = lo; B->win_hi = hi;
  B->w_chunks = B->w_done = B->w_ord = 0;
  B->win_open = true;
  return STRL_OK;
}

extern "C" int strl_bamsort_window_push(strl_ctx *c, const uint8_t *comp, uint64_t comp_bytes, const uint64_t *coff, const uint32_t *clen, const uint32_t *isize,
                                        const uint32_t *crc32, uint32_t n_blocks) {
  int rc;
  if ((rc = bsort_windowed_check(c, "strl_bamsort_window_push"))) return rc;
  strl_bsort *B = c->bsort;
  if (!B->win_open || !c->front || c->front != B->front || c->bai || c->sweep || c->x_open || (n_blocks && (!comp || !coff || !clen || !isize))) {
    set_error("strl_bamsort_window_push: bad argument / no strl_bamsort_window_begin / another pass has taken the context's front end");
    return STRL_ERR_ARG;
  }
  if (!n_blocks) return STRL_OK;
  STRL_HIP(hipSetDevice(c->device));
  strl_front *F = c->front;
  const int si = (int)(B->w_chunks & 1);
  FrontSlot &S = F->slot[si];
  if (S.b_pending) { STRL_HIP(hipEventSynchronize(S.ev_b)); S.b_pending = false; }     // the chunk two back has left the slot
  const FrontChunkDesc d{comp, comp_bytes, coff, clen, isize, crc32, n_blocks};
  if ((rc = front_stage_a(c, F, si, d, B->w_chunks == 0))) return bsort_fail(B, rc);
  ++B->w_chunks;
  // ... and beside this chunk's inflate, the scatter of the previous one
  while (B->w_done + 1 < B->w_chunks) {
    if ((rc = bsort_window_chunk(c, F, B, (int)(B->w_done & 1)))) return bsort_fail(B, rc);
    ++B->w_done;
  }
  return STRL_OK;
}

extern "C" int strl_bamsort_window_end(strl_ctx *c) {
  int rc;
  if ((rc = bsort_windowed_check(c, "strl_bamsort_window_end"))) return rc;
  strl_bsort *B = c->bsort;
  if (!B->win_open || !c->front || c->front != B->front) { set_error("strl_bamsort_window_end without strl_bamsort_window_begin"); return STRL_ERR_ARG; }
  STRL_HIP(hipSetDevice(c->device));
  strl_front *F = c->front;
  hipStream_t st = c->stream;
  for (; B->w_done < B->w_chunks; ++B->w_done)
    if ((rc = bsort_window_chunk(c, F, B, (int)(B->w_done & 1)))) return bsort_fail(B, rc);
  STRL_HIP(hipMemcpyAsync(B->h_wstate, B->wstate.p, sizeof(BsortWinState), hipMemcpyDeviceToHost, st));
  STRL_HIP(hipStreamSynchronize(st));
  B->win_open = false;
  const BsortWinState &H = *B->h_wstate;
  // (these leave the sort usable: another window_begin over the right file goes on)
  if (H.err_ord != ~0ull && H.err_ord < B->n_records) { set_error("the input changed between passes: record %llu", (unsigned long long)H.err_ord); return STRL_ERR_FORMAT; }
  const bool cut = F->last_slot >= 0 && F->slot[F->last_slot].h_info[0].carry_len;
  if (B->w_ord != B->n_records || H.err_ord != ~0ull || cut) {
    set_error("the input changed between passes: %llu records%s, pass 0 read %llu", (unsigned long long)B->w_ord, cut ? " and a part of one" : "", (unsigned long long)B->n_records);
    return STRL_ERR_FORMAT;
  }
  if (!bsort_window_complete(H.placed, B->header_bytes, B->win_lo, B->win_hi)) {
    set_error("internal error: the window [%llu, %llu) holds %llu bytes of records and %llu of the header", (unsigned long long)B->win_lo, (unsigned long long)B->win_hi,
              (unsigned long long)H.placed, (unsigned long long)bsort_window_header(B->header_bytes, B->win_lo, B->win_hi));
    return STRL_ERR_ASSERT;
  }
  B->win_done = true;
  return STRL_OK;
}

extern "C" int strl_bamsort_end(strl_ctx *c) {
  if (!c) { set_error("null argument"); return STRL_ERR_ARG; }
  STRL_HIP(hipSetDevice(c->device));
  if (c->front && c->bsort && c->front == c->bsort->front) {
    for (hipStream_t q : c->front->st_i) if (q) (void)hipStreamSynchronize(q);
    if (c->front->st_a) (void)hipStreamSynchronize(c->front->st_a);
    if (c->front->st_c) (void)hipStreamSynchronize(c->front->st_c);
  }
  STRL_HIP(hipStreamSynchronize(c->stream));
  if (c->bsort) { bsort_destroy(c->bsort); c->bsort = nullptr; }
  return STRL_OK;
}

// test-only, undeclared: the layout, bsort_dest_kernel and the scatter's part arithmetic as a windowed sort runs them, over
// caller-given len[n] (by input ordinal), a caller-given permutation perm[n] (perm[rank] = ordinal), a 64-bit base and a window
// [lo, hi) -- destinations beyond 2^32 without 4 GB of data.  dest_out[n] by ordinal; parts[3 i ..] = (source skip, destination,
// bytes) of ordinal i's part inside the window (bytes 0: outside it).
extern "C" int strl_bamsort_window_probe(strl_ctx *c, const uint32_t *len, const uint32_t *perm, uint32_t n, uint64_t base, uint64_t lo, uint64_t hi, uint64_t *dest_out,
                                         uint64_t *parts) {
  if (!c || (n && (!len || !perm || !dest_out || !parts)) || lo > hi) { set_error("strl_bamsort_window_probe: bad argument"); return STRL_ERR_ARG; }
  for (uint32_t j = 0; j < n; ++j) if (perm[j] >= n) { set_error("strl_bamsort_window_probe: perm[%u] = %u is no ordinal", j, perm[j]); return STRL_ERR_ARG; }
  STRL_HIP(hipSetDevice(c->device));
  hipStream_t st = c->stream;
  const uint32_t n_tiles = (n + BSORT_TILE - 1u) / BSORT_TILE;
  DevBuf d_len, d_perm, d_off, d_tile, d_state, d_dest, d_parts;
  int rc;
  if ((rc = d_len.reserve((size_t)n * 4 + 64)) || (rc = d_perm.reserve((size_t)n * 4 + 64)) || (rc = d_off.reserve(((size_t)n + 1) * 8)) || (rc = d_tile.reserve((size_t)n_tiles * 8 + 64)) ||
      (rc = d_state.reserve(sizeof(BsortState))) || (rc = d_dest.reserve((size_t)n * 8 + 64)) || (rc = d_parts.reserve((size_t)n * 24 + 64)))
    return rc;
  BsortState *S = d_state.as<BsortState>();
  STRL_HIP(hipMemsetAsync(S, 0, sizeof(BsortState), st));
  if (n) {
    STRL_HIP(hipMemcpyAsync(d_len.p, len, (size_t)n * 4, hipMemcpyHostToDevice, st));
    STRL_HIP(hipMemcpyAsync(d_perm.p, perm, (size_t)n * 4, hipMemcpyHostToDevice, st));
    STRL_HIP(hipMemsetAsync(d_dest.p, 0xff, (size_t)n * 8, st));
  }
  if ((rc = bsort_layout(st, d_perm.as<uint32_t>(), d_len.as<uint32_t>(), n, n, base, d_tile.as<uint64_t>(), d_off.as<uint64_t>(), S))) return rc;
  if (n) {
    hipLaunchKernelGGL(bsort_dest_kernel, dim3((n + 255u) / 256u), dim3(256), 0, st, d_perm.as<uint32_t>(), d_off.as<uint64_t>(), n, d_dest.as<uint64_t>());
    hipLaunchKernelGGL(bsort_wparts_kernel, dim3((n + 255u) / 256u), dim3(256), 0, st, d_dest.as<uint64_t>(), d_len.as<uint32_t>(), n, lo, hi, d_parts.as<uint64_t>());
    STRL_HIP(hipGetLastError());
    STRL_HIP(hipMemcpyAsync(dest_out, d_dest.p, (size_t)n * 8, hipMemcpyDeviceToHost, st));
    STRL_HIP(hipMemcpyAsync(parts, d_parts.p, (size_t)n * 24, hipMemcpyDeviceToHost, st));
  }
  STRL_HIP(hipStreamSynchronize(st));
  return STRL_OK;
}

// test-only, undeclared (the strl_sort_probe precedent): the layout and the piece search as the sort runs them, over caller-given
// len[n], a caller-given 64-bit base and a piece [lo, hi) -- offsets beyond 2^32 without 4 GB of data.  off_out[n + 1]; range[2] =
// the touched records; parts[3 k ..] = (source skip, destination, bytes) of the k-th touched record, at most parts_cap of them.
extern "C" int strl_bamsort_probe(strl_ctx *c, const uint32_t *len, uint32_t n, uint64_t base, uint64_t lo, uint64_t hi, uint64_t *off_out, uint64_t *range, uint64_t *parts,
                                  uint64_t parts_cap) {
  if (!c || (n && !len) || !off_out || !range || lo > hi || (parts_cap && !parts)) { set_error("strl_bamsort_probe: bad argument"); return STRL_ERR_ARG; }
  STRL_HIP(hipSetDevice(c->device));
  hipStream_t st = c->stream;
  const uint32_t n_tiles = (n + BSORT_TILE - 1u) / BSORT_TILE;
  DevBuf d_len, d_perm, d_off, d_tile, d_state, d_parts;
  int rc;
  if ((rc = d_len.reserve((size_t)n * 4 + 64)) || (rc = d_perm.reserve((size_t)n * 4 + 64)) || (rc = d_off.reserve(((size_t)n + 1) * 8)) || (rc = d_tile.reserve((size_t)n_tiles * 8 + 64)) ||
      (rc = d_state.reserve(sizeof(BsortState))) || (rc = d_parts.reserve((size_t)parts_cap * 24 + 64)))
    return rc;
  BsortState *S = d_state.as<BsortState>();
  STRL_HIP(hipMemsetAsync(S, 0, sizeof(BsortState), st));
  if (n) {
    STRL_HIP(hipMemcpyAsync(d_len.p, len, (size_t)n * 4, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(bsort_iota_kernel, dim3((n + 255u) / 256u), dim3(256), 0, st, d_perm.as<uint32_t>(), n);
  }
  if ((rc = bsort_layout(st, d_perm.as<uint32_t>(), d_len.as<uint32_t>(), n, n, base, d_tile.as<uint64_t>(), d_off.as<uint64_t>(), S))) return rc;
  hipLaunchKernelGGL(bsort_range_kernel, dim3(1), dim3(64), 0, st, d_off.as<uint64_t>(), (uint64_t)n, lo, hi, S);
  if (parts_cap) hipLaunchKernelGGL(bsort_parts_kernel, dim3(64), dim3(256), 0, st, d_off.as<uint64_t>(), (uint64_t)n, lo, hi, S, d_parts.as<uint64_t>(), parts_cap);
  STRL_HIP(hipGetLastError());
  BsortState H;
  STRL_HIP(hipMemcpyAsync(off_out, d_off.p, ((size_t)n + 1) * 8, hipMemcpyDeviceToHost, st));
  STRL_HIP(hipMemcpyAsync(&H, S, sizeof H, hipMemcpyDeviceToHost, st));
  STRL_HIP(hipStreamSynchronize(st));
  range[0] = H.range[0]; range[1] = H.range[1];
  const uint64_t touched = std::min<uint64_t>(H.range[1] - H.range[0], parts_cap);
  if (touched) STRL_HIP(hipMemcpy(parts, d_parts.p, (size_t)touched * 24, hipMemcpyDeviceToHost));
  return STRL_OK;
}
