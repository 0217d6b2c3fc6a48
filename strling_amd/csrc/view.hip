// view.hip -- `strling view`: a chunk's records as SAM text on the device (gfx950), behind the front end's record scan.  The rule
// is view_core.h's.  DESIGN section 24.5.
//   front_stage_a      (front.hip)   copy + inflate + CRC + record scan: recoff[] of the chunk, its records contiguous
//   view_size_kernel   16 lanes a record: every inner length held against the record before use; the CIGAR's operations strided
//                      over the group (their digits, the reference length, the op codes), the head, RNEXT PNEXT TLEN, the tag walk and
//                      SEQ QUAL one lane each; the line's length (0: not kept), where its variable parts start, the hard mark; kept,
//                      dropped and hard counts and the lowest refused ordinal with its field code by integer atomics
//   view_tile / _scan  a tiled 64-bit exclusive prefix sum of the lengths: off[0..n] and the chunk's text bytes
//   view_text_kernel   the hot path, 16 lanes a record: lane 0 the head and RNEXT PNEXT TLEN, lane 1 the CIGAR, lane 2 the tags, all
//                      lanes SEQ and QUAL -- bytes up to a 16-byte boundary of the destination, then whole aligned 16-byte stores
//                      each assembled in registers (SEQ's from 8 bytes of packed bases, QUAL's from 16 bytes clamped and rebased),
//                      then the tail bytewise.  Nothing outside [off[i], off[i + 1]) is written for record i.
// A chunk with a float that view_float_g does not answer goes back to the host twin (view_host), the same bytes.
#include <stdlib.h>
#include <algorithm>
#include "front.h"
#include "device_util.h"
#include "view_core.h"

namespace strl {

namespace {

constexpr uint32_t VIEW_G = 16;                            // lanes a record
constexpr int VIEW_TEXT = 0, VIEW_COUNT = 1, VIEW_NEED = 2;   // what view_chunk_run is asked for
constexpr uint32_t VIEW_TILE = 2048;                       // records per workgroup of the prefix sum: 256 lanes x 8

struct ViewState {
  uint64_t err;              // (ordinal << 8 | field code) of the first refused record; ~0 = none
  uint64_t kept, dropped, hard, total;
};

struct ViewChunk {
  const uint8_t *U;          // the records lie in U[start0, rec_end)
  const uint32_t *recoff;
  uint32_t n, start0, rec_end;
  uint64_t ord0;             // ordinal of the chunk's first record
  ViewRefs F;
  ViewOpts o;
  uint32_t *len;             // [n] bytes of the record's line
  ViewParts *parts;          // [n]
  uint64_t *off;             // [n + 1]
  uint8_t *text;             // 16-byte aligned
  ViewState *S;
};

// record i inside the chunk's bytes, or null
__device__ __forceinline__ const uint8_t *view_at(const ViewChunk &P, uint32_t i, uint64_t *len) {
  const uint32_t q = P.recoff[i];
  if (q < P.start0 || q > P.rec_end || P.rec_end - q < MDUP_FIXED) return nullptr;
  const uint64_t l = (uint64_t)ld32u(P.U + q) + 4u;
  if (l > P.rec_end - q) return nullptr;
  *len = l;
  return P.U + q;
}

__device__ __forceinline__ uint64_t view_gsum(uint64_t v) { for (int d = 8; d > 0; d >>= 1) v += __shfl_xor(v, d, (int)VIEW_G); return v; }
__device__ __forceinline__ uint32_t view_gsum(uint32_t v) { for (int d = 8; d > 0; d >>= 1) v += __shfl_xor(v, d, (int)VIEW_G); return v; }
__device__ __forceinline__ uint32_t view_gmin(uint32_t v) { for (int d = 8; d > 0; d >>= 1) v = min(v, (uint32_t)__shfl_xor(v, d, (int)VIEW_G)); return v; }

__global__ __launch_bounds__(256) void view_size_kernel(ViewChunk P) {
  const uint32_t g = threadIdx.x % VIEW_G;
  const uint64_t group = ((uint64_t)blockIdx.x * 256u + threadIdx.x) / VIEW_G, n_groups = (uint64_t)gridDim.x * 256u / VIEW_G;
  uint32_t n_kept = 0, n_dropped = 0, n_hard = 0;             // lane 0's
  for (uint64_t i = group; i < P.n; i += n_groups) {
    uint64_t rlen = 0;
    const uint8_t *rec = view_at(P, (uint32_t)i, &rlen);
    ViewRec R;
    const bool ok = rec && view_rec(rec, rlen, &R);
    uint32_t clen = 0, cig_bad = 0;
    uint64_t reflen = 0;
    for (uint32_t k = g; ok && k < R.f.n_cigar; k += VIEW_G) {
      const uint32_t w = mdup_ld32(rec + R.f.cigar_at + 4u * k), op = w & 15u;
      cig_bad |= op > 8u ? 1u : 0u;
      clen += view_udigits(w >> 4) + 1u;
      if (view_cigar_on_ref(op)) reflen += w >> 4;
    }
    clen = view_gsum(clen); cig_bad = view_gsum(cig_bad); reflen = view_gsum(reflen);
    const bool kept = ok && view_kept(R, P.o, reflen);
    uint32_t part = 0, hard = 0, e = 0;
    if (kept) {
      ViewCount s;
      if (g == 0) { if (R.f.tid >= P.F.n_ref) e = VIEW_E_RNAME; else view_head_emit(s, rec, R, P.F); }
      else if (g == 1) { if (R.mtid >= P.F.n_ref) e = VIEW_E_RNEXT; else view_mid_emit(s, R, P.F); }
      else if (g == 2) e = view_tags_emit(s, rec + R.tags_at, R.n_tags, &hard);
      else if (g == 3) s.n = (uint64_t)view_seq_len(R) + 1u + view_qual_len(rec, R);
      else if (g == 4) { if (cig_bad) e = VIEW_E_CIGAR; s.n = R.f.n_cigar ? clen : 1u; }
      part = (uint32_t)s.n;                                   // (a record holds at most 2^28 bytes: its line fits 32 bits)
    }
    const uint32_t head = __shfl(part, 0, (int)VIEW_G), mid = __shfl(part, 1, (int)VIEW_G), tags = __shfl(part, 2, (int)VIEW_G), sq = __shfl(part, 3, (int)VIEW_G),
                   cg = __shfl(part, 4, (int)VIEW_G);
    hard = __shfl(hard, 2, (int)VIEW_G);
    e = view_gmin(e ? e : 0xffu);
    if (!ok) e = VIEW_E_SIZE; else if (e == 0xffu) e = 0;
    if (g == 0) {
      if (e) atomicMin(reinterpret_cast<unsigned long long *>(&P.S->err), (unsigned long long)((P.ord0 + i) << 8 | e));
      const bool line = kept && !e;
      P.len[i] = line ? head + cg + mid + sq + tags + 1u : 0u;
      P.parts[i] = ViewParts{head, head + cg, head + cg + mid, head + cg + mid + sq};
      if (line) ++n_kept; else ++n_dropped;
      if (line && hard) ++n_hard;
    }
  }
  uint32_t what[3] = {n_kept, n_dropped, n_hard};
  uint64_t *to[3] = {&P.S->kept, &P.S->dropped, &P.S->hard};
  for (int k = 0; k < 3; ++k) {
    uint32_t v = what[k];
    for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d);
    if ((threadIdx.x & 63u) == 0 && v) atomicAdd(reinterpret_cast<unsigned long long *>(to[k]), (unsigned long long)v);
  }
}

// exclusive sum over the 256 lanes of a workgroup (sh: 4 words); *block_total = the sum of all
__device__ __forceinline__ uint64_t view_block_excl(uint64_t v, uint64_t *sh, uint64_t *block_total) {
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
template <bool ADD> __global__ __launch_bounds__(256) void view_tile_kernel(const uint32_t *len, uint32_t n, uint64_t *tile, uint64_t *off) {
  __shared__ uint64_t sh[4];
  const uint64_t j0 = (uint64_t)blockIdx.x * VIEW_TILE + (uint64_t)threadIdx.x * 8u;
  uint64_t l[8], mine = 0;
  for (uint32_t k = 0; k < 8u; ++k) {
    const uint64_t j = j0 + k;
    l[k] = j < n ? (uint64_t)len[j] : 0ull;
    mine += l[k];
  }
  uint64_t tot;
  uint64_t at = view_block_excl(mine, sh, &tot);
  if constexpr (!ADD) {
    if (threadIdx.x == 0) tile[blockIdx.x] = tot;
  } else {
    at += tile[blockIdx.x];
    for (uint32_t k = 0; k < 8u; ++k) { const uint64_t j = j0 + k; if (j < n) off[j] = at; at += l[k]; }
  }
}
// one workgroup: tile[0, n_tiles) -> exclusive sums in place, the total to S->total and to off[n]
__global__ __launch_bounds__(1024) void view_scan_kernel(uint64_t *tile, uint32_t n_tiles, uint64_t *off, uint32_t n, ViewState *S) {
  __shared__ uint64_t part[1024];
  const uint32_t t = threadIdx.x, per = (n_tiles + 1023u) / 1024u, a = min(n_tiles, t * per), b = min(n_tiles, a + per);
  uint64_t s = 0;
  for (uint32_t k = a; k < b; ++k) s += tile[k];
  part[t] = s;
  __syncthreads();
  if (t == 0) {
    uint64_t run = 0;
    for (int k = 0; k < 1024; ++k) { const uint64_t v = part[k]; part[k] = run; run += v; }
    S->total = run; off[n] = run;
  }
  __syncthreads();
  uint64_t run = part[t];
  for (uint32_t k = a; k < b; ++k) { const uint64_t v = tile[k]; tile[k] = run; run += v; }
}

// ---- SEQ and QUAL: text[a0, a0 + l), lane g of 16 ------------------------------------------------------------------------------------
// the ends around the whole 16-byte words [w0, w1) of the destination: [a0, w0) and [w1, a1), or all of it where it holds no word
template <typename Byte> __device__ __forceinline__ void view_put_ends(uint8_t *text, uint64_t a0, uint64_t a1, uint64_t w0, uint64_t w1, uint32_t g, Byte &&byte) {
  const bool words = w0 < w1;
  const uint64_t n_head = (words ? w0 : a1) - a0, tail_at = words ? w1 : a1, n_ends = n_head + (a1 - tail_at);
  for (uint64_t x = g; x < n_ends; x += VIEW_G) {
    const uint64_t k = x < n_head ? a0 + x : tail_at + (x - n_head);
    text[k] = byte((uint32_t)(k - a0));
  }
}
__device__ __forceinline__ void view_put_seq(uint8_t *text, uint64_t a0, const uint8_t *seq, uint32_t l, uint32_t g) {
  const uint64_t a1 = a0 + l, w0 = (a0 + 15u) & ~15ull, w1 = a1 & ~15ull;
  for (uint64_t w = w0 + 16u * g; w < w1; w += 16u * VIEW_G) {
    const uint32_t j0 = (uint32_t)(w - a0);                   // bases j0 .. j0 + 15, all inside the read
    uint64_t x;
    __builtin_memcpy(&x, seq + (j0 >> 1), 8);
    x = (x & 0x0f0f0f0f0f0f0f0full) << 4 | (x >> 4 & 0x0f0f0f0f0f0f0f0full);      // nibble i (bits 4 i) = base 2 (j0 / 2) + i
    if (j0 & 1u) x = x >> 4 | (uint64_t)(seq[(j0 >> 1) + 8u] >> 4) << 60;
    uint64_t q0 = 0, q1 = 0;
#pragma unroll
    for (uint32_t k = 0; k < 8u; ++k) {
      q0 |= (uint64_t)view_base((uint32_t)(x >> (4u * k)) & 15u) << (8u * k);
      q1 |= (uint64_t)view_base((uint32_t)(x >> (32u + 4u * k)) & 15u) << (8u * k);
    }
    *reinterpret_cast<uint4 *>(text + w) = make_uint4((uint32_t)q0, (uint32_t)(q0 >> 32), (uint32_t)q1, (uint32_t)(q1 >> 32));
  }
  view_put_ends(text, a0, a1, w0, w1, g, [seq](uint32_t j) { return view_base((uint32_t)(seq[j >> 1] >> ((~j & 1u) << 2)) & 15u); });
}
// min(q, 93) + 33 in each of a word's eight bytes
__device__ __forceinline__ uint64_t view_qual8(uint64_t x) {
  constexpr uint64_t ones = 0x0101010101010101ull;
  const uint64_t over = (((x & 0x7f * ones) + (127u - VIEW_QUAL_MAX) * ones) | x) & 0x80 * ones;      // bit 7 of a byte above 93
  const uint64_t m = (over >> 7) * 0xffu;
  return ((x & ~m) | (VIEW_QUAL_MAX * ones & m)) + 33u * ones;
}
__device__ __forceinline__ void view_put_qual(uint8_t *text, uint64_t a0, const uint8_t *qual, uint32_t l, uint32_t g) {
  const uint64_t a1 = a0 + l, w0 = (a0 + 15u) & ~15ull, w1 = a1 & ~15ull;
  for (uint64_t w = w0 + 16u * g; w < w1; w += 16u * VIEW_G) {
    uint64_t x0, x1;
    __builtin_memcpy(&x0, qual + (w - a0), 8);
    __builtin_memcpy(&x1, qual + (w - a0) + 8u, 8);
    const uint64_t q0 = view_qual8(x0), q1 = view_qual8(x1);
    *reinterpret_cast<uint4 *>(text + w) = make_uint4((uint32_t)q0, (uint32_t)(q0 >> 32), (uint32_t)q1, (uint32_t)(q1 >> 32));
  }
  view_put_ends(text, a0, a1, w0, w1, g, [qual](uint32_t j) { return view_qual(qual[j]); });
}

__global__ __launch_bounds__(256) void view_text_kernel(ViewChunk P) {
  const uint32_t g = threadIdx.x % VIEW_G;
  const uint64_t group = ((uint64_t)blockIdx.x * 256u + threadIdx.x) / VIEW_G, n_groups = (uint64_t)gridDim.x * 256u / VIEW_G;
  const uint64_t total = P.off[P.n];
  for (uint64_t i = group; i < P.n; i += n_groups) {
    const uint64_t L = P.len[i], A = P.off[i], B = P.off[i + 1];
    if (!L || B < A || B - A != L || B > total) continue;
    uint64_t rlen = 0;
    const uint8_t *rec = view_at(P, (uint32_t)i, &rlen);
    ViewRec R;
    if (!rec || !view_rec(rec, rlen, &R)) continue;
    const ViewParts pt = P.parts[i];
    const uint32_t sl = view_seq_len(R), ql = view_qual_len(rec, R);
    // the parts add up, or the record is left alone
    if (pt.cigar_at > pt.mid_at || pt.mid_at > pt.seq_at || (uint64_t)pt.seq_at + sl + 1u + ql != pt.tags_at || pt.tags_at >= L) continue;
    uint8_t *d = P.text + A;
    if (g == 0) {
      ViewStore s{d, d + pt.cigar_at};
      view_head_emit(s, rec, R, P.F);
      ViewStore m{d + pt.mid_at, d + pt.seq_at};
      view_mid_emit(m, R, P.F);
      d[pt.seq_at + sl] = '\t';
      d[L - 1u] = '\n';
    } else if (g == 1) {
      ViewStore s{d + pt.cigar_at, d + pt.mid_at};
      view_cigar_emit(s, rec, R);
    } else if (g == 2) {
      ViewStore s{d + pt.tags_at, d + (L - 1u)};
      uint32_t hard = 0;
      (void)view_tags_emit(s, rec + R.tags_at, R.n_tags, &hard);
    }
    if (!R.f.l_seq) { if (g == 3) d[pt.seq_at] = '*'; }
    else view_put_seq(P.text, A + pt.seq_at, rec + R.seq_at, R.f.l_seq, g);
    if (ql != R.f.l_seq || !R.f.l_seq) { if (g == 3) d[pt.seq_at + sl + 1u] = '*'; }
    else view_put_qual(P.text, A + pt.seq_at + sl + 1u, rec + R.f.qual_at, R.f.l_seq, g);
  }
}

// ---- what a chunk's two kernels need on the host's side -------------------------------------------------------------------------------
struct ViewWork {
  DevBuf len, parts, off, tile, state, text, names, name_off, rec_bytes, rec_off;      // rec_*: strl_view_records' upload
  ViewState *h_state = nullptr;                               // page-locked
  uint8_t *h_text[2] = {nullptr, nullptr};                    // page-locked: the lines of the chunk handed out last / before
  size_t h_cap[2] = {0, 0};
  std::vector<uint8_t> host_text[2], raw;                     // a hard chunk's lines, its records
  hipEvent_t e[4] = {};
  std::vector<uint8_t> names_h;
  std::vector<uint32_t> name_off_h;
  int32_t n_ref = 0;
  ViewOpts o{};
  strl_view_info info{};
  ~ViewWork() {
    if (h_state) (void)hipHostFree(h_state);
    for (uint8_t *p : h_text) if (p) (void)hipHostFree(p);
    for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x);
  }
};

int view_work_init(strl_ctx *c, ViewWork &W, const uint8_t *names, const uint32_t *name_off, int32_t n_ref, const strl_view_opts *opts) {
  W.o = ViewOpts{opts->require, opts->exclude, opts->exclude_all, opts->min_mapq, opts->tid, opts->beg, opts->end};
  W.n_ref = n_ref;
  W.name_off_h.assign((size_t)n_ref + 1, 0);
  for (int32_t r = 0; r < n_ref; ++r) {
    if (name_off[r + 1] < name_off[r]) { set_error("name_off must ascend"); return STRL_ERR_ARG; }
    W.name_off_h[(size_t)r + 1] = name_off[r + 1] - name_off[0];
  }
  if (n_ref) W.names_h.assign(names + name_off[0], names + name_off[n_ref]);
  int rc;
  if ((rc = W.names.reserve(W.names_h.size() + 64)) || (rc = W.name_off.reserve(W.name_off_h.size() * 4 + 64)) || (rc = W.state.reserve(sizeof(ViewState)))) return rc;
  STRL_HIP(hipHostMalloc(reinterpret_cast<void **>(&W.h_state), sizeof(ViewState), hipHostMallocDefault));
  for (hipEvent_t &x : W.e) STRL_HIP(hipEventCreate(&x));
  if (!W.names_h.empty()) STRL_HIP(hipMemcpyAsync(W.names.p, W.names_h.data(), W.names_h.size(), hipMemcpyHostToDevice, c->stream));
  STRL_HIP(hipMemcpyAsync(W.name_off.p, W.name_off_h.data(), W.name_off_h.size() * 4, hipMemcpyHostToDevice, c->stream));
  STRL_HIP(hipStreamSynchronize(c->stream));
  return STRL_OK;
}

// The lines of the n records of U[start0, rec_end) (device memory).  dst null: they go to the page-locked buffer `slot` (or, for a hard
// chunk, to the host twin's vector) and *text names them; else they go to dst[0, cap), STRL_ERR_CAPACITY with *bytes = the need.
// mode VIEW_COUNT: the counts alone (`view -c`); VIEW_NEED: the counts and *bytes = the room the text needs.  In neither does the text
// kernel run or anything get copied, and dst is not looked at.
int view_chunk_run(strl_ctx *c, ViewWork &W, const uint8_t *U, const uint32_t *recoff, uint32_t n, uint32_t start0, uint32_t rec_end, uint64_t ord0, int slot, uint8_t *dst,
                   uint64_t cap, int mode, const uint8_t **text, uint64_t *bytes) {
  const bool size_only = mode != VIEW_TEXT;
  *text = nullptr; *bytes = 0;
  if (!n) return STRL_OK;
  hipStream_t st = c->stream;
  const uint32_t n_tiles = (n + VIEW_TILE - 1u) / VIEW_TILE;
  int rc;
  if ((rc = W.len.reserve((size_t)n * 4 + 64)) || (rc = W.parts.reserve((size_t)n * sizeof(ViewParts) + 64)) || (rc = W.off.reserve(((size_t)n + 1) * 8 + 64)) ||
      (rc = W.tile.reserve((size_t)n_tiles * 8 + 64)))
    return rc;
  ViewState &H = *W.h_state;
  H = ViewState{~0ull, 0, 0, 0, 0};
  ViewState *S = W.state.as<ViewState>();
  STRL_HIP(hipMemcpyAsync(S, &H, sizeof H, hipMemcpyHostToDevice, st));
  ViewChunk P{U, recoff, n, start0, rec_end, ord0, ViewRefs{W.names.as<uint8_t>(), W.name_off.as<uint32_t>(), W.n_ref}, W.o,
              W.len.as<uint32_t>(), W.parts.as<ViewParts>(), W.off.as<uint64_t>(), nullptr, S};
  const unsigned grid = (unsigned)std::min<uint64_t>(8192, ((uint64_t)n * VIEW_G + 255u) / 256u);
  STRL_HIP(hipEventRecord(W.e[0], st));
  hipLaunchKernelGGL(view_size_kernel, dim3(grid), dim3(256), 0, st, P);
  hipLaunchKernelGGL(view_tile_kernel<false>, dim3(n_tiles), dim3(256), 0, st, P.len, n, W.tile.as<uint64_t>(), P.off);
  hipLaunchKernelGGL(view_scan_kernel, dim3(1), dim3(1024), 0, st, W.tile.as<uint64_t>(), n_tiles, P.off, n, S);
  hipLaunchKernelGGL(view_tile_kernel<true>, dim3(n_tiles), dim3(256), 0, st, P.len, n, W.tile.as<uint64_t>(), P.off);
  STRL_HIP(hipGetLastError());
  STRL_HIP(hipEventRecord(W.e[1], st));
  STRL_HIP(hipMemcpyAsync(&H, S, sizeof H, hipMemcpyDeviceToHost, st));      // the total and the hard count in one small copy
  STRL_HIP(hipStreamSynchronize(st));
  float ms = 0.f;
  if (hipEventElapsedTime(&ms, W.e[0], W.e[1]) == hipSuccess) W.info.size_ms += ms; else (void)hipGetLastError();
  if (H.err != ~0ull) {
    set_error("malformed BAM record %llu: %s", (unsigned long long)(H.err >> 8), view_refusal_text((uint32_t)(H.err & 255u)));
    return STRL_ERR_FORMAT;
  }
  ++W.info.chunks;
  W.info.records += n; W.info.written += H.kept; W.info.dropped += H.dropped;
  if (H.hard && mode == VIEW_COUNT) { *bytes = 0; return STRL_OK; }      // (a count: the kept records are known, the hard floats' bytes are not asked for)
  if (H.hard) {
    // the host twin: the chunk's records back, the same header's function over them
    ++W.info.host_chunks;
    W.raw.resize((size_t)(rec_end - start0));
    STRL_HIP(hipMemcpy(W.raw.data(), U + start0, W.raw.size(), hipMemcpyDeviceToHost));
    std::vector<uint8_t> &out = W.host_text[slot];
    out.clear();
    uint32_t code = 0;
    ViewCounts C{};
    const int64_t bad = view_host(W.raw.data(), W.raw.size(), ViewRefs{W.names_h.data(), W.name_off_h.data(), W.n_ref}, W.o, out, &C, ord0, &code);
    if (bad >= 0) { set_error("malformed BAM record %lld: %s", (long long)bad, view_refusal_text(code)); return STRL_ERR_FORMAT; }
    *bytes = out.size();
    if (size_only) return STRL_OK;
    if (dst && out.size() > cap) return STRL_ERR_CAPACITY;
    W.info.text_bytes += out.size();
    if (dst) memcpy(dst, out.data(), out.size());
    else *text = out.data();
    return STRL_OK;
  }
  const uint64_t total = H.total;
  *bytes = total;
  if (!total || size_only) return STRL_OK;
  if (dst && total > cap) return STRL_ERR_CAPACITY;
  if ((rc = W.text.reserve((size_t)total + 64))) return rc;
  if (!dst && W.h_cap[slot] < total) {
    if (W.h_text[slot]) { (void)hipHostFree(W.h_text[slot]); W.h_text[slot] = nullptr; W.h_cap[slot] = 0; }
    const size_t want = (size_t)total + (size_t)total / 4 + 4096;
    STRL_HIP(hipHostMalloc(reinterpret_cast<void **>(&W.h_text[slot]), want, hipHostMallocDefault));
    W.h_cap[slot] = want;
  }
  P.text = W.text.as<uint8_t>();
  STRL_HIP(hipEventRecord(W.e[2], st));
  hipLaunchKernelGGL(view_text_kernel, dim3(grid), dim3(256), 0, st, P);
  STRL_HIP(hipGetLastError());
  STRL_HIP(hipEventRecord(W.e[3], st));
  uint8_t *to = dst ? dst : W.h_text[slot];
  STRL_HIP(hipMemcpyAsync(to, W.text.p, (size_t)total, hipMemcpyDeviceToHost, st));
  STRL_HIP(hipStreamSynchronize(st));
  if (hipEventElapsedTime(&ms, W.e[2], W.e[3]) == hipSuccess) W.info.text_ms += ms; else (void)hipGetLastError();
  W.info.text_bytes += total;
  if (!dst) *text = to;
  return STRL_OK;
}

}  // namespace

struct strl_view {
  ViewWork W;
  uint64_t chunks = 0, done = 0, n_records = 0;
  bool finished = false, count_only = false;
  int fail_rc = 0;
  std::string fail;
};

void view_destroy(strl_view *V) { delete V; }

static int view_fail(strl_view *V, int rc) {
  V->fail_rc = rc; V->fail = strl_last_error();
  return rc;
}

// the lines of the chunk in slot si (its record scan was enqueued by the push before)
static int view_chunk(strl_ctx *c, strl_front *F, strl_view *V, int si, bool last, const uint8_t **text, uint64_t *bytes) {
  FrontSlot &S = F->slot[si];
  STRL_HIP(hipEventSynchronize(S.ev_a));
  const FrontInfo I = S.h_info[0];
  if (I.err & FRONT_ERR_INFLATE) { set_error("invalid BGZF block (DEFLATE data or ISIZE)"); return STRL_ERR_FORMAT; }
  if (I.err & FRONT_ERR_CRC) { set_error("CRC32 checksum mismatch in a BGZF block"); return STRL_ERR_CRC; }
  if (I.err & FRONT_ERR_RECORD) { set_error("malformed BAM record"); return STRL_ERR_FORMAT; }
  if (I.err & FRONT_ERR_CARRY) { set_error("BAM record of more than %u bytes", FRONT_CARRY_MAX); return STRL_ERR_FORMAT; }
  if (last && I.carry_len) { set_error("the BAM ends inside a record (truncated file)"); return STRL_ERR_FORMAT; }
  const uint32_t n = I.n_records, rec_end = std::min(I.carry_off, I.end);
  int rc = STRL_OK;
  *text = nullptr; *bytes = 0;
  if (n && rec_end > I.start0 && (uint64_t)rec_end <= S.infl.cap)
    rc = view_chunk_run(c, V->W, S.infl.as<uint8_t>(), S.recoff.as<uint32_t>(), n, I.start0, rec_end, V->n_records, (int)(V->done & 1), nullptr, 0, V->count_only ? VIEW_COUNT : VIEW_TEXT, text, bytes);
  if (rc) return rc;
  V->n_records += n;
  STRL_HIP(hipEventRecord(S.ev_b, c->stream));      // the slot's inflated bytes and record table may be overwritten behind this
  S.b_pending = true;
  return STRL_OK;
}

}  // namespace strl

using namespace strl;

extern "C" int strl_view_begin(strl_ctx *c, int32_t n_ref, uint64_t first_record_offset, const uint8_t *names, const uint32_t *name_off, const strl_view_opts *opts) {
  if (!c || n_ref < 0 || !opts || (n_ref && (!names || !name_off))) { set_error("strl_view_begin: bad argument"); return STRL_ERR_ARG; }
  int rc;
  if ((rc = front_begin_scan(c, n_ref, first_record_offset))) return rc;
  if (c->view) { view_destroy(c->view); c->view = nullptr; }
  c->view = new strl_view();
  return view_work_init(c, c->view->W, names, name_off, n_ref, opts);
}

extern "C" int strl_view_reserve(strl_ctx *c, uint32_t max_blocks, uint64_t max_comp_bytes) {
  if (!c || !c->view || !c->front || !max_blocks) { set_error("strl_view_reserve: bad argument / no strl_view_begin"); return STRL_ERR_ARG; }
  STRL_HIP(hipSetDevice(c->device));
  ViewWork &W = c->view->W;
  int rc;
  const uint64_t rec_cap = (uint64_t)max_blocks * 65280u / 36 + 16;      // no record is shorter than 36 bytes (front_reserve's bound)
  if ((rc = W.len.reserve((size_t)rec_cap * 4 + 64)) || (rc = W.parts.reserve((size_t)rec_cap * sizeof(ViewParts) + 64)) || (rc = W.off.reserve((size_t)(rec_cap + 1) * 8 + 64)) ||
      (rc = W.tile.reserve((size_t)(rec_cap / VIEW_TILE + 2) * 8 + 64)))
    return rc;
  return front_reserve(c, c->front, max_blocks, max_comp_bytes);
}

extern "C" int strl_view_push(strl_ctx *c, const uint8_t *comp, uint64_t comp_bytes, const uint64_t *coff, const uint32_t *clen, const uint32_t *isize, const uint32_t *crc32,
                              uint32_t n_blocks, const uint8_t **text, uint64_t *text_bytes) {
  if (!c || !c->view || !c->front || c->view->finished || !text || !text_bytes || (n_blocks && (!comp || !coff || !clen || !isize))) {
    set_error("strl_view_push: bad argument / no strl_view_begin / a chunk behind the finish");
    return STRL_ERR_ARG;
  }
  *text = nullptr; *text_bytes = 0;
  if (!n_blocks) return STRL_OK;
  STRL_HIP(hipSetDevice(c->device));
  strl_front *F = c->front;
  strl_view *V = c->view;
  if (V->fail_rc) { set_error("%s", V->fail.c_str()); return V->fail_rc; }
  const int si = (int)(V->chunks & 1);
  FrontSlot &S = F->slot[si];
  int rc;
  if (S.b_pending) { STRL_HIP(hipEventSynchronize(S.ev_b)); S.b_pending = false; }     // the chunk two back has left the slot
  const FrontChunkDesc d{comp, comp_bytes, coff, clen, isize, crc32, n_blocks};
  if ((rc = front_stage_a(c, F, si, d, V->chunks == 0))) return view_fail(V, rc);
  ++V->chunks;
  // ... and beside this chunk's inflate, the lines of the previous one
  if (V->done + 1 < V->chunks) {
    if ((rc = view_chunk(c, F, V, (int)(V->done & 1), false, text, text_bytes))) return view_fail(V, rc);
    ++V->done;
  }
  return STRL_OK;
}

extern "C" int strl_view_finish(strl_ctx *c, const uint8_t **text, uint64_t *text_bytes, strl_view_info *info) {
  if (!c || !c->view || !c->front || c->view->finished || !text || !text_bytes) { set_error("strl_view_finish without strl_view_begin, or a second time"); return STRL_ERR_ARG; }
  STRL_HIP(hipSetDevice(c->device));
  strl_view *V = c->view;
  *text = nullptr; *text_bytes = 0;
  if (V->fail_rc) { set_error("%s", V->fail.c_str()); return V->fail_rc; }
  int rc;
  if (V->done < V->chunks) {                                // (the pushes leave exactly one chunk behind)
    if ((rc = view_chunk(c, c->front, V, (int)(V->done & 1), true, text, text_bytes))) return view_fail(V, rc);
    ++V->done;
  }
  STRL_HIP(hipStreamSynchronize(c->stream));
  V->finished = true;
  if (info) *info = V->W.info;
  return STRL_OK;
}

extern "C" int strl_view_end(strl_ctx *c) {
  if (!c) { set_error("null argument"); return STRL_ERR_ARG; }
  STRL_HIP(hipSetDevice(c->device));
  if (c->front) {
    for (hipStream_t q : c->front->st_i) if (q) (void)hipStreamSynchronize(q);
    if (c->front->st_a) (void)hipStreamSynchronize(c->front->st_a);
    if (c->front->st_c) (void)hipStreamSynchronize(c->front->st_c);
  }
  STRL_HIP(hipStreamSynchronize(c->stream));
  if (c->view) { view_destroy(c->view); c->view = nullptr; }
  return STRL_OK;
}

extern "C" int strl_view_count_only(strl_ctx *c, int on) {
  if (!c || !c->view || c->view->chunks) { set_error("strl_view_count_only: between strl_view_begin and the first push"); return STRL_ERR_ARG; }
  c->view->count_only = on != 0;
  return STRL_OK;
}

extern "C" int strl_view_records_at(strl_ctx *c, const uint8_t *records, uint64_t bytes, const uint8_t *names, const uint32_t *name_off, int32_t n_ref, const strl_view_opts *opts,
                                    uint64_t first_ordinal, uint8_t *out, uint64_t cap, uint64_t *out_bytes, strl_view_info *info) {
  if (!c || (bytes && !records) || !opts || !out_bytes || n_ref < 0 || (n_ref && (!names || !name_off)) || (cap && !out)) { set_error("strl_view_records: bad argument"); return STRL_ERR_ARG; }
  if (bytes > 0xfffffff0ull - 64u) { set_error("strl_view_records: at most 4 GiB of records a call"); return STRL_ERR_ARG; }
  STRL_HIP(hipSetDevice(c->device));
  *out_bytes = 0;
  if (info) *info = strl_view_info{};
  // the record table, as the record scan gives it for a chunk: the records the walk reaches
  std::vector<uint32_t> recoff;
  bool cut = false;
  for (uint64_t q = 0; q < bytes;) {
    if (bytes - q < 4 || (uint64_t)mdup_ld32(records + q) + 4u > bytes - q) { cut = true; break; }
    recoff.push_back((uint32_t)q);
    q += (uint64_t)mdup_ld32(records + q) + 4u;
  }
  const uint32_t n = (uint32_t)recoff.size();
  int rc = STRL_OK;
  strl_view_info I{};
  if (n) {
    // the work of the calls of a context is kept: events, page-locked state and buffers are made once, the names uploaded again only
    // when they differ
    strl_view *K = c->view_rec;
    const size_t nb = n_ref ? (size_t)(name_off[n_ref] - name_off[0]) : 0;
    bool same = K && K->W.n_ref == n_ref && K->W.names_h.size() == nb && (!nb || !memcmp(K->W.names_h.data(), names + name_off[0], nb));
    for (int32_t r = 0; same && r <= n_ref; ++r) same = K->W.name_off_h[(size_t)r] == (n_ref ? name_off[r] - name_off[0] : 0u);
    if (!same) {
      if (K) { STRL_HIP(hipStreamSynchronize(c->stream)); view_destroy(K); c->view_rec = nullptr; }
      K = c->view_rec = new strl_view();
      if ((rc = view_work_init(c, K->W, names, name_off, n_ref, opts))) { view_destroy(K); c->view_rec = nullptr; return rc; }
    }
    ViewWork &W = K->W;
    W.o = ViewOpts{opts->require, opts->exclude, opts->exclude_all, opts->min_mapq, opts->tid, opts->beg, opts->end};
    W.info = strl_view_info{};
    if ((rc = W.rec_bytes.reserve((size_t)bytes + 64)) || (rc = W.rec_off.reserve((size_t)n * 4 + 64))) return rc;
    STRL_HIP(hipMemcpyAsync(W.rec_bytes.p, records, (size_t)bytes, hipMemcpyHostToDevice, c->stream));
    STRL_HIP(hipMemcpyAsync(W.rec_off.p, recoff.data(), (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    const uint8_t *text = nullptr;
    const bool size_only = !out;
    rc = view_chunk_run(c, W, W.rec_bytes.as<uint8_t>(), W.rec_off.as<uint32_t>(), n, 0, (uint32_t)bytes, first_ordinal, 0, out, cap, size_only ? VIEW_NEED : VIEW_TEXT, &text, out_bytes);
    STRL_HIP(hipStreamSynchronize(c->stream));
    if (!rc && size_only && *out_bytes) rc = STRL_ERR_CAPACITY;
    if (rc == STRL_ERR_CAPACITY) set_error("strl_view_records: the text holds %llu bytes, room for %llu", (unsigned long long)*out_bytes, (unsigned long long)cap);
    if (rc && rc != STRL_ERR_CAPACITY) return rc;
    I = W.info;
  }
  if (cut) { set_error("malformed BAM record %llu: %s", (unsigned long long)(first_ordinal + n), view_refusal_text(VIEW_E_SIZE)); return STRL_ERR_FORMAT; }
  if (info) *info = I;
  return rc;
}

extern "C" int strl_view_records(strl_ctx *c, const uint8_t *records, uint64_t bytes, const uint8_t *names, const uint32_t *name_off, int32_t n_ref, const strl_view_opts *opts,
                                 uint8_t *out, uint64_t cap, uint64_t *out_bytes, strl_view_info *info) {
  return strl_view_records_at(c, records, bytes, names, name_off, n_ref, opts, 0, out, cap, out_bytes, info);
}
