// samparse.hip -- a chunk of SAM text encoded to BAM records on the GPU (gfx950): the second producer of what `strling sort`'s device
// side works from, "records back to back in device memory plus recoff[]" (DESIGN section 24.2).  The rule is sam_core.h's.
//   sam_nl_kernel<false> / sam_scan_kernel / sam_nl_kernel<true>      line scan: byte-parallel, 16 bytes a lane; the newline positions
//                                                                     compacted in order into line_off[]
//   sam_size_kernel<G>                                                G lanes a line: the eleven tabs by ballots inside the group, a
//                                                                     small field to a lane each, QUAL checked by all; the record's
//                                                                     exact length, the first refused line through an integer atomicMin
//   sam_sum_kernel<false> / sam_scan_kernel / sam_sum_kernel<true>    recoff[] = exclusive sums of the lengths, and the chunk's bytes
//   sam_encode_kernel<G>                                              G lanes a line: the record at its offset; SEQ and QUAL by all
//                                                                     lanes with aligned 16-byte stores; a line whose float values
//                                                                     the fast path declines goes on the host's list
// Every load is bounded by the line (the text buffer has 64 readable bytes behind the chunk for the aligned 16-byte loads), every
// store by the record's computed length.
#include <string.h>
#include <algorithm>
#include "samparse.h"
#include "device_util.h"

namespace strl {

constexpr uint32_t SAM_TILE_BYTES = 4096;      // bytes a workgroup of the line scan: 256 lanes x 16
constexpr uint32_t SAM_SUM_TILE = 2048;        // lengths a workgroup of the sums: 256 lanes x 8
constexpr uint32_t SAM_F_HOST = 1u, SAM_F_NOQUAL = 2u;

// ---- bytes ----------------------------------------------------------------------------------------------------------------------------
// 0x80 in every byte of x that is zero, exactly
__device__ __forceinline__ uint32_t sam_zero_bytes(uint32_t x) { return ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x | 0x7f7f7f7fu); }
// bit b = byte b of w equals c
__device__ __forceinline__ uint32_t sam_eq_mask(const uint4 &w, uint32_t c) {
  const uint32_t cc = c * 0x01010101u;
  auto four = [&](uint32_t x) { return ((sam_zero_bytes(x ^ cc) >> 7) * 0x00204081u) >> 21 & 0xfu; };
  return four(w.x) | four(w.y) << 4 | four(w.z) << 8 | four(w.w) << 12;
}
// 16 bytes at any offset o of the 16-byte aligned T; reads [o & ~15, (o & ~15) + 32) at most
__device__ __forceinline__ uint4 sam_ld16(const uint8_t *T, uint64_t o) {
  const uint32_t sh = (uint32_t)(o & 15u);
  const uint4 *p = reinterpret_cast<const uint4 *>(T + (o - sh));
  const uint4 a = p[0];
  if (!sh) return a;
  const uint4 b = p[1];
  const uint32_t ws = sh >> 2, bs = (sh & 3u) * 8u;
  uint32_t x0, x1, x2, x3, x4;
  if (ws == 0) { x0 = a.x; x1 = a.y; x2 = a.z; x3 = a.w; x4 = b.x; }
  else if (ws == 1) { x0 = a.y; x1 = a.z; x2 = a.w; x3 = b.x; x4 = b.y; }
  else if (ws == 2) { x0 = a.z; x1 = a.w; x2 = b.x; x3 = b.y; x4 = b.z; }
  else { x0 = a.w; x1 = b.x; x2 = b.y; x3 = b.z; x4 = b.w; }
  if (!bs) return make_uint4(x0, x1, x2, x3);
  return make_uint4(x0 >> bs | x1 << (32u - bs), x1 >> bs | x2 << (32u - bs), x2 >> bs | x3 << (32u - bs), x3 >> bs | x4 << (32u - bs));
}
// exclusive sum over the 256 lanes, and the workgroup's total; sh: 4 words
__device__ __forceinline__ uint32_t sam_block_excl(uint32_t v, uint32_t *sh, uint32_t *total) {
  const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  uint32_t inc = v;
  for (int d = 1; d < 64; d <<= 1) { const uint32_t o = __shfl_up(inc, d); if ((int)lane >= d) inc += o; }
  if (lane == 63u) sh[w] = inc;
  __syncthreads();
  uint32_t base = 0, tot = 0;
  for (uint32_t k = 0; k < 4u; ++k) { if (k < w) base += sh[k]; tot += sh[k]; }
  *total = tot;
  return base + inc - v;
}

// ---- 1. line scan ----------------------------------------------------------------------------------------------------------------------
template <bool WRITE> __global__ __launch_bounds__(256) void sam_nl_kernel(const uint8_t *T, uint64_t bytes, uint32_t *tile, uint32_t *line_off, uint32_t line_cap) {
  __shared__ uint32_t sh[4];
  const uint64_t o = (uint64_t)blockIdx.x * SAM_TILE_BYTES + (uint64_t)threadIdx.x * 16u;
  uint32_t m = 0;
  if (o < bytes) {
    m = sam_eq_mask(*reinterpret_cast<const uint4 *>(T + o), '\n');
    if (bytes - o < 16u) m &= (1u << (uint32_t)(bytes - o)) - 1u;
  }
  uint32_t tot;
  uint32_t at = sam_block_excl(__popc(m), sh, &tot);
  if constexpr (!WRITE) { if (threadIdx.x == 0) tile[blockIdx.x] = tot; }
  else {
    at += tile[blockIdx.x];
    for (; m; m &= m - 1u, ++at) if (at < line_cap) line_off[at] = (uint32_t)o + (uint32_t)__ffs(m) - 1u;
  }
}
// one workgroup: tile[0, n_tiles) -> exclusive sums in place; the total to S->n_lines (what = 0: held to line_cap, more than that
// sets S->overflow) or to S->total (the chunk's bytes)
__global__ __launch_bounds__(1024) void sam_scan_kernel(uint32_t *tile, uint32_t n_tiles, SamInfo *S, int what, uint32_t line_cap) {
  __shared__ unsigned long long part[1024];
  const uint32_t t = threadIdx.x, per = (n_tiles + 1023u) / 1024u, a = min(n_tiles, t * per), b = min(n_tiles, a + per);
  unsigned long long s = 0;
  for (uint32_t k = a; k < b; ++k) s += tile[k];
  part[t] = s;
  __syncthreads();
  if (t == 0) {
    unsigned long long run = 0;
    for (int k = 0; k < 1024; ++k) { const unsigned long long v = part[k]; part[k] = run; run += v; }
    if (what == 0) { S->overflow = run > line_cap ? 1u : 0u; S->n_lines = (uint32_t)(run > line_cap ? line_cap : run); }
    else S->total = run;
  }
  __syncthreads();
  unsigned long long run = part[t];
  for (uint32_t k = a; k < b; ++k) { const uint32_t v = tile[k]; tile[k] = (uint32_t)run; run += v; }
}

// ---- the group's tools ------------------------------------------------------------------------------------------------------------------
template <uint32_t G> __device__ __forceinline__ uint32_t sam_group_ballot(bool p) {
  const unsigned long long m = __ballot(p);
  const uint32_t base = (threadIdx.x & 63u) & ~(G - 1u);
  if constexpr (G == 64) return 0;             // (not used: a wave's ballot is the group's, see sam_find_tabs)
  else return (uint32_t)(m >> base) & (G == 32 ? 0xffffffffu : (1u << (G & 31u)) - 1u);
}
// the first eleven tabs of the line T[beg, beg + len), every lane of the group gets them all; -> how many there are (at most 11)
template <uint32_t G> __device__ __forceinline__ uint32_t sam_find_tabs(const uint8_t *T, uint64_t beg, uint32_t len, uint32_t g, uint32_t *tab) {
  uint32_t found = 0;
  const uint32_t n_words = (len + 15u) >> 4;
  for (uint32_t v0 = 0; v0 < n_words && found < 11u; v0 += G) {
    const uint32_t v = v0 + g;
    uint32_t m = 0;
    if (v < n_words) {
      m = sam_eq_mask(sam_ld16(T, beg + (uint64_t)v * 16u), '\t');
      const uint32_t left = len - v * 16u;
      if (left < 16u) m &= (1u << left) - 1u;
    }
    const uint32_t c = __popc(m);
    uint32_t inc = c;
    for (uint32_t d = 1; d < G; d <<= 1) { const uint32_t o = __shfl_up(inc, d, G); if (g >= d) inc += o; }
    const uint32_t excl = inc - c, tot = __shfl(inc, G - 1, G);
    const uint32_t take = min(tot, 11u - found);
    for (uint32_t k = 0; k < take; ++k) {      // the k-th tab of this stride lies with the one lane that has excl <= k < excl + c
      const bool has = k >= excl && k < excl + c;
      uint32_t cand = 0;
      if (has) { uint32_t mm = m; for (uint32_t d = excl; d < k; ++d) mm &= mm - 1u; cand = v * 16u + (uint32_t)__ffs(mm) - 1u; }
      uint32_t owner;
      if constexpr (G == 64) owner = (uint32_t)__ffsll((unsigned long long)__ballot(has)) - 1u;
      else owner = (uint32_t)__ffs(sam_group_ballot<G>(has)) - 1u;
      tab[found + k] = __shfl(cand, owner & (G - 1u), G);
    }
    found += take;
  }
  return found;
}
template <uint32_t G> __device__ __forceinline__ uint32_t sam_group_min(uint32_t v) {
  for (uint32_t d = G >> 1; d; d >>= 1) v = min(v, __shfl_xor(v, d, G));
  return v;
}

struct SamChunk {
  const uint8_t *T;            // 16-byte aligned, 64 readable bytes behind `bytes`
  uint64_t bytes;
  const uint32_t *line_off;    // [line_cap]: where every line's \n lies
  uint32_t line_cap;
  SamRefs R;
  uint32_t *len;               // [line_cap]: the record's bytes, 0 = refused
  SamMeta *meta;
  const uint32_t *recoff;
  uint8_t *rec;
  uint64_t rec_cap;
  uint32_t *fix, fix_cap;
  SamInfo *S;
};

// ---- 2. size ------------------------------------------------------------------------------------------------------------------------------
template <uint32_t G> __global__ __launch_bounds__(256) void sam_size_kernel(SamChunk P) {
  const uint32_t g = threadIdx.x % G;
  const uint32_t group = (blockIdx.x * 256u + threadIdx.x) / G, n_groups = gridDim.x * 256u / G;
  const uint32_t n = min(P.S->n_lines, P.line_cap);
  for (uint32_t i = group; i < n; i += n_groups) {
    const uint64_t beg = i ? (uint64_t)P.line_off[i - 1] + 1u : 0u, nl = P.line_off[i];
    uint32_t er = SAM_E_NONE, len = 0;
    SamMeta M;
    for (int k = 0; k < 11; ++k) M.tab[k] = 0;
    M.n_cig = M.tag_bytes = M.flags = M.pad = 0;
    if (nl < beg || nl >= P.bytes) er = SAM_E_OVERRUN;               // (never: the scan wrote ascending positions inside the chunk)
    else {
      const uint8_t *L = P.T + beg;
      len = (uint32_t)min(nl - beg, (uint64_t)SAM_LINE_MAX + 2u);
      if (len && L[len - 1] == '\r') --len;
      if (len > SAM_LINE_MAX) er = SAM_E_LONG_LINE;
      else if (!len) er = SAM_E_EMPTY;
    }
    M.len = len;
    uint32_t rec_len = 0;
    if (er == SAM_E_NONE) {
      const uint8_t *L = P.T + beg;
      const uint32_t nt = sam_find_tabs<G>(P.T, beg, len, g, M.tab);
      if (nt < 10u) er = SAM_E_FIELDS;
      else {
        if (nt == 10u) M.tab[10] = len;
        const uint32_t *t = M.tab;
        uint32_t e = SAM_E_NONE, val = 0, val2 = 0;
        uint64_t u;
        int64_t s;
        int32_t id;
        if (g == 0) { if (t[0] < 1u || t[0] > 254u) e = SAM_E_QNAME; }
        else if (g == 1) { if (!sam_udec(L + t[0] + 1, t[1] - t[0] - 1, 65535, &u)) e = SAM_E_FLAG; }
        else if (g == 2) { const uint32_t x = sam_ref_field(P.R, L + t[1] + 1, t[2] - t[1] - 1, false, -1, &id); if (x) e = x; }
        else if (g == 3) { if (!sam_udec(L + t[2] + 1, t[3] - t[2] - 1, 2147483647, &u)) e = SAM_E_POS; }
        else if (g == 4) { if (!sam_udec(L + t[3] + 1, t[4] - t[3] - 1, 255, &u)) e = SAM_E_MAPQ; }
        else if (g == 5) { uint64_t rl; const uint32_t x = sam_cigar(L + t[4] + 1, t[5] - t[4] - 1, nullptr, 0, &val, &rl); if (x) e = x; }
        else if (g == 6) { const uint32_t x = sam_ref_field(P.R, L + t[5] + 1, t[6] - t[5] - 1, true, -1, &id); if (x) e = x; }
        else if (g == 7) { if (!sam_udec(L + t[6] + 1, t[7] - t[6] - 1, 2147483647, &u)) e = SAM_E_PNEXT; }
        else if (g == 8) { if (!sam_sdec(L + t[7] + 1, t[8] - t[7] - 1, -2147483648ll, 2147483647ll, &s)) e = SAM_E_TLEN; }
        else if (g == 9) {
          if (t[10] < len) { const uint32_t x = sam_tags<false>(L + t[10] + 1, len - t[10] - 1, nullptr, 0, &val, &val2); if (x) e = x; }
        }
        // SEQ and QUAL: lengths by every lane, the bytes of QUAL by all of them
        const uint32_t ls = t[9] - t[8] - 1u, lq = t[10] - t[9] - 1u;
        uint32_t l_seq = 0;
        bool noqual = false;
        if (!ls) e = min(e, (uint32_t)SAM_E_SEQ);
        else {
          l_seq = ls == 1u && L[t[8] + 1] == '*' ? 0u : ls;
          noqual = lq == 1u && L[t[9] + 1] == '*';
          if (!noqual) {
            if (!l_seq) e = min(e, (uint32_t)SAM_E_QUAL_NOSEQ);
            else if (lq != l_seq) e = min(e, (uint32_t)SAM_E_QUAL_LEN);
            else {
              const uint64_t q0 = beg + t[9] + 1u;
              bool low = false;
              for (uint32_t v = g; v * 16u < lq; v += G) {
                uint4 w = sam_ld16(P.T, q0 + (uint64_t)v * 16u);
                const uint32_t left = lq - v * 16u;
                uint32_t x[4] = {w.x, w.y, w.z, w.w};
                for (uint32_t b = 0; b < 4u; ++b) {
                  uint32_t y = x[b];
                  if (left < 4u * b + 4u) y |= left <= 4u * b ? 0xffffffffu : 0xffffffffu << ((left - 4u * b) * 8u);      // (bytes behind the field pass)
                  low = low || ((y - 0x21212121u) & ~y & 0x80808080u);
                }
              }
              if (low) e = min(e, (uint32_t)SAM_E_QUAL_BYTE);
            }
          }
        }
        er = sam_group_min<G>(e);
        M.n_cig = __shfl(val, 5, G);
        M.tag_bytes = __shfl(val, 9, G);
        M.flags = (__shfl(val2, 9, G) ? SAM_F_HOST : 0u) | (noqual ? SAM_F_NOQUAL : 0u);
        if (er == SAM_E_NONE) {
          rec_len = sam_rec_len(t[0], M.n_cig, l_seq, M.tag_bytes);
          if (!rec_len) er = SAM_E_RECORD_BIG;
        }
      }
    }
    if (g == 0) {
      if (er != SAM_E_NONE) { rec_len = 0; atomicMin(&P.S->err_line, (unsigned long long)i); }
      P.len[i] = rec_len;
      P.meta[i] = M;
    }
  }
}

// ---- recoff[] ------------------------------------------------------------------------------------------------------------------------------
template <bool ADD> __global__ __launch_bounds__(256) void sam_sum_kernel(const uint32_t *len, uint32_t line_cap, uint32_t *tile, uint32_t *recoff, const SamInfo *S) {
  __shared__ uint32_t sh[4];
  const uint32_t n = min(S->n_lines, line_cap);
  const uint64_t j0 = (uint64_t)blockIdx.x * SAM_SUM_TILE + (uint64_t)threadIdx.x * 8u;
  uint32_t l[8], mine = 0;
  for (uint32_t k = 0; k < 8u; ++k) { l[k] = j0 + k < n ? len[j0 + k] : 0u; mine += l[k]; }
  uint32_t tot;
  uint32_t at = sam_block_excl(mine, sh, &tot);
  if constexpr (!ADD) { if (threadIdx.x == 0) tile[blockIdx.x] = tot; }
  else {
    at += tile[blockIdx.x];
    for (uint32_t k = 0; k < 8u; ++k) { if (j0 + k < n) recoff[j0 + k] = at; at += l[k]; }
  }
}

// ---- 3. encode -----------------------------------------------------------------------------------------------------------------------------
// `count` bytes at dst from a producer of single bytes and one of aligned 16-byte words: the head up to the first 16-byte boundary and
// the tail behind the last whole word go singly, the words between as aligned stores
template <uint32_t G, typename ByteFn, typename WordFn> __device__ __forceinline__ void sam_store_span(uint8_t *dst, uint32_t count, uint32_t g, ByteFn one, WordFn word) {
  const uint32_t to16 = (16u - (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 15u)) & 15u, head = min(count, to16);
  for (uint32_t k = g; k < head; k += G) dst[k] = one(k);
  const uint32_t n_vec = (count - head) >> 4;
  uint4 *da = reinterpret_cast<uint4 *>(dst + head);
  for (uint32_t v = g; v < n_vec; v += G) da[v] = word(head + v * 16u);
  const uint32_t done = head + (n_vec << 4);
  for (uint32_t k = done + g; k < count; k += G) dst[k] = one(k);
}

template <uint32_t G> __global__ __launch_bounds__(256) void sam_encode_kernel(SamChunk P) {
  __shared__ uint8_t code[256];
  code[threadIdx.x] = (uint8_t)sam_seq_code((uint8_t)threadIdx.x);
  __syncthreads();
  const uint32_t g = threadIdx.x % G;
  const uint32_t group = (blockIdx.x * 256u + threadIdx.x) / G, n_groups = gridDim.x * 256u / G;
  const uint32_t n = min(P.S->n_lines, P.line_cap);
  for (uint32_t i = group; i < n; i += n_groups) {
    const uint32_t rl = P.len[i];
    if (!rl) continue;                                              // (refused by the size kernel)
    const uint64_t ro = P.recoff[i];
    const uint64_t beg = i ? (uint64_t)P.line_off[i - 1] + 1u : 0u;
    const SamMeta M = P.meta[i];
    const uint32_t *t = M.tab;
    const uint32_t len = M.len;
    // what the size kernel counted, again from the same numbers: the record's parts lie inside [ro, ro + rl), which lies inside the buffer
    bool sane = ro <= P.rec_cap && rl <= P.rec_cap - ro && beg + len <= P.bytes && t[10] <= len;
    for (int k = 0; k < 10 && sane; ++k) sane = t[k] < t[k + 1];
    const uint32_t ls = sane ? t[9] - t[8] - 1u : 0u;
    const uint8_t *L = P.T + beg;
    const uint32_t l_seq = sane && !(ls == 1u && L[t[8] + 1] == '*') ? ls : 0u;
    const uint32_t o_cig = 36u + t[0] + 1u, o_seq = o_cig + 4u * M.n_cig, o_qual = o_seq + (l_seq + 1u) / 2u, o_tags = o_qual + l_seq;
    sane = sane && sam_rec_len(t[0], M.n_cig, l_seq, M.tag_bytes) == rl && ((M.flags & SAM_F_NOQUAL) || t[10] - t[9] - 1u == l_seq);
    if (!sane) { if (g == 0) atomicMin(&P.S->err_line, (unsigned long long)i); continue; }
    uint8_t *R = P.rec + ro;
    uint32_t val = 0, e = 0;
    uint64_t u = 0;
    int64_t s = 0;
    int32_t id = -1;
    if (g == 1) { e = !sam_udec(L + t[0] + 1, t[1] - t[0] - 1, 65535, &u); val = (uint32_t)u; }
    else if (g == 2) { e = sam_ref_field(P.R, L + t[1] + 1, t[2] - t[1] - 1, false, -1, &id); val = (uint32_t)id; }
    else if (g == 3) { e = !sam_udec(L + t[2] + 1, t[3] - t[2] - 1, 2147483647, &u); val = (uint32_t)u - 1u; }
    else if (g == 4) { e = !sam_udec(L + t[3] + 1, t[4] - t[3] - 1, 255, &u); val = (uint32_t)u; }
    else if (g == 5) {
      uint32_t nc; uint64_t ref;
      e = sam_cigar(L + t[4] + 1, t[5] - t[4] - 1, R + o_cig, M.n_cig, &nc, &ref);
      if (nc != M.n_cig) e = 1;
      val = (uint32_t)min(ref, (uint64_t)0x80000000u);
    } else if (g == 6) {
      int32_t tid = -1;
      e = sam_ref_field(P.R, L + t[1] + 1, t[2] - t[1] - 1, false, -1, &tid);
      if (!e) e = sam_ref_field(P.R, L + t[5] + 1, t[6] - t[5] - 1, true, tid, &id);
      val = (uint32_t)id;
    } else if (g == 7) { e = !sam_udec(L + t[6] + 1, t[7] - t[6] - 1, 2147483647, &u); val = (uint32_t)u - 1u; }
    else if (g == 8) { e = !sam_sdec(L + t[7] + 1, t[8] - t[7] - 1, -2147483648ll, 2147483647ll, &s); val = (uint32_t)(int32_t)s; }
    else if (g == 9) {
      uint32_t nb = 0, nh = 0;
      if (t[10] < len) e = sam_tags<false>(L + t[10] + 1, len - t[10] - 1, R + o_tags, M.tag_bytes, &nb, &nh);
      if (nb != M.tag_bytes) e = 1;
      if (!e && nh) { const uint32_t at = atomicAdd(&P.S->n_fix, 1u); if (at < P.fix_cap) P.fix[at] = i; }
    }
    const uint32_t any = sam_group_min<G>(e ? 0u : 1u);
    SamPlan Q;
    Q.flag = __shfl(val, 1, G); Q.tid = (int32_t)__shfl(val, 2, G); Q.pos = (int32_t)__shfl(val, 3, G); Q.mapq = __shfl(val, 4, G);
    const uint32_t ref = __shfl(val, 5, G);
    Q.mtid = (int32_t)__shfl(val, 6, G); Q.mpos = (int32_t)__shfl(val, 7, G); Q.tlen = (int32_t)__shfl(val, 8, G);
    if (!any) { if (g == 0) atomicMin(&P.S->err_line, (unsigned long long)i); continue; }
    if (g == 0) {
      Q.l_qname = t[0]; Q.n_cig = M.n_cig; Q.l_seq = l_seq; Q.rec_len = rl;
      Q.bin = sam_bin(Q.pos, ref, Q.flag);
      sam_put_fixed(R, Q);
      R[36u + t[0]] = 0;
    }
    for (uint32_t k = g; k < t[0]; k += G) R[36u + k] = L[k];
    // SEQ: two codes a byte, high nibble first; a word of 16 bytes from 32 bases
    const uint64_t s0 = beg + t[8] + 1u;
    const uint8_t *Tx = P.T;
    sam_store_span<G>(R + o_seq, (l_seq + 1u) / 2u, g,
      [&](uint32_t k) -> uint8_t { return (uint8_t)(code[Tx[s0 + 2u * k]] << 4 | (2u * k + 1u < l_seq ? code[Tx[s0 + 2u * k + 1u]] : 0u)); },
      [&](uint32_t k) -> uint4 {
        // whole words only where all 32 bases exist: the span's tail takes the rest
        if (2u * k + 32u > l_seq) {
          uint32_t o[4] = {0, 0, 0, 0};
          for (uint32_t b = 0; b < 16u; ++b) {
            const uint32_t q = 2u * (k + b);
            const uint32_t c = (q < l_seq ? (uint32_t)code[Tx[s0 + q]] << 4 : 0u) | (q + 1u < l_seq ? (uint32_t)code[Tx[s0 + q + 1u]] : 0u);
            o[b >> 2] |= c << ((b & 3u) * 8u);
          }
          return make_uint4(o[0], o[1], o[2], o[3]);
        }
        const uint4 a = sam_ld16(Tx, s0 + 2u * k), b = sam_ld16(Tx, s0 + 2u * k + 16u);
        auto two = [&](uint32_t lo, uint32_t hi) {                   // 8 bases -> 4 bytes
          auto pair = [&](uint32_t w, uint32_t sft) { return (uint32_t)code[w >> sft & 0xffu] << 4 | (uint32_t)code[w >> (sft + 8u) & 0xffu]; };
          return pair(lo, 0) | pair(lo, 16) << 8 | pair(hi, 0) << 16 | pair(hi, 16) << 24;
        };
        return make_uint4(two(a.x, a.y), two(a.z, a.w), two(b.x, b.y), two(b.z, b.w));
      });
    // QUAL: minus 33 (no byte is below: the size kernel has looked), or 0xFF throughout
    const uint64_t q0 = beg + t[9] + 1u;
    if (M.flags & SAM_F_NOQUAL)
      sam_store_span<G>(R + o_qual, l_seq, g, [&](uint32_t) -> uint8_t { return 0xffu; }, [&](uint32_t) -> uint4 { return make_uint4(~0u, ~0u, ~0u, ~0u); });
    else
      sam_store_span<G>(R + o_qual, l_seq, g, [&](uint32_t k) -> uint8_t { return (uint8_t)(Tx[q0 + k] - 33u); },
        [&](uint32_t k) -> uint4 {
          const uint4 w = sam_ld16(Tx, q0 + k);
          auto sub = [](uint32_t x) { return x - 0x21212121u; };     // (every byte is at least 0x21: nothing is borrowed)
          return make_uint4(sub(w.x), sub(w.y), sub(w.z), sub(w.w));
        });
  }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------------
static uint32_t sam_lanes() {
  // lanes a line: STRL_SORT_SAM_LANES = 16 / 32 / 64 to measure again (profiles/sort_sam/README.md)
  const char *e = getenv("STRL_SORT_SAM_LANES");
  const int v = e ? atoi(e) : 16;
  return v == 32 || v == 64 ? (uint32_t)v : 16u;
}

int sam_parser_create(SamParser **out, const uint8_t *names, const uint32_t *name_off, int32_t n_ref, hipStream_t st) {
  SamParser *p = new SamParser();
  *out = p;
  int32_t dup = 0;
  if (!p->refs.build(names, name_off, n_ref, &dup)) { set_error("strl_bamsort_sam_begin: reference name %d occurs twice", dup); return STRL_ERR_FORMAT; }
  p->lanes = sam_lanes();
  int rc;
  const SamRefTable &T = p->refs;
  if ((rc = p->d_names.reserve(T.names.size() + 64)) || (rc = p->d_off.reserve(T.off.size() * 4 + 64)) || (rc = p->d_slot.reserve(T.slot.size() * 4 + 64))) return rc;
  if (!T.names.empty()) STRL_HIP(hipMemcpyAsync(p->d_names.p, T.names.data(), T.names.size(), hipMemcpyHostToDevice, st));
  STRL_HIP(hipMemcpyAsync(p->d_off.p, T.off.data(), T.off.size() * 4, hipMemcpyHostToDevice, st));
  STRL_HIP(hipMemcpyAsync(p->d_slot.p, T.slot.data(), T.slot.size() * 4, hipMemcpyHostToDevice, st));
  STRL_HIP(hipStreamSynchronize(st));
  p->d_refs = SamRefs{p->d_names.as<uint8_t>(), p->d_off.as<uint32_t>(), p->d_slot.as<int32_t>(), (uint32_t)T.slot.size() - 1u, n_ref};
  for (SamSlot &S : p->slot) {
    STRL_HIP(hipHostMalloc(reinterpret_cast<void **>(&S.h_info), sizeof(SamInfo), hipHostMallocDefault));
    STRL_HIP(hipEventCreate(&S.ev_copy));
    STRL_HIP(hipEventCreate(&S.ev_a));
    for (hipEvent_t &e : S.ev_t) STRL_HIP(hipEventCreate(&e));
    if ((rc = S.state.reserve(sizeof(SamInfo)))) return rc;
  }
  return STRL_OK;
}

void sam_parser_destroy(SamParser *p) {
  if (!p) return;
  for (SamSlot &S : p->slot) {
    if (S.h_info) (void)hipHostFree(S.h_info);
    if (S.ev_copy) (void)hipEventDestroy(S.ev_copy);
    if (S.ev_a) (void)hipEventDestroy(S.ev_a);
    for (hipEvent_t e : S.ev_t) if (e) (void)hipEventDestroy(e);
  }
  delete p;
}

int sam_parser_reserve(SamParser *p, uint64_t max_text) {
  if (!max_text || max_text > ((uint64_t)512 << 20)) { set_error("strl_bamsort_sam_reserve: a chunk holds 1 byte to 512 MiB of text (got %llu)", (unsigned long long)max_text); return STRL_ERR_ARG; }
  if (max_text <= p->max_text) return STRL_OK;
  // a valid line takes SAM_MIN_LINE bytes and its \n; a record at most 2 x its line + 36 bytes (a B array's ",1" becomes four bytes)
  const uint32_t line_cap = (uint32_t)(max_text / (SAM_MIN_LINE + 1u)) + 2u;
  const uint64_t rec_cap = 2u * max_text + 36ull * line_cap + 64u;
  const uint32_t n_tiles = (uint32_t)std::max<uint64_t>((max_text + SAM_TILE_BYTES - 1) / SAM_TILE_BYTES, (line_cap + SAM_SUM_TILE - 1) / SAM_SUM_TILE) + 1u;
  int rc;
  for (SamSlot &S : p->slot)
    if ((rc = S.text.reserve(max_text + 64)) || (rc = S.line_off.reserve((size_t)line_cap * 4 + 64)) || (rc = S.len.reserve((size_t)line_cap * 4 + 64)) ||
        (rc = S.meta.reserve((size_t)line_cap * sizeof(SamMeta) + 64)) || (rc = S.recoff.reserve((size_t)line_cap * 4 + 64)) || (rc = S.rec.reserve(rec_cap + 64)) ||
        (rc = S.tile.reserve((size_t)n_tiles * 4 + 64)) || (rc = S.fix.reserve((size_t)line_cap * 4 + 64)))
      return rc;
  p->max_text = max_text; p->line_cap = line_cap; p->rec_cap = rec_cap;
  return STRL_OK;
}

template <uint32_t G> static void sam_launch_size_encode(const SamChunk &C, unsigned grid, hipStream_t st, SamSlot &S, uint32_t n_sum_tiles) {
  hipLaunchKernelGGL(sam_size_kernel<G>, dim3(grid), dim3(256), 0, st, C);
  (void)hipEventRecord(S.ev_t[3], st);
  hipLaunchKernelGGL(sam_sum_kernel<false>, dim3(n_sum_tiles), dim3(256), 0, st, C.len, C.line_cap, S.tile.as<uint32_t>(), S.recoff.as<uint32_t>(), C.S);
  hipLaunchKernelGGL(sam_scan_kernel, dim3(1), dim3(1024), 0, st, S.tile.as<uint32_t>(), n_sum_tiles, C.S, 1, C.line_cap);
  hipLaunchKernelGGL(sam_sum_kernel<true>, dim3(n_sum_tiles), dim3(256), 0, st, C.len, C.line_cap, S.tile.as<uint32_t>(), S.recoff.as<uint32_t>(), C.S);
  (void)hipEventRecord(S.ev_t[4], st);
  hipLaunchKernelGGL(sam_encode_kernel<G>, dim3(grid), dim3(256), 0, st, C);
}

int sam_parser_enqueue(SamParser *p, int si, const uint8_t *text, uint64_t bytes, uint64_t line0, hipStream_t st) {
  if (!bytes || bytes > p->max_text || text[bytes - 1] != '\n') { set_error("strl_bamsort_push_sam: a chunk is whole lines, its last byte a newline, and at most what strl_bamsort_sam_reserve was told"); return STRL_ERR_ARG; }
  SamSlot &S = p->slot[si];
  S.text_bytes = bytes; S.line0 = line0;
  SamInfo *D = S.state.as<SamInfo>();
  SamInfo &H = *S.h_info;
  H = SamInfo{~0ull, 0, 0, 0, 0, 0};
  STRL_HIP(hipEventRecord(S.ev_t[0], st));
  STRL_HIP(hipMemcpyAsync(D, &H, sizeof H, hipMemcpyHostToDevice, st));
  STRL_HIP(hipMemcpyAsync(S.text.p, text, bytes, hipMemcpyHostToDevice, st));
  STRL_HIP(hipEventRecord(S.ev_copy, st));
  const uint32_t n_tiles = (uint32_t)((bytes + SAM_TILE_BYTES - 1) / SAM_TILE_BYTES);
  // the tables hold line_cap lines, but this chunk of `bytes` cannot hold more valid ones than this: the sums' grid follows it
  const uint32_t lines_here = (uint32_t)std::min<uint64_t>(p->line_cap, bytes / (SAM_MIN_LINE + 1u) + 2u);
  const uint32_t n_sum_tiles = (lines_here + SAM_SUM_TILE - 1) / SAM_SUM_TILE;
  STRL_HIP(hipEventRecord(S.ev_t[1], st));
  hipLaunchKernelGGL(sam_nl_kernel<false>, dim3(n_tiles), dim3(256), 0, st, S.text.as<uint8_t>(), bytes, S.tile.as<uint32_t>(), S.line_off.as<uint32_t>(), lines_here);
  hipLaunchKernelGGL(sam_scan_kernel, dim3(1), dim3(1024), 0, st, S.tile.as<uint32_t>(), n_tiles, D, 0, lines_here);
  hipLaunchKernelGGL(sam_nl_kernel<true>, dim3(n_tiles), dim3(256), 0, st, S.text.as<uint8_t>(), bytes, S.tile.as<uint32_t>(), S.line_off.as<uint32_t>(), lines_here);
  STRL_HIP(hipGetLastError());
  STRL_HIP(hipEventRecord(S.ev_t[2], st));
  const SamChunk C{S.text.as<uint8_t>(), bytes, S.line_off.as<uint32_t>(), lines_here, p->d_refs, S.len.as<uint32_t>(), S.meta.as<SamMeta>(), S.recoff.as<uint32_t>(),
                   S.rec.as<uint8_t>(), p->rec_cap, S.fix.as<uint32_t>(), lines_here, D};
  const uint32_t G = p->lanes;
  const unsigned grid = (unsigned)std::min<uint64_t>(4096, std::max<uint64_t>(1, ((uint64_t)lines_here * G + 255u) / 256u));
  if (G == 32) sam_launch_size_encode<32>(C, grid, st, S, n_sum_tiles);
  else if (G == 64) sam_launch_size_encode<64>(C, grid, st, S, n_sum_tiles);
  else sam_launch_size_encode<16>(C, grid, st, S, n_sum_tiles);
  STRL_HIP(hipGetLastError());
  STRL_HIP(hipEventRecord(S.ev_t[5], st));
  STRL_HIP(hipMemcpyAsync(&H, D, sizeof H, hipMemcpyDeviceToHost, st));
  STRL_HIP(hipEventRecord(S.ev_a, st));
  S.timed = true;
  STRL_HIP(hipEventSynchronize(S.ev_copy));      // the caller's text may be reused
  return STRL_OK;
}

// the chunk's text walked by the host's encoder up to its first refusal
static int sam_refuse(SamParser *p, SamSlot &S, hipStream_t st, unsigned long long device_line) {
  p->h_text.resize((size_t)S.text_bytes);
  STRL_HIP(hipMemcpyAsync(p->h_text.data(), S.text.p, S.text_bytes, hipMemcpyDeviceToHost, st));
  STRL_HIP(hipStreamSynchronize(st));
  const SamRefs R = p->refs.view();
  std::vector<uint8_t> rec;
  std::string why;
  uint64_t k = 0;
  for (size_t at = 0; at < p->h_text.size(); ++k) {
    const uint8_t *nl = static_cast<const uint8_t *>(memchr(p->h_text.data() + at, '\n', p->h_text.size() - at));
    const size_t end = nl ? (size_t)(nl - p->h_text.data()) : p->h_text.size();
    rec.clear();
    if (end - at > (size_t)SAM_LINE_MAX + 1u) why = sam_err_words(SAM_E_LONG_LINE);
    else if (!sam_encode_line(p->h_text.data() + at, (uint32_t)(end - at), R, rec, why)) why.clear();
    if (!why.empty()) { set_error("%s", sam_refusal(S.line0 + k + 1, why).c_str()); return STRL_ERR_FORMAT; }
    at = end + 1;
  }
  set_error("internal error: the device refused SAM line %llu, which the host's encoder accepts", S.line0 + device_line + 1);
  return STRL_ERR_ASSERT;
}

int sam_parser_collect(SamParser *p, int si, hipStream_t st, SamInfo *info) {
  SamSlot &S = p->slot[si];
  STRL_HIP(hipEventSynchronize(S.ev_a));
  const SamInfo I = *S.h_info;
  if (S.timed) {                                 // ev_t: 0 | copy | 1 | scan | 2 | size | 3 | sums | 4 | encode | 5 -- the size figure takes the sums in
    float ms[5] = {0, 0, 0, 0, 0};
    for (int k = 0; k < 5; ++k) if (hipEventElapsedTime(&ms[k], S.ev_t[k], S.ev_t[k + 1]) != hipSuccess) (void)hipGetLastError();
    p->fig.copy_ms += ms[0]; p->fig.scan_ms += ms[1]; p->fig.size_ms += ms[2] + ms[3]; p->fig.encode_ms += ms[4];
    S.timed = false;
  }
  if (I.overflow || I.err_line != ~0ull) return sam_refuse(p, S, st, I.err_line);
  if (I.total > p->rec_cap || I.n_fix > I.n_lines) { set_error("internal error: a SAM chunk's records take %llu bytes, past the slot's %llu", I.total, (unsigned long long)p->rec_cap); return STRL_ERR_ASSERT; }
  if (I.n_fix) {
    // the lines whose float values the fast path declined: the host encodes each and copies the record over its place
    const size_t n = I.n_lines;
    p->h_text.resize((size_t)S.text_bytes); p->h_rec.resize((size_t)I.total); p->h_fix.resize(I.n_fix); p->h_off.resize(n); p->h_recoff.resize(n);
    STRL_HIP(hipMemcpyAsync(p->h_text.data(), S.text.p, S.text_bytes, hipMemcpyDeviceToHost, st));
    STRL_HIP(hipMemcpyAsync(p->h_rec.data(), S.rec.p, I.total, hipMemcpyDeviceToHost, st));
    STRL_HIP(hipMemcpyAsync(p->h_fix.data(), S.fix.p, (size_t)I.n_fix * 4, hipMemcpyDeviceToHost, st));
    STRL_HIP(hipMemcpyAsync(p->h_off.data(), S.line_off.p, n * 4, hipMemcpyDeviceToHost, st));
    STRL_HIP(hipMemcpyAsync(p->h_recoff.data(), S.recoff.p, n * 4, hipMemcpyDeviceToHost, st));
    STRL_HIP(hipStreamSynchronize(st));
    std::sort(p->h_fix.begin(), p->h_fix.end());
    const SamRefs R = p->refs.view();
    std::vector<uint8_t> rec;
    std::string why;
    for (const uint32_t i : p->h_fix) {
      if (i >= n) { set_error("internal error: the host-finish list names line %u of %zu", i, n); return STRL_ERR_ASSERT; }
      const size_t beg = i ? (size_t)p->h_off[i - 1] + 1 : 0, end = p->h_off[i];
      rec.clear();
      if (end < beg || end > p->h_text.size()) { set_error("internal error: line table"); return STRL_ERR_ASSERT; }
      if (sam_encode_line(p->h_text.data() + beg, (uint32_t)(end - beg), R, rec, why)) { set_error("%s", sam_refusal(S.line0 + i + 1, why).c_str()); return STRL_ERR_FORMAT; }
      const size_t ro = p->h_recoff[i], next = (size_t)i + 1 < n ? p->h_recoff[i + 1] : (size_t)I.total;
      if (ro > next || next > p->h_rec.size() || rec.size() != next - ro) { set_error("internal error: SAM line %llu is %zu bytes on the host and %zu on the device", S.line0 + i + 1ull, rec.size(), next - ro); return STRL_ERR_ASSERT; }
      memcpy(p->h_rec.data() + ro, rec.data(), rec.size());
    }
    STRL_HIP(hipMemcpyAsync(S.rec.p, p->h_rec.data(), I.total, hipMemcpyHostToDevice, st));
    STRL_HIP(hipStreamSynchronize(st));
  }
  p->fig.lines += I.n_lines; p->fig.text_bytes += S.text_bytes; p->fig.host_finished += I.n_fix; ++p->fig.chunks;
  *info = I;
  return STRL_OK;
}

}  // namespace strl
