// assign.hip -- strl_assign_reads_loci_device: loci given with -l / -b take their reads on the device (gfx950).  The rule and the
// kernels' bodies: assign_core.h.  The host function (call_logic.cpp strl_assign_reads_loci) groups the treads in a hash table,
// sorts every group and erases from a vector once per locus; here the treads are sorted once by (group, position, input order)
// with the clustering path's key layout, every locus finds its range by binary search, and only the taking itself is
// sequential -- per group, one wave each:
//   upload -> check (largest tid, units) -> [host reads 16 bytes] -> keys -> radix sort (sort.hip) -> gather
//          -> loci keys -> radix sort -> ranges -> take -> scan -> fill -> marks -> [host reads the results]
// Two host synchronisations a call: the key's width comes from the largest tid, the results are the second.
#include <string.h>
#include <algorithm>
#include <chrono>
#include <vector>
#include "common.h"
#include "sort.h"
#include "assign_core.h"

namespace strl {

constexpr uint32_t AS_TB = 256;
constexpr uint32_t AS_MAX_WAVES = 1u << 20;     // waves of a take / fill launch at most: they stride over the loci

__global__ __launch_bounds__(AS_TB) void assign_check_kernel(AsParams P) {
  int32_t tid = -1;
  uint32_t err = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * AS_TB + threadIdx.x; i < P.n; i += (uint64_t)gridDim.x * AS_TB) {
    const int32_t t = as_check_body(P, (uint32_t)i, err);
    tid = t > tid ? t : tid;
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    const int32_t o = __shfl_xor(tid, d);
    tid = o > tid ? o : tid;
    err |= (uint32_t)__shfl_xor((int)err, d);
  }
  if ((threadIdx.x & 63u) == 0) {
    if (tid > -1) atomicMax(&P.stat->max_tid, tid);
    if (err) atomicOr(&P.stat->err, err);
  }
}
__global__ __launch_bounds__(AS_TB) void assign_keys_kernel(AsParams P) {
  const uint32_t i = blockIdx.x * AS_TB + threadIdx.x;
  if (i < P.n) as_keys_body(P, i);
}
__global__ __launch_bounds__(AS_TB) void assign_regather_kernel(AsParams P, const uint32_t *perm, uint64_t *out) {
  const uint32_t i = blockIdx.x * AS_TB + threadIdx.x;
  if (i < P.n) out[i] = P.gk_in[perm[i]];
}
__global__ __launch_bounds__(AS_TB) void assign_gather_kernel(AsParams P) {
  const uint32_t i = blockIdx.x * AS_TB + threadIdx.x;
  if (i < P.n) as_gather_body(P, i);
}
__global__ __launch_bounds__(AS_TB) void assign_lkeys_kernel(AsParams P) {
  const uint32_t j = blockIdx.x * AS_TB + threadIdx.x;
  if (j < P.n_loci) as_lkeys_body(P, j);
}
__global__ __launch_bounds__(AS_TB) void assign_ranges_kernel(AsParams P) {
  const uint32_t k = blockIdx.x * AS_TB + threadIdx.x;
  if (k < P.n_loci) as_ranges_body(P, k);
}
// one wave a workgroup: the barrier between two loci of a group is the workgroup's
__global__ __launch_bounds__(AS_WAVE) void assign_take_kernel(AsParams P) {
  for (uint32_t k = blockIdx.x; k < P.n_loci; k += gridDim.x) as_take_body(AsWave{threadIdx.x}, P, k);
}
__global__ __launch_bounds__(AS_SCAN_MAX) void assign_scan_kernel(AsParams P) {
  __shared__ uint64_t sh[AS_SCAN_MAX];
  as_scan_body(AsBlock{threadIdx.x, blockDim.x}, P, sh);
}
__global__ __launch_bounds__(AS_WAVE) void assign_fill_kernel(AsParams P) {
  for (uint32_t j = blockIdx.x; j < P.n_loci; j += gridDim.x) as_fill_body(AsWave{threadIdx.x}, P, j);
}
__global__ __launch_bounds__(AS_TB) void assign_marks_kernel(AsParams P) {
  const uint32_t i = blockIdx.x * AS_TB + threadIdx.x;
  if (i < P.n) as_marks_body(P, i);
}

static inline int bits_for(uint64_t v) { int b = 1; while (b < 64 && (v >> b)) ++b; return b; }

enum { A_TREADS, A_LOCI, A_KEY0, A_KEY1, A_VAL0, A_VAL1, A_GK, A_SORT, A_DN, A_SG, A_SPOS, A_SSPLIT, A_OWNER, A_LKEY0, A_LKEY1, A_LVAL0, A_LVAL1,
       A_RANGE, A_CNT, A_OFF, A_ASSIGNED, A_MARK, A_STAT, A_N };
static_assert(A_N <= (int)(sizeof(((strl_ctx *)nullptr)->as_buf) / sizeof(DevBuf)), "strl_ctx::as_buf is too short");

}  // namespace strl

using namespace strl;

extern "C" int strl_assign_reads_loci_device(strl_ctx *c, strl_tread *treads, uint64_t n64, int mode, strl_locus *loci, uint64_t n_loci64,
                                             uint64_t *assigned_off, uint32_t *assigned, uint64_t cap) {
  if (!c || (n64 && !treads) || (n_loci64 && (!loci || !assigned_off))) { set_error("null argument"); return STRL_ERR_ARG; }
  if (n64 > 0x7ffffff0ull) { set_error("too many treads"); return STRL_ERR_ARG; }
  if (n_loci64 > 0x7ffffff0ull) { set_error("too many loci"); return STRL_ERR_ARG; }
  const auto t0 = std::chrono::steady_clock::now();
  const uint32_t n = (uint32_t)n64, n_loci = (uint32_t)n_loci64;
  c->as_info = strl_assign_info{};
  c->as_info.n_loci = n_loci;
  if (n_loci == 0) return STRL_OK;
  if (n == 0) {                                          // nothing to take: every locus counts zero reads
    for (uint32_t j = 0; j < n_loci; ++j) { loci[j].b.n_total = 0; loci[j].b.n_left = 0; loci[j].b.n_right = 0; assigned_off[j] = 0; }
    assigned_off[n_loci] = 0;
    return STRL_OK;
  }
  STRL_HIP(hipSetDevice(c->device));
  DevBuf *B = c->as_buf;
  hipStream_t st = c->stream;
  int rc;
  auto need = [&](int i, size_t bytes) { return B[i].reserve(std::max<size_t>(bytes, 256)); };
  const uint32_t m = std::max(n, n_loci);
  const size_t sb = radix_sort_scratch_bytes(m, 64);
  if ((rc = need(A_TREADS, (size_t)n * sizeof(strl_tread))) || (rc = need(A_LOCI, (size_t)n_loci * sizeof(AsLocus))) || (rc = need(A_KEY0, (size_t)n * 8)) ||
      (rc = need(A_KEY1, (size_t)n * 8)) || (rc = need(A_VAL0, (size_t)n * 4)) || (rc = need(A_VAL1, (size_t)n * 4)) || (rc = need(A_SORT, sb)) ||
      (rc = need(A_DN, 256)) || (rc = need(A_SG, (size_t)n * 8)) || (rc = need(A_SPOS, (size_t)n * 4)) || (rc = need(A_SSPLIT, n)) ||
      (rc = need(A_OWNER, (size_t)n * 4)) || (rc = need(A_LKEY0, (size_t)n_loci * 8)) || (rc = need(A_LKEY1, (size_t)n_loci * 8)) ||
      (rc = need(A_LVAL0, (size_t)n_loci * 4)) || (rc = need(A_LVAL1, (size_t)n_loci * 4)) || (rc = need(A_RANGE, (size_t)n_loci * 12)) ||
      (rc = need(A_CNT, (size_t)n_loci * 12)) || (rc = need(A_OFF, ((size_t)n_loci + 1) * 8)) || (rc = need(A_MARK, n)) || (rc = need(A_STAT, sizeof(AsStat))) ||
      (assigned && (rc = need(A_ASSIGNED, (size_t)n * 4))))
    return rc;
  std::vector<AsLocus> hl(n_loci);
  for (uint32_t j = 0; j < n_loci; ++j) {
    const strl_bounds &b = loci[j].b;
    hl[j].tid = b.tid; hl[j].left_most = b.left_most; hl[j].right_most = b.right_most;
    memset(hl[j].rep, 0, sizeof hl[j].rep);
    memcpy(hl[j].rep, b.repeat, strnlen(b.repeat, 6));
  }
  const uint32_t dn[2] = {n, n_loci};
  const AsStat s0{0u, -1, 0u, 0u};
  STRL_HIP(hipMemcpyAsync(B[A_TREADS].p, treads, (size_t)n * sizeof(strl_tread), hipMemcpyHostToDevice, st));
  STRL_HIP(hipMemcpyAsync(B[A_LOCI].p, hl.data(), (size_t)n_loci * sizeof(AsLocus), hipMemcpyHostToDevice, st));
  STRL_HIP(hipMemcpyAsync(B[A_DN].p, dn, sizeof dn, hipMemcpyHostToDevice, st));
  STRL_HIP(hipMemcpyAsync(B[A_STAT].p, &s0, sizeof s0, hipMemcpyHostToDevice, st));
  AsParams P{};
  P.treads = B[A_TREADS].as<strl_tread>(); P.n = n; P.mode = mode;
  P.loci = B[A_LOCI].as<AsLocus>(); P.n_loci = n_loci;
  P.stat = B[A_STAT].as<AsStat>();
  const uint32_t nb = (n + AS_TB - 1u) / AS_TB, lb = (n_loci + AS_TB - 1u) / AS_TB;
  hipLaunchKernelGGL(assign_check_kernel, dim3(std::min(nb, 4096u)), dim3(AS_TB), 0, st, P);
  STRL_HIP(hipGetLastError());
  AsStat hs;
  STRL_HIP(hipMemcpyAsync(&hs, P.stat, sizeof hs, hipMemcpyDeviceToHost, st));
  STRL_HIP(hipStreamSynchronize(st));
  if (hs.err & AS_E_UNIT) { set_error("a tread's repeat unit is not a NUL-padded ACGT string"); return STRL_ERR_ARG; }
  if (hs.err & AS_E_TID) { set_error("a tread's tid is below -1"); return STRL_ERR_ARG; }
  // ---- treads: keys, sort, the sorted columns ------------------------------------------------------------------------
  const uint64_t top = (uint64_t)(uint32_t)(hs.max_tid + 1);
  const int kbits = bits_for(top) + 15;
  P.max_tid = hs.max_tid;
  P.excl = (top << 15) | (7ull << 12);                   // (no unit has 7 letters)
  P.composite = kbits <= 32 ? 1 : 0;
  P.key = B[A_KEY0].as<uint64_t>(); P.val = B[A_VAL0].as<uint32_t>();
  if (!P.composite) { if ((rc = need(A_GK, (size_t)n * 8))) return rc; P.gk_in = B[A_GK].as<uint64_t>(); }
  hipLaunchKernelGGL(assign_keys_kernel, dim3(nb), dim3(AS_TB), 0, st, P);
  uint64_t *sk = nullptr;
  uint32_t *sv = nullptr;
  const uint32_t *d_n = B[A_DN].as<uint32_t>();
  int e = radix_sort_pairs(st, d_n, n, B[A_KEY0].as<uint64_t>(), B[A_VAL0].as<uint32_t>(), B[A_KEY1].as<uint64_t>(), B[A_VAL1].as<uint32_t>(), B[A_SORT].p,
                           B[A_SORT].cap, 0, P.composite ? 32 + kbits : 32, &sk, &sv);
  if (!e && !P.composite) {                              // stable by position, then stable by group
    uint64_t *ok = sk == B[A_KEY0].as<uint64_t>() ? B[A_KEY1].as<uint64_t>() : B[A_KEY0].as<uint64_t>();
    uint32_t *ov = sv == B[A_VAL0].as<uint32_t>() ? B[A_VAL1].as<uint32_t>() : B[A_VAL0].as<uint32_t>();
    hipLaunchKernelGGL(assign_regather_kernel, dim3(nb), dim3(AS_TB), 0, st, P, sv, sk);
    e = radix_sort_pairs(st, d_n, n, sk, sv, ok, ov, B[A_SORT].p, B[A_SORT].cap, 0, kbits, &sk, &sv);
  }
  if (e) { set_error("radix_sort_pairs failed: %s", hipGetErrorString((hipError_t)e)); return STRL_ERR_HIP; }
  P.skey = sk; P.sval = sv;
  P.s_g = B[A_SG].as<uint64_t>(); P.s_pos = B[A_SPOS].as<uint32_t>(); P.s_split = B[A_SSPLIT].as<uint8_t>(); P.owner = B[A_OWNER].as<uint32_t>();
  hipLaunchKernelGGL(assign_gather_kernel, dim3(nb), dim3(AS_TB), 0, st, P);
  // ---- loci: keys, sort, ranges -----------------------------------------------------------------------------
  P.lkey = B[A_LKEY0].as<uint64_t>(); P.lval = B[A_LVAL0].as<uint32_t>();
  hipLaunchKernelGGL(assign_lkeys_kernel, dim3(lb), dim3(AS_TB), 0, st, P);
  uint64_t *slk = nullptr;
  uint32_t *slv = nullptr;
  e = radix_sort_pairs(st, d_n + 1, n_loci, B[A_LKEY0].as<uint64_t>(), B[A_LVAL0].as<uint32_t>(), B[A_LKEY1].as<uint64_t>(), B[A_LVAL1].as<uint32_t>(),
                       B[A_SORT].p, B[A_SORT].cap, 0, kbits, &slk, &slv);
  if (e) { set_error("radix_sort_pairs failed: %s", hipGetErrorString((hipError_t)e)); return STRL_ERR_HIP; }
  P.slkey = slk; P.slval = slv;
  P.p0 = B[A_RANGE].as<uint32_t>(); P.p1 = P.p0 + n_loci; P.ge = P.p1 + n_loci;
  P.cnt = B[A_CNT].as<uint32_t>(); P.off = B[A_OFF].as<uint64_t>();
  P.assigned = assigned ? B[A_ASSIGNED].as<uint32_t>() : nullptr; P.mark = B[A_MARK].as<uint8_t>();
  hipLaunchKernelGGL(assign_ranges_kernel, dim3(lb), dim3(AS_TB), 0, st, P);
  // ---- take, offsets, lists, marks --------------------------------------------------------------------------
  const uint32_t waves = std::min(n_loci, AS_MAX_WAVES);
  hipLaunchKernelGGL(assign_take_kernel, dim3(waves), dim3(AS_WAVE), 0, st, P);
  hipLaunchKernelGGL(assign_scan_kernel, dim3(1), dim3(AS_SCAN_MAX), 0, st, P);
  if (assigned) hipLaunchKernelGGL(assign_fill_kernel, dim3(waves), dim3(AS_WAVE), 0, st, P);
  hipLaunchKernelGGL(assign_marks_kernel, dim3(nb), dim3(AS_TB), 0, st, P);
  STRL_HIP(hipGetLastError());
  std::vector<uint32_t> cnt((size_t)n_loci * 3);
  std::vector<uint8_t> mark(n);
  STRL_HIP(hipMemcpyAsync(cnt.data(), P.cnt, (size_t)n_loci * 12, hipMemcpyDeviceToHost, st));
  STRL_HIP(hipMemcpyAsync(assigned_off, P.off, ((size_t)n_loci + 1) * 8, hipMemcpyDeviceToHost, st));
  STRL_HIP(hipMemcpyAsync(mark.data(), P.mark, n, hipMemcpyDeviceToHost, st));
  STRL_HIP(hipMemcpyAsync(&hs, P.stat, sizeof hs, hipMemcpyDeviceToHost, st));
  STRL_HIP(hipStreamSynchronize(st));
  const uint64_t tot = assigned_off[n_loci];
  if (tot > n) { set_error("strl_assign_reads_loci_device: %llu reads assigned of %u", (unsigned long long)tot, n); return STRL_ERR_HIP; }
  if (assigned && std::min(tot, cap)) STRL_HIP(hipMemcpy(assigned, P.assigned, (size_t)std::min(tot, cap) * 4, hipMemcpyDeviceToHost));
  for (uint32_t j = 0; j < n_loci; ++j) {                // (uint16 fields: they wrap as the host function's do)
    strl_bounds &b = loci[j].b;
    b.n_total = (uint16_t)cnt[j]; b.n_left = (uint16_t)cnt[(size_t)n_loci + j]; b.n_right = (uint16_t)cnt[2 * (size_t)n_loci + j];
  }
  for (uint32_t i = 0; i < n; ++i) if (mark[i]) treads[i].split = STRL_SOFT_TAKEN;
  c->as_info.n_groups = hs.n_groups; c->as_info.n_assigned = tot; c->as_info.n_lost = hs.n_lost;
  c->as_info.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  if (assigned && tot > cap) { set_error("assigned capacity %llu too small, need %llu", (unsigned long long)cap, (unsigned long long)tot); return STRL_ERR_CAPACITY; }
  return STRL_OK;
}

extern "C" int strl_assign_info_last(strl_ctx *c, strl_assign_info *info) {
  if (!c || !info) { set_error("null argument"); return STRL_ERR_ARG; }
  *info = c->as_info;
  return STRL_OK;
}
