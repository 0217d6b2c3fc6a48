// deflate.hip -- the BGZF compressor on the GPU (gfx950): the output side of `strling pull --deflate=device`
// (extract_region.nim:70-80 writes its BAM through htslib, i.e. zlib on the host).
//
//   deflate_dense_kernel : the same with the dense rule (DflDense: chains in a head table and a ring of links, ~125 KB of LDS)
//   deflate_kernel : ONE WORKGROUP of 256 per BGZF block of <= 0xFF00 input bytes, the whole rule of deflate_core.h with the
//                    block's bytes, the hash table, the histograms and the code tables in LDS (DflWork: ~107 KB, one
//                    workgroup per CU).  The tokens of the greedy parse go to a scratch in HBM, one slice per workgroup; the
//                    bits of the dynamic form are OR-ed together in LDS over the block's bytes and leave in one pass.
//                    Members land in slots n + 31 bytes apart, their sizes in csize[].
//   pack_kernel    : a workgroup per member: the slots' bytes back to back, once the host has summed the sizes.
// The host twin (strl_bgzf_deflate_host) runs the same header with a team of one and writes the same bytes.
#include <algorithm>
#include "common.h"
#include "deflate_core.h"

namespace strl {

constexpr uint32_t DFL_THREADS = 256;
constexpr uint32_t DFL_MAX_GRID = 512;          // workgroups of a launch (each owns a token slice); blocks beyond are taken in turn

struct DflGroup {
  static constexpr uint32_t N = DFL_THREADS;
  static constexpr bool IN_ORDER = false;      // lanes side by side
  __device__ __forceinline__ uint32_t tid() const { return threadIdx.x; }
  __device__ __forceinline__ void sync() const { __syncthreads(); }
  __device__ __forceinline__ void max_u32(uint32_t *p, uint32_t v) const { atomicMax(p, v); }
  __device__ __forceinline__ void or_u32(uint32_t *p, uint32_t v) const { atomicOr(p, v); }
  __device__ __forceinline__ void xor_u32(uint32_t *p, uint32_t v) const { atomicXor(p, v); }
};
static_assert(DFL_THREADS == DFL_BATCH, "a lane per position of a batch");

struct DeflateParams {
  const uint8_t *in;
  uint64_t in_bytes;
  uint32_t block_bytes, n_blocks;
  uint32_t *tok;             // [gridDim.x][block_bytes]
  uint8_t *slots;            // [n_blocks][stride]
  uint64_t stride;           // >= block_bytes + 31
  uint32_t *csize;           // [n_blocks] member size | stored << 31
  const DflCrc *crc;
};

template <class Rule>
__device__ __forceinline__ void deflate_blocks(const DeflateParams &P) {
  __shared__ DflWorkT<Rule> W;
  const DflGroup T;
  for (uint32_t k = blockIdx.x; k < P.n_blocks; k += gridDim.x) {
    const uint64_t off = (uint64_t)k * P.block_bytes;
    if (off >= P.in_bytes) break;
    const uint64_t left = P.in_bytes - off;
    const uint32_t n = left < P.block_bytes ? (uint32_t)left : P.block_bytes;
    uint32_t stored = 0;
    const uint32_t size = dfl_block(T, W, *P.crc, P.in + off, n, P.tok + (uint64_t)blockIdx.x * P.block_bytes, P.slots + (uint64_t)k * P.stride, &stored);
    if (threadIdx.x == 0) P.csize[k] = size | stored << 31;
    __syncthreads();
  }
}
__global__ __launch_bounds__(DFL_THREADS) void deflate_kernel(DeflateParams P) { deflate_blocks<DflFast>(P); }
__global__ __launch_bounds__(DFL_THREADS) void deflate_dense_kernel(DeflateParams P) { deflate_blocks<DflDense>(P); }

__global__ __launch_bounds__(256) void deflate_pack_kernel(const uint8_t *slots, uint64_t stride, const uint32_t *csize, const uint64_t *at, uint32_t n_blocks, uint8_t *out,
                                                           uint64_t out_bytes) {
  for (uint32_t k = blockIdx.x; k < n_blocks; k += gridDim.x) {
    const uint32_t size = csize[k] & 0x7fffffffu;
    const uint64_t o = at[k];
    if (size > stride || o + size > out_bytes) continue;
    const uint8_t *src = slots + (uint64_t)k * stride;
    for (uint32_t i = threadIdx.x; i < size; i += 256u) out[o + i] = src[i];
  }
}

}  // namespace strl

using namespace strl;

extern "C" uint64_t strl_bgzf_deflate_bound(uint64_t in_bytes, uint32_t block_bytes) {
  return block_bytes >= 1u && block_bytes <= DFL_MAX_BLOCK ? dfl_bound(in_bytes, block_bytes) : 0;
}

static int deflate_refusal(int rc, uint64_t in_bytes, uint32_t block_bytes, uint64_t out_cap) {
  if (rc == STRL_ERR_CAPACITY) set_error("bgzf deflate: %llu output bytes may be needed, room for %llu", (unsigned long long)dfl_bound(in_bytes, block_bytes), (unsigned long long)out_cap);
  else if (rc == STRL_ERR_ARG) set_error(block_bytes < 1u || block_bytes > DFL_MAX_BLOCK ? "bgzf deflate: block_bytes must be in [1, 0xFF00]" : "null argument");
  return rc;
}

static bool deflate_mode_ok(int mode) {
  if (mode == STRL_DEFLATE_FAST || mode == STRL_DEFLATE_DENSE) return true;
  set_error("bgzf deflate: mode %d is neither STRL_DEFLATE_FAST nor STRL_DEFLATE_DENSE", mode);
  return false;
}

extern "C" int strl_bgzf_deflate_host(const uint8_t *in, uint64_t in_bytes, uint32_t block_bytes, uint8_t *out, uint64_t out_cap, uint64_t *out_bytes, uint32_t *csize,
                                      uint32_t *n_stored) {
  return deflate_refusal(dfl_deflate_host(in, in_bytes, block_bytes, out, out_cap, out_bytes, csize, n_stored), in_bytes, block_bytes, out_cap);
}
extern "C" int strl_bgzf_deflate_host_mode(int mode, const uint8_t *in, uint64_t in_bytes, uint32_t block_bytes, uint8_t *out, uint64_t out_cap, uint64_t *out_bytes,
                                           uint32_t *csize, uint32_t *n_stored) {
  if (!deflate_mode_ok(mode)) return STRL_ERR_ARG;
  return deflate_refusal(dfl_deflate_host_mode(mode, in, in_bytes, block_bytes, out, out_cap, out_bytes, csize, n_stored), in_bytes, block_bytes, out_cap);
}

// strl_bgzf_deflate; on_device: `in` lies on the context's device already (written on its stream): no copy in
static int deflate_run(strl_ctx *c, int mode, const uint8_t *in, bool on_device, uint64_t in_bytes, uint32_t block_bytes, uint8_t *out, uint64_t out_cap, uint64_t *out_bytes,
                       uint32_t *csize, uint32_t *n_stored) {
  if (!c) { set_error("null argument"); return STRL_ERR_ARG; }
  if (!deflate_mode_ok(mode)) return STRL_ERR_ARG;
  if (block_bytes < 1u || block_bytes > DFL_MAX_BLOCK || !out_bytes || (in_bytes && (!in || !out))) return deflate_refusal(STRL_ERR_ARG, in_bytes, block_bytes, out_cap);
  if (out_cap < dfl_bound(in_bytes, block_bytes)) return deflate_refusal(STRL_ERR_CAPACITY, in_bytes, block_bytes, out_cap);
  *out_bytes = 0;
  if (n_stored) *n_stored = 0;
  c->deflate_ms = 0;
  if (!in_bytes) return STRL_OK;
  const uint64_t nb64 = (in_bytes + block_bytes - 1) / block_bytes;
  if (nb64 > 0x7fffffffull) { set_error("bgzf deflate: %llu blocks in one call", (unsigned long long)nb64); return STRL_ERR_ARG; }
  const uint32_t nb = (uint32_t)nb64, grid = std::min(nb, DFL_MAX_GRID);
  const uint64_t stride = ((uint64_t)block_bytes + DFL_MEMBER_EXTRA + 15) & ~(uint64_t)15;
  STRL_HIP(hipSetDevice(c->device));
  int rc;
  if ((!on_device && (rc = c->dfl_in.reserve(in_bytes + 16))) || (rc = c->dfl_slots.reserve(nb * stride)) || (rc = c->dfl_tok.reserve((size_t)grid * block_bytes * 4)) ||
      (rc = c->dfl_meta.reserve((size_t)nb * 12 + 64)))
    return rc;
  hipStream_t st = c->stream;
  if (!c->dfl_crc.p) {
    if ((rc = c->dfl_crc.reserve(sizeof(DflCrc)))) return rc;
    if (hipMemcpy(c->dfl_crc.p, &dfl_crc_tables(), sizeof(DflCrc), hipMemcpyHostToDevice) != hipSuccess) { c->dfl_crc.release(); set_error("bgzf deflate: CRC tables"); return STRL_ERR_HIP; }
  }
  uint64_t *d_at = c->dfl_meta.as<uint64_t>();
  uint32_t *d_csize = reinterpret_cast<uint32_t *>(d_at + nb);
  hipEvent_t ev[4];
  for (hipEvent_t &e : ev) STRL_HIP(hipEventCreate(&e));
  auto drop_events = [&] { for (hipEvent_t &e : ev) (void)hipEventDestroy(e); };
  auto fail = [&](hipError_t e, const char *what) { set_error("bgzf deflate: %s failed: %s", what, hipGetErrorString(e)); drop_events(); return STRL_ERR_HIP; };
  hipError_t he;
  if (!on_device && (he = hipMemcpyAsync(c->dfl_in.p, in, in_bytes, hipMemcpyHostToDevice, st)) != hipSuccess) return fail(he, "copy in");
  DeflateParams P{on_device ? in : c->dfl_in.as<uint8_t>(), in_bytes, block_bytes, nb, c->dfl_tok.as<uint32_t>(), c->dfl_slots.as<uint8_t>(), stride, d_csize, c->dfl_crc.as<DflCrc>()};
  (void)hipEventRecord(ev[0], st);
  if (mode == STRL_DEFLATE_DENSE) hipLaunchKernelGGL(deflate_dense_kernel, dim3(grid), dim3(DFL_THREADS), 0, st, P);
  else hipLaunchKernelGGL(deflate_kernel, dim3(grid), dim3(DFL_THREADS), 0, st, P);
  if ((he = hipGetLastError()) != hipSuccess) return fail(he, "deflate_kernel");
  (void)hipEventRecord(ev[1], st);
  std::vector<uint32_t> cs(nb);
  if ((he = hipMemcpyAsync(cs.data(), d_csize, (size_t)nb * 4, hipMemcpyDeviceToHost, st)) != hipSuccess) return fail(he, "copy sizes");
  if ((he = hipStreamSynchronize(st)) != hipSuccess) return fail(he, "deflate_kernel");
  std::vector<uint64_t> at(nb);
  uint64_t total = 0;
  uint32_t stored = 0;
  for (uint32_t k = 0; k < nb; ++k) {
    const uint32_t size = cs[k] & 0x7fffffffu;
    if (size < 18u + 8u || size > stride) { drop_events(); set_error("bgzf deflate: member %u of %u bytes", k, size); return STRL_ERR_ASSERT; }
    at[k] = total;
    total += size;
    stored += cs[k] >> 31;
  }
  if (total > out_cap) { drop_events(); set_error("bgzf deflate: %llu bytes, room for %llu", (unsigned long long)total, (unsigned long long)out_cap); return STRL_ERR_CAPACITY; }
  if ((rc = c->dfl_pack.reserve(total + 16))) { drop_events(); return rc; }
  if ((he = hipMemcpyAsync(d_at, at.data(), (size_t)nb * 8, hipMemcpyHostToDevice, st)) != hipSuccess) return fail(he, "copy offsets");
  (void)hipEventRecord(ev[2], st);
  hipLaunchKernelGGL(deflate_pack_kernel, dim3(std::min<uint32_t>(nb, 4096u)), dim3(256), 0, st, c->dfl_slots.as<uint8_t>(), stride, d_csize, d_at, nb, c->dfl_pack.as<uint8_t>(), total);
  if ((he = hipGetLastError()) != hipSuccess) return fail(he, "deflate_pack_kernel");
  (void)hipEventRecord(ev[3], st);
  if ((he = hipMemcpyAsync(out, c->dfl_pack.p, total, hipMemcpyDeviceToHost, st)) != hipSuccess) return fail(he, "copy out");
  if ((he = hipStreamSynchronize(st)) != hipSuccess) return fail(he, "deflate_pack_kernel");
  float a = 0.f, b = 0.f;
  (void)hipEventElapsedTime(&a, ev[0], ev[1]);
  (void)hipEventElapsedTime(&b, ev[2], ev[3]);
  c->deflate_ms = (double)a + (double)b;
  drop_events();
  if (csize) for (uint32_t k = 0; k < nb; ++k) csize[k] = cs[k] & 0x7fffffffu;
  if (n_stored) *n_stored = stored;
  *out_bytes = total;
  return STRL_OK;
}

extern "C" int strl_bgzf_deflate(strl_ctx *c, const uint8_t *in, uint64_t in_bytes, uint32_t block_bytes, uint8_t *out, uint64_t out_cap, uint64_t *out_bytes,
                                 uint32_t *csize, uint32_t *n_stored) {
  return deflate_run(c, STRL_DEFLATE_FAST, in, false, in_bytes, block_bytes, out, out_cap, out_bytes, csize, n_stored);
}
extern "C" int strl_bgzf_deflate_mode(strl_ctx *c, int mode, const uint8_t *in, uint64_t in_bytes, uint32_t block_bytes, uint8_t *out, uint64_t out_cap,
                                      uint64_t *out_bytes, uint32_t *csize, uint32_t *n_stored) {
  return deflate_run(c, mode, in, false, in_bytes, block_bytes, out, out_cap, out_bytes, csize, n_stored);
}
int strl::bgzf_deflate_device(strl_ctx *c, int mode, const uint8_t *d_in, uint64_t in_bytes, uint32_t block_bytes, uint8_t *out, uint64_t out_cap, uint64_t *out_bytes,
                              uint32_t *csize, uint32_t *n_stored) {
  return deflate_run(c, mode, d_in, true, in_bytes, block_bytes, out, out_cap, out_bytes, csize, n_stored);
}

// HIP-event time (ms) of the kernels of the last strl_bgzf_deflate call on this context (copies excluded).
extern "C" int strl_ctx_deflate_ms(strl_ctx *c, double *ms) {
  if (!c || !ms) return STRL_ERR_ARG;
  *ms = c->deflate_ms;
  return STRL_OK;
}
