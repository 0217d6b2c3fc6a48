// outliers.hip -- the statistics of the reference's outlier stage (scripts/strling-outliers.py, "the script") on gfx950.
//
// Everything is fp64 with IEEE division and sqrt (no fast-math), no floating-point atomics, and every reduction runs in a
// fixed order, so two runs give the same bits.  Four stages, each a C ABI entry point (include/strling_amd.h):
//
//   * row medians (:247, :281-282, :296): one workgroup per row; exact selection by an 8-bit radix select on the
//     order-preserving 64-bit image of the doubles (integer LDS histograms), NaN skipped; an even count takes the mean of
//     the two middle values as numpy's median does.
//   * Huber's proposal 2 per locus row (hubers_est :115-136 = statsmodels 0.12.2 robust.scale.Huber(maxiter=1000)): one
//     workgroup per row.  Rows of at most OUT_LDS_CAP finite values are compacted (in order, by a ballot scan) into LDS;
//     wider rows are read from global memory in place (the wide path).  The fixed-point loop restates _estimate_both
//     element by element and raises the script's fallback where numpy would have warned: every divide-by-zero, invalid
//     or overflow event leaves a non-finite intermediate behind, and any non-finite intermediate means MAD.
//   * z / p / BH (:138-141, :359-404): z and p elementwise (p = scipy's ndtr(-z) structure); Benjamini-Hochberg per sample
//     column over the finite p values through two stable radix sorts (sort.hip: p bits, then column), then one workgroup
//     per column for p / (k / n) and the reverse cumulative minimum.
//   * output order (:451): two stable radix sorts of descending-with-NaN-last keys (allele2_est, then outlier) over the
//     (sample, locus) enumeration, so ties keep sample-name, then locus order.
#include "common.h"
#include "device_util.h"
#include "sort.h"

#include <math.h>

namespace strl {
namespace {

constexpr int OT = 256;                              // threads per workgroup (4 waves)
constexpr uint32_t OUT_LDS_CAP = 4096;               // finite values of one row held in LDS (32 KiB); wider rows: global path
constexpr double HUBER_C = 1.5;
constexpr double HUBER_TOL = 1.0e-08;
constexpr int HUBER_MAXITER = 1000;
// statsmodels Huber.gamma = tmp + c^2 (1 - tmp) - 2 c pdf(c), tmp = 2 cdf(c) - 1, c = 1.5: its bits as statsmodels computes them
constexpr double HUBER_GAMMA = 0x1.8e92fe2915f98p-1;
constexpr double MAD_C = 0.6744897501960817;         // robust.mad's c = norm.ppf(3/4)

__device__ __forceinline__ uint64_t ord_key(double d) {          // ascending order of doubles as unsigned integers
  const uint64_t u = (uint64_t)__double_as_longlong(d == 0.0 ? 0.0 : d);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double ord_val(uint64_t k) {
  const uint64_t u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  return __longlong_as_double((long long)u);
}
// descending, NaN after everything (sort_values(ascending=False), na_position='last')
__device__ __forceinline__ uint64_t desc_key(double d) { return d != d ? ~0ull : ~ord_key(d); }

// block-wide sum in a fixed order: every thread's partial, a shuffle tree per wave, the four wave sums in order
__device__ double block_sum(double v, double *sh) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) sh[w] = v;
  __syncthreads();
  const double r = ((sh[0] + sh[1]) + sh[2]) + sh[3];
  __syncthreads();
  return r;
}
__device__ uint32_t block_count(uint32_t v, uint32_t *sh) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) sh[w] = v;
  __syncthreads();
  const uint32_t r = sh[0] + sh[1] + sh[2] + sh[3];
  __syncthreads();
  return r;
}
__device__ bool block_any(bool b, uint32_t *sh) { return block_count(b ? 1u : 0u, sh) != 0; }

struct SelShared {
  uint32_t hist[256];
  uint32_t red[4];
  uint32_t digit, rank;
  double dred[4];
};

// k-th smallest (0-based) of the values get(i) for i in [0, m) that are not NaN: 8 passes of 8-bit digits, MSB first.
// The caller guarantees k < number of non-NaN values.
template <class Get>
__device__ double block_select(const Get &get, uint32_t m, uint32_t k, SelShared &S) {
  uint64_t prefix = 0, mask = 0;
  if (threadIdx.x == 0) S.rank = k;
  for (int shift = 56; shift >= 0; shift -= 8) {
    S.hist[threadIdx.x] = 0;
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < m; i += OT) {
      const double v = get(i);
      if (v != v) continue;
      const uint64_t key = ord_key(v);
      if ((key & mask) == prefix) atomicAdd(&S.hist[(uint32_t)(key >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      uint32_t r = S.rank, d = 0;
      for (; d < 255; ++d) {
        if (r < S.hist[d]) break;
        r -= S.hist[d];
      }
      S.digit = d;
      S.rank = r;
    }
    __syncthreads();
    prefix |= (uint64_t)S.digit << shift;
    mask |= 255ull << shift;
    __syncthreads();
  }
  return ord_val(prefix);
}

// np.median of the n non-NaN values among get(i), i in [0, m)
template <class Get>
__device__ double block_median(const Get &get, uint32_t m, uint32_t n, SelShared &S) {
  if (n == 0) return __longlong_as_double(0x7ff8000000000000ll);
  if (n & 1u) return block_select(get, m, n / 2, S);
  const double a = block_select(get, m, n / 2 - 1, S), b = block_select(get, m, n / 2, S);
  return (a + b) / 2.0;
}

// ---------------------------------------------------------------- row medians (depth medians :247, :281-282, :296)
// Per row r: m_all = median of the non-NaN x; with keep (per column, may be null = all): m_kept = median over kept columns
// with 0 -> NaN (:280-282); m_filled = median over kept columns of the value with NaN / 0 filled by m_kept (:296).
__global__ __launch_bounds__(OT) void row_medians_kernel(const double *x, uint64_t rows, uint64_t cols, const uint8_t *keep,
                                                         double *m_all, double *m_kept, double *m_filled) {
  __shared__ SelShared S;
  const uint64_t r = blockIdx.x;
  if (r >= rows) return;
  const double *row = x + r * cols;
  const uint32_t m = (uint32_t)cols;
  const double NaN = __longlong_as_double(0x7ff8000000000000ll);
  auto all = [&](uint32_t i) { return row[i]; };
  auto kept = [&](uint32_t i) { const double v = row[i]; return (keep && !keep[i]) || v == 0.0 ? NaN : v; };
  uint32_t c0 = 0, c1 = 0;
  for (uint32_t i = threadIdx.x; i < m; i += OT) { c0 += all(i) == all(i); c1 += kept(i) == kept(i); }
  const uint32_t n0 = block_count(c0, S.red), n1 = block_count(c1, S.red);
  const double a = block_median(all, m, n0, S);
  const double b = block_median(kept, m, n1, S);
  auto filled = [&](uint32_t i) { if (keep && !keep[i]) return NaN; const double v = kept(i); return v == v ? v : b; };
  uint32_t c2 = 0;
  for (uint32_t i = threadIdx.x; i < m; i += OT) c2 += filled(i) == filled(i);
  const uint32_t n2 = block_count(c2, S.red);
  const double c = block_median(filled, m, n2, S);
  if (threadIdx.x == 0) {
    if (m_all) m_all[r] = a;
    if (m_kept) m_kept[r] = b;
    if (m_filled) m_filled[r] = c;
  }
}

// ---------------------------------------------------------------- Huber (hubers_est :115-136)
__device__ __forceinline__ bool fin(double v) { return isfinite(v); }

template <bool WIDE>
__global__ __launch_bounds__(OT) void huber_kernel(const double *x, uint64_t rows, uint64_t cols, double *mu_out, double *sd_out,
                                                   uint8_t *method_out) {
  __shared__ SelShared S;
  __shared__ double vals[WIDE ? 1 : OUT_LDS_CAP];
  __shared__ uint32_t wbase[4];
  const uint64_t r = blockIdx.x;
  if (r >= rows) return;
  const double *row = x + r * cols;
  const double NaN = __longlong_as_double(0x7ff8000000000000ll);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  uint32_t m;      // elements get() ranges over
  uint32_t n;      // finite (non-NaN) values: the x of :120
  if (!WIDE) {
    // compact the non-NaN values into LDS, in column order (ballot scan per 256-column chunk)
    uint32_t base = 0;
    for (uint64_t c0 = 0; c0 < cols; c0 += OT) {
      const uint64_t c = c0 + threadIdx.x;
      const double v = c < cols ? row[c] : NaN;
      const bool keepv = v == v;
      const unsigned long long b = __ballot(keepv);
      if (lane == 0) wbase[w] = (uint32_t)__popcll(b);
      __syncthreads();
      uint32_t off = base;
      for (int q = 0; q < w; ++q) off += wbase[q];
      const uint32_t tot = wbase[0] + wbase[1] + wbase[2] + wbase[3];
      if (keepv) vals[off + (uint32_t)__popcll(b & ((1ull << lane) - 1ull))] = v;
      base += tot;
      __syncthreads();
    }
    m = n = base;
  } else {
    m = (uint32_t)cols;
    uint32_t cnt = 0;
    for (uint32_t i = threadIdx.x; i < m; i += OT) cnt += row[i] == row[i];
    n = block_count(cnt, S.red);
  }
  auto get = [&](uint32_t i) -> double { return WIDE ? row[i] : vals[i]; };
  if (n == 0) {            // (the script stops here: np.median of an empty array warns inside its handler)
    if (threadIdx.x == 0) { mu_out[r] = NaN; sd_out[r] = NaN; method_out[r] = 1; }
    return;
  }
  const double med = block_median(get, m, n, S);
  auto dev = [&](uint32_t i) -> double { const double v = get(i); return v == v ? fabs(v - med) / MAD_C : NaN; };
  const double mad = block_median(dev, m, n, S);

  // statsmodels Huber._estimate_both, est_mu, norm=None
  const double c = HUBER_C;
  const double nm1 = (double)(n - 1), len = (double)n;
  double mu = med, scale = mad;
  bool bad = false, done = false;
  double rmu = NaN, rs = NaN;
  for (int it = 0; it < HUBER_MAXITER && !bad && !done; ++it) {
    // (a - mu) / scale over a non-empty array: scale == 0 divides by zero (or 0 / 0)
    if (scale == 0.0) { bad = true; break; }
    const double cs = c * scale, lo = mu - cs, hi = mu + cs;
    if (!fin(cs) || !fin(lo) || !fin(hi)) { bad = true; break; }
    double part = 0.0;
    uint32_t card = 0;
    bool nf = false;
    for (uint32_t i = threadIdx.x; i < m; i += OT) {
      const double v = get(i);
      if (v != v) continue;
      part += fmin(fmax(v, lo), hi);                                   // np.clip(a, mu - c s, mu + c s)
      const double t = fabs((v - mu) / scale);
      nf |= !fin(t);
      card += t <= c;                                                  // subset: the OLD mu and scale
    }
    const double sum = block_sum(part, S.dred);
    const uint32_t cardall = block_count(card, S.red);
    const double nmu = sum / len;
    double part2 = 0.0;
    for (uint32_t i = threadIdx.x; i < m; i += OT) {
      const double v = get(i);
      if (v != v) continue;
      const double d = v - nmu, d2 = d * d;
      nf |= !fin(d2);
      if (fabs((v - mu) / scale) <= c) part2 += d2;                    // subset * (a - nmu) ** 2
    }
    const double num = block_sum(part2, S.dred);
    if (block_any(nf, S.red) || !fin(sum) || !fin(nmu) || !fin(num)) { bad = true; break; }
    const double den = nm1 * HUBER_GAMMA - (len - (double)cardall) * (c * c);
    const double q = num / den;
    if (!fin(q) || q < 0.0) { bad = true; break; }                      // x / 0, 0 / 0, sqrt of a negative (not of -0.0)
    const double ns = sqrt(q);
    if (fabs(scale - ns) <= ns * HUBER_TOL && fabs(mu - nmu) <= ns * HUBER_TOL) { rmu = nmu; rs = ns; done = true; break; }
    mu = nmu;
    scale = ns;
  }
  if (threadIdx.x == 0) {
    double omu, os;
    uint8_t meth;
    if (done) { omu = rmu; os = rs; meth = 0; }
    else { omu = med; os = mad; meth = 1; }                            // :128-132 (no convergence: ValueError)
    if (os == 0.0) os = NaN;                                           // :133-134
    mu_out[r] = omu;
    sd_out[r] = os;
    method_out[r] = meth;
  }
}

// ---------------------------------------------------------------- z, p (:138-141, :381 / :395)
__device__ __forceinline__ double norm_sf(double z) {      // scipy.special.ndtr(-z)
  if (z != z) return z;
  const double t = -z * 0.70710678118654752440;
  const double a = fabs(t);
  double y;
  if (a < 0.70710678118654752440) y = 0.5 + 0.5 * erf(t);
  else {
    // cephes erfc (scipy's) returns 0 once exp(-a^2) underflows, -a^2 < -MAXLOG: no subnormal tail, as the script prints it
    y = a * a > 7.09782712893383996843e2 ? 0.0 : 0.5 * erfc(a);
    if (t > 0) y = 1.0 - y;
  }
  return y;
}

// rows 0 .. rows-1: x[r, s] against (mu[r], sd[r]); rows .. rows + n_null - 1: the control-only rows, null_x[s] (NaN when
// null_x is null) against (null_mu[j], null_sd[j]).  Writes z, p and p_adj = p (BH overwrites the finite ones) for all,
// BH keys (p bits; non-finite last) and values (flat index).
__global__ void z_p_kernel(const double *x, const double *mu, const double *sd, uint64_t rows, uint64_t cols, const double *null_x,
                           const double *null_mu, const double *null_sd, uint64_t n_null, double *z, double *p, double *padj, uint64_t *keys,
                           uint32_t *vals) {
  const uint64_t n = (rows + n_null) * cols;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t r = i / cols, s = i - r * cols;
    double v, m, d;
    if (r < rows) { v = x[i]; m = mu[r]; d = sd[r]; }
    else { v = null_x ? null_x[s] : __longlong_as_double(0x7ff8000000000000ll); m = null_mu[r - rows]; d = null_sd[r - rows]; }
    const double zz = (v - m) / d;
    const double pp = norm_sf(zz);
    z[i] = zz;
    p[i] = pp;
    padj[i] = pp;
    keys[i] = isfinite(pp) ? (uint64_t)__double_as_longlong(pp == 0.0 ? 0.0 : pp) : ~0ull;   // p >= 0: bits ascend with value
    vals[i] = (uint32_t)i;
  }
}

__global__ void column_key_kernel(const uint32_t *vals, uint64_t n, uint64_t cols, uint64_t *keys) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
    keys[i] = vals[i] % cols;
}

// one workgroup per column: its R entries sit at [s R, (s + 1) R) of the sorted order, finite p first, ascending.
// fdrcorrection: raw_k = p_k / ((k + 1) / n), reverse cumulative minimum, > 1 -> 1, scattered back (:167).
__global__ __launch_bounds__(OT) void bh_kernel(const uint32_t *vals, const double *p, uint64_t R, uint64_t cols, double *padj) {
  __shared__ uint32_t red[4];
  __shared__ double wmin[4];
  __shared__ double carry_sh;
  const uint64_t s = blockIdx.x;
  if (s >= cols) return;
  const uint32_t *seg = vals + s * R;
  uint32_t cnt = 0;
  for (uint64_t k = threadIdx.x; k < R; k += OT) cnt += isfinite(p[seg[k]]);
  const uint32_t nf = block_count(cnt, red);
  if (nf == 0) return;
  const double nd = (double)nf;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  double carry = __longlong_as_double(0x7ff0000000000000ll);     // +inf
  const uint64_t nchunks = ((uint64_t)nf + OT - 1) / OT;
  for (uint64_t ch = nchunks; ch-- > 0;) {
    const uint64_t k = ch * OT + threadIdx.x;
    const uint32_t idx = k < nf ? seg[k] : 0u;
    double v = k < nf ? p[idx] / ((double)(k + 1) / nd) : __longlong_as_double(0x7ff0000000000000ll);
    // inclusive suffix minimum inside the wave (lanes above), then across waves (waves above), then the carry
    for (int o = 1; o < 64; o <<= 1) {
      const double u = __shfl_down(v, o);
      if (lane + o < 64) v = fmin(v, u);
    }
    if (lane == 0) wmin[w] = v;
    __syncthreads();
    for (int q = w + 1; q < 4; ++q) v = fmin(v, wmin[q]);
    v = fmin(v, carry);
    if (k < nf) padj[idx] = v > 1.0 ? 1.0 : v;
    if (threadIdx.x == 0) carry_sh = v;                                // thread 0 holds the minimum of the whole chunk
    __syncthreads();
    carry = carry_sh;
    __syncthreads();
  }
}

// ---------------------------------------------------------------- order (:451)
// enumeration v = s * rows + r (sample, then locus); key of a cell = desc_key of `a` at (r, s)
__global__ void order_init_kernel(const double *a, uint64_t rows, uint64_t cols, uint64_t *keys, uint32_t *vals) {
  const uint64_t n = rows * cols;
  for (uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; v < n; v += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t s = v / rows, r = v - s * rows;
    keys[v] = desc_key(a[r * cols + s]);
    vals[v] = (uint32_t)v;
  }
}
__global__ void order_rekey_kernel(const double *a, uint64_t rows, uint64_t cols, const uint32_t *vals, uint64_t *keys) {
  const uint64_t n = rows * cols;
  for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t v = vals[k], s = v / rows, r = v - s * rows;
    keys[k] = desc_key(a[r * cols + s]);
  }
}
__global__ void order_out_kernel(const uint32_t *vals, uint64_t rows, uint64_t cols, uint32_t *order) {
  const uint64_t n = rows * cols;
  for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t v = vals[k], s = v / rows, r = v - s * rows;
    order[k] = (uint32_t)(r * cols + s);
  }
}

inline unsigned grid_for(uint64_t n) {
  const uint64_t b = (n + OT - 1) / OT;
  return (unsigned)(b < 1 ? 1 : (b > 65536 ? 65536 : b));
}

// host or device arrays: device views of the inputs (copied in when host), outputs written back when host
struct Io {
  strl_ctx *c;
  int mem;
  std::vector<DevBuf> owned;
  template <typename T> int in(const T *h, size_t n, const T **d) {
    if (!h || mem == STRL_MEM_DEVICE) { *d = h; return STRL_OK; }
    owned.emplace_back();
    DevBuf &s = owned.back();
    int rc = s.reserve(n * sizeof(T));
    if (rc) return rc;
    STRL_HIP(hipMemcpyAsync(s.p, h, n * sizeof(T), hipMemcpyHostToDevice, c->stream));
    *d = s.as<T>();
    return STRL_OK;
  }
  template <typename T> int out(T *h, size_t n, T **d) {
    if (!h || mem == STRL_MEM_DEVICE) { *d = h; return STRL_OK; }
    owned.emplace_back();
    DevBuf &s = owned.back();
    int rc = s.reserve(n * sizeof(T));
    if (rc) return rc;
    *d = s.as<T>();
    return STRL_OK;
  }
  template <typename T> int back(T *h, const T *d, size_t n) {
    if (!h || mem == STRL_MEM_DEVICE || !n) return STRL_OK;
    STRL_HIP(hipMemcpyAsync(h, d, n * sizeof(T), hipMemcpyDeviceToHost, c->stream));
    return STRL_OK;
  }
};

int bits_for(uint64_t n) {       // bits that hold 0 .. n - 1
  int b = 0;
  while (b < 64 && (1ull << b) < n) ++b;
  return b;
}

// stable sort of (keys, vals)[0, n) by key bits [0, bits) (sort.hip), result back in (keys, vals)
int sort_in_place(strl_ctx *c, uint64_t *&keys, uint32_t *&vals, uint64_t *&k_alt, uint32_t *&v_alt, uint64_t n, int bits, DevBuf &scratch,
                  DevBuf &dn) {
  if (bits <= 0 || n <= 1) return STRL_OK;
  const size_t sb = radix_sort_scratch_bytes((uint32_t)n, bits);
  int rc;
  if ((rc = scratch.reserve(sb))) return rc;
  const uint32_t n32 = (uint32_t)n;
  STRL_HIP(hipMemcpyAsync(dn.p, &n32, 4, hipMemcpyHostToDevice, c->stream));
  uint64_t *ok = nullptr;
  uint32_t *ov = nullptr;
  const int e = radix_sort_pairs(c->stream, dn.as<uint32_t>(), n32, keys, vals, k_alt, v_alt, scratch.p, sb, 0, bits, &ok, &ov);
  if (e) { set_error("radix_sort_pairs failed: %s", hipGetErrorString((hipError_t)e)); return STRL_ERR_HIP; }
  if (ok != keys) { std::swap(keys, k_alt); std::swap(vals, v_alt); }
  // the host copy of n32 above must outlive the enqueued copy
  STRL_HIP(hipStreamSynchronize(c->stream));
  return STRL_OK;
}

bool huber_wide_forced() {
  static const bool f = getenv("STRL_OUTLIERS_WIDE") && getenv("STRL_OUTLIERS_WIDE")[0] == '1';
  return f;
}

}  // namespace
}  // namespace strl

using namespace strl;

extern "C" int strl_dev_alloc(strl_ctx *c, uint64_t bytes, void **p) {
  if (!c || !p) { set_error("null argument"); return STRL_ERR_ARG; }
  *p = nullptr;
  STRL_HIP(hipSetDevice(c->device));
  const hipError_t e = hipMalloc(p, bytes ? bytes : 8);
  if (e != hipSuccess) { *p = nullptr; set_error("hipMalloc(%llu) failed: %s", (unsigned long long)bytes, hipGetErrorString(e)); return STRL_ERR_NOMEM; }
  return STRL_OK;
}

extern "C" int strl_dev_free(strl_ctx *c, void *p) {
  if (!c) { set_error("null argument"); return STRL_ERR_ARG; }
  if (p) STRL_HIP(hipFree(p));
  return STRL_OK;
}

extern "C" int strl_copy(strl_ctx *c, void *dst, const void *src, uint64_t bytes, int to_device) {
  if (!c || (bytes && (!dst || !src))) { set_error("null argument"); return STRL_ERR_ARG; }
  if (!bytes) return STRL_OK;
  STRL_HIP(hipMemcpyAsync(dst, src, bytes, to_device ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost, c->stream));
  STRL_HIP(hipStreamSynchronize(c->stream));
  return STRL_OK;
}

extern "C" int strl_outliers_row_medians(strl_ctx *c, const double *x, uint64_t rows, uint64_t cols, const uint8_t *keep, double *m_all,
                                         double *m_kept, double *m_filled, int mem) {
  if (!c || (!x && rows * cols)) { set_error("null argument"); return STRL_ERR_ARG; }
  if (cols > 0xffffffffull) { set_error("rows wider than 2^32 - 1"); return STRL_ERR_ARG; }
  if (!rows) return STRL_OK;
  STRL_HIP(hipSetDevice(c->device));
  Io io{c, mem, {}};
  const double *dx;
  const uint8_t *dk;
  double *da, *db, *dc;
  int rc;
  if ((rc = io.in(x, rows * cols, &dx)) || (rc = io.in(keep, cols, &dk)) || (rc = io.out(m_all, rows, &da)) || (rc = io.out(m_kept, rows, &db)) ||
      (rc = io.out(m_filled, rows, &dc)))
    return rc;
  hipLaunchKernelGGL(row_medians_kernel, dim3((unsigned)rows), dim3(OT), 0, c->stream, dx, rows, cols, dk, da, db, dc);
  STRL_HIP(hipGetLastError());
  if ((rc = io.back(m_all, da, rows)) || (rc = io.back(m_kept, db, rows)) || (rc = io.back(m_filled, dc, rows))) return rc;
  STRL_HIP(hipStreamSynchronize(c->stream));
  return STRL_OK;
}

extern "C" int strl_outliers_huber(strl_ctx *c, const double *x, uint64_t rows, uint64_t cols, double *mu, double *sd, uint8_t *method,
                                   int mem) {
  if (!c || (!x && rows * cols) || (rows && (!mu || !sd || !method))) { set_error("null argument"); return STRL_ERR_ARG; }
  if (cols > 0xffffffffull) { set_error("rows wider than 2^32 - 1"); return STRL_ERR_ARG; }
  if (!rows) return STRL_OK;
  STRL_HIP(hipSetDevice(c->device));
  Io io{c, mem, {}};
  const double *dx;
  double *dm, *ds;
  uint8_t *dt;
  int rc;
  if ((rc = io.in(x, rows * cols, &dx)) || (rc = io.out(mu, rows, &dm)) || (rc = io.out(sd, rows, &ds)) || (rc = io.out(method, rows, &dt)))
    return rc;
  if (cols > OUT_LDS_CAP || huber_wide_forced())
    hipLaunchKernelGGL(huber_kernel<true>, dim3((unsigned)rows), dim3(OT), 0, c->stream, dx, rows, cols, dm, ds, dt);
  else
    hipLaunchKernelGGL(huber_kernel<false>, dim3((unsigned)rows), dim3(OT), 0, c->stream, dx, rows, cols, dm, ds, dt);
  STRL_HIP(hipGetLastError());
  if ((rc = io.back(mu, dm, rows)) || (rc = io.back(sd, ds, rows)) || (rc = io.back(method, dt, rows))) return rc;
  STRL_HIP(hipStreamSynchronize(c->stream));
  return STRL_OK;
}

extern "C" int strl_outliers_scores(strl_ctx *c, const double *x, const double *mu, const double *sd, uint64_t rows, uint64_t cols,
                                    const double *null_x, const double *null_mu, const double *null_sd, uint64_t n_null, double *z, double *p,
                                    double *p_adj, int mem) {
  if (!c || (rows * cols && (!x || !mu || !sd || !z || !p || !p_adj)) || (n_null && (!null_mu || !null_sd))) {
    set_error("null argument");
    return STRL_ERR_ARG;
  }
  const uint64_t R = rows + n_null, n = R * cols;
  if (n > 0x7fffffffull) { set_error("%llu cells: more than the sort takes (2^31 - 1)", (unsigned long long)n); return STRL_ERR_ARG; }
  if (!rows || !cols) return STRL_OK;
  STRL_HIP(hipSetDevice(c->device));
  Io io{c, mem, {}};
  const double *dx, *dm, *ds, *dnx, *dnm, *dns;
  double *dz, *dp, *dq;
  int rc;
  if ((rc = io.in(x, rows * cols, &dx)) || (rc = io.in(mu, rows, &dm)) || (rc = io.in(sd, rows, &ds)) || (rc = io.in(null_x, cols, &dnx)) ||
      (rc = io.in(null_mu, n_null, &dnm)) || (rc = io.in(null_sd, n_null, &dns)))
    return rc;
  // z / p / p_adj of the control-only rows are computed but not returned: they only count in BH
  DevBuf zb, pb, qb, k0, k1, v0, v1, scratch, dn;
  if ((rc = zb.reserve(n * 8)) || (rc = pb.reserve(n * 8)) || (rc = qb.reserve(n * 8)) || (rc = k0.reserve(n * 8)) || (rc = k1.reserve(n * 8)) ||
      (rc = v0.reserve(n * 4)) || (rc = v1.reserve(n * 4)) || (rc = dn.reserve(256)))
    return rc;
  dz = zb.as<double>(); dp = pb.as<double>(); dq = qb.as<double>();
  uint64_t *keys = k0.as<uint64_t>(), *ka = k1.as<uint64_t>();
  uint32_t *vals = v0.as<uint32_t>(), *va = v1.as<uint32_t>();
  hipLaunchKernelGGL(z_p_kernel, dim3(grid_for(n)), dim3(OT), 0, c->stream, dx, dm, ds, rows, cols, dnx, dnm, dns, n_null, dz, dp, dq, keys, vals);
  STRL_HIP(hipGetLastError());
  // BH (one locus: p / (1 / 1) = p, the script's unadjusted branch :377-386 comes out the same).  By p (64 key bits,
  // non-finite = all ones, last), then stably by column: every column's R entries end up together, in p order.
  if ((rc = sort_in_place(c, keys, vals, ka, va, n, 64, scratch, dn))) return rc;
  hipLaunchKernelGGL(column_key_kernel, dim3(grid_for(n)), dim3(OT), 0, c->stream, vals, n, cols, keys);
  STRL_HIP(hipGetLastError());
  if ((rc = sort_in_place(c, keys, vals, ka, va, n, bits_for(cols), scratch, dn))) return rc;
  hipLaunchKernelGGL(bh_kernel, dim3((unsigned)cols), dim3(OT), 0, c->stream, vals, dp, R, cols, dq);
  STRL_HIP(hipGetLastError());
  const size_t bytes = rows * cols * 8;      // the first `rows` rows are the caller's
  const hipMemcpyKind kind = mem == STRL_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  STRL_HIP(hipMemcpyAsync(z, dz, bytes, kind, c->stream));
  STRL_HIP(hipMemcpyAsync(p, dp, bytes, kind, c->stream));
  STRL_HIP(hipMemcpyAsync(p_adj, dq, bytes, kind, c->stream));
  STRL_HIP(hipStreamSynchronize(c->stream));
  return STRL_OK;
}

extern "C" int strl_outliers_order(strl_ctx *c, const double *outlier, const double *allele2, uint64_t rows, uint64_t cols, uint32_t *order,
                                   int mem) {
  if (!c || (rows * cols && (!outlier || !allele2 || !order))) { set_error("null argument"); return STRL_ERR_ARG; }
  const uint64_t n = rows * cols;
  if (n > 0x7fffffffull) { set_error("%llu cells: more than the sort takes (2^31 - 1)", (unsigned long long)n); return STRL_ERR_ARG; }
  if (!n) return STRL_OK;
  STRL_HIP(hipSetDevice(c->device));
  Io io{c, mem, {}};
  const double *dz, *da;
  uint32_t *dord;
  int rc;
  if ((rc = io.in(outlier, n, &dz)) || (rc = io.in(allele2, n, &da)) || (rc = io.out(order, n, &dord))) return rc;
  DevBuf k0, k1, v0, v1, scratch, dn;
  if ((rc = k0.reserve(n * 8)) || (rc = k1.reserve(n * 8)) || (rc = v0.reserve(n * 4)) || (rc = v1.reserve(n * 4)) || (rc = dn.reserve(256)))
    return rc;
  uint64_t *keys = k0.as<uint64_t>(), *ka = k1.as<uint64_t>();
  uint32_t *vals = v0.as<uint32_t>(), *va = v1.as<uint32_t>();
  // LSD: the secondary key (allele2_est) first, then the primary (outlier); both stable over (sample, locus)
  hipLaunchKernelGGL(order_init_kernel, dim3(grid_for(n)), dim3(OT), 0, c->stream, da, rows, cols, keys, vals);
  STRL_HIP(hipGetLastError());
  if ((rc = sort_in_place(c, keys, vals, ka, va, n, 64, scratch, dn))) return rc;
  hipLaunchKernelGGL(order_rekey_kernel, dim3(grid_for(n)), dim3(OT), 0, c->stream, dz, rows, cols, vals, keys);
  STRL_HIP(hipGetLastError());
  if ((rc = sort_in_place(c, keys, vals, ka, va, n, 64, scratch, dn))) return rc;
  hipLaunchKernelGGL(order_out_kernel, dim3(grid_for(n)), dim3(OT), 0, c->stream, vals, rows, cols, dord);
  STRL_HIP(hipGetLastError());
  if ((rc = io.back(order, dord, n))) return rc;
  STRL_HIP(hipStreamSynchronize(c->stream));
  return STRL_OK;
}
