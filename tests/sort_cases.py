"""Cases for the device radix sort (strling_amd/csrc/sort.hip) as the pipelines call it, their reference and a model.

tests/test_sort.py sends random keys through strl_sort_pairs: *d_n == n, a fresh and exactly sized scratch, the sort zeroes its
own tables.  The callers do otherwise: the count lives on the device and may be 0 or exceed n_max (pair.hip's emit counter),
the scratch is dirty from the batch before, its chunk tables are zeroed by the caller (radix_sort_tables + zero_words2), and
sorts of different pass counts are chained on one scratch without a sync (cluster.hip, assign.hip).  The cases here reach
those, the ends of the bit window and the digit patterns random 64-bit keys never form.  Every size derives from the constants
of sort.h, read by regex.

  reference(case)   numpy's stable argsort of the masked field over the first min(d_n, n_max) elements, stage after stage
  model(case, v)    one pass as the kernels do it -- per-tile rows H, per-chunk rows C, `below` and `tot` from "chunk rows
                    before mine plus tile rows of my chunk before me", digit bases, in-wave rank by peer group -- on a scratch
                    of words that starts out poisoned; v names a deliberate mistake (VARIANTS).  A restatement for tests: it
                    shows on the CPU that the case list would catch such a mistake (tests/test_sort_cases.py); no mutated
                    kernel ever runs.

tests/test_sort_edges_device.py runs every case through strl_sort_probe on the GPU.
"""
import collections
import functools
import os
import re
import zlib

import numpy as np

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "strling_amd", "csrc")


def _const(text, name):
    m = re.search(r"constexpr uint32_t %s = ([^;]+);" % name, text)
    if not m:
        raise AssertionError("tests/sort_cases.py: %s not found in sort.h: the sort changed, restate the cases" % name)
    return m.group(1).strip()


_HDR = open(os.path.join(CSRC, "sort.h")).read()
SORT_THREADS = int(_const(_HDR, "SORT_THREADS"))
SORT_KPT = int(_const(_HDR, "SORT_KPT"))
SORT_CHUNK = int(_const(_HDR, "SORT_CHUNK"))
assert _const(_HDR, "SORT_TILE") == "SORT_THREADS * SORT_KPT", "sort.h: SORT_TILE is no longer SORT_THREADS * SORT_KPT"
SORT_TILE = SORT_THREADS * SORT_KPT
WAVE = 64
WAVES = SORT_THREADS // WAVE            # waves of a tile
SHARE = SORT_KPT * WAVE                 # consecutive keys of a tile one wave owns
T, CT = SORT_TILE, SORT_CHUNK * SORT_TILE
ROW = 256 * 4                           # bytes of one histogram row
M32, M64 = (1 << 32) - 1, (1 << 64) - 1
HIP_INVALID = 1                         # hipErrorInvalidValue

Case = collections.namedtuple("Case", "name keys vals alt_keys alt_vals cap d_n n_max stages skew delta poison meta")


def div_up(a, b):
    return (a + b - 1) // b


# ---- sort.h's formulas, restated ---------------------------------------------------------------------------------------------
def passes(bits):
    return (bits + 7) // 8


def tiles_chunks(n_max):
    nt = div_up(n_max if n_max else 1, T)
    return nt, div_up(nt, SORT_CHUNK)


def scratch_bytes(n_max, bits):
    nt, nc = tiles_chunks(n_max)
    return max(passes(bits), 1) * (nt + nc) * ROW + 256


def tables_region(skew, n_max, bits):
    """(offset from the scratch pointer, bytes) of the chunk tables, the scratch pointer being `skew` past a 256-byte boundary"""
    if bits <= 0 or n_max == 0:
        return -1, 0
    return (-skew) % 256, passes(bits) * tiles_chunks(n_max)[1] * ROW


def used_end(skew, n_max, bits):
    """offset from the scratch pointer of the end of everything a sort touches: chunk tables, then tile tables"""
    nt, nc = tiles_chunks(n_max)
    return (-skew) % 256 + passes(bits) * (nc + nt) * ROW


# ---- keys ---------------------------------------------------------------------------------------------------------------
def _rng(name):
    return np.random.Generator(np.random.Philox(key=[zlib.crc32(name.encode()), 11]))


def _u64(rng, n):
    return rng.integers(0, 1 << 32, size=n, dtype=np.uint64) << np.uint64(32) | rng.integers(0, 1 << 32, size=n, dtype=np.uint64)


def field_of(keys, lo, bits):
    if bits == 0:
        return np.zeros(keys.size, np.uint64)
    f = keys >> np.uint64(lo)
    return f & np.uint64((1 << bits) - 1) if bits < 64 else f


def compose(field, lo, bits, first=0):
    """keys with `field` in bits [lo, lo + bits) and, in every other bit, the DESCENDING element index: a sort that looked
    outside its window would reverse the ties, and the index makes every key a name for its element"""
    n = field.size
    desc = np.uint64(M64) - np.arange(first, first + n, dtype=np.uint64)
    k = (field.astype(np.uint64) << np.uint64(lo)) if bits else np.zeros(n, np.uint64)
    if lo:
        k |= desc & np.uint64((1 << lo) - 1)
    if lo + bits < 64:
        k |= desc << np.uint64(lo + bits)
    return k


def ties(rng, n, bits):
    """a field with many ties: n draws from about n / 3 values of the window, 0 and the largest among them"""
    if bits == 0:
        return np.zeros(n, np.uint64)
    m = max(2, min(n // 3, 1 << min(bits, 40)))
    pal = _u64(rng, m) & np.uint64((1 << bits) - 1)
    pal[0], pal[-1] = 0, (1 << bits) - 1
    return pal[rng.integers(0, m, size=n)]


def _vals(rng, n):
    v = rng.integers(0, 1 << 32, size=n, dtype=np.uint32)
    v[rng.integers(0, n, size=max(1, n // 50))] = 0
    v[rng.integers(0, n, size=max(1, n // 50))] = M32
    if n > 1:
        v[0], v[-1] = M32, 0
    return v


def make(name, body, n_max, stages, d_n=None, cap=None, skew=0, delta=0, poison=0xA5, **meta):
    """body: the keys of the first min(d_n, n_max) elements.  Behind them up to `cap` stand decoys: their field in the first
    stage's window is 0, so a sort that took them in would put them FIRST.  The alternate buffers hold noise."""
    rng = _rng(name + "/fill")
    d_n = n_max if d_n is None else d_n
    cap = n_max + 131 if cap is None else cap
    n_eff = min(d_n, n_max)
    assert body.size == n_eff and cap >= n_max
    lo, bits = stages[0][0], stages[0][1]
    keys = np.concatenate([body.astype(np.uint64), compose(np.zeros(cap - n_eff, np.uint64), lo, bits, first=n_eff)])
    meta.setdefault("rc", [0] * len(stages))
    return Case(name, keys, _vals(rng, cap), _u64(rng, cap), rng.integers(0, 1 << 32, size=cap, dtype=np.uint32), cap, d_n, n_max,
                [tuple(s) for s in stages], skew, delta, poison, meta)


# ---- the case list: name -> builder -----------------------------------------------------------------------------------------
SPECS = collections.OrderedDict()


def _spec(name, fn):
    assert name not in SPECS, name
    SPECS[name] = fn


def _random_case(name, n, lo, bits, **kw):
    zeroed = kw.pop("zeroed", 0)
    _spec(name, lambda: make(name, compose(ties(_rng(name), min(kw.get("d_n", n), n), bits), lo, bits), n, [(lo, bits, zeroed)], **kw))


# counts: a wave round, a wave's share, a tile, a chunk; the tile index at which wave q enters row_sums' unrolled loop on H is
# CHUNK - 3 + q (29 + q today)
COUNTS = [1, WAVE - 1, WAVE, WAVE + 1, SHARE - 1, SHARE, SHARE + 1, T - 1, T, T + 1, CT - 1, CT, CT + 1] + \
         [k * T + 77 for k in range(SORT_CHUNK - 3, SORT_CHUNK + 1)]
for _n in COUNTS:
    _random_case("count_%d" % _n, _n, 0, 64)

# the same loop on C: no wave unrolled, wave 0 only, all four with empty tails, unrolled plus a tail row.  ~2 M keys each,
# so a 12-bit window: two passes, the second of 4 bits
NCHUNKS = [SORT_CHUNK - 4, SORT_CHUNK - 3, SORT_CHUNK - 1, SORT_CHUNK, SORT_CHUNK + 1]
for _c in NCHUNKS:
    _random_case("nchunks_%d" % _c, (_c - 1) * CT + T + 77, 5, 12, nchunks=_c)

# the device count against n_max
NMAX_A = 2 * T + 77
for _d in [0, 1, NMAX_A - 1, NMAX_A, NMAX_A + 1, M32]:
    _random_case("dn_%d_of_%d" % (_d, NMAX_A), NMAX_A, 0, 24, d_n=_d, cap=NMAX_A + 300)
_random_case("dn_%d_of_70000" % (T + 1), 70000, 0, 24, d_n=T + 1, cap=70000 + 131)
_random_case("dn_0_of_70000_zeroed", 70000, 0, 24, d_n=0, zeroed=1)

# bit windows at the ends; (5, 9): the second pass has a 1-bit digit and a partial mask
WINDOWS = [(0, 0), (0, 1), (63, 1), (0, 7), (5, 9), (31, 2), (56, 8), (57, 7), (1, 63), (0, 64)]
for _lo, _b in WINDOWS:
    _random_case("window_%d_%d" % (_lo, _b), 2 * T + 77, _lo, _b)

# digit patterns; "small": three tiles, the last partly filled; "seam": two chunks
SIZES = {"small": 2 * T + 77, "seam": CT + T + 77}


def _pattern(pname, lo, bits, fn):
    for sname, n in SIZES.items():
        name = "%s_%s" % (pname, sname)
        _spec(name, (lambda name=name, n=n: make(name, fn(n, _rng(name)), n, [(lo, bits, 0)], pattern=pname)))


def _seam_field(n, rng):
    f = rng.integers(0, 16, size=n).astype(np.uint64)
    for s in (T, CT):
        if s + 100 <= n:
            f[s - 100:s + 100] = 9
    return f


E = lambda n: np.arange(n, dtype=np.uint64)
_pattern("equal", 0, 64, lambda n, r: np.full(n, 0x0123456789ABCDEF, np.uint64))
_pattern("zeros", 0, 64, lambda n, r: np.zeros(n, np.uint64))
_pattern("ones", 0, 64, lambda n, r: np.full(n, M64, np.uint64))                # real keys that equal the padding lanes' value
_pattern("alternating", 8, 8, lambda n, r: compose(np.where(E(n) % 2 == 0, 200, 3), 8, 8))
_pattern("ascending", 0, 17, lambda n, r: compose(E(n), 0, 17))
_pattern("descending", 0, 17, lambda n, r: compose(np.uint64(n - 1) - E(n), 0, 17))
_pattern("distinct64", 3, 8, lambda n, r: compose((E(n) % WAVE + WAVE * ((E(n) // WAVE) % 4)) % 256, 3, 8))   # 64 digits per wave round
_pattern("onedigit", 3, 8, lambda n, r: compose((E(n) // WAVE) * 37 % 256, 3, 8))        # one peer group of 64 lanes per round
_pattern("allbutfirst", 3, 8, lambda n, r: compose(np.where(E(n) == 0, 200, 7), 3, 8))
_pattern("allbutlast", 3, 8, lambda n, r: compose(np.where(E(n) == n - 1, 3, 7), 3, 8))
_pattern("digits0and255", 3, 8, lambda n, r: compose(r.integers(0, 2, size=n).astype(np.uint64) * 255, 3, 8))
_pattern("seamrun", 3, 8, lambda n, r: compose(_seam_field(n, r), 3, 8))

# the scratch: dirty, skewed, exactly sized; tables zeroed by the sort and by the caller
POISONS, SKEWS = [0x00, 0xA5, 0xFF], [0, 4, 252]
for _p in POISONS:
    for _s in SKEWS:
        for _z in (0, 1):
            _random_case("scratch_p%02x_s%d_z%d" % (_p, _s, _z), CT + T + 77, 5, 9, zeroed=_z, poison=_p, skew=_s)
_spec("scratch_short", lambda: make("scratch_short", compose(ties(_rng("scratch_short"), CT + T + 77, 9), 5, 9), CT + T + 77,
                                     [(5, 9, 0), (5, 9, 1)], delta=-1, rc=[HIP_INVALID, HIP_INVALID]))

# chains on one scratch, no sync in between
CLUSTER_K = 11


def _chain(name, n, whole, stages, **kw):
    _spec(name, lambda: make(name, compose(ties(_rng(name), min(kw.get("d_n", n), n), whole[1]), *whole), n, stages, whole=whole, **kw))


_chain("chain_cluster", CT + T + 77, (0, 32 + CLUSTER_K), [(0, 32, 1), (32, CLUSTER_K, 0)])          # cluster.hip's two-sort path
_chain("chain_cluster_clean", CT + T + 77, (0, 32 + CLUSTER_K), [(0, 32, 1), (32, CLUSTER_K, 0)], poison=0)
_chain("chain_wide_narrow", CT + T + 77, (0, 45), [(0, 40, 0), (40, 5, 1)])                       # 5 passes, then 1: the tables overlay
_chain("chain_narrow_wide", CT + T + 77, (13, 44), [(13, 7, 1), (20, 37, 0)])
_chain("chain_zero_bits_between", 2 * T + 77, (0, 16), [(0, 8, 0), (0, 0, 1), (8, 8, 1)])
_chain("chain_short_count", 70000, (0, 43), [(0, 32, 1), (32, CLUSTER_K, 1)], d_n=T + 1)

NAMES = list(SPECS)
LAYOUT_NMAX, LAYOUT_BITS = [1, T, T + 1, CT, CT + 1], [1, 8, 9, 64]     # the host-side layout check that runs before any device case
BIG = [n for n in NAMES if n.startswith("nchunks_")]


@functools.lru_cache(maxsize=6)
def case(name):
    return SPECS[name]()


# ---- the reference -----------------------------------------------------------------------------------------------------------
def reference(c):
    """-> (keys, vals) of the result's first n_eff elements, n_eff.  A refused scratch sorts nothing."""
    n_eff = min(c.d_n, c.n_max)
    k, v = c.keys[:n_eff].copy(), c.vals[:n_eff].copy()
    for (lo, bits, _), rc in zip(c.stages, c.meta["rc"]):
        if rc == 0 and bits:
            o = np.argsort(field_of(k, lo, bits), kind="stable")
            k, v = k[o], v[o]
    return k, v, n_eff


# ---- the model --------------------------------------------------------------------------------------------------------------
VARIANTS = ["cut_inclusive", "chunk_off_by_one", "full_mask", "pad_peers", "pad_peers_zero", "no_clamp", "lane_rank", "not_zeroed"]


class ModelFault(Exception):
    """the modelled kernel would read or write outside its buffers"""


def _rank_in_group(g):
    """position of every element among the elements of its group, in element order"""
    order = np.argsort(g, kind="stable")
    sg = g[order]
    start = np.flatnonzero(np.r_[True, sg[1:] != sg[:-1]])
    pos = np.arange(g.size) - np.repeat(start, np.diff(np.r_[start, g.size]))
    out = np.empty(g.size, np.int64)
    out[order] = pos
    return out


def model_pass(kin, vin, kout, vout, d_n, n_max, shift, mask, Cw, Hw, v=None):
    """one histogram + scatter launch pair.  Cw [chunks of n_max][256], Hw [tiles of n_max][256]: uint32 views of the scratch."""
    cap = kin.size
    n = d_n if v == "no_clamp" else min(d_n, n_max)
    launched = div_up(n_max, T)
    m = min(n, launched * T)                            # a tile returns when it starts at or past n
    if m == 0:
        return
    if m > cap:
        raise ModelFault("reads past the buffers")
    ta = div_up(m, T)
    pad = 0 if v == "pad_peers_zero" else M64
    key = np.full(ta * T, pad, np.uint64)
    key[:m] = kin[:m]
    e = np.arange(ta * T)
    valid = e < m
    part = np.ones(ta * T, bool) if v in ("pad_peers", "pad_peers_zero") else valid     # lanes that count and rank
    d = ((key >> np.uint64(shift)) & np.uint64(0xFF if v == "full_mask" else mask)).astype(np.int64)
    tile = e // T
    # histogram kernel: the tile's row, added to its chunk's row
    Hrows = np.bincount((tile * 256 + d)[part], minlength=ta * 256).reshape(ta, 256)
    Hw[:ta] = Hrows
    acc = Cw.astype(np.int64)
    np.add.at(acc, np.arange(ta) // SORT_CHUNK, Hrows)
    Cw[:] = acc & M32
    # scatter kernel: totals of all chunk rows, `below` = chunk rows before mine + tile rows of my chunk before me
    ntiles = div_up(n, T)
    nchunks = div_up(ntiles, SORT_CHUNK)
    if nchunks > Cw.shape[0]:
        raise ModelFault("reads past the chunk tables")
    Ccum = np.concatenate([np.zeros((1, 256), np.int64), np.cumsum(Cw[:nchunks].astype(np.int64), axis=0)])
    Hcum = np.concatenate([np.zeros((1, 256), np.int64), np.cumsum(Hw[:ta].astype(np.int64), axis=0)])
    t = np.arange(ta)
    c = (t + (1 if v == "chunk_off_by_one" else 0)) // SORT_CHUNK
    cut = np.minimum(c + (1 if v == "cut_inclusive" else 0), nchunks)
    lo = np.minimum(c * SORT_CHUNK, t)
    tot = Ccum[-1] & M32
    base = (np.cumsum(tot) - tot) & M32
    off = (base[None, :] + Ccum[cut] + Hcum[t] - Hcum[lo]) & M32
    # in-wave rank by peer group: the lanes of a round with my digit, plus what earlier rounds of my wave left in the counter
    ep, dp = e[part], d[part]
    r_round = _rank_in_group((ep // WAVE) * 256 + dp)
    r_wave = _rank_in_group((ep // SHARE) * 256 + dp)
    rank = (r_wave - r_round) + (ep % WAVE if v == "lane_rank" else r_round)
    cnt = np.bincount((ep // SHARE) * 256 + dp, minlength=ta * WAVES * 256).reshape(ta, WAVES, 256)
    wbase = np.cumsum(cnt, axis=1) - cnt
    p = (off[tile[part], dp] + wbase[tile[part], (ep // SHARE) % WAVES, dp] + rank) & M32
    p = p[valid[part]]
    if p.size and int(p.max()) >= cap:
        raise ModelFault("writes past the buffers")
    kout[p] = kin[:m]
    vout[p] = vin[:m]


def model(c, v=None):
    """-> (keys, vals, alt_keys, alt_vals, result_in_alt, rc per stage) after the case's stages, as the kernels would leave them"""
    bufs = [(c.keys.copy(), c.vals.copy()), (c.alt_keys.copy(), c.alt_vals.copy())]
    cur, rcs = 0, []
    wide = max(s[1] for s in c.stages)
    have = scratch_bytes(c.n_max, wide) + c.delta
    nt, nc = tiles_chunks(c.n_max)
    scratch = np.full(max(passes(wide), 1) * (nt + nc) * 256, c.poison * 0x01010101, np.uint32)
    for lo, bits, zeroed in c.stages:
        if bits <= 0 or c.n_max == 0:
            rcs.append(0)
            continue
        if have < scratch_bytes(c.n_max, bits):
            rcs.append(HIP_INVALID)
            continue
        P = passes(bits)
        Cw = scratch[:P * nc * 256].reshape(P, nc, 256)
        Hw = scratch[P * nc * 256:P * (nc + nt) * 256].reshape(P, nt, 256)
        if v != "not_zeroed":
            Cw[:] = 0                                    # by the caller (tables_zeroed) or by the sort: the same region
        for p in range(P):
            rem = bits - 8 * p
            (kin, vin), (kout, vout) = bufs[cur], bufs[cur ^ 1]
            model_pass(kin, vin, kout, vout, c.d_n, c.n_max, lo + 8 * p, 0xFF if rem >= 8 else (1 << rem) - 1, Cw[p], Hw[p], v)
            cur ^= 1
        rcs.append(0)
    return bufs[0][0], bufs[0][1], bufs[1][0], bufs[1][1], bool(cur), rcs


def verdict(c, got):
    """what the device test asserts of a probe's answer, as a list of failures (empty: right).  got = (keys, vals, alt_keys,
    alt_vals, result_in_alt, rc per stage)"""
    k0, v0, k1, v1, in_alt, rcs = got
    rk, rv, n_eff = reference(c)
    bad = []
    if list(rcs) != list(c.meta["rc"]):
        bad.append("rc %r, expected %r" % (list(rcs), c.meta["rc"]))
    ok, ov = (k1, v1) if in_alt else (k0, v0)
    if not np.array_equal(ok[:n_eff], rk):
        bad.append("keys differ from the reference, first at %d" % int(np.flatnonzero(ok[:n_eff] != rk)[0]))
    if not np.array_equal(ov[:n_eff], rv):
        bad.append("values differ from the reference, first at %d" % int(np.flatnonzero(ov[:n_eff] != rv)[0]))
    for what, a, b in (("keys", k0, c.keys), ("vals", v0, c.vals), ("alt_keys", k1, c.alt_keys), ("alt_vals", v1, c.alt_vals)):
        if not np.array_equal(a[n_eff:], b[n_eff:]):
            bad.append("%s[n_eff, cap) changed, first at %d" % (what, n_eff + int(np.flatnonzero(a[n_eff:] != b[n_eff:])[0])))
    if all(bits == 0 or rc for (_, bits, _), rc in zip(c.stages, c.meta["rc"])):      # nothing sorted: the input buffers, unchanged
        if in_alt or not (np.array_equal(k0, c.keys) and np.array_equal(v0, c.vals) and np.array_equal(k1, c.alt_keys) and np.array_equal(v1, c.alt_vals)):
            bad.append("nothing to sort, yet a buffer changed or the result moved")
    return bad
