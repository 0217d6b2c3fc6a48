"""Inputs that put the streaming kernels of the extract path (classify_kernel, score_kernel, the compaction kernels and
pair_probe_kernel: strling_amd/csrc/score.hip, pair.hip) through MORE THAN ONE TURN of their loops, and a model of their
launch arithmetic that says whether an input does.

The host sizes every grid from the batch, so below ~2^21 reads every wave runs its loop body once: what a wave carries from
one turn to the next (the merge-join window, the prefetched vectors, the LDS stage and its flush, the histogram rows and mask
slots of the scorer) is only reached when STRL_GRID_A / _B / _C / _P / _K shrink the grids.  The builders here are plain and
seeded (no GPU code); a case is a RecordBatch, a GenomeStr or None, the options and a `meta` dict that names its edge.
`Model` reads the kernels' constants and grid formulas out of the source text and restates the LAUNCH ARITHMETIC ONLY (which
reads a wave owns, where its iterations start, what a lane's stride is, how many rounds a block runs): never the predicate or
the scorer.  tests/test_loop_cases.py asserts with it, on the CPU, that every case reaches its edge under every grid
configuration it is run with; tests/test_loop_device.py runs the cases through the kernels.
"""
import collections
import functools
import os
import re

import numpy as np

from strling_amd.records import GenomeStr, RecordBatch

N = 8192 + 77             # with STRL_GRID_C=1 a classify wave owns 2304 reads (4.5 iterations), the last wave 1357 (not a multiple of 4)
N3 = 2 * 8192 + 77        # three rounds of the compaction kernels under STRL_GRID_K=1
MEDIAN = 350
OPTS = (0.8, 40, MEDIAN)  # (proportion_repeat, min_mapq, median fragment length)
Case = collections.namedtuple("Case", "name rec genome opts meta")

# the grid configurations of tests/test_loop_device.py: environment of one child process each ("default": the parent itself)
CONFIGS = {
    "one": dict(STRL_GRID_A=1, STRL_GRID_B=1, STRL_GRID_C=1, STRL_GRID_P=1, STRL_GRID_K=1),
    "odd": dict(STRL_GRID_A=3, STRL_GRID_B=2, STRL_GRID_C=2, STRL_GRID_P=3, STRL_GRID_K=2),
    "split": dict(STRL_GRID_A=1, STRL_GRID_B=1, STRL_GRID_C=1, STRL_GRID_P=1, STRL_GRID_K=1, STRL_SPLIT_SEGMENTS=1),
}
GRID_VARS = ("STRL_GRID_A", "STRL_GRID_B", "STRL_GRID_C", "STRL_GRID_P", "STRL_GRID_K", "STRL_SPLIT_SEGMENTS")

BASES = np.frombuffer(b"ACGT", np.uint8)


def _rng(*seed):
    return np.random.Generator(np.random.Philox(key=[int(sum((s + 1) * 1000003 ** i for i, s in enumerate(seed))) % (1 << 63), 7]))


def _rand(rng, n):
    return BASES[rng.integers(0, 4, n)].tobytes().decode()


def _batch(tid, pos, cigars, seqs, mapq=None, flag=None, mtid=None, mpos=None, qnames=None, n_targets=8):
    n = len(seqs)
    return RecordBatch.from_fields(tid, pos, tid if mtid is None else mtid, pos if mpos is None else mpos, [99] * n if flag is None else flag,
                                   [60] * n if mapq is None else mapq, cigars, seqs, qnames or ["q%06d" % i for i in range(n)],
                                   targets=[("chr%d" % t, 1 << 28) for t in range(n_targets)])


def _read_seq(rng, L):
    """one read in eight a tract (its word counts, so a kept read's word is more than zero), the others random"""
    if L >= 12 and rng.random() < 0.125:
        u = ["CAG", "AC", "AAAG", "T"][int(rng.integers(0, 4))]
        return (u * (L // len(u) + 1))[:L]
    return _rand(rng, L)


def _sparse_intervals(rng, lo, hi, every=3000):
    out, s = [], lo + int(rng.integers(0, every))
    while s < hi:
        out.append((s, s + int(rng.integers(30, 300))))
        s += int(rng.integers(every // 2, every * 3 // 2))
    return out


def _plain(rng, tid, pos, L=100):
    """single-M reads at the given positions"""
    pos = [int(p) for p in pos]
    return _batch([tid] * len(pos) if np.isscalar(tid) else list(tid), pos, ["%dM" % L] * len(pos), [_read_seq(rng, L) for _ in pos])


# ---- 1. the skip predicate ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def nested():
    """one interval of 60 kb with dozens of short ones starting inside it; most reads overlap only the long one, far behind many
    later starts: what answers for them is the running-max-stop column of the table"""
    rng = _rng(1)
    long_iv = (100_000, 160_000)
    inner, s = [], 100_400
    while s < 159_000:
        inner.append((s, s + int(rng.integers(30, 300))))
        s += int(rng.integers(600, 1000))
    ivs = [(92_000, 92_100), (95_500, 95_640), long_iv] + inner + [(162_000 + 1500 * k, 162_060 + 1500 * k + 17 * k) for k in range(8)]
    pos = np.sort(rng.integers(90_000, 175_000, N))
    rec = _plain(rng, 0, pos)
    g = GenomeStr.from_lists(2, {0: ivs, 1: []})
    return Case("nested", rec, g, OPTS, dict(edge="running max stop", long=long_iv, inner=inner))


@functools.lru_cache(maxsize=None)
def dense():
    """40 starts inside one 4 KiB bin (more than JOIN_WIN): the merge join gives up and skip_one scans more than one step"""
    rng = _rng(2)
    bin0 = 30 << 12
    cluster = [(bin0 + 100 * j, bin0 + 100 * j + 12) for j in range(40)]
    ivs = [(110_000, 110_200), (115_000, 115_090)] + cluster + [(135_000, 135_040), (139_000, 139_250)]
    pos = np.sort(rng.integers(118_000, 131_000, N))
    rec = _plain(rng, 0, pos, L=40)
    return Case("dense", rec, GenomeStr.from_lists(1, {0: ivs}), OPTS, dict(edge="more than JOIN_WIN starts in a span", bin=30, cluster=cluster))


EDGE_IVS = [(0, 1), (5000, 5100), (5300, 5350), (8192, 8200), (12287, 12290), (20400, 20420), (40000, 40050), (60000, 60030)]
# (pos, length, skipped?, what): hand-derived, the CPU test holds the oracle AND the brute-force predicate to them
EDGE_PROBES = [
    (0, 1, False, "inside the interval (0, 1)"),
    (1, 100, True, "starts where (0, 1) stops"),
    (5100, 100, True, "read start = interval stop"),
    (5099, 100, False, "read start = interval stop - 1"),
    (5200, 100, True, "read stop = interval start"),
    (5201, 100, False, "read stop = interval start + 1"),
    (8092, 100, True, "read stop = a start on 2 * 4096"),
    (8093, 100, False, "read stop = a start on 2 * 4096, + 1"),
    (12187, 100, True, "read stop = a start on 3 * 4096 - 1"),
    (12188, 100, False, "read stop = 3 * 4096: one past the start on 3 * 4096 - 1"),
    (60029, 100, False, "last base of the last interval"),
    (60030, 100, True, "behind the last interval, inside the last bin"),
    (61340, 100, True, "stop on the edge behind the last bin"),
]
EDGE_PILE = (20380, 100, 1700)      # 1700 reads whose stop is 5 * 4096: iterations that reuse a window with smin == J.lo
EDGE_TAIL = 1500                    # reads behind the last bin (15 bins: starts below 61 440), the last wave's among them: the all-sentinel window


@functools.lru_cache(maxsize=None)
def edges():
    rng = _rng(3)
    rows = [(p, L, sk, what) for p, L, sk, what in EDGE_PROBES]
    rows += [(EDGE_PILE[0], EDGE_PILE[1], False, "pile")] * EDGE_PILE[2]
    rows += [(int(p), 100, True, "tail") for p in rng.integers(61_500, 90_000, EDGE_TAIL)]
    rows += [(int(p), 100 if rng.random() < 0.8 else 50, None, "") for p in rng.integers(0, 60_000, N - len(rows))]
    rows.sort(key=lambda r: r[0])
    rec = _batch([0] * N, [r[0] for r in rows], ["%dM" % r[1] for r in rows], [_read_seq(rng, r[1]) for r in rows])
    expect = {i: (r[2], r[3]) for i, r in enumerate(rows) if r[2] is not None}
    return Case("edges", rec, GenomeStr.from_lists(1, {0: EDGE_IVS}), OPTS,
                dict(edge="touching ends, starts on bin edges, stops on a bin edge, the all-sentinel window", expect=expect))


@functools.lru_cache(maxsize=None)
def backwards():
    """the records of `edges`, their blocks of 512 in reverse order: every iteration lies BELOW the window the one before it
    left (smin < J.lo), which must reload"""
    e = edges()
    order = np.concatenate([np.arange(b, min(b + 512, N)) for b in range((N - 1) // 512 * 512, -1, -512)])
    rec = _batch([0] * N, e.rec.pos[order].tolist(), ["%dM" % (int(c) >> 4) for c in e.rec.cigar[order]], [e.rec.sequence(int(i)) for i in order])
    expect = {int(np.flatnonzero(order == i)[0]): v for i, v in e.meta["expect"].items()}
    return Case("backwards", rec, e.genome, OPTS, dict(edge="smin below the carried window", expect=expect, order=order))


# where the contigs of `contigs` change, by read index: 300 and 4700 lie inside an iteration (mixed contigs: the fallback);
# 1024 starts an iteration of a wave under STRL_GRID_C=1 and =2, 1792 only under =2 (1280 + 512), 2816 only under =1 (2304 + 512)
CONTIG_SEGMENTS = [(0, 0), (300, 1), (1024, 2), (1792, 3), (2816, 4), (4700, 6), (5300, -1), (5900, 5), (6912, 0)]
CONTIG_NONE = (3800, 4400)          # soft-clipped reads, no candidate: covers the iteration [3840, 4352) of both partitions
CONTIG_TABLE_TIDS = 6               # tid 6 (and 7) lie beyond the table; tid 2 is no key of it; tid 3 is a key without intervals


@functools.lru_cache(maxsize=None)
def contigs():
    rng = _rng(4)
    tid = np.zeros(N, np.int64)
    for (a, t), (b, _) in zip(CONTIG_SEGMENTS, CONTIG_SEGMENTS[1:] + [(N, 0)]):
        tid[a:b] = t
    pos = np.zeros(N, np.int64)
    for (a, _), (b, _) in zip(CONTIG_SEGMENTS, CONTIG_SEGMENTS[1:] + [(N, 0)]):
        pos[a:b] = np.sort(rng.integers(0, 200_000, b - a))
    cig, seqs = [], []
    for i in range(N):
        soft = CONTIG_NONE[0] <= i < CONTIG_NONE[1]
        cig.append("20S80M" if soft else "100M")
        seqs.append(_read_seq(rng, 100))
    rec = _batch(tid.tolist(), pos.tolist(), cig, seqs)
    per = {t: _sparse_intervals(_rng(40, t), 0, 200_000) for t in (0, 1, 4, 5)}
    per[3] = []
    return Case("contigs", rec, GenomeStr.from_lists(CONTIG_TABLE_TIDS, per), OPTS,
                dict(edge="contig changes inside and on iteration boundaries, contigs outside the table, an iteration without candidates",
                     boundaries={"one": 2816, "odd": 1792, "both": 1024}, inside=[300, 4700]))


CARRY_CHANGES = (1024, 4352)        # a turn of a wave starts here under STRL_GRID_C=1 and under =2, and not the wave's first


@functools.lru_cache(maxsize=None)
def contig_carry():
    """the contig changes on a turn's boundary while the coordinates go on ascending, so that the window the wave carries (the
    other contig's) would pass the reuse test if the change did not invalidate it -- and would answer wrongly: contig 0 has no
    interval near the reads (all skipped), contig 1 one interval over all of them (all kept)"""
    rng = _rng(7)
    tid = np.zeros(N, np.int64)
    tid[CARRY_CHANGES[0]:CARRY_CHANGES[1]] = 1
    rec = _plain(rng, tid.tolist(), np.sort(rng.integers(50_000, 58_000, N)))
    g = GenomeStr.from_lists(2, {0: [(1000, 1100)], 1: [(49_000, 60_000)]})
    return Case("contig_carry", rec, g, OPTS, dict(edge="a carried window that fits the next contig's reads", changes=CARRY_CHANGES))


@functools.lru_cache(maxsize=None)
def keep_all():
    """no table: every read is queued, classify's stage fills and flushes in every iteration"""
    rng = _rng(5)
    rec = _plain(rng, 0, np.sort(rng.integers(0, 500_000, N)), L=60)
    return Case("keep_all", rec, None, OPTS, dict(edge="mid-loop flush at exactly CL_STAGE"))


@functools.lru_cache(maxsize=None)
def keep_half():
    """covered and bare stretches of irregular length: about half of the reads are kept, in irregular runs, so that the stage
    passes CL_STAGE between two iterations and is flushed at a count strictly inside (CL_STAGE, 2 * CL_STAGE)"""
    rng = _rng(6)
    ivs, s = [], 0
    while s < 400_000:
        a = s + int(rng.integers(150, 2500))
        b = a + int(rng.integers(150, 2500))
        ivs.append((a, b))
        s = b
    rec = _plain(rng, 0, np.sort(rng.integers(0, 400_000, N)), L=60)
    return Case("keep_half", rec, GenomeStr.from_lists(1, {0: ivs}), OPTS, dict(edge="mid-loop flush at a ragged count"))


SKIP_CASES = ("nested", "dense", "edges", "contigs", "contig_carry", "backwards", "keep_all", "keep_half")


def brute_force_skipped(rec, g):
    """extract.nim:30-34 as an all-pairs numpy predicate: single-M cigar, contig a key of the table, no interval with
    start < read stop and stop > read start.  (Every read of these cases is mapped: its stop is pos + its M / D / N / = / X ops.)"""
    n = rec.n
    ncig = np.diff(rec.cigar_off.astype(np.int64))
    first = rec.cigar[np.minimum(rec.cigar_off[:-1].astype(np.int64), max(len(rec.cigar) - 1, 0))] if len(rec.cigar) else np.zeros(n, np.uint32)
    single_m = (ncig == 1) & ((first & 15) == 0)
    if g is None:
        return np.zeros(n, bool)
    stop = rec.pos.astype(np.int64) + np.where(single_m, first >> 4, 0)
    tid = rec.tid.astype(np.int64)
    in_tbl = (tid >= 0) & (tid < g.n_tid)
    has = np.zeros(n, bool)
    has[in_tbl] = g.has_chrom[tid[in_tbl]] != 0
    iv_tid = np.repeat(np.arange(g.n_tid), np.diff(g.iv_off))
    hit = ((iv_tid[None, :] == tid[:, None]) & (g.iv_start[None, :].astype(np.int64) < stop[:, None]) &
           (g.iv_stop[None, :].astype(np.int64) > rec.pos[:, None].astype(np.int64))).any(axis=1)
    return single_m & has & ~hit


# ---- 2. the scorer -------------------------------------------------------------------------------------------------------
IUPAC = "NNNNRYKMSWBDHV"
RAGGED = {160: [0, 1, 2, 3, 5, 6, 7, 15, 16, 17, 31, 32, 33, 64, 100, 149, 150, 151, 159, 160],
          256: [0, 1, 7, 16, 17, 33, 64, 150, 160, 161, 200, 250, 255, 256],
          510: [0, 1, 16, 33, 150, 160, 161, 256, 257, 300, 400, 509, 510]}
KINDS = ("nheavy", "nfew", "clean", "longest", "one", "perfect", "perfect4", "random")


def _mix_read(rng, kind, max_l):
    """-> (sequence, attributes of the read the neighbour conditions are stated in)"""
    lens = RAGGED[max_l]
    if kind == "one":
        s = _rand(rng, 1)
    elif kind == "longest":
        s = _rand(rng, max_l)
    elif kind in ("perfect", "perfect4"):
        k = int(rng.integers(1, 5 if kind == "perfect4" else 7))
        L = max_l if kind == "perfect4" else int(rng.choice([x for x in lens if x >= 16]))
        u = _rand(rng, k)
        # (a count stays below 256, extract.nim:72: beyond 255 bases no unit of one letter)
        while L // k > 250 or (L > 250 and len(set(u)) == 1):
            k, u = k + 1, _rand(rng, k + 1)
        s = (u * (L // k + 2))[int(rng.integers(0, k)):][:L]
    elif kind == "nheavy":
        L = int(rng.choice([x for x in lens if x >= 5]))
        how = int(rng.integers(0, 3))
        if how == 0:
            s = "N" * L
        elif how == 1:
            s = "".join(rng.choice(list("ACGTN"), L))
        else:                      # a tract with a fifth of its bases replaced: the literal recount, fed by the masks, decides
            u = _rand(rng, int(rng.integers(1, 7)))
            t = list((u * (L + 6))[:L])
            for j in rng.choice(L, max(1, L // 5), replace=False):
                t[int(j)] = IUPAC[int(rng.integers(0, len(IUPAC)))]
            s = "".join(t)
    elif kind == "nfew":
        L = int(rng.choice([x for x in lens if x >= 16]))
        u = _rand(rng, int(rng.integers(1, 7)))
        a = int(rng.integers(0, L))
        t = list(_rand(rng, a) + (u * L)[:L - a])
        for _ in range(int(rng.choice([1, 1, 2, 5]))):
            t[int(rng.integers(0, L))] = IUPAC[int(rng.integers(0, len(IUPAC)))]
        s = "".join(t)
    else:                          # clean, random: random bases of a ragged length
        s = _rand(rng, int(rng.choice(lens)))
    acgt = sum(s.count(b) for b in "ACGT")
    return s, dict(kind=kind, len=len(s), has_n=acgt < len(s), n_heavy=len(s) >= 5 and (len(s) - acgt) * 5 >= len(s))


# the neighbour pairs one lane has to meet in consecutive turns of score_kernel's item loop: (name, earlier item, later item)
NEIGHBOURS = [
    ("N-heavy then clean", lambda a, m: a["n_heavy"], lambda a, m: not a["has_n"] and a["len"] >= 16),
    ("longest then one base", lambda a, m: a["len"] == m and not a["has_n"], lambda a, m: a["len"] == 1),
    ("perfect repeat then random", lambda a, m: a["kind"] in ("perfect", "perfect4") and a["len"] >= 32, lambda a, m: a["kind"] in ("random", "clean", "longest") and a["len"] >= 32),
    # random sequence of some length survives k = 2..4 and goes on to stage B; a perfect tract of a unit of up to four bases ends in stage A
    ("stage B then stage A", lambda a, m: a["kind"] in ("random", "clean", "longest") and a["len"] >= 64, lambda a, m: a["kind"] == "perfect4"),
]


def _mix(name, max_l, seed):
    """every read kind of the ragged-length and not-ACGT parity tests, drawn per read, so that under ANY order of the scoring
    queue (the order in which classify's waves flush is not fixed) a lane meets every neighbour pair many times; the reads of
    every other block of 256 mostly carry bases that are not ACGT: far more than 16 such lanes in the waves that take them"""
    rng = _rng(seed)
    seqs, cig, attrs = [], [], []
    for i in range(N):
        rich = (i // 256) % 2 == 0
        w = np.array([6.0 if rich else 0.6, 3.0 if rich else 0.4, 1.5, 1.5, 1.2, 1.5, 1.5, 1.5])
        s, a = _mix_read(rng, KINDS[int(rng.choice(len(KINDS), p=w / w.sum()))], max_l)
        L = len(s)
        if L >= 40 and rng.random() < 0.3:
            c = int(rng.integers(1, L // 2))
            cig.append("%dS%dM" % (c, L - c) if rng.random() < 0.5 else "%dM%dS" % (L - c, c))
        elif L >= 60 and rng.random() < 0.1:
            c, d = int(rng.integers(17, L // 3)), int(rng.integers(17, L // 3))
            cig.append("%dS%dM%dS" % (c, L - c - d, d))
        else:
            cig.append("%dM" % L if L else "*")
        seqs.append(s)
        attrs.append(a)
    # every maximal length of the class is present, so the batch takes the kernel class it is named for
    assert max(a["len"] for a in attrs) == max_l
    rec = _batch([0] * N, list(range(100, 100 + N)), cig, seqs, mapq=[60 if i % 7 else 39 for i in range(N)])
    return Case(name, rec, None, OPTS, dict(edge="consecutive items of one lane differ in length class, N content and liveness", attrs=attrs, max_l=max_l))


@functools.lru_cache(maxsize=None)
def short_mix():
    return _mix("short_mix", 160, 11)


@functools.lru_cache(maxsize=None)
def mid_mix():
    return _mix("mid_mix", 256, 12)


@functools.lru_cache(maxsize=None)
def long_mix():
    return _mix("long_mix", 510, 13)


def _tract(rng, unit, n, n_bad):
    s = list((unit * (n // len(unit) + 2))[int(rng.integers(0, len(unit))):][:n])
    for j in (rng.choice(n, min(n_bad, n), replace=False) if n_bad else []):
        s[int(j)] = "ACGT"[("ACGT".index(s[int(j)]) + 1) % 4]
    return "".join(s)


CLIP_UNITS = ["A", "AC", "AG", "CAG", "AAT", "AAAG", "ACGT", "AACCT", "AAAAT", "AACCGT", "AAAAAG"]


def _clip_batch(name, n, read_lens, max_clip, seed):
    """pairs of a clipped read and its mate: the clips are tracts (pure, or with a few wrong bases) or random, their lengths run
    over every length class of the soft-item compaction (eight bases per class from 17 up)"""
    rng = _rng(seed)
    rows = []            # (pos, mpos, flag, mapq, cigar, seq, qname)
    n_pairs = n // 2
    for c in range(n_pairs):
        L = int(rng.choice(read_lens))
        unit = CLIP_UNITS[int(rng.integers(0, len(CLIP_UNITS)))]

        def clip_len():
            return int(min(17 + (c * 8 + int(rng.integers(0, 8))) % (max_clip - 16), L - 1))

        def clip(m):
            r = rng.random()
            return _rand(rng, m) if r < 0.2 else _tract(rng, unit, m, 0 if r < 0.6 else int(rng.integers(1, 2 + m // 10)))
        side = min(int(rng.integers(0, 4)), 2)          # left, right, and twice as often both
        cl, cr = clip_len(), clip_len()
        body = (lambda m: _tract(rng, unit, m, int(rng.integers(0, 4)))) if rng.random() < 0.5 else (lambda m: _rand(rng, m))
        if side == 2 and cl + cr > L - 4:
            side = c % 2
        if c % 50 == 7: seq, cig = clip(L), "%dS" % L              # the whole read one clip (a cigar of one op: its left end only)
        elif side == 0: seq, cig = clip(cl) + body(L - cl), "%dS%dM" % (cl, L - cl)
        elif side == 1: seq, cig = body(L - cr) + clip(cr), "%dM%dS" % (L - cr, cr)
        else: seq, cig = clip(cl) + body(L - cl - cr) + clip(cr), "%dS%dM%dS" % (cl, L - cl - cr, cr)
        base = 3000 + 40 * c
        first = rng.random() < 0.5
        pc, pm = (base, base + 320) if first else (base + 320, base)
        rev = int(rng.integers(0, 2))
        q = "c%06d" % c
        rows.append((pc, pm, 1 | 2 | 0x40 | (0x10 if rev else 0x20), int(rng.choice([60] * 9 + [41, 40, 39])), cig, seq, q))
        rows.append((pm, pc, 1 | 2 | 0x80 | (0x20 if rev else 0x10), int(rng.choice([60, 60, 40, 0])), "150M", _rand(rng, 150), q))
    for j in range(n - 2 * n_pairs):
        rows.append((10 + j, 10 + j, 0, 60, "100M", _rand(rng, 100), "x%d" % j))
    rows.sort(key=lambda r: r[0])
    rec = _batch([0] * n, [r[0] for r in rows], [r[4] for r in rows], [r[5] for r in rows], mapq=[r[3] for r in rows], flag=[r[2] for r in rows],
                 mpos=[r[1] for r in rows], qnames=[r[6] for r in rows])
    return Case(name, rec, None, OPTS, dict(edge="rounds of the compaction kernels, turns of the segment scorers", max_l=max(read_lens)))


@functools.lru_cache(maxsize=None)
def clips():
    """short-read class (one fused segment launch, or the three launches under STRL_SPLIT_SEGMENTS): 3 x 8192 scored reads in the
    soft-item compaction, more than 8192 clipped ends in the survivor compaction, more than 2048 soft records in the pair logic"""
    return _clip_batch("clips", N3, [160, 160, 150, 100], 160, 21)


@functools.lru_cache(maxsize=None)
def clips_long():
    """clips beyond 160 bases (the last length class of the compaction), in reads of the long-read class"""
    return _clip_batch("clips_long", N, [300, 500, 160], 400, 22)


SCORER_CASES = ("short_mix", "mid_mix", "long_mix", "clips", "clips_long")

# ---- 3. the pair probe ---------------------------------------------------------------------------------------------------
HOT_SEQ = "CAG" * 50


def _hot(name, n, seed):
    """three qname groups in four are a pair of repeats (both reads mark and hit the Bloom bitmap), in no regular order: a probe
    wave that owns 2048 reads and more collects PR_STAGE hits before its last iteration and flushes inside the loop"""
    N = n
    rng = _rng(seed)
    tid, pos, mpos, flag, qn, seqs = [], [], [], [], [], []
    g = 0
    while len(pos) < N:
        g += 1
        is_hot = rng.random() < 0.78
        m = 3 if N - len(pos) == 3 else 2
        for j in range(m):
            before = j % 2 == 0
            pos.append(1000 + g if before else 900_000 + g)
            mpos.append(900_000 + g if before else 1000 + g)
            flag.append(99 if before else 147)
            qn.append("h%05d" % g)
            seqs.append(HOT_SEQ if is_hot else _rand(rng, 150))
    rec = _batch([0] * N, pos, ["150M"] * N, seqs, flag=flag, mpos=mpos, qnames=qn)
    return Case(name, rec, None, OPTS, dict(edge="mid-loop flush of the pair probe"))


@functools.lru_cache(maxsize=None)
def hot():
    """STRL_GRID_P=1: four probe waves of 2112 reads (five turns)"""
    return _hot("hot", N, 31)


@functools.lru_cache(maxsize=None)
def hot_wide():
    """STRL_GRID_P=3 makes twelve waves: of `hot` each would own 704 reads and never fill its stage; of these, 2112"""
    return _hot("hot_wide", 3 * 8192 + 77, 32)


PAIR_CASES = ("hot", "hot_wide")
ALL_CASES = SKIP_CASES + SCORER_CASES + PAIR_CASES
EXTRACT_CASES = ("hot", "hot_wide", "clips")          # also run through the whole extract (scorer + pair logic)


def case(name):
    return globals()[name]()


@functools.lru_cache(maxsize=None)
def expected(name):
    """the oracle's answers for a case, computed once per process and shared: skipped flags, packed words, the soft records add_soft
    looks at, and for the cases that go through the whole extract its treads"""
    from oracle import oracle as O
    from helpers import oracle_words, soft_items_expected
    c = case(name)
    opts = O.make_opts(c.opts[2], c.opts[0], c.opts[1])
    whole, soft = oracle_words(O, c.rec, c.genome, opts)
    items = soft_items_expected(c.rec, whole, c.opts[1])
    out = dict(whole=whole, skipped=(whole & 0x8000) != 0, items=items,
               soft_side=np.array([(i << 1) | s for i, s in items], np.uint32),
               soft_first=np.array([soft[it][0] for it in items], np.uint32), soft_after=np.array([soft[it][1] for it in items], np.uint32))
    if name in EXTRACT_CASES:
        out["treads"] = O.extract(c.rec, c.genome, opts, 0)
        # a qname group is hot when a word of one of its reads (or of a clipped end add_soft looks at) counts: its reads hit the bitmap
        hot_read = ((whole >> 16) != 0) & ~out["skipped"]
        for (i, s), a, b in zip(items, out["soft_first"], out["soft_after"]):
            if (int(a) >> 16) or (int(b) >> 16):
                hot_read[i] = True
        grp = qname_groups(c.rec)
        hot_grp = np.zeros(grp.max() + 1, bool)
        hot_grp[grp[hot_read]] = True
        out["probe_hit"] = hot_grp[grp]
        out["n_hot_soft"] = int(sum(1 for a, b in zip(out["soft_first"], out["soft_after"]) if (int(a) >> 16) or (int(b) >> 16)))
    return out


def qname_groups(rec):
    """-> group index of every read (reads of one qname share it)"""
    names = {}
    return np.array([names.setdefault(rec.qname(i), len(names)) for i in range(rec.n)])


# ---- 4. the launch arithmetic, read off the source ---------------------------------------------------------------------------
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "strling_amd", "csrc")


def _find(text, pattern, what):
    m = re.search(pattern, text)
    if not m:
        raise AssertionError("tests/loop_cases.py: %s not found in the source (pattern %r): the kernel changed, restate the model" % (what, pattern))
    return m


class Model:
    """constants and grid formulas of score.hip / pair.hip / score.h, found by regex (an AssertionError names what is missing)"""

    def __init__(self):
        score = open(os.path.join(CSRC, "score.hip")).read()
        pair = open(os.path.join(CSRC, "pair.hip")).read()
        hdr = open(os.path.join(CSRC, "score.h")).read()
        num = lambda text, name: int(_find(text, r"constexpr int [^;]*\b%s = (\d+)" % name, name).group(1))
        self.CL_STAGE, self.CL_ILP, self.JOIN_WIN = num(score, "CL_STAGE"), num(score, "CL_ILP"), num(score, "JOIN_WIN")
        self.PR_STAGE, self.PR_ILP = num(pair, "PR_STAGE"), num(pair, "PR_ILP")
        self.BIN_SHIFT = num(hdr, "BIN_SHIFT")
        cl = score[score.index("void classify_kernel("):score.index("void compact_kernel(")]
        pr = pair[pair.index("void pair_probe_kernel("):]
        # a wave's share: ceil(n / waves) rounded up to 256 (classify: groups of four reads per lane) and to 64 (probe)
        self.cl_round = int(_find(cl, r"per = \(\(\(P\.n \+ n_waves - 1\) / n_waves\) \+ (\d+)ull\) & ~(\d+)ull;", "classify's rounding").group(1)) + 1
        self.pr_round = int(_find(pr, r"per = \(\(\(P\.n \+ n_waves - 1\) / n_waves\) \+ (\d+)ull\) & ~(\d+)ull;", "the probe's rounding").group(1)) + 1
        _find(cl, r"n_waves = \(uint64_t\)gridDim\.x \* 4u;", "classify's waves per block")
        _find(pr, r"n_waves = \(uint64_t\)gridDim\.x \* 4u;", "the probe's waves per block")
        _find(cl, r"for \(uint64_t base = r0; base < r1; base \+= 64 \* CL_ILP\)", "classify's iteration")
        _find(pr, r"for \(uint64_t base = r0; base < r1; base \+= 64 \* PR_ILP\)", "the probe's iteration")
        _find(cl, r"VEC \? base \+ 256ull \* \(uint64_t\)\(j >> 2\) \+ 4ull \* \(uint64_t\)lane \+ \(uint64_t\)\(j & 3\) : base \+ 64ull \* \(uint64_t\)j \+ \(uint64_t\)lane", "classify's read index")
        _find(cl, r"if \(cnt >= CL_STAGE\) flush\(\);", "classify's mid-loop flush")
        _find(pr, r"if \(cnt >= PR_STAGE\) flush\(\);", "the probe's mid-loop flush")
        _find(cl, r"join\.t = -2; join\.valid = 0;", "the join state's start")
        _find(score, r"if \(!\(J\.valid && smin >= J\.lo && J\.e\[WIN - 1\]\.x >= smax\)\)", "the window-reuse test")
        m = _find(score, r"cblocks = \(int\)std::min<uint64_t>\(\(n \+ (\d+)\) / (\d+), env_c > 0 \? \(uint64_t\)env_c : (\d+)\)", "classify's grid")
        self.cl_reads_per_block, self.cl_max_blocks = int(m.group(2)), int(m.group(3))
        assert int(m.group(1)) + 1 == self.cl_reads_per_block
        m = _find(pair, r"pblocks = \(int\)std::min<uint64_t>\(\(n \+ (\d+)\) / (\d+), env_p > 0 \? \(uint64_t\)env_p : (\d+)\)", "the probe's grid")
        self.pr_reads_per_block, self.pr_max_blocks = int(m.group(2)), int(m.group(3))
        # the scorer: ga / gb, the clamps of the long-read classes, block sizes
        m = _find(score, r"ga = env_a > 0 \? env_a : \(int\)std::min<uint64_t>\((\d+), std::max<uint64_t>\((\d+), \(upper \+ 255\) / 256\)\)", "stage A's grid")
        self.ga_max, self.ga_min = int(m.group(1)), int(m.group(2))
        m = _find(score, r"gb = env_b > 0 \? env_b : std::max\((\d+), ga / (\d+)\)", "stage B's grid")
        self.gb_min, self.gb_div = int(m.group(1)), int(m.group(2))
        self.classes = {}      # longest read of the class -> (threads per block, stage A clamp (min, divisor), stage B clamp)
        m = _find(score, r"if \(max_l <= (\d+)\) rc = launch_score<10, 64, MODE, 0, (\d+)>\(ctx, P, ga\);", "the short-read class")
        self.classes[int(m.group(1))] = (int(m.group(2)), None, None)
        ma = _find(score, r"else if \(max_l <= (\d+)\) rc = launch_score<16, 128, MODE, 0, (\d+)>\(ctx, P, env_a > 0 \? env_a : std::max\((\d+), ga / (\d+)\)\);", "the middle class, stage A")
        mb = _find(score, r"if \(max_l <= \d+\) return launch_score<16, 128, MODE, 1, \d+>\(ctx, P, env_b > 0 \? env_b : std::max\((\d+), gb / (\d+)\)\);", "the middle class, stage B")
        self.classes[int(ma.group(1))] = (int(ma.group(2)), (int(ma.group(3)), int(ma.group(4))), (int(mb.group(1)), int(mb.group(2))))
        ma = _find(score, r"else rc = launch_score<32, 256, MODE, 0, (\d+)>\(ctx, P, env_a > 0 \? env_a : std::max\((\d+), ga / (\d+)\)\);", "the long class, stage A")
        mb = _find(score, r"return launch_score<32, 256, MODE, 1, \d+>\(ctx, P, env_b > 0 \? env_b : std::max\((\d+), gb / (\d+)\)\);", "the long class, stage B")
        self.classes[1 << 30] = (int(ma.group(1)), (int(ma.group(2)), int(ma.group(3))), (int(mb.group(1)), int(mb.group(2))))
        _find(score, r"const uint32_t stride = gridDim\.x \* BLOCK;", "the scorer's stride")
        _find(score, r"cur_r = nxt_r; nxt_r = nn_r;", "the scorer's pipeline hand-over")
        # the compaction kernels: slots per thread and round (U), 1024 threads, default grids
        ck = score[score.index("void compact_kernel("):score.index("void soft_compact_kernel(")]
        sk = score[score.index("void soft_compact_kernel("):score.index("table_rows()")]
        pk = pair[pair.index("void pair_soft_items_kernel("):pair.index("void pair_probe_kernel(")]
        self.rounds = {}       # kernel -> (slots per block and round, default grid)
        for name, body, text, launch in (("compact_kernel", ck, score, r"\(compact_kernel<1, MODE>\), dim3\(compact_grid\((\d+)\)\), dim3\(1024\)"),
                                         ("soft_compact_kernel", sk, score, r"soft_compact_kernel, dim3\(strl::compact_grid\((\d+)\)\), dim3\(1024\)"),
                                         ("pair_soft_items_kernel", pk, pair, r"pair_soft_items_kernel, dim3\(compact_grid\((\d+)\)\), dim3\(1024\)")):
            u = int(_find(body, r"constexpr int U = (\d+);", "U of " + name).group(1))
            _find(body, r"b0 = blockIdx\.x \* \(1024u \* U\); b0 < n_src; b0 \+= gridDim\.x \* \(1024u \* U\)", "the round loop of " + name)
            self.rounds[name] = (1024 * u, int(_find(text, launch, "the grid of " + name).group(1)))
        _find(score, r"env_k = getenv\(\"STRL_GRID_K\"\)", "STRL_GRID_K")

    # -- grids --
    @staticmethod
    def _env(cfg, k):
        return int((cfg or {}).get(k, 0))

    def wave_ranges(self, n, kernel, cfg):
        """[(r0, r1)] of every wave of classify_kernel ('C') or pair_probe_kernel ('P') that owns a read"""
        per_block, mx, rnd, env = ((self.cl_reads_per_block, self.cl_max_blocks, self.cl_round, self._env(cfg, "STRL_GRID_C")) if kernel == "C" else
                                   (self.pr_reads_per_block, self.pr_max_blocks, self.pr_round, self._env(cfg, "STRL_GRID_P")))
        blocks = min(-(-n // per_block), env if env > 0 else mx)
        waves = 4 * blocks
        per = -(-(-(-n // waves)) // rnd) * rnd
        return [(w * per, min(w * per + per, n)) for w in range(waves) if w * per < n]

    def iterations(self, n, kernel, cfg):
        """[[(base, end)] per wave]: the reads of every turn of a wave's loop"""
        step = 64 * (self.CL_ILP if kernel == "C" else self.PR_ILP)
        return [[(b, min(b + step, r1)) for b in range(r0, r1, step)] for r0, r1 in self.wave_ranges(n, kernel, cfg)]

    def iteration_order(self, base, end, vec):
        """the reads of classify's iteration [base, end) in the order its lanes stage them (sub-item j outermost, then the lane)"""
        j, lane = np.meshgrid(np.arange(self.CL_ILP), np.arange(64), indexing="ij")
        r = (base + 256 * (j >> 2) + 4 * lane + (j & 3)) if vec else (base + 64 * j + lane)
        r = r.reshape(-1)
        return r[r < end]

    def score_grid(self, upper, max_l, stage, cfg):
        """(blocks, threads per block) of score_kernel for a queue of at most `upper` items"""
        ea, eb = self._env(cfg, "STRL_GRID_A"), self._env(cfg, "STRL_GRID_B")
        ga = ea if ea > 0 else min(self.ga_max, max(self.ga_min, -(-upper // 256)))
        gb = eb if eb > 0 else max(self.gb_min, ga // self.gb_div)
        block, ca, cb = self.classes[min(k for k in self.classes if max_l <= k)]
        if stage == "A":
            return (ga if ca is None or ea > 0 else max(ca[0], ga // ca[1])), block
        return (gb if cb is None or eb > 0 else max(cb[0], gb // cb[1])), block

    def compaction_rounds(self, kernel, n_src, cfg):
        """turns of the round loop of block 0 of a compaction kernel over n_src slots"""
        per, dflt = self.rounds[kernel]
        k = self._env(cfg, "STRL_GRID_K")
        grid = k if k > 0 else dflt
        return len(range(0, n_src, grid * per))

    # -- classify: the control flow of the merge join's carried state (never the predicate itself) --
    def classify_trace(self, case, cfg, kept):
        """one dict per (wave, iteration): what of the join state the iteration found and left, and the stage count.
        kept: bool per read (the ORACLE's: not skipped), for the stage counts only."""
        rec, g = case.rec, case.genome
        n = rec.n
        ncig = np.diff(rec.cigar_off.astype(np.int64))
        first = rec.cigar[np.minimum(rec.cigar_off[:-1].astype(np.int64), len(rec.cigar) - 1)]
        n_tid = g.n_tid if g is not None else 0
        cand0 = (ncig == 1) & ((first & 15) == 0) & (rec.tid >= 0) & (rec.tid < n_tid)
        # a mapped read's stop as the batch's `end` column has it (strl_soa_from_records): pos + reference-consuming ops; here M only or S + M
        ref_len = np.zeros(n, np.int64)
        for i in range(n):
            for c in rec.cigar[int(rec.cigar_off[i]):int(rec.cigar_off[i + 1])]:
                if (int(c) & 15) in (0, 2, 3, 7, 8):
                    ref_len[i] += int(c) >> 4
        stop = rec.pos.astype(np.int64) + np.maximum(ref_len, 1)
        starts = {}
        if g is not None:
            for t in range(n_tid):
                starts[t] = np.sort(g.iv_start[int(g.iv_off[t]):int(g.iv_off[t + 1])].astype(np.int64))
        out = []
        for w, its in enumerate(self.iterations(n, "C", cfg)):
            J = dict(t=-2, valid=False, lo=0, last=None)
            cnt = 0
            for k, (a, b) in enumerate(its):
                idx = np.arange(a, b)
                c = cand0[idx]
                row = dict(wave=w, turn=k, base=a, end=b, last_turn=k == len(its) - 1, any=bool(c.any()), uniform=False, contig_changed=False,
                           window="none", fallback=False, cnt_before=cnt)
                if c.any():
                    tids = np.unique(rec.tid[idx][c])
                    row["uniform"] = len(tids) == 1
                    if len(tids) == 1:
                        t0 = int(tids[0])
                        prev = dict(J)
                        if t0 != J["t"]:
                            row["contig_changed"] = J["t"] != -2
                            J.update(t=t0, valid=False)
                        row["tid"] = t0
                        if g.has_chrom[t0]:
                            smin, smax = int(stop[idx][c].min()), int(stop[idx][c].max())
                            st = starts[t0]
                            n_bins = ((max(int(st[-1]), 0) >> self.BIN_SHIFT) + 1) if len(st) else 0
                            last_ok = J["valid"] and (J["last"] is None or J["last"] >= smax)
                            # the window of the contig before would pass the reuse test, had the change not invalidated it
                            row["stale_fits"] = bool(row["contig_changed"] and prev["valid"] and smin >= prev["lo"] and (prev["last"] is None or prev["last"] >= smax))
                            row.update(smin=smin, smax=smax, below=bool(J["valid"] and smin < J["lo"]), at_lo=bool(J["valid"] and smin == J["lo"]))
                            if J["valid"] and smin >= J["lo"] and last_ok:
                                row["window"] = "reused"
                            else:
                                b0 = (smin >> self.BIN_SHIFT) if smin > 0 else 0
                                i0 = int(np.searchsorted(st, b0 << self.BIN_SHIFT, "left")) if b0 < n_bins else len(st)
                                # entry WIN - 1 of the window: a start, or the sentinel (None) when fewer than WIN starts remain
                                J.update(valid=True, lo=b0 << self.BIN_SHIFT, last=int(st[i0 + self.JOIN_WIN - 1]) if i0 + self.JOIN_WIN - 1 < len(st) else None)
                                row["window"] = "loaded"
                                row["all_sentinel"] = i0 == len(st)
                            row["starts_in_span"] = int(np.searchsorted(st, smax, "left") - np.searchsorted(st, J["lo"], "left"))
                            row["fallback"] = not (J["last"] is None or J["last"] >= smax)
                    else:
                        row["fallback"] = True
                cnt += int(kept[idx].sum())
                row["cnt_after"] = cnt
                row["flushed"] = cnt >= self.CL_STAGE
                if row["flushed"]:
                    cnt = 0
                out.append(row)
        return out

    def queue_orders(self, n, cfg, kept, vec=True):
        """the scoring queue under the two extreme orders in which classify's waves may reserve their space: wave after wave, and
        turn by turn across the waves (the true order lies between them and is not fixed) -> {name: read index per queue slot}"""
        chunks = []      # (wave, flush number, reads)
        for w, its in enumerate(self.iterations(n, "C", cfg)):
            buf, nf = [], 0
            for a, b in its:
                r = self.iteration_order(a, b, vec)
                buf.extend(r[kept[r]].tolist())
                if len(buf) >= self.CL_STAGE:
                    chunks.append((w, nf, buf)); buf = []; nf += 1
            if buf:
                chunks.append((w, nf, buf))
        cat = lambda cs: np.array([r for c in cs for r in c[2]], np.int64)
        return {"wave after wave": cat(sorted(chunks, key=lambda c: (c[0], c[1]))), "turn by turn": cat(sorted(chunks, key=lambda c: (c[1], c[0])))}
