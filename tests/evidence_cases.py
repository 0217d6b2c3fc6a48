"""Inputs that put the evidence kernel (strling_amd/csrc/evidence.hip, its per-record rule in evidence_core.h) on its own
arithmetic edges: the 70 % cut of the unit count, the uint8 wraps, find_read_position's branches, the comparisons of
expected_spanning_probability, the depth array's clamps and the median rule, qnames with equal murmur values, the walk and
the ballot ranks at their counts.

Plain builders, no GPU code.  Every case is one region: a name, a family (a .. i), the region's records (a RecordBatch, or
raw bytes for the malformed ones of family i), a bound, a window, a fragment histogram, min_mapq, and a WITNESS: a predicate
over the reference answer (oracle.spanners: supports, median, expected spanners) that proves the case reaches its edge, so
that no test built on the table compares two answers that are equal because nothing happened.  Every case of a .. h stays
inside the capacity rule (at most 4096 records, right - left + 2 * window <= 9190); the cases of i are the inputs the kernel
refuses (status 2).  tests/test_evidence_cases.py runs the table on the CPU, tests/test_evidence_edges_device.py on the device.
"""
import functools
import struct

import numpy as np

from oracle import oracle as O
from strling_amd import api, bamio
from strling_amd.records import RecordBatch, encode_cigar

TARGETS = [("chr1", 1_000_000), ("chr2", 1_000_000)]
MAX_RECORDS, MAX_SPAN = 4096, 9190
UNITS = {1: "A", 2: "AC", 3: "CAG", 4: "AAAG", 5: "AACCT", 6: "AACCGT"}
SLENS = [1, 2, 3, 7, 10, 13, 20, 33, 99, 100, 143, 250]
COLLIDING = (b"r0152670", b"r0193733")         # the same Nim murmur value, 0x14a79bc7
QUERY_OPS, REF_OPS = (0, 1, 4, 7, 8), (0, 2, 3, 7, 8)
INT32_MIN = -2 ** 31


def frag_wide():
    """mass in every bin out to 4095: no distance at which cd[] has reached 1 before the table's last entry"""
    f = np.full(4096, 2, np.uint32)
    f[300:500] += 30
    return f


FRAG_WIDE = frag_wide()      # every case's histogram, unless it brings its own


def cumulative(frag):
    """cd[] of spanning.nim:7-20, as the oracle makes it"""
    cd = np.zeros(4096, np.float32)
    O.lib().orc_cumulative(np.ascontiguousarray(frag, np.uint32).ctypes.data, cd.ctypes.data)
    return cd


def synthetic_cd():
    """a table that is NOT a cumulative distribution: cd[4095] < 1, so that a probability at dist = 4095 is not zero and the
    comparison `dist > 4095` shows in the output (with a table of orc_cumulative cd[4095] is 1.0 exactly, and 1.0f - 1.0f is
    the zero the comparison returns)"""
    return (np.arange(4096, dtype=np.float32) / np.float32(8192)).astype(np.float32)


def nim_hash(name):
    return int(O.lib().orc_nim_hash_bytes(bytes(name), len(name))) & 0xffffffff


def probability(cd, start, stop, reverse, left, right):
    return float(O.lib().orc_expected_spanning_probability(cd.ctypes.data, int(start), int(stop), int(bool(reverse)), int(left), int(right)))


def bound(tid, left, right, unit):
    b = np.zeros(1, api.BOUNDS_DTYPE)
    b["tid"], b["left"], b["right"], b["repeat"] = tid, left, right, unit
    return b[0]


def query_len(cigar):
    return sum(c >> 4 for c in encode_cigar(cigar) if (c & 15) in QUERY_OPS)


def rd(pos, cigar, seq=None, name=None, flag=0, mapq=60, tid=0, mtid=-1, mpos=-1, isize=0):
    """one record; SEQ defaults to as many C as the CIGAR's query length"""
    return dict(pos=pos, cigar=cigar, seq="C" * query_len(cigar) if seq is None else seq, name=name, flag=flag, mapq=mapq, tid=tid, mtid=mtid, mpos=mpos, isize=isize)


def batch(recs):
    names = [(b"q%d" % i) if r["name"] is None else r["name"] for i, r in enumerate(recs)]
    return RecordBatch.from_fields([r["tid"] for r in recs], [r["pos"] for r in recs], [r["mtid"] for r in recs], [r["mpos"] for r in recs],
                                   [r["flag"] for r in recs], [r["mapq"] for r in recs], [r["cigar"] for r in recs], [r["seq"] for r in recs], names,
                                   isize=[r["isize"] for r in recs], targets=TARGETS)


def raw_of(rec):
    return bytes(bamio._raw_records(rec, 0, rec.n))


def rec_stop(rec, i):
    """Rec::stop: bam_endpos, one base behind pos for an unmapped record or a CIGAR without reference bases"""
    cig = rec.cigar[int(rec.cigar_off[i]):int(rec.cigar_off[i + 1])]
    rl = 0 if int(rec.flag[i]) & 4 else int(sum(int(c) >> 4 for c in cig if (int(c) & 15) in REF_OPS))
    return int(rec.pos[i]) + (rl or 1)


class Case:
    def __init__(self, family, name, recs, b, window=500, frag=None, min_mapq=20, witness=None, raw=None):
        self.family, self.name, self.bound, self.window, self.min_mapq = family, name, b, window, min_mapq
        self.frag = FRAG_WIDE if frag is None else frag
        self.rec = None if recs is None else (recs if isinstance(recs, RecordBatch) else batch(recs))
        self.raw = raw_of(self.rec) if raw is None else raw
        self.witness = witness
        self.refused = family == "i"
        span = int(b["right"]) - int(b["left"]) + 2 * window
        if not self.refused:
            assert self.rec.n <= MAX_RECORDS and 1 <= span <= MAX_SPAN, (name, self.rec.n, span)

    @property
    def id(self):
        return f"{self.family}-{self.name}"

    def __repr__(self):
        return f"Case({self.id})"


# ---- what a witness reads out of (supports, median, expected) -----------------------------------------------------------
def reads(ref):
    """the supports of reads (type 1 spanning, 2 overlapping), in record order"""
    return [s for s in ref[0] if s["type"] != 0]


def counts(ref):
    return [int(s["repeat_count"]) for s in reads(ref)]


def types(ref):
    return [int(s["type"]) for s in reads(ref)]


def fragments(ref):
    return [s for s in ref[0] if s["type"] == 0]


def kept_by_support(ref):
    return [int(s["rec"]) for s in reads(ref)]


# ---- a. the unit count ----------------------------------------------------------------------------------------------------
def _filler(unit):
    return "G" if "T" in unit and "G" not in unit else ("T" if "T" not in unit else "N")


def _count_read(slen, k, n_units, pos=900, left=1000):
    """a read of one M operation over the bound [left, left + slen) with n_units copies of the unit at the bound's first base and
    a base that belongs to no copy everywhere else"""
    unit, qlen = UNITS[k], (left - pos) + slen + 50
    fill = _filler(unit)
    seq = fill * (left - pos) + unit * n_units
    seq += fill * (qlen - len(seq))
    return rd(pos, f"{qlen}M", seq)


def family_a():
    out = []
    for slen in SLENS:
        for k in range(1, 7):
            thr = int(slen * 0.7 / k)
            b = bound(0, 1000, 1000 + slen, UNITS[k])
            out.append(Case("a", f"cut-slen{slen}-k{k}-at", [_count_read(slen, k, thr)], b, witness=lambda r, t=thr: counts(r) == [t]))
            if thr >= 1:
                out.append(Case("a", f"cut-slen{slen}-k{k}-below", [_count_read(slen, k, thr - 1)], b, witness=lambda r: counts(r) == [0]))
    fl = "C" * 100
    out.append(Case("a", "greedy", [rd(900, "150M", fl + "AAAAA" + "C" * 45)], bound(0, 1000, 1005, "AA"), witness=lambda r: counts(r) == [2]))
    out.append(Case("a", "odd-read-left", [rd(901, "150M", "T" * 99 + "CAG" * 7 + "T" * 30)], bound(0, 1000, 1021, "CAG"), witness=lambda r: counts(r) == [7]))
    out.append(Case("a", "even-read-left", [rd(900, "150M", "T" * 100 + "CAG" * 7 + "T" * 29)], bound(0, 1000, 1021, "CAG"), witness=lambda r: counts(r) == [7]))
    out.append(Case("a", "k6-one-base-slide", [rd(900, "200M", "T" * 100 + "A" + "AACCGT" * 5 + "AACCGA" + "AACCGT" * 3 + "T" * 45)], bound(0, 1000, 1055, "AACCGT"),
                    witness=lambda r: counts(r) == [8]))
    out.append(Case("a", "codes-outside-acgt", [rd(900, "150M", "T" * 100 + "ACNAC=ACRACYACMACKACSACWACBACDACHACVAC" + "T" * 12)], bound(0, 1000, 1038, "AC"),
                    witness=lambda r: counts(r) == [13]))
    out.append(Case("a", "unit-n", [rd(900, "150M", "T" * 100 + "N" * 10 + "T" * 40)], bound(0, 1000, 1010, "N"), witness=lambda r: counts(r) == [10]))
    out.append(Case("a", "read-starts-inside", [rd(1005, "100M", "AC" * 50)], bound(0, 1000, 1030, "AC"), witness=lambda r: counts(r) == [12]))
    out.append(Case("a", "read-ends-inside", [rd(950, "70M", "AC" * 35)], bound(0, 1000, 1030, "AC"), witness=lambda r: counts(r) == [10]))
    out.append(Case("a", "left-equals-right", [rd(900, "150M", "A" * 150)], bound(0, 1000, 1000, "A"), witness=lambda r: counts(r) == [0] and types(r) == [1]))
    out.append(Case("a", "count-300-wraps", [rd(950, "400M", "A" * 400)], bound(0, 1000, 1300, "A"), witness=lambda r: counts(r) == [44]))
    return out


# ---- b. the CIGAR walk ----------------------------------------------------------------------------------------------------
def family_b():
    out = []
    B = bound(0, 1000, 1020, "A")

    def one(name, pos, cigar, want, b=B, **kw):
        """a read of A's: its count is the length of the query stretch find_read_position cuts out, 0 below the 70 % cut"""
        out.append(Case("b", name, [rd(pos, cigar, "A" * query_len(cigar), **kw)], b, witness=lambda r, w=want: counts(r) == [w]))

    one("left-at-end-of-m", 900, "100M10I50M", 30)
    one("right-at-end-of-m", 900, "120M5D30M", 20)
    one("left-inside-d", 900, "90M20D60M", 100)
    one("left-inside-n", 900, "90M20N60M", 100)
    one("right-inside-d", 900, "110M20D40M", 50)
    one("right-inside-n", 900, "110M20N40M", 50)
    one("left-behind-an-i", 950, "50M7I100M", 20, b=bound(0, 1001, 1021, "A"))
    one("left-at-an-i", 950, "50M7I100M", 27)                                  # position == r_off at the M's end: the query offset in front of the I
    one("bound-at-first-base", 1000, "60M", 60, b=bound(0, 1000, 1100, "A"))    # over == q_off: position 0, not -1
    one("bound-at-first-base-narrow", 1000, "60M", 20)
    one("over-exceeds-q-off", 1000, "10M100D10M", 0, b=bound(0, 1015, 1200, "A"))
    one("leading-s", 1000, "10S50M", 50, b=bound(0, 1000, 1100, "A"))           # find_read_position gives 10: the first aligned base
    one("leading-h", 1000, "10H50M", 0, b=bound(0, 1000, 1100, "A"))            # H consumes nothing: -1, and the right end is outside too
    one("leading-h-right-inside", 1000, "10H50M", 20)
    one("leading-s-and-h", 990, "5H10S80M", 20)
    one("eq-x-p", 950, "30=5X2P65=", 20)
    out.append(Case("b", "no-cigar-placed-unmapped", [rd(1005, "*", "A" * 50, flag=0x1 | 0x4, mapq=0)], B, min_mapq=0,
                    witness=lambda r: counts(r) == [0] and types(r) == [2]))
    out.append(Case("b", "unmapped-with-cigar", [rd(1005, "50M", "A" * 50, flag=0x1 | 0x4, mapq=0)], B, min_mapq=0,
                    witness=lambda r: counts(r) == [15] and types(r) == [2]))
    out.append(Case("b", "ins-del-300", [rd(900, "50M300I50M300D100M")], B,
                    witness=lambda r: types(r) == [1] and int(reads(r)[0]["cigar_ins"]) == 44 and int(reads(r)[0]["cigar_del"]) == 44))
    out.append(Case("b", "ins-del-sum-wraps", [rd(900, "40M100I10M100I10M100I40M90D10M90D10M90D50M")], B,
                    witness=lambda r: types(r) == [1] and int(reads(r)[0]["cigar_ins"]) == 44 and int(reads(r)[0]["cigar_del"]) == 14))
    for width in (0, 4, 5, 40):
        for k in (1, 6):
            left, right = 1000, 1000 + width
            slop = k - 1 + max(0, 5 - width)
            a, z = left - slop, right + slop
            recs = [rd(a - 1, f"{z + 1 - (a - 1)}M"), rd(a - 1, f"{z - (a - 1)}M"), rd(a, f"{z + 1 - a}M"), rd(a, f"{z + 200 - a}M")]
            out.append(Case("b", f"spanning-width{width}-k{k}", recs, bound(0, left, right, UNITS[k]), witness=lambda r: types(r) == [1, 2, 2, 2]))
    return out


# ---- c. the filters -------------------------------------------------------------------------------------------------------
def family_c():
    """window 0: the query is the bound itself, so a record on the query's edge would be an overlapping read (the overlap test
    is closed on both sides) if the filter let it through -- the supports name the kept records"""
    b = bound(0, 1000, 1100, "A")
    recs = [rd(900, "100M"),                     # 0  stop == beg: dropped
            rd(901, "100M"),                     # 1  stop == beg + 1
            rd(1050, "20M", tid=1),              # 2  another tid
            rd(1050, "20M", flag=0x100),         # 3
            rd(1050, "20M"),                     # 4
            rd(1050, "20M", flag=0x400),         # 5
            rd(1050, "20M", mapq=20),            # 6  mapq == min_mapq
            rd(1050, "20M", flag=0x800),         # 7
            rd(1050, "20M", mapq=19),            # 8  mapq == min_mapq - 1
            rd(1099, "20M"),                     # 9  start == end - 1
            rd(1100, "20M")]                     # 10 start == end: dropped
    return [Case("c", "filters-interleaved", recs, b, window=0, witness=lambda r: kept_by_support(r) == [1, 4, 6, 9])]


# ---- d. the spanning probability ------------------------------------------------------------------------------------------
def d_cases():
    """(name, records, bound, [is the record's probability nonzero, by design])"""
    out = []
    L, R = 5000, 5010                                       # width 10; ev_stop - 20 = 4990
    out.append(("start-at-stop-minus-20", [rd(4989, "100M"), rd(4990, "100M"), rd(4991, "100M"),
                                           rd(4989, "100M", flag=0x10), rd(4990, "100M", flag=0x10), rd(4991, "100M", flag=0x10)],
                bound(0, L, R, "A"), [True, False, False, False, True, True]))
    # reverse reads, dist = stop - 5010: dist + width of 19 and 20
    out.append(("dist-plus-width-19-20", [rd(4990, "29M", flag=0x10), rd(4990, "30M", flag=0x10)], bound(0, L, R, "A"), [False, True]))
    L2, R2 = 5000, 5040                                     # width 40: dist of 0 and -1 on either strand
    out.append(("dist-0-and-minus-1", [rd(5000, "100M"), rd(5001, "100M"), rd(5020, "19M", flag=0x10), rd(5020, "20M", flag=0x10)],
                bound(0, L2, R2, "A"), [True, False, False, True]))
    # dist + 20 + width of 4094, 4095 and 4096: forward dist = 5000 - start, reverse dist = stop - 5010
    out.append(("dist-at-4095", [rd(934, "100M"), rd(935, "100M"), rd(936, "100M"),
                                 rd(4990, "50M3984N50M", flag=0x10), rd(4990, "50M3985N50M", flag=0x10), rd(4990, "50M3986N50M", flag=0x10)],
                bound(0, L, R, "A"), [False, None, True, True, None, False]))
    return out


def _d_witness(recs, b, want, frag):
    """the oracle's probability of every record is nonzero on one side of each edge and zero on the other.  At dist + 20 + width
    = 4095 (want None) the probability is 1 - cd[4095] = 0 with any table of orc_cumulative, as behind the comparison: there the
    edge shows with synthetic_cd() only, nonzero at 4095 and zero at 4096"""
    rec = batch(recs)
    cd, syn = cumulative(frag), synthetic_cd()
    left, right = int(b["left"]), int(b["right"])

    def w(ref):
        for i, nz in enumerate(want):
            args = (int(rec.pos[i]), rec_stop(rec, i), int(rec.flag[i]) & 0x10, left, right)
            p = probability(cd, *args)
            if nz is None:
                if p != 0 or probability(syn, *args) <= 0:
                    return False
            elif (p > 0) != nz or (probability(syn, *args) > 0) != nz:
                return False
        return ref[2] > 0
    return w


def family_d():
    return [Case("d", name, recs, b, window=4095, witness=_d_witness(recs, b, want, FRAG_WIDE)) for name, recs, b, want in d_cases()]


# ---- e. pairs ---------------------------------------------------------------------------------------------------------------
def _pair(name, isize, mtid=0, left=800, right=1100, tid=0):
    return [rd(left, "100M", name=name, flag=0x1 | 0x20 | 0x40, tid=tid, mtid=mtid, mpos=right, isize=isize),
            rd(right, "100M", name=name, flag=0x1 | 0x10 | 0x80, tid=tid, mtid=mtid, mpos=left, isize=-isize if isize != INT32_MIN else INT32_MIN)]


def family_e():
    B = bound(0, 1000, 1020, "AC")
    out = []

    def frag_lens(r):
        return sorted(int(s["frag_len"]) for s in fragments(r))

    out.append(Case("e", "both-mates", _pair(b"p", 400), B, witness=lambda r: frag_lens(r) == [400]))
    for isz, want in ((5000, [5000]), (-5000, [5000]), (5001, []), (-5001, []), (INT32_MIN, [])):
        out.append(Case("e", f"isize{isz}", _pair(b"p", isz), B, witness=lambda r, w=want: frag_lens(r) == w and len(reads(r)) == 0))
    out.append(Case("e", "mtid-differs", _pair(b"p", 400, mtid=1), B, witness=lambda r: frag_lens(r) == []))
    out.append(Case("e", "mtid-minus-1", _pair(b"p", 400, mtid=-1), B, witness=lambda r: frag_lens(r) == []))
    three = _pair(b"p", 400) + [rd(1150, "100M", name=b"p", flag=0x1 | 0x10 | 0x80, mtid=0, mpos=800, isize=-450)]
    out.append(Case("e", "three-under-one-name", three, B, witness=lambda r: frag_lens(r) == []))
    mixed = [_pair(b"p", 400)[0], _pair(b"q", 5001)[0], _pair(b"s", 300)[0], _pair(b"p", 400)[1], _pair(b"q", 5001)[1], _pair(b"s", 300)[1]]
    out.append(Case("e", "pairs-interleaved", mixed, B, witness=lambda r: frag_lens(r) == [300, 400]))
    return out


# ---- f. depth and median ----------------------------------------------------------------------------------------------------
def family_f():
    out = []
    for D, width, window in ((1, 1, 0), (2, 2, 0), (255, 255, 0), (256, 256, 0), (257, 257, 0), (MAX_SPAN, 1000, 4095)):
        left = 5000
        wl, wr = left - window, left + width + window
        # three records over the whole array (the first starts in front of wl: slot 0; they end behind it: slot D - 1), one
        # that ends exactly at slot D - 1, one that ends in front of it
        recs = [rd(wl - 5, f"{D + 10}M"), rd(wl, f"{D + 1}M"), rd(wl, f"{D + 300}M"), rd(wl, f"{D}M")]
        if D > 2:
            recs.append(rd(wl + 1, f"{D - 2}M"))
        want = 0 if D == 1 else (4 if D == 2 else 5)        # D == 1: +1 and -1 meet in the one slot; D == 2: the tie rule below
        out.append(Case("f", f"depth-n{D}-window{window}", recs, bound(0, left, left + width, "A"), window=window,
                        witness=lambda r, w=want: r[1] == w))
    b = bound(0, 1000, 1020, "A")
    out.append(Case("f", "stacked-1200", [rd(970, "100M") for _ in range(1200)], b, window=0, witness=lambda r: r[1] == 1047))
    # even D = 256, slots 0 .. 127 at depth 1 and 128 at depth 0: the running sum is D / 2 exactly at depth 0 and passes it at
    # depth 1; with one slot fewer at depth 1 the sum passes D / 2 at depth 0; odd D = 257 has no tie
    b256, b257 = bound(0, 5000, 5256, "A"), bound(0, 5000, 5257, "A")
    out.append(Case("f", "median-tie-even", [rd(5001, "128M")], b256, window=0, witness=lambda r: r[1] == 1))
    out.append(Case("f", "median-below-tie-even", [rd(5001, "127M")], b256, window=0, witness=lambda r: r[1] == 0))
    out.append(Case("f", "median-odd-129-of-257", [rd(5001, "129M")], b257, window=0, witness=lambda r: r[1] == 1))
    out.append(Case("f", "median-odd-128-of-257", [rd(5001, "128M")], b257, window=0, witness=lambda r: r[1] == 0))
    return out


# ---- g. names ---------------------------------------------------------------------------------------------------------------
def family_g():
    out = []
    B = bound(0, 1000, 1020, "AC")
    x, y = COLLIDING
    assert nim_hash(x) == nim_hash(y) == 0x14a79bc7 and x != y
    px, py = _pair(x, 400), _pair(y, 380, left=810, right=1090)
    # prob > 0 for all four (forward in front of the bound, reverse behind it; FRAG_WIDE): two names fold two values each
    out.append(Case("g", "colliding-names", [px[0], py[0], py[1], px[1]], B,
                    witness=lambda r: sorted(int(s["frag_len"]) for s in fragments(r)) == [380, 400] and r[2] > 0))
    for ln in (0, 1, 2, 3, 4, 5, 254):
        nm = bytes((0x41 + (j % 26)) for j in range(ln))
        out.append(Case("g", f"name-length-{ln}", [rd(990, "50M", name=nm), rd(995, "50M", name=b"other")], B, witness=lambda r: types(r) == [1, 1]))
    out.append(Case("g", "two-empty-names", _pair(b"", 400), B, witness=lambda r: len(fragments(r)) == 1))
    n = MAX_RECORDS
    same = [rd(900 + i // 50, "30M", name=b"same", flag=0x1, mtid=0, mpos=900, isize=100) for i in range(n)]
    out.append(Case("g", "4096-one-name", same, B, witness=lambda r: len(fragments(r)) == 0 and len(reads(r)) > 50 and r[2] > 0))
    dist = [rd(900 + i // 50, "30M", name=b"n%04d" % i, flag=0x1, mtid=0, mpos=900, isize=100) for i in range(n)]
    out.append(Case("g", "4096-distinct-names", dist, B, witness=lambda r: len(fragments(r)) == 0 and len(reads(r)) > 50 and r[2] > 0))
    return out


# ---- h. counts and layout -----------------------------------------------------------------------------------------------------
def _short(n, mapq=60):
    """n short records, every fourth one dropped by its flag so that the kept ones have gaps in every ballot word"""
    return [rd(960 + i // 128, "80M", "AC" * 40, flag=0x400 if i % 4 == 3 else 0, mapq=mapq) for i in range(n)]


def small_region():
    """the region of the alignment cases: a pair that spans, a read that overlaps, a dropped record"""
    return _pair(b"al", 400) + [rd(990, "50M", "AC" * 25), rd(995, "50M", flag=0x800)]


def family_h():
    out = []
    B = bound(0, 1000, 1020, "AC")
    for n in (0, 1, 255, 256, 257, MAX_RECORDS):
        kept = n - n // 4
        out.append(Case("h", f"records-{n}", _short(n), B, witness=lambda r, k=kept: len(reads(r)) == k and set(counts(r)) <= {9, 10}))
    out.append(Case("h", "all-dropped", _short(300, mapq=3), B, witness=lambda r: len(r[0]) == 0 and r[1] == 0))
    out.append(Case("h", "read-of-20000-bases", [rd(100, "20000M", "AC" * 10000), rd(9000, "100M", "AC" * 50)], bound(0, 9000, 9100, "AC"),
                    witness=lambda r: counts(r) == [50, 50] and types(r) == [1, 2]))
    s = small_region()
    out.append(Case("h", "small-region", sorted(s, key=lambda r: r["pos"]), B, witness=lambda r: len(fragments(r)) == 1 and counts(r) == [10]))
    return out


# ---- i. refused bytes ---------------------------------------------------------------------------------------------------------
def _offsets(raw):
    off, p = [], 0
    while p < len(raw):
        off.append(p)
        p += 4 + struct.unpack_from("<I", raw, p)[0]
    return off


def _patch(raw, at, fmt, v):
    b = bytearray(raw)
    struct.pack_into(fmt, b, at, v)
    return bytes(b)


def family_i():
    B = bound(0, 1000, 1020, "A")
    good = raw_of(batch([rd(950, "100M", "A" * 100), rd(960, "100M", "A" * 100), rd(970, "100M", "A" * 100)]))
    off = _offsets(good)
    size = len(good) - off[2]
    out = [("cut-in-header", good[:off[2] + 20]),
           ("cut-in-body", good[:off[2] + 50]),
           ("block-size-31", _patch(good, off[1], "<I", 31)),
           ("block-size-past-the-range", _patch(good, off[2], "<I", size - 4 + 100)),
           ("l-seq-negative", _patch(good, off[1] + 20, "<i", -1)),
           ("fields-exceed-block-size", _patch(good, off[1] + 16, "<H", 60000))]
    cases = [Case("i", name, None, B, raw=raw) for name, raw in out]
    cases.append(Case("i", "cigar-exceeds-seq", batch([rd(950, "100M", "A" * 10)]), B))
    cases.append(Case("i", "records-4097", batch([rd(990, "30M") for _ in range(MAX_RECORDS + 1)]), B))
    return cases


@functools.lru_cache(maxsize=None)
def answered():
    """the cases of a .. h, in table order"""
    return tuple(family_a() + family_b() + family_c() + family_d() + family_e() + family_f() + family_g() + family_h())


@functools.lru_cache(maxsize=None)
def refused():
    return tuple(family_i())


@functools.lru_cache(maxsize=None)
def references():
    """{case id: oracle.spanners(...)} of every answered case, computed once and shared"""
    return {c.id: O.spanners(c.rec, c.bound, c.window, c.frag, c.min_mapq) for c in answered()}


def alignment_regions():
    """the small region behind fillers (valid one-record regions whose name length sets their size) so that its first byte takes
    every alignment mod 16 in the joined buffer: [(raw, bound, is_copy)], the residues reached"""
    B = bound(0, 1000, 1020, "AC")
    small = raw_of(batch(sorted(small_region(), key=lambda r: r["pos"])))
    regions, at, reached = [], 0, []
    for want in range(16):
        base = len(raw_of(batch([rd(990, "30M", name=b"f")])))
        ln = 1 + (want - at - base) % 16
        fill = raw_of(batch([rd(990, "30M", name=b"f" * ln)]))
        regions.append((fill, B, False))
        at += len(fill)
        reached.append(at % 16)
        regions.append((small, B, True))
        at += len(small)
    return regions, reached
