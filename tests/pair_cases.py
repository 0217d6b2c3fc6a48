"""Inputs that put the device pair logic (strling_amd/csrc/pair.hip) on its arithmetic and staging edges.

Plain builders, no GPU code: every builder is fully determined by its arguments and comes with conditions that are checked on
the ORACLE's output alone (`*_conditions`), so that a test built on it cannot compare two empty results.  The CPU half of
tests/test_pair_edges.py asserts the conditions and runs the host twins; the -m gpu half asserts them again and runs the same
inputs through the kernels.
"""
import ctypes as C
import functools
import itertools

import numpy as np

from oracle import oracle as O
from strling_amd import api
from strling_amd.records import RecordBatch

F_PAIRED, F_PROPER, F_UNMAP, F_MUNMAP, F_REVERSE, F_MREVERSE, F_READ1, F_READ2, F_SECONDARY, F_SUPPL = 1, 2, 4, 8, 0x10, 0x20, 0x40, 0x80, 0x100, 0x800
LEFT, RIGHT, BOTH, NONE, NONE_RIGHT, NONE_LEFT = 0, 1, 2, 3, 4, 5          # tread.split (cluster.nim:13-21)
TREAD_FIELDS = ("tid", "position", "repeat", "flag", "split", "mapping_quality", "repeat_count", "align_length", "qname_id")
PQ = [(0.8, 40), (0.5, 0)]           # (proportion_repeat, min_mapq) every record-level case is run with
MEDIAN = 350


def _rng(*seed):
    return np.random.Generator(np.random.Philox(key=[int(sum((s + 1) * 1000003 ** i for i, s in enumerate(seed))) % (1 << 63), 0]))


def fmix64(h):
    """common.h fmix64 on a uint64 array"""
    h = np.asarray(h, np.uint64).copy()
    with np.errstate(over="ignore"):
        h ^= h >> np.uint64(33); h *= np.uint64(0xff51afd7ed558ccd)
        h ^= h >> np.uint64(33); h *= np.uint64(0xc4ceb9fe1a85ec53)
        h ^= h >> np.uint64(33)
    return h


def to_oracle(t):
    out = np.zeros(len(t), O.TREAD_DTYPE)
    for f in TREAD_FIELDS:
        out[f] = t[f]
    return out


# ---- 1. the rule functions on a grid ------------------------------------------------------------------------------------
RULE_OPTS = [(p, q, med) for q in (0, 40) for p in (0.8, 0.5) for med in (0, 350, 4000)]      # (p, min_mapq, frag_median)
COUNTS = [0, 1, 30, 50, 85, 86, 100, 128, 255]
KS = [1, 2, 3, 4, 5, 6]
ALS = [0, 1, 30, 44, 150, 255]
FLAGS = [a | b | c for a in (0, F_PROPER) for b in (0, F_REVERSE) for c in (0, F_MREVERSE)]
SPLITS = [LEFT, RIGHT, BOTH, NONE, NONE_RIGHT, NONE_LEFT]
B_POSITIONS = [0, 10, 349, 350, 351, 2 ** 31, 2 ** 32 - 1]
A_POSITIONS = [0, 1000, 2 ** 32 - 1]
UNITS = {1: [b"A", b"G"], 2: [b"AC", b"CT"], 3: [b"CAG", b"AAT"], 4: [b"AAAG", b"CTTT"], 5: [b"AACCT", b"AGGTT"], 6: [b"AACCGT", b"ACTGCT"]}
A_TID, B_TID = 7, 3            # distinct, so that `A.tid = B.tid` (extract.nim:171) shows in the output
# (count, k, align_length) whose proportion sits exactly on a threshold or whose uint8 product wraps: 120/150 = 0.8, 30/150 = 0.2,
# 15/30 = 0.5, 6/30 = 0.2, 100 x 3 = 300 -> 44, 86 x 3 = 258 -> 2, 128 x 2 = 256 -> 0
TIES = [(30, 4, 150), (30, 1, 150), (15, 1, 30), (6, 1, 30), (100, 3, 150), (100, 3, 44), (86, 3, 150), (128, 2, 150)]
# the factors of one case, in the order of the columns of RuleGrid.factors
FACTORS = [("a_count", len(COUNTS)), ("a_k", 6), ("a_al", len(ALS)), ("a_mapq", 5), ("a_flag", 8), ("a_pos", len(A_POSITIONS)), ("a_unit", 2),
           ("b_count", len(COUNTS)), ("b_k", 6), ("b_al", len(ALS)), ("b_mapq", 5), ("b_flag", 8), ("b_split", 6), ("b_pos", len(B_POSITIONS)),
           ("b_unit", 2), ("min_mapq", 2), ("p", 2), ("median", 3)]
N_CASE_FACTORS = 15            # the rest are the option set
RULE_SAMPLE = 2100             # random cases per option set: 12 x 2100 = 25 200 in all


def mapq_values(min_mapq):
    """{0, min_mapq - 1, min_mapq, min_mapq + 1, 60}; below 0 there is nothing: the value repeats 0"""
    return [0, max(min_mapq - 1, 0), min_mapq, min_mapq + 1, 60]


class RuleGrid:
    """A, B (api.TREAD_DTYPE), B_position, and the option set of every case; cases of one option set are contiguous"""

    def __init__(self, A, B, bpos, opt, factors):
        self.A, self.B, self.bpos, self.opt, self.factors = A, B, bpos, opt, factors
        self.n = len(A)

    def of_opts(self, j):
        return np.flatnonzero(self.opt == j)


def _treads_from(count, k, al, mapq, flag, pos, unit_v, tid, split):
    t = np.zeros(len(count), api.TREAD_DTYPE)
    t["repeat_count"], t["align_length"], t["mapping_quality"], t["flag"], t["position"], t["tid"], t["split"] = count, al, mapq, flag, pos, tid, split
    t["repeat"] = [UNITS[int(kk)][int(u)] for kk, u in zip(k, unit_v)]
    return t


@functools.lru_cache(maxsize=None)
def rule_grid():
    """the seeded sample of the cross product of the issue's values (every pairwise combination present, see
    rule_grid_conditions) plus, per option set, the exact ties and wrapping products crossed with each other"""
    parts, opt, fac = [], [], []
    for j, (p, q, med) in enumerate(RULE_OPTS):
        rng = _rng(11, j)
        f = np.stack([rng.integers(0, n, RULE_SAMPLE) for _, n in FACTORS[:N_CASE_FACTORS]], axis=1)
        # ties: A's triple x B's triple x the mapq of both at and just above min_mapq, the rest random
        tie = [(a, b, ma, mb) for a in range(len(TIES)) for b in range(len(TIES)) for ma in (2, 3) for mb in (2, 3)]
        g = np.stack([rng.integers(0, n, len(tie)) for _, n in FACTORS[:N_CASE_FACTORS]], axis=1)
        mq = np.asarray(mapq_values(q))

        def build(ff, tie_rows=None):
            cols = {name: ff[:, c] for c, (name, _) in enumerate(FACTORS[:N_CASE_FACTORS])}
            ac, ak, aal = np.asarray(COUNTS)[cols["a_count"]], np.asarray(KS)[cols["a_k"]], np.asarray(ALS)[cols["a_al"]]
            bc, bk, bal = np.asarray(COUNTS)[cols["b_count"]], np.asarray(KS)[cols["b_k"]], np.asarray(ALS)[cols["b_al"]]
            am, bm = mq[cols["a_mapq"]], mq[cols["b_mapq"]]
            if tie_rows is not None:
                ta, tb = np.asarray([TIES[r[0]] for r in tie_rows]), np.asarray([TIES[r[1]] for r in tie_rows])
                ac, ak, aal, bc, bk, bal = ta[:, 0], ta[:, 1], ta[:, 2], tb[:, 0], tb[:, 1], tb[:, 2]
                am, bm = mq[[r[2] for r in tie_rows]], mq[[r[3] for r in tie_rows]]
            A = _treads_from(ac, ak, aal, am, np.asarray(FLAGS)[cols["a_flag"]], np.asarray(A_POSITIONS, np.uint64)[cols["a_pos"]].astype(np.uint32),
                             cols["a_unit"], A_TID, LEFT)
            B = _treads_from(bc, bk, bal, bm, np.asarray(FLAGS)[cols["b_flag"]], 0, cols["b_unit"], B_TID, np.asarray(SPLITS)[cols["b_split"]])
            bpos = np.asarray(B_POSITIONS, np.uint64)[cols["b_pos"]].astype(np.uint32)
            B["position"] = bpos
            return A, B, bpos

        for ff, rows in ((f, None), (g, tie)):
            parts.append(build(ff, rows))
            opt.append(np.full(len(ff), j))
        o3 = np.tile([[(0, 40).index(q), (0.8, 0.5).index(p), (0, 350, 4000).index(med)]], (len(f), 1))
        fac.append(np.concatenate([f, o3], axis=1))
    A = np.concatenate([x[0] for x in parts]); B = np.concatenate([x[1] for x in parts]); bpos = np.concatenate([x[2] for x in parts])
    for i, t in enumerate((A, B)):
        t["qname_id"] = np.arange(len(t)) * 2 + i
    return RuleGrid(A, B, bpos, np.concatenate(opt), np.concatenate(fac))


def rule_grid_conditions(grid):
    """what the sample itself must hold: size, every pairwise combination of the factors' values (option sets included), the ties"""
    f = grid.factors
    assert len(f) >= 20_000 and grid.n > len(f)
    for (c0, (n0, m0)), (c1, (n1, m1)) in itertools.combinations(enumerate(FACTORS), 2):
        seen = np.unique(f[:, c0] * m1 + f[:, c1])
        assert seen.size == m0 * m1, (n0, n1, seen.size)
    triple = lambda t: set(zip(t["repeat_count"].tolist(), [len(r) for r in t["repeat"]], t["align_length"].tolist()))
    for t in (grid.A, grid.B):
        assert set(TIES) <= triple(t)
    for j in range(len(RULE_OPTS)):       # ... each with each, under every option set
        idx = grid.of_opts(j)
        assert {(a, b) for a in TIES for b in TIES} <= set(zip(_triples(grid.A[idx]), _triples(grid.B[idx])))


def _triples(t):
    return list(zip(t["repeat_count"].tolist(), [len(r) for r in t["repeat"]], t["align_length"].tolist()))


def _oracle_rule(op, A, B, bpos, opts):
    """orc_adjust_by / orc_unplaced_pair case by case -> (results, A after) in the oracle's dtype"""
    L = O.lib()
    a, b = to_oracle(A), to_oracle(B)
    o = O.make_opts(int(opts[2]), float(opts[0]), int(opts[1]))
    res = np.zeros(len(a), np.int32)
    PT, sz, pa, pb = C.POINTER(O.Tread), O.TREAD_DTYPE.itemsize, a.ctypes.data, b.ctypes.data
    for i in range(len(a)):
        x, y = C.cast(pa + i * sz, PT), C.cast(pb + i * sz, PT)
        res[i] = L.orc_adjust_by(x, y, C.byref(o), int(bpos[i])) if op == 0 else L.orc_unplaced_pair(x, y, C.byref(o))
    return res, a


def oracle_p_repeat(t):
    L = O.lib()
    a = to_oracle(t)
    PT, sz, pa = C.POINTER(O.Tread), O.TREAD_DTYPE.itemsize, a.ctypes.data
    return np.array([L.orc_p_repeat(C.cast(pa + i * sz, PT)) for i in range(len(a))])


@functools.lru_cache(maxsize=None)
def rule_expect():
    """{(op, option set): (case indices, oracle results, oracle's A after)} for op 0 (adjust_by) and 1 (unplaced_pair)"""
    g = rule_grid()
    out = {}
    for j, opts in enumerate(RULE_OPTS):
        idx = g.of_opts(j)
        for op in (0, 1):
            res, a = _oracle_rule(op, g.A[idx], g.B[idx], g.bpos[idx], opts)
            out[(op, j)] = (idx, res, a)
    return out


def rule_conditions(grid, expect):
    """every outcome of the two rules, as the ORACLE decided it, is taken at least 50 times -> the counts"""
    n = dict(ret_false=0, placed_by_mate=0, own_middle=0, untouched=0, pos_reverse=0, pos_reverse_exact=0, pos_forward=0, pos_forward_exact=0,
             below_zero=0, unplaced_both=0, unplaced_a_lowq_b=0, unplaced_b_lowq_a=0, unplaced_false=0, wrapped_product=0)
    for j, (p, q, med) in enumerate(RULE_OPTS):
        idx, res, a = expect[(0, j)]
        A, B, bpos = grid.A[idx], grid.B[idx], grid.bpos[idx].astype(np.int64)
        n["ret_false"] += int((res == 0).sum())
        first = (res == 1) & (a["tid"] == B_TID)                      # extract.nim:171: only the first arm moves A to B's contig
        changed = (a["position"] != A["position"]) | (a["mapping_quality"] != A["mapping_quality"])
        n["placed_by_mate"] += int(first.sum())
        n["own_middle"] += int(((res == 1) & ~first & changed).sum())            # a lower bound: align_length 0 moves nothing
        n["untouched"] += int(((res == 1) & ~first & ~changed).sum())
        rev, nl, nr = (B["flag"] & F_REVERSE) != 0, B["split"] == NONE_LEFT, B["split"] == NONE_RIGHT
        n["pos_reverse"] += int((first & rev & ~nl).sum())
        n["pos_reverse_exact"] += int((first & rev & nl).sum())
        n["pos_forward"] += int((first & ~rev & ~nr).sum())
        n["pos_forward_exact"] += int((first & ~rev & nr).sum())
        assert np.array_equal(a["position"][first & rev & nl], B["position"][first & rev & nl])
        # B_position + B.align_length + half <= B_position + 255 + 128: anything farther right came round from below zero
        n["below_zero"] += int((first & rev & ~nl & (a["position"].astype(np.int64) > bpos + 383)).sum())
        idx, res, _ = expect[(1, j)]
        pa, pb = oracle_p_repeat(A), oracle_p_repeat(B)
        both = (pa > p) & (pb > p)
        arm2 = ~both & (pa > p) & (B["mapping_quality"] < q)
        assert np.array_equal(res == 1, both | arm2 | ((pb > p) & (A["mapping_quality"] < q)))
        n["unplaced_both"] += int(both.sum())
        n["unplaced_a_lowq_b"] += int(arm2.sum())
        n["unplaced_b_lowq_a"] += int(((res == 1) & ~both & ~arm2).sum())
        n["unplaced_false"] += int((res == 0).sum())
        k = np.array([len(r) for r in A["repeat"]])
        n["wrapped_product"] += int((A["repeat_count"].astype(np.int64) * k > 255).sum())
    assert all(v >= 50 for v in n.values()), n
    return n


def all_units():
    """every unit of 1..6 bases over ACGT: 5460"""
    return [("".join(u)).encode() for k in range(1, 7) for u in itertools.product("ACGT", repeat=k)]


# ---- 2. crafted records --------------------------------------------------------------------------------------------------
LENGTHS = [150, 255, 256, 257, 300, 384, 510]
TRACT_UNITS = {1: ["A", "T", "C"], 2: ["AC", "GT", "AG", "CT"], 3: ["CAG", "CTG", "AAT", "CCG"], 4: ["AAAG", "CTTT", "ACGT", "AATG"],
               5: ["AACCT", "AGGTT", "AAAAT"], 6: ["AACCGT", "ACTGCT", "AAAAAG"]}
MAPQS = [0, 39, 40, 41, 60]
OTHER = {"A": "C", "C": "G", "G": "T", "T": "A"}


def _rand(rng, n):
    return np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].tobytes().decode()


def _tract(rng, unit, n, n_bad=0):
    """n bases of `unit` from a random phase, n_bad of them replaced by another base"""
    s = list((unit * (n // len(unit) + 2))[int(rng.integers(0, len(unit))):][:n])
    for j in rng.choice(n, min(n_bad, n), replace=False) if n_bad else []:
        s[int(j)] = OTHER[s[int(j)]]
    return "".join(s)


def _unit_for(rng, L):
    """a unit whose tract of L bases keeps repeat_count below 256 (doAssert extract.nim:72): L / k <= 255, and beyond 255 bases
    no base makes up more than half of the unit, so that its count as a 1-mer stays below 256 as well"""
    k = int(rng.choice([k for k in range(1, 7) if L // k <= 255]))
    units = [u for u in TRACT_UNITS[k] if L <= 255 or max(u.count(b) for b in "ACGT") * 2 <= len(u)]
    return units[int(rng.integers(0, len(units)))]


def _read(rng, kind, L):
    if kind == "rand":
        return _rand(rng, L)
    unit = _unit_for(rng, L)
    return _tract(rng, unit, L, 0 if kind == "rep" else int(rng.integers(1, max(2, L // 12))))


@functools.lru_cache(maxsize=None)
def crafted_batch(reps=10, n_clip=3000, seed=5):
    """-> (RecordBatch in coordinate order with the unmapped tail last, n_tail)"""
    rng = _rng(seed)
    rows = []          # (tid, pos, mtid, mpos, flag, mapq, cigar, seq, qname)
    gi = 0

    def name(fam):
        nonlocal gi
        gi += 1
        return "%s%06d" % (fam, gi)

    def place(kind, slot):
        """((tid, pos) of read 1, (tid, pos) of read 2)"""
        base = 3000 + 700 * slot
        if kind == "normal": return (0, base), (0, base + 310)
        if kind == "swapped": return (0, base + 310), (0, base)
        if kind in ("equal12", "equal21"): return (0, base), (0, base)
        if kind == "mate_higher_tid": return (0, base), (1, 500 + slot)
        if kind == "mate_lower_tid": return (1, 500 + slot), (0, base)
        if kind == "pos0": return (0, 0), (0, int(rng.integers(0, 400)))
        if kind == "near0": return (0, int(rng.integers(0, 60))), (0, int(rng.integers(0, 60)))
        raise AssertionError(kind)

    PLACES = ["normal", "swapped", "equal12", "equal21", "mate_higher_tid", "mate_lower_tid", "pos0", "near0", "near0", "near0", "mate_unmapped",
              "both_unmapped"]
    KINDS = [("rep", "rand"), ("rand", "rep"), ("rep", "rep"), ("near", "rand"), ("rep", "near"), ("rand", "rand")]
    slot = 0
    for rep in range(reps):
        for rev, mrev, proper, mq1, mq2 in itertools.product((0, 1), (0, 1), (0, 1), MAPQS, MAPQS):
            slot += 1
            q = name("p")
            k1, k2 = KINDS[int(rng.integers(0, len(KINDS)))]
            s1, s2 = _read(rng, k1, int(rng.choice(LENGTHS))), _read(rng, k2, int(rng.choice(LENGTHS)))
            pl = PLACES[int(rng.integers(0, len(PLACES)))]
            f1 = F_PAIRED | F_READ1 | (F_PROPER if proper else 0) | (F_REVERSE if rev else 0) | (F_MREVERSE if mrev else 0)
            f2 = F_PAIRED | F_READ2 | (F_PROPER if proper else 0) | (F_REVERSE if mrev else 0) | (F_MREVERSE if rev else 0)
            if pl == "both_unmapped":
                rows.append((-1, -1, -1, -1, 77, 0, "*", s1, q))
                rows.append((-1, -1, -1, -1, 141, 0, "*", s2, q))
                continue
            if pl == "mate_unmapped":            # the unmapped read sits beside its mate, with the mate's coordinates
                t, p = 0, 3000 + 700 * slot
                rows.append((t, p, t, p, (f1 | F_MUNMAP) & ~F_PROPER, mq1, "%dM" % len(s1), s1, q))
                rows.append((t, p, t, p, (f2 | F_UNMAP) & ~F_PROPER, 0, "*", s2, q))
                continue
            (t1, p1), (t2, p2) = place(pl, slot)
            r1 = (t1, p1, t2, p2, f1, mq1, "%dM" % len(s1), s1, q)
            r2 = (t2, p2, t1, p1, f2, mq2, "%dM" % len(s2), s2, q)
            rows.extend([r2, r1] if pl == "equal21" else [r1, r2])
            extra = slot % 12
            if extra == 0:                       # a third primary record under the qname
                rows.append((t1, p1 + 5, t2, p2, f1, mq1, "%dM" % len(s1), s1, q))
            elif extra == 1:
                rows.append((t1, p1 + 7, t2, p2, f1 | F_SECONDARY, mq1, "%dM" % len(s1), s1, q))
            elif extra == 2:
                rows.append((t2, p2 + 9, t1, p1, f2 | F_SUPPL, mq2, "%dM" % len(s2), s2, q))
    # soft-clipped reads: the clip a (near-)pure tract, the rest of the read random or a tract of the same unit
    for c in range(n_clip):
        slot += 1
        q = name("s")
        L = int(rng.choice([150, 150, 150, 300]))
        unit = _unit_for(rng, 40 if L == 150 else L)
        cl, cr = int(rng.choice([16, 17, 40])), int(rng.choice([16, 17, 40]))
        side = int(rng.integers(0, 4))           # left, right, both, a cigar of one S op
        bad = lambda n: int(rng.choice([0, 0, 1, 2, 3, 4, 5, 6])) if n == 40 else int(rng.choice([0, 0, 1, 2, 3]))
        body_rep = rng.random() < 0.6
        body = lambda n: _tract(rng, unit, n, int(rng.integers(0, 4))) if body_rep else _rand(rng, n)
        if side == 0: seq, cig = _tract(rng, unit, cl, bad(cl)) + body(L - cl), "%dS%dM" % (cl, L - cl)
        elif side == 1: seq, cig = body(L - cr) + _tract(rng, unit, cr, bad(cr)), "%dM%dS" % (L - cr, cr)
        elif side == 2: seq, cig = _tract(rng, unit, cl, bad(cl)) + body(L - cl - cr) + _tract(rng, unit, cr, bad(cr)), "%dS%dM%dS" % (cl, L - cl - cr, cr)
        else: seq, cig = _tract(rng, unit, L, int(rng.integers(0, 12))), "%dS" % L
        mq = int(rng.choice([60, 60, 41, 40, 39, 0]))
        mate = _rand(rng, 150)
        base = 3000 + 700 * slot
        first = rng.random() < 0.5                # the clipped read is seen before / after its mate: two thresholds (extract.nim:208, :242)
        pc, pm = (base, base + 320) if first else (base + 320, base)
        rev = int(rng.integers(0, 2))
        fc = F_PAIRED | F_PROPER | F_READ1 | (F_REVERSE if rev else F_MREVERSE)
        fm = F_PAIRED | F_PROPER | F_READ2 | (F_MREVERSE if rev else F_REVERSE)
        rows.append((0, pc, 0, pm, fc, mq, cig, seq, q))
        # (a mate at or below min_mapq cannot place the clipped read: its tread keeps none_left / none_right, extract.nim:149,177)
        rows.append((0, pm, 0, pc, fm, int(rng.choice([60, 60, 40, 40, 0, 0])), "150M", mate, q))
    order = sorted(range(len(rows)), key=lambda i: ((1 << 40) if rows[i][0] < 0 else (rows[i][0] << 32) + max(rows[i][1], 0)))
    rows = [rows[i] for i in order]
    rec = RecordBatch.from_fields(*[[r[j] for r in rows] for j in range(9)])
    return rec, int((rec.tid < 0).sum())


@functools.lru_cache(maxsize=None)
def crafted_scores(p, q):
    """the oracle's scorer results for every record; no count reaches 256 (the oracle, like the reference, stops there: extract.nim:72)"""
    rec, _ = crafted_batch()
    sc = O.score_records_packed(rec, None, O.make_opts(MEDIAN, p, q))
    assert int(sc[2].max()) < 256 and int(sc[4].max()) < 256
    return sc


@functools.lru_cache(maxsize=None)
def crafted_expect(p, q):
    rec, n_tail = crafted_batch()
    crafted_scores(p, q)
    return O.extract(rec, None, O.make_opts(MEDIAN, p, q), n_tail)


def crafted_conditions(rec, exp, p, q):
    """the minima of the crafted batch on the oracle's treads -> the counts reached"""
    sk, wu, wc, su, sc = crafted_scores(p, q)
    rid = exp["qname_id"]
    whole = np.isin(exp["split"], (NONE, NONE_LEFT, NONE_RIGHT))
    n = dict(treads=len(exp), align_length_not_l_seq=int((exp["align_length"] != rec.l_seq[rid]).sum()),
             unplaced=int((exp["tid"] == -1).sum()), beyond_2_31=int((exp["position"] > 2 ** 31).sum()),
             unit_changed=int((whole & (exp["repeat"] != wu[rid])).sum()),
             long_reads=int((rec.l_seq[rid] > 255).sum()),
             wrapped_product=int((exp["repeat_count"].astype(np.int64) * np.char.str_len(exp["repeat"]) > 255).sum()))
    for s in (LEFT, RIGHT, BOTH, NONE, NONE_RIGHT, NONE_LEFT):
        n["split_%d" % s] = int((exp["split"] == s).sum())
    # clip results on both sides of 0.9 (extract.nim:131), from the scorer's own words for the clipped ends
    k = np.char.str_len(su)
    clen = np.zeros(su.shape, np.int64)
    for i in range(rec.n):
        a, b = int(rec.cigar_off[i]), int(rec.cigar_off[i + 1])
        if b > a and (int(rec.cigar[a]) & 15) == 4: clen[i, 0:2] = int(rec.cigar[a]) >> 4
        if b > a and (int(rec.cigar[b - 1]) & 15) == 4: clen[i, 2:4] = int(rec.cigar[b - 1]) >> 4
    frac = np.where(clen > 0, ((sc * k) % 256) / np.maximum(clen % 256, 1), -1.0)
    n["clip_below_0.9"], n["clip_at_least_0.9"] = int(((frac >= 0) & (sc > 0) & (frac < 0.9)).sum()), int((frac >= 0.9).sum())
    flags = {int(f) & (F_REVERSE | F_MREVERSE | F_PROPER) for f in rec.flag}
    assert len(flags) == 8                                          # REVERSE x MREVERSE x PROPER
    assert n["align_length_not_l_seq"] >= 100 and n["unplaced"] >= 50 and n["beyond_2_31"] >= 20 and n["unit_changed"] >= 50, n
    assert all(n["split_%d" % s] >= 100 for s in (LEFT, RIGHT, NONE, NONE_RIGHT, NONE_LEFT)), n
    # no statement of extract.nim assigns Soft.both (:80 none, :85 none_left, :87 none_right, :126 left / right): the oracle has none
    assert n["split_%d" % BOTH] == 0, n
    assert n["long_reads"] >= 100 and n["wrapped_product"] >= 100 and n["clip_below_0.9"] >= 20 and n["clip_at_least_0.9"] >= 100, n
    return n


def cuts_between_mates(rec, n_tail):
    """record indices to cut a chunked run at: three between two adjacent records of one qname, one between the mates of an
    unmapped pair of the tail, and two that part mates lying far apart"""
    adj = [i + 1 for i in range(rec.n - n_tail - 1) if rec.qname(i) == rec.qname(i + 1)]
    tail = [i + 1 for i in range(rec.n - n_tail, rec.n - 1) if rec.qname(i) == rec.qname(i + 1)]
    assert len(adj) >= 3 and tail
    return sorted({adj[0], adj[len(adj) // 2], adj[-1], tail[len(tail) // 2], rec.n // 3, rec.n // 3 + 1})


# ---- 3. staging edges ----------------------------------------------------------------------------------------------------
HOT = "CAG" * 50


def hot_batch(groups):
    """all-hot batch: groups = [(qname, n records)]; every read 150 bases of CAG on 150M, so the join items are exactly the
    records.  Within a qname the records alternate before / after their mate: records 2j, 2j + 1 pair up and, both being
    repeats, come out as an unplaced pair (2 treads)."""
    tid, pos, mpos, flag, qn = [], [], [], [], []
    for g, (q, n) in enumerate(groups):
        for j in range(n):
            before = j % 2 == 0
            pos.append(1000 + g if before else 900_000 + g)
            mpos.append(900_000 + g if before else 1000 + g)
            flag.append(99 if before else 147)
            qn.append(q)
    n = len(pos)
    return RecordBatch.from_fields([0] * n, pos, [0] * n, mpos, flag, [60] * n, ["150M"] * n, [HOT] * n, qn)


def hot_expect(rec, p=0.8, q=40):
    return O.extract(rec, None, O.make_opts(MEDIAN, p, q), 0)


def one_qname(n, n_pairs=300):
    """one qname on n alternating records among n_pairs ordinary hot pairs"""
    return hot_batch([("pair%05d" % i, 2) for i in range(n_pairs // 2)] + [("many", n)] + [("pair%05d" % i, 2) for i in range(n_pairs // 2, n_pairs)])


def many_long_runs():
    """70 qnames of 20 records: more runs than pair_long_kernel has blocks (64)"""
    return hot_batch([("long%03d" % i, 20) for i in range(70)])


def hot_pairs(n):
    return hot_batch([("hp%06d" % i, 2) for i in range(n)])


PG_BLOCK = 512
# (block, index in the block, items) of the runs laid across the seams of pair_groups_kernel's 512-item blocks
SEAM_RUNS = [(0, 511, 15), (1, 498, 14), (2, 498, 15), (3, 505, 15), (4, 511, 16)]


def join_order(qhash):
    """DERIVED FROM pair.hip's JOIN ORDER -- re-derive if that changes: the join sorts the items by the low 32 bits of
    fmix64(qname hash) (strl_pair_device: radix_sort_pairs over bits [0, 32)), so the items of one qname are adjacent and the
    qnames follow each other by that key.  -> (low-32 key of every record, start of every run in the sorted item array, run lengths)"""
    lo = (fmix64(qhash) & np.uint64(0xFFFFFFFF)).astype(np.uint64)
    s = np.sort(lo, kind="stable")
    starts = np.flatnonzero(np.r_[True, s[1:] != s[:-1]])
    return lo, starts, np.diff(np.r_[starts, len(s)])


@functools.lru_cache(maxsize=None)
def seam_batch(n_names=1500):
    """qnames sized 2..16 in the order the join will put them, so that the runs of SEAM_RUNS start where they are named"""
    names = ["seam%05d" % i for i in range(n_names)]
    probe = RecordBatch.from_fields([0] * n_names, [0] * n_names, [0] * n_names, [0] * n_names, [99] * n_names, [60] * n_names, ["1M"] * n_names,
                                    ["A"] * n_names, names)
    lo = (fmix64(api.qname_hash(probe)) & np.uint64(0xFFFFFFFF))
    assert np.unique(lo).size == n_names                     # no two qnames share a run
    order = np.argsort(lo, kind="stable")
    sizes = np.zeros(n_names, np.int64)
    at, g = 0, 0
    for block, idx, items in SEAM_RUNS:
        target = block * PG_BLOCK + idx
        gap = target - at
        assert gap == 0 or gap >= 2
        if gap % 2:                                          # pairs, and one qname of three records where the gap is odd
            sizes[order[g]] = 3; g += 1; gap -= 3
        for _ in range(gap // 2):
            sizes[order[g]] = 2; g += 1
        sizes[order[g]] = items; g += 1
        at = target + items
    sizes[order[g:]] = 2
    return hot_batch([(names[i], int(sizes[i])) for i in range(n_names)])


def seam_conditions(rec, qhash, exp):
    """the layout, from the batch's own qname hashes (soa.pair_rows()), and what the oracle emits for it"""
    lo, starts, lens = join_order(qhash)
    assert len(lo) == rec.n and len(starts) == len({rec.qname(i) for i in range(rec.n)})
    assert lens.min() >= 2 and lens.max() == 16
    runs = dict(zip(starts.tolist(), lens.tolist()))
    for block, idx, items in SEAM_RUNS:
        assert runs.get(block * PG_BLOCK + idx) == items, (block, idx, items)
    assert (0 * PG_BLOCK + 511 + 15) > PG_BLOCK and 1 * PG_BLOCK + 498 + 14 == 2 * PG_BLOCK       # in the halo / ends on the seam
    n_blocks = -(-rec.n // PG_BLOCK)
    assert n_blocks >= 6
    assert len(exp) == int((lens // 2 * 2).sum()) and len(exp) > 256 * n_blocks     # pigeonhole: some block passes its 256-tread stage
    return dict(items=rec.n, runs=len(starts), blocks=n_blocks, treads=len(exp))
