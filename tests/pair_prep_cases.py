"""Inputs for what the replay of pair.hip prepares once per join item and what its group heads then only read: the two classes
of p_repeat, adjust_by's half, both forms of the unit, the unpacked soft-clip words, the place of the doAssert, and the treads
that are spelled out while the stage is copied out.

A batch is a list of qname groups IN JOIN ORDER, each a list of rows in file order (`build`): the names come from
pair_dense_cases._name_pool, so that a group can be put on a chosen item of a 512-item block.  Reads are written so that the
ORACLE's scorer gives them a chosen (repeat_count, unit, align_length) -- `READS` says which, `read_conditions` asserts it --
and every `*_conditions` function asserts on the oracle's treads alone that the case reaches the edge it is named for and that
its neighbour comes out differently, so that a comparison turned the wrong way round cannot hide.
"""
import functools

import numpy as np

import pair_cases as pc
import pair_dense_cases as dc
from helpers import oracle_words, soft_items_expected
from oracle import oracle as O
from strling_amd import api
from strling_amd.records import RecordBatch

PG_BLOCK, PG_HALO, PG_EMIT, PAIR_MAXM = 512, 16, 256, 15        # restated from pair.hip
NONE, NONE_RIGHT, NONE_LEFT = pc.NONE, pc.NONE_RIGHT, pc.NONE_LEFT
# 161 bases without a repeat: no k-mer of 2..6 bases comes near the scorer's thresholds
FILL = "ACGTTGCATGACTAGCTAGGATCCAGTCATGCAAGTCCGATAGCTTACGGATTCAGGCTAACGTTAGCCTGAATCGGTACCATGGTCAAGCTTGACGTCAGTACGCATTGCAGCTGATCGGCTATGCCAGTTAGCACTGAGTCCATGACGTTACAGGCATTCGA"


def tract(unit, copies, length):
    return (unit * copies + FILL * 8)[:length]


# name -> (sequence, unit the oracle finds, its count, (count * k) mod 256, align_length mod 256)
READS = {
    # 94 x 4 = 376 -> 120; 406 -> 150: 120 / 150 is 0.8 itself, 120 / 149 the first proportion above, 120 / 151 the first below
    "hi_on": (tract("AAAG", 94, 406), b"AAAG", 94, 120, 150),
    "hi_over": (tract("AAAG", 94, 405), b"AAAG", 94, 120, 149),
    "hi_under": (tract("AAAG", 94, 407), b"AAAG", 94, 120, 151),
    # 133 x 6 = 798 -> 30; 918 -> 150: 30 / 150 is 0.2 itself
    "lo_on": (tract("AAAAAG", 133, 918), b"AAAAAG", 133, 30, 150),
    "lo_over": (tract("AAAAAG", 133, 917), b"AAAAAG", 133, 30, 149),
    "lo_under": (tract("AAAAAG", 133, 919), b"AAAAAG", 133, 30, 151),
    # 132 x 2 = 264 -> 8; 300 -> 44: nine tenths of the read are the repeat, the uint8 proportion is 0.18
    "wrap": (tract("AC", 128, 300), b"CA", 132, 8, 44),
    # 256 -> align_length 0: the divisor becomes 1, the half 0
    "al0": (tract("AAG", 85, 256), b"AAG", 85, 255, 0),
    "hot": (pc.HOT, b"CAG", 50, 150, 150),
    "cold": (FILL[:150], b"", 0, 0, 150),
}
# units of every length: (read, unit found, canonical form); self = its own reverse complement, rc = the canonical form is the
# reverse complement's rotation, own = already canonical
UNITS = {
    "A_own": (tract("A", 150, 150), b"A", b"A"), "G_rc": (tract("G", 150, 150), b"G", b"C"),
    "AT_self": (tract("AT", 75, 150), b"AT", b"AT"), "CG_self": (tract("CG", 75, 150), b"CG", b"CG"),
    "AG_own": (tract("AG", 75, 150), b"AG", b"AG"), "CT_rc": (tract("CT", 75, 150), b"CT", b"AG"),
    "AAT_own": (tract("AAT", 50, 150), b"AAT", b"AAT"), "CTG_rc": (tract("CTG", 50, 150), b"CTG", b"CAG"), "CAG_own": (pc.HOT, b"CAG", b"CAG"),
    "ACGT_self": (tract("ACGT", 37, 150), b"CGTA", b"CGTA"), "AAAG_own": (tract("AAAG", 37, 150), b"AAAG", b"AAAG"),
    "CTTT_rc": (tract("CTTT", 37, 150), b"CTTT", b"AAAG"),
    "AAAAT_own": (tract("AAAAT", 30, 150), b"AAAAT", b"AAAAT"), "ATTTT_rc": (tract("ATTTT", 30, 150), b"ATTTT", b"AAAAT"),
    "AACCGT_own": (tract("AACCGT", 25, 150), b"CCGTAA", b"CCGTAA"), "ACGGTT_rc": (tract("ACGGTT", 25, 150), b"CGGTTA", b"CCGTAA"),
    "AACGTT_self": (tract("AACGTT", 25, 150), b"CGTTAA", b"CGTTAA"),
}


def _score(seqs, cigars, p, q):
    n = len(seqs)
    rec = RecordBatch.from_fields([0] * n, list(range(n)), [0] * n, [0] * n, [99] * n, [60] * n, cigars, seqs, ["r%d" % i for i in range(n)])
    return O.score_records_packed(rec, None, O.make_opts(pc.MEDIAN, p, q))


@functools.lru_cache(maxsize=None)
def read_conditions():
    """the oracle's scorer gives every read of READS and UNITS what its entry says, under both option sets; the three 'hi' reads
    straddle 0.8 and the three 'lo' reads 0.2 in p_repeat's own arithmetic -> {name: p_repeat}"""
    names = list(READS)
    out = {}
    for p, q in pc.PQ:
        sk, wu, wc, su, sc = _score([READS[n][0] for n in names], ["%dM" % len(READS[n][0]) for n in names], p, q)
        for i, n in enumerate(names):
            seq, unit, count, prod, al = READS[n]
            assert (wu[i], int(wc[i])) == (unit, count) and count < 256, (n, wu[i], wc[i])
            assert (count * len(unit)) % 256 == prod and len(seq) % 256 == al
            t = np.zeros(1, api.TREAD_DTYPE)
            t["repeat"], t["repeat_count"], t["align_length"] = unit, count, al
            out[n] = float(pc.oracle_p_repeat(t)[0])
    assert out["hi_under"] < out["hi_on"] == 0.8 < out["hi_over"] and out["lo_under"] < out["lo_on"] == 0.2 < out["lo_over"]
    assert out["wrap"] < 0.2 and 264 > 0.8 * 300 and out["al0"] == 255.0 and out["cold"] == 0.0 and out["hot"] == 1.0
    names = list(UNITS)
    sk, wu, wc, su, sc = _score([UNITS[n][0] for n in names], ["150M"] * len(names), 0.8, 40)
    for i, n in enumerate(names):
        seq, unit, canon = UNITS[n]
        assert wu[i] == unit and int(wc[i]) * len(unit) > 120, (n, wu[i], wc[i])
        assert O.canonical_repeat(unit.decode()).encode() == canon
        mrc = O.min_rev_complement(unit.decode()).encode()
        kind = n.split("_")[1]
        assert {"self": mrc == unit == canon, "rc": canon == mrc != unit, "own": canon == unit != mrc}[kind], n
    assert sorted({len(u[1]) for u in UNITS.values()}) == [1, 2, 3, 4, 5, 6]
    for k in (2, 4, 6):
        assert any(len(u[1]) == k and n.endswith("self") for n, u in UNITS.items())
    for k in range(1, 7):
        assert {n.split("_")[1] for n, u in UNITS.items() if len(u[1]) == k} >= {"own", "rc"}
    return out


# ---- rows and batches ------------------------------------------------------------------------------------------------------
F_PAIRED, F_PROPER, F_REVERSE, F_MREVERSE, F_READ1, F_READ2, F_SECONDARY = pc.F_PAIRED, pc.F_PROPER, pc.F_REVERSE, pc.F_MREVERSE, pc.F_READ1, pc.F_READ2, pc.F_SECONDARY


def before(seq, mapq=60, flag=99, cigar=None):
    """a record that lies before its mate: Cache.add stores it (or takes what is stored)"""
    return ("lo", "hi", flag, mapq, cigar or "%dM" % len(seq), seq)


def after(seq, mapq=60, flag=147, cigar=None):
    """a record that lies after its mate: Cache.add pairs it with what is stored, or returns"""
    return ("hi", "lo", flag, mapq, cigar or "%dM" % len(seq), seq)


def tail(seq, mapq=0, flag=77, mate="tail"):
    """an unmapped record of the tail (visited twice); mate: 'tail' or the position word of a mapped mate"""
    return ("tail", mate, flag, mapq, "*", seq)


def pair(a, b, mq=(60, 60), flags=(99, 147)):
    return [before(a, mq[0], flags[0]), after(b, mq[1], flags[1])]


def build(groups, prefix):
    """groups in join order -> (RecordBatch, n_tail, record indices of every group's rows).  Records are written group by group
    in NAME order, the unmapped tail last; group g's records lie at 1000 + 2 g ('lo') and 900 000 + 2 g ('hi')"""
    names = dc._name_pool(prefix, len(groups))
    rows, tl = [], []
    for q, g in sorted(zip(names, range(len(groups)))):
        where = {"lo": (0, 1000 + 2 * g), "hi": (0, 900_000 + 2 * g), "tail": (-1, -1)}
        for j, (at, mate, flag, mapq, cigar, seq) in enumerate(groups[g]):
            (tid, pos), (mtid, mpos) = where[at], where[mate]
            (tl if at == "tail" else rows).append((tid, pos, mtid, mpos, flag, mapq, cigar, seq, q, g, j))
    rows += tl
    index = [[None] * len(g) for g in groups]
    for i, r in enumerate(rows):
        index[r[9]][r[10]] = i
    return RecordBatch.from_fields(*[[r[c] for r in rows] for c in range(9)]), len(tl), index


def item_model(rec, p, q):
    """the join items of a batch, from the oracle's scorer words and the batch's own qname hashes: every record of a group
    with a hot member, and one item per soft-clip record with a result -> (start of every run of the sorted item array, lengths)"""
    qh = api.Soa(rec).pair_rows()[1]
    whole, softd = oracle_words(O, rec, None, O.make_opts(pc.MEDIAN, p, q))
    lo = (pc.fmix64(qh) & np.uint64(0xFFFFFFFF)).astype(np.uint64)
    soft_reads = [i for i, s in soft_items_expected(rec, whole, 0) if (softd[(i, s)][0] >> 16) or (softd[(i, s)][1] >> 16)]
    hot = set(lo[[i for i in range(rec.n) if whole[i] >> 16]].tolist()) | set(lo[soft_reads].tolist())
    keys = np.sort(np.concatenate([lo[[i for i in range(rec.n) if int(lo[i]) in hot]], lo[soft_reads]]))
    starts = np.flatnonzero(np.r_[True, keys[1:] != keys[:-1]])
    return starts, np.diff(np.r_[starts, len(keys)])


def by_record(exp):
    """{record index: [its treads in .bin order as (tid, position, repeat, split, mapq, count, align_length)]}"""
    out = {}
    for t in exp:
        out.setdefault(int(t["qname_id"]), []).append((int(t["tid"]), int(t["position"]), bytes(t["repeat"]), int(t["split"]), int(t["mapping_quality"]),
                                                       int(t["repeat_count"]), int(t["align_length"])))
    return out


def group_out(exp_by, index, g):
    return [exp_by.get(i, []) for i in index[g]]


# ---- 1. the classes through the whole replay ----------------------------------------------------------------------------------
KINDS = list(READS)
MAPQ_PAIRS = [(60, 60), (39, 60), (60, 39), (40, 60), (60, 40), (40, 40), (41, 40), (40, 41), (0, 1), (1, 0)]      # ties at min_mapq 40 and 0
FLAG_PAIRS = [(99, 147), (97, 145)]                                                             # proper, not proper


def classes_groups():
    return [pair(READS[a][0], READS[b][0], mq, fl) for a in KINDS for b in KINDS for mq in MAPQ_PAIRS for fl in FLAG_PAIRS]


def classes_at(a, b, mq=(60, 60), fl=(99, 147)):
    return ((KINDS.index(a) * len(KINDS) + KINDS.index(b)) * len(MAPQ_PAIRS) + MAPQ_PAIRS.index(mq)) * len(FLAG_PAIRS) + FLAG_PAIRS.index(fl)


def classes_conditions(p, q):
    spec, rec, n_tail, index, exp = case("classes", p, q)
    by = by_record(exp)
    out = lambda a, b, **kw: group_out(by, index, classes_at(a, b, **kw))
    unplaced = lambda o: [[t[0] for t in r] for r in o] == [[-1], [-1]]
    n = dict(treads=len(exp), unplaced=int((exp["tid"] == -1).sum()))
    if (p, q) == (0.8, 40):
        # unplaced_pair: only the read above 0.8 is unplaced with a hot mate; on and under the threshold the pair is adjusted
        assert unplaced(out("hot", "hi_over")) and unplaced(out("hi_over", "hot"))
        for k in ("hi_on", "hi_under", "wrap", "lo_over"):
            assert not unplaced(out("hot", k)) and not unplaced(out(k, "hot")), k
        assert unplaced(out("hot", "al0")) and unplaced(out("al0", "al0"))
        # ... and at mapq 39 / 40 of the other read
        assert unplaced(out("hot", "hi_on", mq=(60, 39))) and not unplaced(out("hot", "hi_on", mq=(60, 40)))
        assert unplaced(out("hi_on", "hot", mq=(39, 60))) and not unplaced(out("hi_on", "hot", mq=(40, 60)))
        # adjust_by, first branch: a read above 0.8 is placed by a mate below 0.2 of mapq above 40 -- not by one at 0.2, not by
        # mapq 40, and the read at 0.8 is not placed at all
        placed = lambda o, r: o[r][0][3] == NONE and o[r][0][1] not in (1000, 900_000)
        own = lambda a, b, r, **kw: out(a, b, **kw)[r][0][1] - (1000 + 2 * classes_at(a, b, **kw) if r == 0 else 900_000 + 2 * classes_at(a, b, **kw))
        for lo_kind, is_lo in (("lo_under", True), ("lo_on", False), ("lo_over", False), ("wrap", True), ("cold", True)):
            o = out("hi_over", lo_kind)
            moved = abs(own("hi_over", lo_kind, 0)) > 300               # to the mate's side: ~ 900 000 - 350
            assert moved == is_lo, (lo_kind, o)
            o = out(lo_kind, "hi_over")
            assert (abs(own(lo_kind, "hi_over", 1)) > 300) == is_lo, (lo_kind, o)
        assert abs(own("hi_over", "cold", 0, mq=(40, 41))) > 300 and abs(own("hi_over", "cold", 0, mq=(60, 40))) < 300
        for k in ("hi_on", "hi_under"):
            assert own(k, "cold", 0) == (len(READS[k][0]) % 256 + 1) // 2           # second branch: its own middle
        assert own("al0", "hot", 0, mq=(60, 39)) == -(1000 + 2 * classes_at("al0", "hot", mq=(60, 39)))      # unplaced: position 0
        # second branch at mapq 39 / 40 of the read itself, not proper: moved only from 40 on; a proper read always
        assert own("hi_on", "cold", 0, mq=(39, 60), fl=(97, 145)) > 300 and own("hi_on", "cold", 0, mq=(40, 40), fl=(97, 145)) == 75
        assert own("hi_on", "cold", 0, mq=(39, 60)) == 75
    else:
        assert unplaced(out("hot", "hi_on")) and unplaced(out("wrap", "wrap")) is False
    return n


# ---- 1b. soft clips around 0.9 and around 16 bases ---------------------------------------------------------------------------------
def clip_read(unit, copies, clen, body, side="L"):
    c = tract(unit, copies, clen)
    b = body[:150 - clen]
    return (c + b, "%dS%dM" % (clen, len(b))) if side == "L" else (b + c, "%dM%dS" % (len(b), clen))


# (name, unit, copies, clip length, body): the clip's count x 2 / length against 0.9, and 16 against 17 bases under a read
# with and without a unit of its own
CLIPS = [("on_0.9", "AG", 9, 20, "cold"), ("under_0.9", "AG", 8, 20, "cold"), ("over_0.9", "AG", 10, 20, "cold"), ("under_by_length", "AG", 9, 21, "cold"),
         ("over_by_length", "AG", 9, 19, "cold"), ("16_cold", "AG", 8, 16, "cold"), ("17_cold", "AG", 8, 17, "cold"), ("16_hot", "AG", 8, 16, "hot"),
         ("17_hot", "AG", 8, 17, "hot")]
CLIP_MAPQ = [60, 40, 39]


def clips_groups():
    out = []
    for name, unit, copies, clen, body in CLIPS:
        for side in "LR":
            seq, cig = clip_read(unit, copies, clen, FILL[20:] if body == "cold" else pc.HOT, side)
            for mq in CLIP_MAPQ:
                out.append([before(seq, mq, 99, cig), after(pc.HOT)])          # the clipped read is seen first (p - 0.07) ...
                out.append([before(pc.HOT), after(seq, mq, 147, cig)])         # ... or after its mate (min(p, 0.6))
    return out


def clips_at(name, side="L", mq=60, first=True):
    return (([c[0] for c in CLIPS].index(name) * 2 + "LR".index(side)) * len(CLIP_MAPQ) + CLIP_MAPQ.index(mq)) * 2 + (0 if first else 1)


def clips_conditions(p, q):
    spec, rec, n_tail, index, exp = case("clips", p, q)
    by = by_record(exp)
    n_clip = lambda name, **kw: sum(t[3] in (pc.LEFT, pc.RIGHT) for r in group_out(by, index, clips_at(name, **kw)) for t in r)
    for side in "LR":
        for first in (True, False):
            kw = dict(side=side, first=first)
            assert [n_clip(c, **kw) for c in ("on_0.9", "under_0.9", "over_0.9", "under_by_length", "over_by_length")] == [1, 0, 1, 0, 1], kw
            assert [n_clip(c, **kw) for c in ("16_cold", "17_cold", "16_hot", "17_hot")] == [0, 1, 1, 1], kw
            assert n_clip("on_0.9", mq=40, **kw) == 1 and n_clip("on_0.9", mq=39, **kw) == (0 if q == 40 else 1)
    return dict(treads=len(exp), clips=int(np.isin(exp["split"], (pc.LEFT, pc.RIGHT)).sum()))


# ---- 2. the second visit of the unmapped tail ---------------------------------------------------------------------------------------
def tail_groups():
    hot, cold, aaag = pc.HOT, FILL[:150], UNITS["CTTT_rc"][0]
    g = []
    for rep in range(40):
        g.append([tail(hot), tail(aaag, flag=141)])                              # 0: both hot: unplaced on either visit
        g.append([tail(aaag, 60), tail(cold, 60, 141)])                          # 1: mapq 60: the hot read is placed by its mate (adjust_by)
        g.append([tail(cold, 60), tail(hot, 60, 141)])                           # 2: ... the hot read second
        g.append([tail(hot, 0), tail(cold, 0, 141)])                             # 3: mapq 0
        g.append([("lo", "lo", 73, 60, "150M", hot), tail(aaag, 0, 133, "lo")])  # 4: the mate is mapped
        g.append([("lo", "lo", 73, 60, "150M", cold), tail(hot, 60, 133, "lo")])  # 5
        g.append(pair(hot, hot))                                                 # 6: no tail record
        g.append([tail(hot), tail(aaag, flag=141), tail(UNITS["AT_self"][0])])   # 7: the third stays stored: the second visit pairs it with the first
    return g


def tail_conditions(p, q):
    spec, rec, n_tail, index, exp = case("tail", p, q)
    assert n_tail == 40 * 13 and (rec.tid[rec.n - n_tail:] == -1).all() and (rec.tid[:rec.n - n_tail] >= 0).all()
    by = by_record(exp)
    once = by_record(dc.expect(rec, 0, p, q))                 # the same batch without the second visit
    kinds = {}
    for g in range(len(spec)):
        o, o1 = group_out(by, index, g), group_out(once, index, g)
        kinds.setdefault(g % 8, set()).add(str([[t[1:] for t in r] for r in o]))
        assert len(kinds[g % 8]) == 1                          # the 40 repetitions come out alike
        n2, n1 = sum(map(len, o)), sum(map(len, o1))
        if g % 8 in (0, 1, 2, 3):
            # both mates in the tail: the second visit emits exactly what the first did -- the rules saw unchanged treads
            assert n2 == 2 * n1 and all(r[:len(r) // 2] == r[len(r) // 2:] for r in o), (g % 8, o)
        if g % 8 == 6:
            assert o == o1 and n1 == 2
    first = lambda k: group_out(by, index, k)
    assert sum(map(len, first(0))) == 4 and all(t[0] == -1 for r in first(0) for t in r)          # unplaced twice
    if q == 40:
        assert sum(map(len, first(1))) == 2 and first(1)[0][0][3] == NONE and first(1)[0][0][2] != b"CTTT"      # placed, twice
        assert sum(map(len, first(2))) == 2 and first(2)[1][0][3] == NONE
        assert sum(map(len, first(3))) == 0                     # unplaced_pair holds, one read has no unit: nothing
    else:
        assert sum(map(len, first(3))) == 2
    # a tail record with a mapped mate: the mate comes first and finds nothing, the tail record is stored, then taken by its own
    # second visit -- the reference emits nothing for them
    assert sum(map(len, first(4))) + sum(map(len, first(5))) == 0
    # three tail records: a + b on the first visit; c stays stored, so the second visit pairs a with c, stores b, and c takes b
    o7, o7_once = first(7), group_out(once, index, 7)
    assert [len(r) for r in o7_once] == [1, 1, 0] and [len(r) for r in o7] == [2, 2, 2] and o7[2][0][2] == b"AT"
    return dict(treads=len(exp), without_second_visit=sum(map(len, once.values())))


# ---- 3. three and four primary records under one qname ------------------------------------------------------------------------------
def stored_groups():
    a, b, c, d = pc.HOT, UNITS["AAAG_own"][0], UNITS["AT_self"][0], FILL[:150]
    g = []
    for rep in range(30):
        g.append([before(a), before(b), after(c)])                 # 0: the second take empties the table: the third finds nothing
        g.append([before(a), after(c), after(b)])                  # 1: one pair, the third finds nothing
        g.append([before(a), before(b), before(c), after(d)])      # 2: c is stored: d places it
        g.append([before(a), before(b), before(d), after(c)])      # 3: d is stored: c is placed by it
        g.append([before(a), after(d), before(b), after(c)])       # 4: two pairs
        g.append([before(b), before(a), before(a), after(c)])      # 5: a (the third record) is stored
        g.append([before(d), before(a), after(c)])                 # 6: nothing stored when c comes
    return g


def stored_conditions(p, q):
    spec, rec, n_tail, index, exp = case("stored", p, q)
    by = by_record(exp)
    o = [group_out(by, index, k) for k in range(7)]
    n = [[len(r) for r in x] for x in o]
    assert n[0] == [0, 0, 0] and n[1] == [1, 1, 0] and n[6] == [0, 0, 0]
    assert n[2] == [0, 0, 1, 0] and o[2][2][0][2] == b"AT" and o[2][2][0][3] == NONE and o[2][2][0][0] == 0       # c, placed by d
    assert n[3] == [0, 0, 0, 1] and o[3][3][0][2] == b"AT"
    assert n[4] == [1, 0, 1, 1] and n[5] == [0, 0, 1, 1] and {o[5][2][0][2], o[5][3][0][2]} == {b"CAG", b"AT"} and o[5][2][0][0] == -1
    assert o[2] != o[3] and o[0] != o[1]
    return dict(treads=len(exp))


# ---- 4. the halo ------------------------------------------------------------------------------------------------------------------
def _clipped(body, mapq=60):
    """a read with a hot clip on either side: three join items (the read and its two soft-clip records)"""
    seq = tract("AG", 10, 20) + body[:110] + tract("AG", 10, 20)
    return seq, "20S110M20S"


def halo_groups():
    hot = pc.HOT
    s, cig = _clipped(hot)
    six = [before(s, 60, 99, cig), after(s, 60, 147, cig)]                                   # 2 reads + 4 soft-clip records
    fourteen = [before(s, 60, 99, cig), before(UNITS["AT_self"][0]), before(s, 60, 99, cig), after(s, 60, 147, cig), after(hot), after(s, 60, 147, cig)]
    three = [before(hot), before(UNITS["AAAG_own"][0]), before(UNITS["AT_self"][0])]
    pairs = lambda n: [pair(hot, UNITS["CTG_rc"][0]) for _ in range(n)]
    # items: 502 | 3 -> 505: fourteen items 505 .. 518 | 502 -> 1021: six items 1021 .. 1026 | 508 -> 1535: six items 1535 .. 1540 |
    # 500 -> 2041: six items 2041 .. 2046 = the array's last
    return pairs(251) + [three, fourteen] + pairs(251) + [six] + pairs(254) + [six] + pairs(250) + [six]


HALO_RUNS = [(505, 14), (1021, 6), (1535, 6), (2041, 6)]


def halo_conditions(p, q):
    spec, rec, n_tail, index, exp = case("halo", p, q)
    starts, lens = item_model(rec, p, q)
    runs = dict(zip(starts.tolist(), lens.tolist()))
    n_items = int(lens.sum())
    assert lens.max() <= PAIR_MAXM
    for s, m in HALO_RUNS[:3]:
        assert runs.get(s) == m and 505 <= s % PG_BLOCK <= 511 and s % PG_BLOCK + m > PG_BLOCK and s % PG_BLOCK + m <= PG_BLOCK + PG_HALO, (s, m)
    s, m = HALO_RUNS[3]
    assert runs.get(s) == m and s + m == n_items and s % PG_BLOCK == 505 and n_items % PG_BLOCK == 511          # the last tile's halo lies beyond the array
    assert n_items > 3 * PG_BLOCK                       # a grid of one or two blocks takes tiles one after the other
    by = by_record(exp)
    at = [len(spec) - 1, len(spec) - 252, len(spec) - 507, 252]
    for g in at:                                         # every such group emits its clips, from records on either side of the seam
        o = group_out(by, index, g)
        assert sum(t[3] in (pc.LEFT, pc.RIGHT) for r in o for t in r) >= 4 and sum(len(r) > 0 for r in o) >= 2, o
    return dict(items=n_items, treads=len(exp))


# ---- 5. where the doAssert is raised ----------------------------------------------------------------------------------------------
def assert_groups(kind):
    hot = pc.HOT
    base = [pair(hot, hot) for _ in range(50)]
    if kind == "after_nothing_stored":
        return base + [[after(dc.HOMO)]] + base
    if kind == "secondary":
        return base + [[before(hot), before(dc.HOMO, 60, 99 | F_SECONDARY), after(hot), after(dc.HOMO, 60, 147 | 0x800)]] + base
    if kind == "reached":
        return base + [[before(hot), after(dc.HOMO)]] + base
    raise AssertionError(kind)


def assert_conditions(kind):
    """the one 510-base homopolymer's word counts 510; where the reference never reaches it the oracle's result is that of the
    batch without it"""
    rec, n_tail, index = build(assert_groups(kind), "pa_" + kind[:3])
    wc = O.score_records_packed(rec, None, O.make_opts(pc.MEDIAN, 0.8, 40))[2]
    homo = np.flatnonzero(rec.l_seq == 510)
    assert len(homo) == (2 if kind == "secondary" else 1) and (wc[homo] == 510).all() and int(np.delete(wc, homo).max()) < 256
    if kind == "reached":
        i = int(homo[0])
        assert rec.pos[i] > rec.mpos[i] and not rec.flag[i] & 0x900           # after its mate, which is stored: to_tread
        return rec, n_tail, None
    exp = dc.expect(rec, n_tail)
    assert not np.isin(exp["qname_id"], homo).any() and len(exp) == (200 if kind == "after_nothing_stored" else 202)
    return rec, n_tail, exp


# ---- 6. + 8. units of every length, in blocks that emit more than their stage holds ----------------------------------------------------
REV_FALSE = (99, 147)      # should_reverse holds where F_REVERSE == F_MREVERSE


def units_groups():
    cold = FILL[:150]
    g = []
    for rep in range(8):
        for n, (seq, unit, canon) in UNITS.items():
            g.append(pair(seq, seq))                                    # unplaced: both canonical
            g.append(pair(seq, cold, flags=(113, 177)))             # placed by the mate, should_reverse true (both strands reverse)
            g.append(pair(cold, seq, flags=(65, 129)))                  # ... the hot read second, should_reverse true (neither)
            g.append(pair(seq, cold, flags=REV_FALSE))                  # should_reverse false
            g.append(pair(pc.HOT, seq))                                 # unplaced beside another unit
    return g


def units_conditions(p, q):
    spec, rec, n_tail, index, exp = case("units", p, q)
    by = by_record(exp)
    for j, (n, (seq, unit, canon)) in enumerate(UNITS.items()):
        mrc = O.min_rev_complement(unit.decode()).encode()
        o = [group_out(by, index, 5 * j + k) for k in range(5)]
        assert [t[2] for r in o[0] for t in r] == [canon, canon] and all(t[0] == -1 for r in o[0] for t in r), (n, o[0])
        assert [t[2] for t in o[1][0]] == [mrc] and o[1][0][0][3] == NONE and o[1][1] == [], (n, o[1])
        assert [t[2] for t in o[2][1]] == [mrc] and o[2][0] == [], (n, o[2])
        assert [t[2] for t in o[3][0]] == [unit] and o[3][0][0][3] == NONE, (n, o[3])
        assert [t[2] for r in o[4] for t in r] == [b"CAG", canon] and o[4][1][0][0] == -1, (n, o[4])
    starts, lens = item_model(rec, p, q)
    n_blocks = -(-int(lens.sum()) // PG_BLOCK)
    assert len(exp) > PG_EMIT * n_blocks                               # pigeonhole: a block emits more than its stage holds
    assert sorted(set(np.char.str_len(exp["repeat"]).tolist())) == [1, 2, 3, 4, 5, 6]
    return dict(treads=len(exp), blocks=n_blocks)


# ---- 7. the same inside runs of more than 15 items ------------------------------------------------------------------------------------
def long_groups():
    R = {k: v[0] for k, v in READS.items()}
    hot, cold, at = pc.HOT, FILL[:150], UNITS["AT_self"][0]
    s, cig = _clipped(cold)
    classes = []
    for a, b in (("hot", "hi_over"), ("hot", "hi_on"), ("hi_over", "lo_under"), ("hi_over", "lo_on"), ("hi_on", "cold"), ("wrap", "hot"), ("al0", "hot"), ("hot", "hi_under")):
        classes += pair(R[a], R[b])
    stored = [before(hot), before(at), after(cold), before(hot), before(at), before(cold), after(UNITS["CTG_rc"][0]), before(at), after(hot), after(hot),
              before(cold), before(hot), before(s, 60, 99, cig), after(s, 60, 147, cig), after(at), before(UNITS["G_rc"][0]), after(UNITS["CTTT_rc"][0])]
    tl = [before(hot), after(at)] * 6 + [before(cold), tail(hot, 60), tail(cold, 60, 141), tail(at, 0), tail(UNITS["CTTT_rc"][0], 0, 141)]
    return [pair(hot, hot) for _ in range(100)] + [classes + [before(hot)], stored, tl] + [pair(hot, at) for _ in range(100)]


def long_conditions(p, q):
    spec, rec, n_tail, index, exp = case("long", p, q)
    starts, lens = item_model(rec, p, q)
    assert sorted(lens.tolist())[-3:] == [17, 17 + 4, 17] or sorted(l for l in lens.tolist() if l > PAIR_MAXM) == [17, 17, 21]
    assert [len(g) for g in spec[100:103]] == [17, 17, 17] and n_tail == 4
    by = by_record(exp)
    o = [group_out(by, index, g) for g in (100, 101, 102)]
    tid = lambda r: [t[0] for t in r]
    if (p, q) == (0.8, 40):
        assert tid(o[0][0]) == [-1] and tid(o[0][2]) == [0] and tid(o[0][3]) == [0]         # hot + hi_over unplaced, hot + hi_on adjusted
        assert abs(o[0][4][0][1] - 1000) > 300 and abs(o[0][6][0][1] - 1000) < 300          # placed by lo_under, not by lo_on
    assert sum(map(len, o[1])) >= 8 and o[1][0] == [] and o[1][2] == []                    # a, b taken; c finds nothing
    assert any(t[3] in (pc.LEFT, pc.RIGHT) for r in o[1] for t in r)
    once = by_record(dc.expect(rec, 0, p, q))
    t4, t4_once = [by.get(i, []) for i in index[102][13:]], [once.get(i, []) for i in index[102][13:]]
    assert sum(map(len, t4)) > sum(map(len, t4_once)) > 0              # the tail records emit on either visit
    return dict(treads=len(exp), long_runs=int((lens > PAIR_MAXM).sum()))


# ---- the cases ---------------------------------------------------------------------------------------------------------------------
BUILDERS = {"classes": classes_groups, "clips": clips_groups, "tail": tail_groups, "stored": stored_groups, "halo": halo_groups, "units": units_groups,
            "long": long_groups}
CONDITIONS = {"classes": classes_conditions, "clips": clips_conditions, "tail": tail_conditions, "stored": stored_conditions, "halo": halo_conditions,
              "units": units_conditions, "long": long_conditions}
# (case, proportion_repeat, min_mapq): the classes, the clips and the tail under both option sets
CASES = [(n, p, q) for n in BUILDERS for p, q in (pc.PQ if n in ("classes", "clips", "tail") else pc.PQ[:1])]
ASSERT_KINDS = ("after_nothing_stored", "secondary", "reached")


@functools.lru_cache(maxsize=None)
def batch(name):
    groups = BUILDERS[name]()
    return (groups,) + build(groups, "pp_" + name[:3])


@functools.lru_cache(maxsize=None)
def case(name, p, q):
    """-> (groups, RecordBatch, n_tail, record indices per group, the oracle's treads); built once, shared, never modified"""
    groups, rec, n_tail, index = batch(name)
    return groups, rec, n_tail, index, dc.expect(rec, n_tail, p, q)


def conditions(name, p, q):
    read_conditions()
    return CONDITIONS[name](p, q)
