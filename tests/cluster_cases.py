"""Inputs that put the clustering kernels (strling_amd/csrc/cluster.hip) on their edges.

Plain builders, no GPU code: every builder returns a `Case` -- treads in the oracle's TREAD_DTYPE plus the clustering
arguments -- fully determined by its arguments.  tests/test_cluster_cases.py proves with the oracle alone that each case
reaches the edge it is named for; tests/test_cluster_device.py runs the same cases through the kernels.
"""
import numpy as np

from oracle.oracle import TREAD_DTYPE

MODE_MERGE, MODE_CALL = 0, 1
LEFT, RIGHT, NONE = 0, 1, 3          # tread.split: soft-clipped on the left / right, not clipped (an anchor)
WINDOW = 560

# CountTable[uint32] starts at 16 slots and doubles when a new key arrives with 2 * len < 3 * counter: the 12th, 23rd, 44th,
# 87th, 172nd and 343rd distinct key.  Each triple is (two sizes before the step, the first size after it).
TIE_STEPS = [(10, 11, 12), (21, 22, 23), (42, 43, 44), (85, 86, 87), (170, 171, 172), (341, 342, 343)]
TIE_D = [2, 4] + [d for s in TIE_STEPS for d in s]
SIZES = [(255, 0), (256, 0), (257, 0), (300, 0), (1000, 0), (5000, 0), (255, 1), (256, 1), (257, 1)]   # (after trim, trimmed)
GATE_N = [65534, 65535, 65536, 70000]
SAMPLE_N = [8, 9, 16, 17, 128, 129, 256, 257]
SAMPLE_STRIDE = [1, 4096]
SEAM_HEADS = [63, 64, 65, 511, 512, 513, 2047, 2048, 2049]
SEAM_LAYOUTS = [("heads", 2100), ("own", 1), ("own", 64), ("own", 2048), ("own", 2049), ("own", 5000), ("big", 5000)]
MANY_TILES_N = 4096 * 2048 + 1
UNITS = [b"A", b"AC", b"AGC", b"AATG", b"CCG", b"AAAT", b"ACGTC", b"AACCGT"]


class Case:
    def __init__(self, name, treads, window=WINDOW, min_support=5, max_clip_dist=200, modes=(MODE_CALL,), **meta):
        self.name, self.treads, self.window, self.min_support, self.max_clip_dist, self.modes = name, treads, window, min_support, max_clip_dist, modes
        self.meta = meta

    def kw(self):
        return dict(min_support=self.min_support, max_clip_dist=self.max_clip_dist)

    def expect(self, oracle, mode):
        """-> (rows, unplaced) of the oracle"""
        return oracle.call_bounds(self.treads, mode, self.window, **self.kw())

    def __repr__(self):
        return self.name


def _rng(*seed):
    return np.random.Generator(np.random.Philox(key=[int(sum((s + 1) * 1000003 ** i for i, s in enumerate(seed))) % (1 << 63), 0]))


def _treads(pos, split, tid=0, repeat=b"AC", qname_id=0):
    pos = np.asarray(pos, np.int64)
    assert pos.size == 0 or (pos.min() >= 0 and pos.max() < 1 << 32)
    t = np.zeros(pos.size, TREAD_DTYPE)
    t["position"] = pos.astype(np.uint32)
    t["split"], t["tid"], t["repeat"], t["qname_id"] = split, tid, repeat, qname_id
    t["mapping_quality"], t["repeat_count"], t["align_length"] = 60, 40, 150
    return t


def group_keys(t):
    """the device's group key of every tread: (tid + 1, unit length, unit in C<A<T<G code)"""
    code = np.zeros(t.size, np.int64)
    ln = np.zeros(t.size, np.int64)
    rep = np.frombuffer(np.ascontiguousarray(t["repeat"]).tobytes(), np.uint8).reshape(t.size, 6)
    lut = np.zeros(256, np.int64)
    lut[ord("C")], lut[ord("A")], lut[ord("T")], lut[ord("G")] = 0, 1, 2, 3
    for j in range(6):
        on = rep[:, j] != 0
        code = np.where(on, code * 4 + lut[rep[:, j]], code)
        ln += on
    return ((t["tid"].astype(np.int64) + 1) << 15) | (ln << 12) | code


def sort_key_order(t):
    """-> (the order the device sorts into: group key, then position, stable; the group keys)"""
    gkey = group_keys(t)
    return np.lexsort((t["position"], gkey)), gkey


def count_groups_clusters(t, window):
    """(n_groups, n_clusters) of a tread set, from the sorted input and the growth rule alone (cluster.nim:330-340): a read joins
    while its position <= median of the cluster's first min(9, n) reads + window + 100 (uint32 arithmetic); unplaced
    groups are not swept."""
    order, gkey = sort_key_order(t)
    pos, gk = t["position"][order].astype(np.int64), gkey[order]
    starts = np.concatenate([[0], np.nonzero(np.diff(gk))[0] + 1, [t.size]]) if t.size else np.array([0])
    nc = 0
    for a, e in zip(starts[:-1], starts[1:]):
        if (gk[a] >> 15) == 0:
            continue
        s = a
        while s < e:
            nc += 1
            j, n = s + 1, 1
            while j < e and pos[j] <= ((pos[s + (min(n, 9) - 1) // 2] + window + 100) & 0xffffffff):
                j, n = j + 1, n + 1
            s = j
    return len(starts) - 1, nc


# ---- a. ties between modal clip positions, across every CountTable growth step ---------------------------------------
TIE_BASE = 1_002_164     # at this base the oracle's modal choice is the same either side of each pair below a growth step and
                         # changes on both clip sides at every step (found by trying bases upwards from 1_000_000)


def clip_ties(d, variant="tied", base=TIE_BASE):
    """One group, one cluster: d distinct right-clip positions base + j and d distinct left-clip positions base + 400 + j,
    ten anchors between them.  variant "tied": every position twice (d keys tied at the maximum, the table's slot order
    decides); "single": every position once (`val > 1` fails); "split": one position per side d + 1 times (more than half
    the distinct count, split_cluster fires).  The window is 560 wherever the cluster fits under it: the growth limit is
    base + 2 + window + 100, the last left clip sits at base + 400 + d - 1, so d > 263 takes window 760."""
    j = np.arange(d)
    cnt = np.full(d, 1 if variant == "single" else 2)
    if variant == "split":
        assert d >= 12
        cnt[d // 3] = d + 1
    rights, lefts = np.repeat(base + j, cnt), np.repeat(base + 400 + j, cnt)
    anchors = base + 350 + 5 * np.arange(10)
    pos = np.concatenate([rights, anchors, lefts])
    split = np.concatenate([np.full(rights.size, RIGHT), np.full(10, NONE), np.full(lefts.size, LEFT)])
    t = _treads(pos, split, tid=3, repeat=b"AC", qname_id=np.arange(pos.size) % 3)
    t = t[_rng(1, d, base % 977).permutation(t.size)]
    window = WINDOW if 400 + d - 1 <= 2 + WINDOW + 100 else 760
    return Case(f"clip_ties-{variant}-d{d}-base{base}", t, window=window, min_support=2, max_clip_dist=1000, modes=(MODE_MERGE, MODE_CALL),
                d=d, base=base, variant=variant, n_groups=1, n_clusters=1)


# ---- b. clusters around the LDS / global switch ---------------------------------------------------------------------
def _size_cluster(rng, S, n, trimmed):
    """n reads in [S, S + 600) -- two anchors at S, the rest at S + 100 and above -- and, when `trimmed`, one anchor at
    S - 600 in front: it joins (S <= S - 600 + 660) and, once the median of the first nine is at S + 100 or above, lies
    more than max_dist + 100 below it.  (The 5th read joined against the 2nd, so no more than the 1st can ever be trimmed.)"""
    n_clip = min(n // 4, 400)
    k = max(40, n_clip // 2)                       # distinct clip positions per side: the table grows at least twice
    rc = 1 + rng.multinomial(n_clip - k, np.full(k, 1.0 / k))
    lc = 1 + rng.multinomial(n_clip - k, np.full(k, 1.0 / k))
    rights, lefts = np.repeat(S + 100 + np.arange(k), rc), np.repeat(S + 400 + np.arange(k), lc)
    anchors = np.concatenate([[S, S], S + 100 + rng.integers(0, 500, n - 2 - 2 * n_clip)])
    pos = np.concatenate([rights, lefts, anchors] + ([[S - 600]] if trimmed else []))
    split = np.concatenate([np.full(rights.size, RIGHT), np.full(lefts.size, LEFT), np.full(anchors.size + (1 if trimmed else 0), NONE)])
    return pos, split


def sizes(n_after_trim, n_trimmed):
    """Three clusters of n_after_trim reads after the trim (two in one group, one in another), each with n_trimmed (0 or 1)
    reads in front that the trim removes."""
    assert n_trimmed in (0, 1)
    rng = _rng(2, n_after_trim, n_trimmed)
    parts = []
    for S, tid, unit in ((10_000, 1, b"AC"), (20_000, 1, b"AC"), (5_000, 2, b"AGC")):
        pos, split = _size_cluster(rng, S, n_after_trim, n_trimmed)
        parts.append(_treads(pos, split, tid=tid, repeat=unit, qname_id=rng.integers(0, 7, pos.size)))
    t = np.concatenate(parts)
    t = t[rng.permutation(t.size)]
    return Case(f"sizes-{n_after_trim}+{n_trimmed}", t, min_support=5, max_clip_dist=300, modes=(MODE_MERGE, MODE_CALL),
                n=n_after_trim, n_trimmed=n_trimmed, n_groups=2, n_clusters=3)


# ---- c. the n >= 65535 gate and the 16-bit counts ----------------------------------------------------------------
def gate(n, mode=MODE_CALL):
    """One cluster of n reads from one sample: anchors cycling over 300 positions and three right clips at one position.
    n = 70000 also has three left clips at one position 100 further on, so split_cluster halves it below the gate."""
    base = 50_000
    split_it = n > 65536
    n_anchor = n - (6 if split_it else 3)
    pos = [base + np.arange(n_anchor) % 300, np.full(3, base + (100 if split_it else 150))]
    split = [np.full(n_anchor, NONE), np.full(3, RIGHT)]
    if split_it:
        pos.append(np.full(3, base + 200))
        split.append(np.full(3, LEFT))
    t = _treads(np.concatenate(pos), np.concatenate(split), tid=0, repeat=b"AGC", qname_id=0)
    t = t[_rng(3, n).permutation(t.size)]
    return Case(f"gate-{n}-mode{mode}", t, min_support=3, modes=(mode,), n=n, n_groups=1, n_clusters=1)


# ---- d. the per-sample count table of merge mode -----------------------------------------------------------------
def sample_table(n, stride, doubled=False):
    """One cluster of n reads with qname_id = i * stride (stride 4096: every id hashes to slot 0 of a table of up to 4096
    slots).  doubled: the last read carries the id of read n // 2, and min_support is 2 -- that pair is the only support."""
    rng = _rng(4, n, stride)
    pos = np.concatenate([np.full(3, 7_000 + 40), 7_000 + rng.integers(0, 200, n - 3)])
    split = np.concatenate([np.full(3, RIGHT), np.full(n - 3, NONE)])
    order = rng.permutation(n)
    q = np.arange(n, dtype=np.int64) * stride
    if doubled:
        q[n - 1] = q[n // 2]
    t = _treads(pos[order], split[order], tid=4, repeat=b"AAAT", qname_id=q)
    return Case(f"sample_table-{n}-stride{stride}" + ("-doubled" if doubled else ""), t, min_support=2 if doubled else 1, modes=(MODE_MERGE,),
                n=n, n_groups=1, n_clusters=1)


# ---- e. group heads on the seams of heads_kernel / gather_kernel ---------------------------------------------------
def _seam_group(rng, size, tid, unit):
    base = 1_000 + int(rng.integers(0, 3_000_000))
    pos = base + rng.integers(0, 300, size)
    split = np.full(size, NONE)
    if size >= 6:     # a clip pair; every clip position once, so split_cluster (modal count / distinct > 0.5) stays quiet
        pos[:4] = base + np.array([10, 20, 110, 120])
        split[:4] = [RIGHT, RIGHT, LEFT, LEFT]
    return _treads(pos, split, tid=tid, repeat=unit, qname_id=rng.integers(0, 3, size))


def seams(layout, n):
    """Every group is one cluster and yields one row at min_support 1; the input is shuffled, so the groups' first
    appearances -- which fix the row order -- are not in key order.
    "heads": group heads at sorted indices 0, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049 and n - 1;
    "own": every tread its own group (tid i // 2, two units); "big": one group of n treads between 2 x 20 small groups."""
    rng = _rng(5, n, len(layout))
    if layout == "heads":
        heads = [0] + SEAM_HEADS + [n - 1, n]
        sizes_ = list(np.diff(heads))
    elif layout == "own":
        sizes_ = [1] * n
    else:
        sizes_ = [int(x) for x in rng.integers(1, 4, 20)] + [n] + [int(x) for x in rng.integers(1, 4, 20)]
    parts = []
    for g, size in enumerate(sizes_):
        tid, unit = (g // 2, (b"A", b"CT")[g % 2]) if layout == "own" else (g, b"ACG")
        parts.append(_seam_group(rng, int(size), tid, unit))
    t = np.concatenate(parts)
    heads = np.concatenate([[0], np.cumsum(sizes_)[:-1]])
    t = t[rng.permutation(t.size)]
    return Case(f"seams-{layout}-{n}", t, min_support=1, modes=(MODE_MERGE, MODE_CALL), heads=heads, n_groups=len(sizes_), n_clusters=len(sizes_))


# ---- f. gaps at the growth rule's and the trim's threshold -------------------------------------------------------
def gaps(seed, min_support):
    """About 400 groups of 1 to 40 reads whose consecutive gaps sit on max_dist + 100 - 1 / + 0 / + 1; a quarter start below
    position 3000 (left_most = median - max_dist wraps), a few are unplaced."""
    rng = _rng(6, seed)
    md = WINDOW
    gap_set = np.array([0, 0, 1, 1, 2, 50, md + 99, md + 100, md + 101, 2 * md + 300])
    parts = []
    for g in range(400):
        size = int(rng.integers(1, 41))
        start = int(rng.integers(0, 3000)) if g % 4 == 0 else int(rng.integers(1_000_000, 3_000_000_000))
        pos = start + np.concatenate([[0], np.cumsum(rng.choice(gap_set, size - 1))])
        split = rng.choice([LEFT, RIGHT, NONE, NONE], size)
        unplaced = g % 37 == 5
        parts.append(_treads(np.zeros(size, np.int64) if unplaced else pos, split, tid=-1 if unplaced else g % 50, repeat=UNITS[g // 50],
                             qname_id=rng.integers(0, 3, size)))
    t = np.concatenate(parts)
    t = t[rng.permutation(t.size)]
    return Case(f"gaps-{seed}-s{min_support}", t, min_support=min_support, modes=(MODE_MERGE, MODE_CALL))


# ---- g. more than 4096 tiles: tile_scan_kernel and its carry -----------------------------------------------------
def many_tiles():
    """The smallest n that takes the scanned path: 4097 tiles, so the scan's carry crosses four blocks of 1024 tiles."""
    rng = _rng(7)
    n = MANY_TILES_N
    t = np.zeros(n, TREAD_DTYPE)
    t["position"] = rng.integers(0, 1 << 22, n, dtype=np.uint32)
    t["tid"] = rng.integers(0, 50, n, dtype=np.int32)
    t["repeat"] = np.array(UNITS[:4])[rng.integers(0, 4, n)]
    t["split"] = np.array([LEFT, RIGHT, NONE, NONE], np.uint8)[rng.integers(0, 4, n)]
    t["mapping_quality"], t["repeat_count"], t["align_length"] = 60, 40, 150
    return Case("many_tiles", t, min_support=5, n_groups=200)


# ---- h. the step between one composite sort and two sorts ----------------------------------------------------------
def key_width(max_tid):
    """max_tid 131070: tid + 1 needs 17 bits, 17 + 15 unit bits + 32 position bits = 64, one sort.  131071: 65 bits, two sorts."""
    from strling_amd import synth
    t = synth.synth_treads(n_samples=2, n_loci=200, seed=9, contig_len=1_000_000, dtype=TREAD_DTYPE)
    t["tid"] += max_tid - int(t["tid"].max())
    t["position"][0] = (1 << 31) + 5          # pos_bits = 32
    return Case(f"key_width-{max_tid}", t, min_support=3, max_clip_dist=175, modes=(MODE_MERGE, MODE_CALL), max_tid=max_tid)


# ---- i. the folded position field of the resident entry ------------------------------------------------------------
def folded(pos_bits, bad=False):
    """Positions in [0, 2^(pos_bits-1)) plus, in some groups, positions 2^32 - k: clips that adjust_by wrapped below zero.
    bad: one more tread in the uncovered middle of the range (at 2^pos_bits)."""
    rng = _rng(8, pos_bits)
    half = 1 << (pos_bits - 1)
    parts = []
    for g in range(60):
        tid, unit = g % 25, UNITS[g // 25]
        for kind in range(3):
            size = int(rng.integers(6, 20))
            base = (0, half - 700, int(rng.integers(1000, half - 2000)))[kind]
            pos = base + rng.integers(0, 500, size)
            split = rng.choice([LEFT, RIGHT, NONE, NONE], size)
            pos[:4], split[:4] = base + np.array([30, 30, 90, 90]), [RIGHT, RIGHT, LEFT, LEFT]
            if kind == 0 and g % 2 == 0:      # wrapped right clips and an anchor.  median + max_dist + 100 wraps too, so each is a
                k = int(rng.integers(2, 50))  # cluster of its own behind every other read of its group; at min_support 1 the anchor writes a row
                pos = np.concatenate([pos, [(1 << 32) - k, (1 << 32) - k, (1 << 32) - 1 - int(rng.integers(0, 60)), (1 << 32) - k - 1]])
                split = np.concatenate([split, [RIGHT, RIGHT, RIGHT, NONE]])
            parts.append(_treads(pos, split, tid=tid, repeat=unit, qname_id=0))
    # the four corners of the field
    parts.append(_treads([0, half - 1, (1 << 32) - half, (1 << 32) - 1], [NONE] * 4, tid=24, repeat=b"CCG"))
    if bad:
        parts.append(_treads([1 << pos_bits], [NONE], tid=3, repeat=b"CCG"))
    t = np.concatenate(parts)
    t = t[rng.permutation(t.size)]
    return Case(f"folded-{pos_bits}" + ("-bad" if bad else ""), t, min_support=1, pos_bits=pos_bits, n_tid=25)


def folded_bad(pos_bits):
    """folded(pos_bits) and one tread at 2^pos_bits: neither below 2^(pos_bits-1) nor within 2^(pos_bits-1) of 2^32"""
    return folded(pos_bits, bad=True)


def bad_unit(kind):
    """a valid array with one tread whose unit has a non-ACGT letter ("letter") or a letter after a NUL ("gap")"""
    c = sizes(255, 0)
    t = c.treads.copy()
    t["repeat"][17] = {"letter": b"ANT", "gap": b"A\0C"}[kind]
    return Case(f"bad_unit-{kind}", t, min_support=5, max_clip_dist=300, modes=(MODE_MERGE, MODE_CALL))
