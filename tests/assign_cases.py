"""Tables for the tests of strl_assign_reads_loci_device (test_assign_emu.py on the CPU, test_assign_device.py on the GPU): the
edge tables of the rule, tables of given group widths, drawn tables, and the comparison with the host function
(api.assign_reads_loci), which is the yardstick in every test.  A tread is (tid, position, split, unit), a locus
(tid, left_most, right_most, unit)."""
import numpy as np

from strling_amd import api

LEFT, RIGHT, BOTH, NONE, TAKEN = 0, 1, 2, 3, 255
M32 = 0xFFFFFFFF


def treads_of(rows):
    t = np.zeros(len(rows), api.TREAD_DTYPE)
    for i, (tid, pos, split, unit) in enumerate(rows):
        t[i] = (tid, pos, unit, 0, split, 60, 10, 100, i)
    return t


def loci_of(rows):
    lo = np.zeros(len(rows), api.LOCUS_DTYPE)
    for j, (tid, lm, rm, unit) in enumerate(rows):
        b = lo["b"][j]
        b["tid"], b["left_most"], b["right_most"], b["repeat"] = tid, lm, rm, unit
        b["left"], b["right"], b["center_mass"] = lm, rm, lm
        b["n_left"], b["n_right"], b["n_total"] = 7, 8, 9          # (recounted: what comes in is reset)
        lo["name"][j] = b"locus%d" % j
    return lo


def _line(tid, unit, positions, split=NONE):
    return [(tid, p, split, unit) for p in positions]


def edge_tables():
    """name -> (tread rows, locus rows); every one is run in both modes"""
    E = {}
    abc = _line(0, b"AC", (100, 200, 300))
    E["empty_range_loses_the_read_behind"] = (abc, [(0, 150, 160, b"AC")])
    E["range_at_the_end_of_its_group"] = (abc + _line(1, b"AC", (50,)) + _line(0, b"AG", (400,)), [(0, 250, 400, b"AC")])
    E["right_most_below_left_most"] = (abc, [(0, 300, 100, b"AC"), (0, 201, 5, b"AC")])
    E["left_most_0_and_1"] = (_line(0, b"AC", (0, 0, 1, 2)), [(0, 0, 0, b"AC"), (0, 1, 0, b"AC")])
    E["left_most_1_first"] = (_line(0, b"AC", (0, 0, 1, 2)), [(0, 1, 0, b"AC"), (0, 0, 0, b"AC")])
    E["right_most_all_ones"] = (_line(0, b"AC", (7, M32 - 1, M32, M32)), [(0, 9, M32, b"AC"), (0, 0, M32, b"AC")])
    high = _line(0, b"AGC", (2 ** 31 - 1, 2 ** 31, 2 ** 31 + 5, M32 - 1, M32, 3))
    E["positions_from_2_31_on"] = (high, [(0, 2 ** 31, 2 ** 31, b"AGC"), (0, M32, M32, b"AGC"), (0, 2 ** 31 + 6, M32 - 2, b"AGC")])
    ties = [(0, 500, s, b"AC") for s in (LEFT, RIGHT, NONE, BOTH, LEFT)]
    ties = ties[:2] + _line(0, b"AC", (400, 600, 500)) + ties[2:] + _line(0, b"AC", (500, 499))
    E["equal_positions_keep_input_order"] = (ties, [(0, 500, 500, b"AC")])
    many = [(0, p, (LEFT, RIGHT, NONE)[p % 3], b"AAG") for p in range(100, 130)]
    E["the_same_locus_twice"] = (many, [(0, 105, 110, b"AAG"), (0, 105, 110, b"AAG"), (0, 105, 110, b"AAG")])
    E["overlapping_loci_a_b"] = (many, [(0, 105, 115, b"AAG"), (0, 110, 120, b"AAG")])
    E["overlapping_loci_b_a"] = (many, [(0, 110, 120, b"AAG"), (0, 105, 115, b"AAG")])
    units = _line(0, b"A", (10, 20, 30)) + _line(0, b"AA", (10, 20, 30)) + _line(0, b"AAAAAA", (10, 20, 30))
    E["units_A_AA_AAAAAA_are_three_groups"] = (units[::2] + units[1::2], [(0, 15, 25, b"AAAAAA"), (0, 5, 12, b"A"), (0, 1, 100, b"AA"), (0, 1, 100, b"AAA")])
    E["a_group_without_treads"] = (abc, [(0, 1, 1000, b"ACG"), (3, 1, 1000, b"AC"), (-5, 1, 1000, b"AC"), (1, 1, 1000, b"AC"), (0, 1, 1000, b"AC")])
    E["a_locus_with_a_unit_that_is_not_ACGT"] = (abc, [(0, 1, 1000, b"AN"), (0, 1, 1000, b"ac"), (0, 1, 150, b"AC"), (0, 1, 1000, b"")])
    pre = [(0, 100, TAKEN, b"AC"), (0, 200, LEFT, b"AC"), (0, 250, TAKEN, b"AC"), (0, 300, RIGHT, b"AC"), (0, 400, TAKEN, b"AC"), (0, 500, NONE, b"AC")]
    E["treads_that_arrive_taken"] = (pre, [(0, 50, 260, b"AC"), (0, 1, 1000, b"AC")])
    unpl = _line(-1, b"AC", (0, 5, 5, 9), LEFT) + _line(0, b"AC", (5, 6)) + _line(-1, b"AT", (1,))
    E["unplaced_treads"] = (unpl, [(-1, 4, 6, b"AC"), (0, 1, 100, b"AC"), (-1, 0, M32, b"AT"), (-1, 0, 0, b"AC")])
    E["no_treads"] = ([], [(0, 1, 100, b"AC"), (-1, 1, 100, b"AC")])
    E["no_loci"] = (abc, [])
    return E


def widths_table(sizes, loci_per_group=3, seed=0):
    """one group per entry of `sizes` (contigs 0, 1, ...; unit AC), its reads shuffled over a small range of positions, and a few
    loci in each: one over everything, the others drawn"""
    rng = np.random.default_rng(seed)
    rows, loci = [], []
    for g, m in enumerate(sizes):
        span = max(4, m // 3)
        pos = rng.integers(0, span, m)
        sp = rng.choice([LEFT, RIGHT, NONE], m)
        rows += [(g, int(p), int(s), b"AC") for p, s in zip(pos, sp)]
        for _ in range(loci_per_group - 1):
            a = int(rng.integers(0, span))
            loci.append((g, a, a + int(rng.integers(0, span)), b"AC"))
        loci.append((g, 0, span, b"AC"))
    order = rng.permutation(len(rows))
    return [rows[i] for i in order], loci


def chain_table(n=20_000, n_loci=3_000, seed=1):
    """one group, many loci one behind the other in the caller's order (not in position order): the sequential chain"""
    rng = np.random.default_rng(seed)
    pos = rng.integers(0, 60_000, n)
    rows = [(0, int(p), int(s), b"AGG") for p, s in zip(pos, rng.choice([LEFT, RIGHT, NONE], n))]
    a = rng.integers(0, 60_000, n_loci)
    loci = [(0, int(x), int(x) + int(w), b"AGG") for x, w in zip(a, rng.integers(0, 200, n_loci))]
    return rows, loci


def many_groups_table(n_groups=5_000, seed=2):
    """n_groups groups (50 contigs x 100 units) of a few reads, one locus each"""
    rng = np.random.default_rng(seed)
    units = []
    for a in b"ACGT":
        for b in b"ACGT":
            for c in b"ACGT":
                for d in b"ACGT":
                    units.append(bytes([a, b, c, d]))
    rows, loci = [], []
    for g in range(n_groups):
        tid, unit = g // 100, units[g % 100]
        for p in rng.integers(0, 1000, int(rng.integers(1, 6))):
            rows.append((tid, int(p), int(rng.choice([LEFT, RIGHT, NONE])), unit))
        a = int(rng.integers(0, 1000))
        loci.append((tid, a, a + int(rng.integers(0, 500)), unit))
    order = rng.permutation(len(rows))
    lorder = rng.permutation(len(loci))
    return [rows[i] for i in order], [loci[j] for j in lorder]


def wrap_table(m=65_537):
    """one range holding m reads: n_total wraps in its uint16, the list holds them all"""
    rows = [(0, 1000 + (i % 977), (LEFT, RIGHT, NONE)[i % 3], b"AC") for i in range(m)] + [(0, 5000, NONE, b"AC")]
    return rows, [(0, 1, 3000, b"AC"), (0, 1, 9000, b"AC")]


def random_table(seed, n_max=2000, loci_max=300):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, n_max + 1))
    nl = int(rng.integers(1, loci_max + 1))
    n_tid = int(rng.integers(1, 4))
    units = [b"A", b"AC", b"AGC", b"AAAAAG"][:int(rng.integers(1, 5))]
    span = int(rng.choice([20, 200, 3000]))
    base = int(rng.choice([0, 0, 2 ** 31 - span // 2, 2 ** 32 - span]))      # ties and overlaps; some tables near 2^31 and 2^32
    t = np.zeros(n, api.TREAD_DTYPE)
    t["tid"] = rng.integers(-1, n_tid, n)
    t["position"] = (base + rng.integers(0, span, n)).astype(np.uint64).astype(np.uint32)
    t["repeat"] = np.array(units, "S6")[rng.integers(0, len(units), n)]
    t["split"] = rng.choice([LEFT, RIGHT, BOTH, NONE, TAKEN], n, p=[0.3, 0.3, 0.05, 0.3, 0.05])
    t["qname_id"] = np.arange(n)
    loci = []
    for _ in range(nl):
        a = base + int(rng.integers(0, span))
        kind = int(rng.integers(0, 10))
        b = a + int(rng.integers(0, max(2, span // 8))) if kind else a - int(rng.integers(0, 5))
        if kind == 1:
            a = int(rng.integers(0, 2))
        if kind == 2:
            b = M32
        loci.append((int(rng.integers(-1, n_tid + 1)), min(a, M32), max(0, min(b, M32)), units[int(rng.integers(0, len(units)))] if kind != 3 else b"AT"))
    return t, loci_of(loci)


def assert_same(got, want, what=""):
    """(treads, loci, lists) of the device entry point against the host function's: the split column (and every other column,
    untouched), every field of every locus, every assigned list"""
    (gt, gl, ga), (wt, wl, wa) = got, want
    assert np.array_equal(gt["split"], wt["split"]), what
    for f in api.TREAD_DTYPE.names:
        assert np.array_equal(gt[f], wt[f]), (what, f)
    for f in api.BOUNDS_DTYPE.names:
        assert np.array_equal(gl["b"][f], wl["b"][f]), (what, f)
    assert np.array_equal(gl["name"], wl["name"]), what
    assert len(ga) == len(wa), what
    for j, (a, b) in enumerate(zip(ga, wa)):
        assert a.tolist() == b.tolist(), (what, j)
