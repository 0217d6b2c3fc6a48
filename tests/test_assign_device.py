"""strl_assign_reads_loci_device (strling_amd/csrc/assign.hip: given loci take their reads on the device) against the host
function, api.assign_reads_loci, which stays the yardstick: the split column, every field of every locus, every assigned list.
The tables: tests/assign_cases.py."""
import ctypes as C

import numpy as np
import pytest

from strling_amd import api, synth
import assign_cases as AC

pytestmark = pytest.mark.gpu
MODES = [api.MODE_MERGE, api.MODE_CALL]


def both(ctx, t, lo, mode, what=""):
    got = api.assign_reads_loci_device(ctx, t, lo, mode)
    want = api.assign_reads_loci(t, lo, mode)
    AC.assert_same(got, want, what)
    info = api.assign_info_last(ctx)
    assert info.n_loci == len(lo)
    if len(lo) and len(t):
        taken = int(((want[0]["split"] == AC.TAKEN) & (np.asarray(t)["split"] != AC.TAKEN)).sum())
        assert (info.n_assigned, info.n_lost) == (sum(len(x) for x in want[2]), taken - sum(len(x) for x in want[2]))
    return got, want


@pytest.mark.parametrize("mode", MODES)
def test_base_case_and_the_oracles_rows(ctx, oracle, mode):
    """test_call.py's case: three samples, 300 loci and the locus that takes everything; the locus rows are merge.nim's"""
    from test_call import _loci_from_bounds
    t = synth.synth_treads(n_samples=3, n_loci=300, seed=4, n_contigs=4, contig_len=400_000)
    targets = [(f"chr{i + 1}", 400_000) for i in range(4)]
    ot = np.zeros(len(t), oracle.TREAD_DTYPE)
    for f in t.dtype.names:
        ot[f] = t[f]
    base = oracle.merge_text(ot, 560, targets, min_support=3, max_clip_dist=175).splitlines()[1:]
    bed = _loci_from_bounds(base, targets, np.random.default_rng(0), extra=[base[0].split("\t")[0] + "\t0\t399999\t" + base[0].split("\t")[3] + "\teverything"])
    exp = oracle.merge_text(ot, 560, targets, min_support=3, max_clip_dist=175, loci_text=bed).splitlines()[1:]
    loci = oracle.parse_bed(bed, targets, 560)
    lo = np.zeros(len(loci), api.LOCUS_DTYPE)
    for j, L in enumerate(loci):
        for f in api.BOUNDS_DTYPE.names:
            lo["b"][f][j] = getattr(L.b, f)
        lo["name"][j] = L.name
    (t2, lo2, taken), _ = both(ctx, t, lo, mode)
    rows = []
    for j in range(len(lo2)):
        b = lo2["b"][j]
        rows.append("\t".join([targets[int(b["tid"])][0], str(int(b["left"])), str(int(b["right"])), b["repeat"].decode(), lo2["name"][j].decode(),
                               str(int(b["left_most"])), str(int(b["right_most"])), str(int(b["center_mass"])), str(int(b["n_left"])),
                               str(int(b["n_right"])), str(int(b["n_total"]))]))
    assert (t["tid"] >= 0).all() and rows == exp[:len(rows)]         # (no unplaced tread: the two modes take the same)
    assert sum(len(x) for x in taken) > 50


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", sorted(AC.edge_tables()))
def test_edge_tables(ctx, name, mode):
    rows, loci = AC.edge_tables()[name]
    t, lo = AC.treads_of(rows), AC.loci_of(loci)
    (t2, lo2, _), _ = both(ctx, t, lo, mode, name)
    both(ctx, t2, lo, mode, name + ", again on the array the first call marked")


@pytest.mark.parametrize("mode", MODES)
def test_edge_tables_side_by_side(ctx, mode):
    """all edge tables in one call, each on references of its own, their treads and loci interleaved"""
    rows, loci = [], []
    for k, name in enumerate(sorted(AC.edge_tables())):
        r, l = AC.edge_tables()[name]
        rows += [(tid if tid < 0 else tid + 10 * k, p, s, u) for tid, p, s, u in r]
        loci += [(tid if tid < 0 else tid + 10 * k, a, b, u) for tid, a, b, u in l]
    rng = np.random.default_rng(5)
    rows = [rows[i] for i in rng.permutation(len(rows))]
    both(ctx, AC.treads_of(rows), AC.loci_of(loci), mode)


def test_groups_of_the_wave_width_and_the_sort_tile(ctx):
    rows, loci = AC.widths_table([63, 64, 65, 2047, 2048, 2049])
    both(ctx, AC.treads_of(rows), AC.loci_of(loci), api.MODE_CALL)


def test_references_beyond_2_17_take_two_sorts(ctx):
    """a tid of 2^17 or more does not fit the 64-bit key beside the position: sorted by position, then by group"""
    rows, loci = AC.widths_table([5, 64, 300, 2049])
    far = lambda tid: 140_000 + 70_000 * tid
    both(ctx, AC.treads_of([(far(t), p, s, u) for t, p, s, u in rows] + [(0, 7, AC.NONE, b"AC")]),
         AC.loci_of([(far(t), a, b, u) for t, a, b, u in loci] + [(0, 1, 9, b"AC")]), api.MODE_MERGE)


@pytest.fixture(scope="module")
def chain():
    rows, loci = AC.chain_table()
    return AC.treads_of(rows), AC.loci_of(loci)


def test_one_group_of_20000_reads_and_3000_loci(ctx, chain):
    both(ctx, chain[0], chain[1], api.MODE_CALL)


def test_5000_groups_with_one_locus_each(ctx):
    rows, loci = AC.many_groups_table()
    both(ctx, AC.treads_of(rows), AC.loci_of(loci), api.MODE_MERGE)
    assert api.assign_info_last(ctx).n_groups == 5000


def test_a_range_of_65537_reads_wraps_its_count(ctx):
    rows, loci = AC.wrap_table()
    (t2, lo2, taken), _ = both(ctx, AC.treads_of(rows), AC.loci_of(loci), api.MODE_CALL)
    assert int(lo2["b"]["n_total"][0]) == 1 and len(taken[0]) == 65_537
    assert int(lo2["b"]["n_total"][1]) == 0 and len(taken[1]) == 0    # the one read behind the range was lost to the first locus


@pytest.mark.parametrize("part", range(6))
def test_random_tables(ctx, part):
    """300 seeds on one context: n <= 2000, up to 300 loci, positions from a range small enough for ties and overlaps"""
    for seed in range(50 * part, 50 * part + 50):
        t, lo = AC.random_table(seed)
        both(ctx, t, lo, seed % 2, f"seed {seed}")


def test_capacity_one_too_small_then_a_correct_call(ctx):
    rows, loci = AC.edge_tables()["the_same_locus_twice"]
    t, lo = AC.treads_of(rows), AC.loci_of(loci)
    want = api.assign_reads_loci(t, lo, api.MODE_CALL)
    need = sum(len(x) for x in want[2])
    assert need == 7
    with pytest.raises(api.StrlingError, match=r"error -4: .*need 7"):
        api.assign_reads_loci_device(ctx, t, lo, api.MODE_CALL, cap=need - 1)
    AC.assert_same(api.assign_reads_loci_device(ctx, t, lo, api.MODE_CALL, cap=need), want)


@pytest.mark.parametrize("mode", MODES)
def test_bad_treads_are_refused_and_the_context_goes_on(ctx, mode):
    lo = AC.loci_of([(0, 1, 1000, b"AC")])
    good = [(0, 5, AC.NONE, b"AC"), (0, 6, AC.LEFT, b"AC")]
    for bad in ((0, 7, AC.NONE, b"AN"), (0, 7, AC.NONE, b"A\0C"), (0, 7, AC.TAKEN, b"acgt"), (-2, 7, AC.NONE, b"AC")):
        t = AC.treads_of(good + [bad])
        with pytest.raises(api.StrlingError, match="error -3"):
            api.assign_reads_loci_device(ctx, t, lo, mode)
        both(ctx, AC.treads_of(good), lo, mode)
    t = AC.treads_of(good)
    rc = ctx.L.strl_assign_reads_loci_device(ctx.h, t.ctypes.data, 0x7ffffff1, mode, lo.ctypes.data, lo.size, None, None, 0)
    assert rc == -3                                                   # strl_cluster's bound on n, refused before anything is read
    off = np.zeros(lo.size + 1, np.uint64)
    rc = ctx.L.strl_assign_reads_loci_device(ctx.h, t.ctypes.data, 0x7ffffff1, mode, lo.ctypes.data, lo.size, off.ctypes.data, None, 0)
    assert rc == -3 and b"too many treads" in ctx.L.strl_last_error()
    both(ctx, t, lo, mode)


def test_the_largest_cases_twice_give_the_same(ctx, chain):
    rows, loci = AC.wrap_table()
    for t, lo in (chain, (AC.treads_of(rows), AC.loci_of(loci))):
        a = api.assign_reads_loci_device(ctx, t, lo, api.MODE_CALL)
        b = api.assign_reads_loci_device(ctx, t, lo, api.MODE_CALL)
        AC.assert_same(a, b)


def test_no_lists_asked_for(ctx):
    """assigned = NULL (merge -l): marks, counts and offsets all the same"""
    rows, loci = AC.widths_table([65, 300])
    t, lo = AC.treads_of(rows), AC.loci_of(loci)
    want = api.assign_reads_loci(t, lo, api.MODE_MERGE)
    t2, lo2 = t.copy(), lo.copy()
    off = np.zeros(lo.size + 1, np.uint64)
    rc = ctx.L.strl_assign_reads_loci_device(ctx.h, t2.ctypes.data, t2.size, api.MODE_MERGE, lo2.ctypes.data, lo2.size, off.ctypes.data, None, 0)
    assert rc == 0, ctx.L.strl_last_error()
    assert np.array_equal(t2["split"], want[0]["split"]) and np.array_equal(lo2["b"]["n_total"], want[1]["b"]["n_total"])
    assert off.tolist() == np.concatenate([[0], np.cumsum([len(x) for x in want[2]])]).tolist()
