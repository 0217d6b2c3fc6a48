"""pair_groups_kernel (pair.hip) on batches laid out item by item (tests/pair_dense_cases.py): how many runs start in a 512-item
block and where, runs of one item at the ends of the array and on either side of a block seam, and a grid so small that a block
takes many tiles one after the other.

Each case has two halves: the CPU half shows, from the batch's own qname hashes and the oracle, that the batch has the layout the
case is named for; the -m gpu half asserts the same and compares the device join's treads with the oracle's, field by field in
.bin order.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import pair_cases as pc
import pair_dense_cases as dc
from helpers import treads_equal
from strling_amd import api

HERE = os.path.dirname(os.path.abspath(__file__))
SINGLE = [n for n in dc.CASES if n != "all"]


# ---- CPU: the layouts --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(dc.CASES))
def test_case_has_the_layout_it_is_named_for(oracle, name):
    print(name, dc.case_conditions(name))


def test_long_read_case_is_a_lone_read_whose_word_counts_256_or_more(oracle):
    dc.homo_conditions()


def test_mixed_draws_have_their_layouts_and_cover_every_kind_of_group(oracle):
    for d, o in enumerate(dc.mixed_conditions()):
        print("draw", d, o)


def test_small_grids_reach_a_third_tile(oracle):
    spec, rec, n_tail, qh, exp = dc.case("all")
    for grid in (1, 2):
        assert rec.n > 2 * dc.PG_BLOCK * grid


# ---- GPU ---------------------------------------------------------------------------------------------------------------------
def _device(ctx, rec, n_tail=0, p=0.8, q=40):
    """strl_extract_device + strl_treads_fetch: the device join itself, no fallback"""
    ctx.set_opts(p, q, pc.MEDIAN)
    ctx.set_genome(None)
    soa = api.Soa(rec)
    rows, qh = soa.pair_rows()
    ctx.extract_device(soa.c_struct(), api.CPairSoa(rows.ctypes.data, qh.ctypes.data), n_tail)
    return ctx.treads_fetch()[0]


def _same(got, exp):
    ok, why = treads_equal(got, exp)
    assert ok, why


@pytest.mark.gpu
@pytest.mark.parametrize("name", SINGLE)
def test_layout_through_the_device_replay(ctx, oracle, name):
    dc.case_conditions(name)
    spec, rec, n_tail, qh, exp = dc.case(name)
    _same(_device(ctx, rec, n_tail), exp)


@pytest.mark.gpu
def test_lone_read_with_a_count_of_256_fails_where_the_reference_asserts(ctx, oracle):
    """a 510-base homopolymer that is a run of its own in front of the tail: it emits nothing, but to_tread reads its word, and
    the call fails with the reference's doAssert"""
    dc.homo_conditions()
    spec, rec, n_tail, qh = dc.homo_case()
    with pytest.raises(api.StrlingError, match=r"repeat_count >= 256 \(doAssert extract\.nim:72\)"):
        _device(ctx, rec, n_tail)
    # the context is usable afterwards
    spec, rec, n_tail, qh, exp = dc.case("all_pairs")
    _same(_device(ctx, rec, n_tail), exp)


@pytest.mark.gpu
def test_mixed_draws_through_the_device_replay(ctx, oracle):
    dc.mixed_conditions()
    for d in range(dc.N_DRAWS):
        spec, rec, n_tail, qh, exp = dc.mixed_case(d)
        ok, why = treads_equal(_device(ctx, rec, n_tail), exp)
        assert ok, (d, why)


@pytest.mark.gpu
@pytest.mark.parametrize("grid", [1, 2])
def test_every_layout_with_a_grid_of_one_or_two_blocks(oracle, tmp_path, grid):
    """STRL_GRID_G: pair_groups_kernel runs as `grid` blocks, so a block takes seven or fourteen 512-item tiles one after the
    other (the grid-stride rounds the default grid reaches only beyond 2^22 items): the items, the staged treads and the
    emitted count of one tile are overwritten by the next.  In a process of its own (the switch is read once)."""
    dc.case_conditions("all")
    spec, rec, n_tail, qh, exp = dc.case("all")
    assert rec.n > 2 * dc.PG_BLOCK * grid
    script = (
        "import sys, numpy as np\n"
        "sys.path[:0] = [%r, %r]\n"
        "import pair_cases as pc, pair_dense_cases as dc\n"
        "from strling_amd import api\n"
        "spec, rec, n_tail, qh, exp = dc.case('all')\n"
        "c = api.Context(0); c.set_opts(0.8, 40, pc.MEDIAN); c.set_genome(None)\n"
        "soa = api.Soa(rec); rows, qh = soa.pair_rows()\n"
        "c.extract_device(soa.c_struct(), api.CPairSoa(rows.ctypes.data, qh.ctypes.data), n_tail)\n"
        "np.save(sys.argv[1], c.treads_fetch()[0])\n"
        "c.close()\n"
    ) % (os.path.dirname(HERE), HERE)
    out = str(tmp_path / "treads.npy")
    subprocess.run([sys.executable, "-c", script, out], check=True, env=dict(os.environ, STRL_GRID_G=str(grid)))
    _same(np.load(out), exp)
