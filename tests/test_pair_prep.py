"""The replay of pair.hip where its per-item preparation could go wrong (tests/pair_prep_cases.py): proportions exactly on 0.8,
0.2 and 0.9, wrapping products, align_length 0, mapq ties; the second visit of the unmapped tail; which of three or four primary
records was stored; runs that reach into the 16-item halo, on the array's last tile too; the record on which the reference's
doAssert is raised; units of every length in both of their forms; the same in runs of more than 15 items (pair_long_kernel);
blocks that emit more than their stage holds.

CPU half: every case reaches its edge and differs from its neighbour, from the oracle alone.  -m gpu half: the device join's
treads against the oracle's, field by field in .bin order, with the default grid and with a grid of one and of two blocks
(STRL_GRID_G, read once per process: each in a child process that runs every case)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import pair_prep_cases as pp
from helpers import treads_equal

HERE = os.path.dirname(os.path.abspath(__file__))
ASSERT_TEXT = r"repeat_count >= 256 \(doAssert extract\.nim:72\)"


# ---- CPU -----------------------------------------------------------------------------------------------------------------------
def test_reads_score_as_the_cases_say(oracle):
    print(pp.read_conditions())


@pytest.mark.parametrize("name,p,q", pp.CASES)
def test_case_reaches_its_edge(oracle, name, p, q):
    print(name, p, q, pp.conditions(name, p, q))


@pytest.mark.parametrize("kind", pp.ASSERT_KINDS)
def test_long_homopolymer_sits_where_the_case_says(oracle, kind):
    pp.assert_conditions(kind)


# ---- GPU -----------------------------------------------------------------------------------------------------------------------
CHILD = """
import sys, numpy as np
sys.path[:0] = [%r, %r]
import pair_cases as pc, pair_prep_cases as pp
from strling_amd import api
out = sys.argv[1]
c = api.Context(0)
def run(rec, n_tail, p, q):
    c.set_opts(p, q, pc.MEDIAN); c.set_genome(None)
    soa = api.Soa(rec); rows, qh = soa.pair_rows()
    c.extract_device(soa.c_struct(), api.CPairSoa(rows.ctypes.data, qh.ctypes.data), n_tail)
    return c.treads_fetch()[0]
for name, p, q in pp.CASES:
    groups, rec, n_tail, index = pp.batch(name)
    np.save("%%s/%%s_%%s_%%d.npy" %% (out, name, p, q), run(rec, n_tail, p, q))
for kind in pp.ASSERT_KINDS:
    rec, n_tail, index = pp.build(pp.assert_groups(kind), "pa_" + kind[:3])
    try:
        np.save("%%s/assert_%%s.npy" %% (out, kind), run(rec, n_tail, 0.8, 40))
    except api.StrlingError as e:
        open("%%s/assert_%%s.txt" %% (out, kind), "w").write(str(e))
# the context is usable after the error
groups, rec, n_tail, index = pp.batch("stored")
np.save(out + "/after_error.npy", run(rec, n_tail, 0.8, 40))
c.close()
""" % (os.path.dirname(HERE), HERE)


@pytest.mark.gpu
@pytest.mark.parametrize("grid", [None, 1, 2])
def test_every_case_through_the_device_replay(oracle, tmp_path, grid):
    for name, p, q in pp.CASES:
        pp.conditions(name, p, q)
    env = {k: v for k, v in os.environ.items() if k != "STRL_GRID_G"}
    if grid:
        env["STRL_GRID_G"] = str(grid)
    subprocess.run([sys.executable, "-c", CHILD, str(tmp_path)], check=True, env=env)
    for name, p, q in pp.CASES:
        exp = pp.case(name, p, q)[4]
        ok, why = treads_equal(np.load(str(tmp_path / ("%s_%s_%d.npy" % (name, p, q)))), exp)
        assert ok, (name, p, q, grid, why)
    for kind in pp.ASSERT_KINDS:
        rec, n_tail, exp = pp.assert_conditions(kind)
        if kind == "reached":
            assert re.search(ASSERT_TEXT, open(str(tmp_path / "assert_reached.txt")).read())
        else:
            ok, why = treads_equal(np.load(str(tmp_path / ("assert_%s.npy" % kind))), exp)
            assert ok, (kind, grid, why)
    ok, why = treads_equal(np.load(str(tmp_path / "after_error.npy")), pp.case("stored", 0.8, 40)[4])
    assert ok, why
