"""The device radix sort (strling_amd/csrc/sort.hip) called the way the pipelines call it, through strl_sort_probe: every case of
tests/sort_cases.py -- a device count that is 0, short of or beyond n_max; a dirty, skewed, exactly sized scratch with the chunk
tables zeroed by the sort or by the caller; sorts of different pass counts chained without a sync; bit windows at the ends;
digit patterns random keys never form -- against numpy's stable argsort.  Integer equality throughout.

The table layout is checked on the host first (nothing is launched); no case with a dirty scratch runs if it is wrong."""
import numpy as np
import pytest

import sort_cases as sc
from strling_amd import api

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def layout(ctx):
    """radix_sort_tables reports the region the sort accumulates into, as calculated from sort.h's formulas"""
    for n_max in sc.LAYOUT_NMAX:
        k, v = np.zeros(n_max, np.uint64), np.zeros(n_max, np.uint32)
        for bits in sc.LAYOUT_BITS:
            for skew in sc.SKEWS:
                out = ctx.sort_probe(k, v, k, v, 0, n_max, [], scratch_skew=skew, layout_bits=bits)[4]
                assert (out["tables_off"], out["tables_bytes"]) == sc.tables_region(skew, n_max, bits), (n_max, bits, skew)
                assert out["rc"] == [] and out["guard_bad"] == 0
    return True


def test_table_layout(layout):
    assert layout


def _probe(ctx, c):
    k0, v0, k1, v1, out = ctx.sort_probe(c.keys, c.vals, c.alt_keys, c.alt_vals, c.d_n, c.n_max, c.stages, c.skew, c.delta, c.poison)
    return (k0, v0, k1, v1, out["result_in_alt"], out["rc"]), out


@pytest.mark.parametrize("name", sc.NAMES)
def test_sort_case(ctx, layout, name):
    c = sc.case(name)
    got, out = _probe(ctx, c)
    assert sc.verdict(c, got) == []
    assert out["guard_bad"] == 0                              # nothing written in front of or behind the scratch it was handed
    assert (out["tables_off"], out["tables_bytes"]) == sc.tables_region(c.skew, c.n_max, c.stages[0][1])
    again, out2 = _probe(ctx, c)                               # the same context, a second time: the same bytes
    assert out2 == out and again[4:] == got[4:]
    for a, b in zip(got[:4], again[:4]):
        assert a.tobytes() == b.tobytes()
