"""The three kernels behind the inflate of a region read (strling_amd/csrc/bgzf.hip: crc32_kernel, region_walk_kernel,
region_copy_kernel) on the device over the calls of tests/region_cases.py: status, bytes, out_off and out_len of every case
against the plain-Python model, one call per family; the table of one-bit twins through the CRC check of all three callers of
regions_inflate_walk (strl_regions_fetch, strl_regions_evidence, strl_pull_select), each refusal with STRL_ERR_CRC and a good
call behind it; the capacity error and the call that follows it.  tests/test_region_cases.py proves on the CPU that every case
reaches the edge it is named for and that nothing sent here is read outside its buffer."""
import time

import numpy as np
import pytest

import evidence_cases as ec
import region_cases as rc
from strling_amd import api

OTHER_ENTRIES = ("size1-byte0", "size3-byte2", "size4-byte3", "size255-byte254", "size256-byte252", "size257-byte256", "size260-lane63", "size516-byte515",
                 "size65535-byte65534", "size65536-byte256", "nine-blocks-bad0", "nine-blocks-bad5", "nine-blocks-bad8")


def _fetch(ctx, call, **kw):
    return ctx.regions_fetch(call.streams, call.isize, call.requests, crcs=call.crcs, layout=True, **kw)


def _equal(call, answer):
    got, off, ln = answer
    assert len(got) == len(call.cases)
    for c, e, g, eo, el, o, n in zip(call.cases, call.expect, got, call.out_off, call.out_len, off, ln):
        assert g[1] == e[1], (c, "status", g[1], e[1])
        assert (int(o), int(n)) == (eo, el), (c, "out_off, out_len", int(o), int(n), eo, el)
        assert g[0] == e[0], (c, "bytes", len(g[0]), len(e[0]))


@pytest.fixture(scope="module")
def answers(ctx):
    t0 = time.perf_counter()
    out = {c.name: _fetch(ctx, c) for c in rc.calls() if c.name != "c-grid"}
    print(f"{sum(len(c.cases) for c in rc.calls() if c.name != 'c-grid')} cases in {len(out)} calls: {time.perf_counter() - t0:.3f} s")
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", [c.name for c in rc.calls() if c.name != "c-grid"])
def test_every_case_equals_the_model(answers, name):
    call = rc.call(name)
    for c, t in zip(call.cases, call.traces):
        assert c.witness(t, call), c
    _equal(call, answers[name])


@pytest.mark.gpu
def test_the_copy_of_4100_requests():
    """the grid loop's second turn, on a context of its own: its out buffer has never held these bytes"""
    call = rc.call("c-grid")
    assert len(call.requests) > rc.COPY_GRID and all(call.out_len)
    own = api.Context(0)
    try:
        _equal(call, _fetch(own, call))
    finally:
        own.close()


@pytest.mark.gpu
def test_two_runs_of_the_largest_call_give_the_same_bytes(ctx, answers):
    call = max(rc.calls(), key=lambda c: c.tot)
    assert call.name == "w"
    again = _fetch(ctx, call)
    assert again[0] == answers["w"][0] and np.array_equal(again[1], answers["w"][1]) and np.array_equal(again[2], answers["w"][2])


@pytest.mark.gpu
def test_a_capacity_one_byte_short(ctx, answers):
    """STRL_ERR_CAPACITY with the bytes needed in out_off[0]; then the call with exactly that room, on the same context"""
    call = rc.call("c")
    assert call.needed > 0 and call.out_off[0] != call.needed
    with pytest.raises(api.StrlingError) as e:
        _fetch(ctx, call, cap=call.needed - 1)
    assert e.value.code == rc.ERR_CAPACITY and e.value.needed == call.needed
    _equal(call, _fetch(ctx, call, cap=call.needed))


def _refused(fn):
    with pytest.raises(api.StrlingError) as e:
        fn()
    return e.value.code


@pytest.mark.gpu
def test_every_twin_is_refused_by_its_crc(ctx, answers):
    """each row: the twin's CRC refuses the call with STRL_ERR_CRC (the block inflates: not the format error), the block's own
    CRC accepts it, and the good call behind the refusal gives the right bytes"""
    good = rc.call("k")
    t0 = time.perf_counter()
    for r in rc.crc_rows():
        streams = r.streams
        assert _refused(lambda: ctx.regions_fetch(streams, r.sizes, [r.request], crcs=r.refuse)) == rc.ERR_CRC, r
        assert ctx.regions_fetch(streams, r.sizes, [r.request], crcs=r.good) == [(b"", 1)], r
        assert ctx.regions_fetch(good.streams, good.isize, good.requests, crcs=good.crcs) == good.expect, r
    print(f"{len(rc.crc_rows())} refusals, 3 calls each: {time.perf_counter() - t0:.3f} s")


@pytest.mark.gpu
def test_the_other_callers_refuse_with_the_same_code(ctx, answers):
    """strl_regions_evidence and strl_pull_select reach the CRC check through regions_inflate_walk as well"""
    rows = {r.name: r for r in rc.crc_rows()}
    good = rc.call("s")
    bound = np.array([ec.bound(0, 1000, 1020, "A")], api.BOUNDS_DTYPE)
    tile = np.array([(0, 0, 100, 0, 100)], api.PULL_TILE_DTYPE)
    for name in OTHER_ENTRIES:
        r = rows[name]
        streams = r.streams
        assert _refused(lambda: ctx.regions_evidence(streams, r.sizes, [r.request], bound, 500, ec.FRAG_WIDE, 20, crcs=r.refuse)) == rc.ERR_CRC, r
        assert [d[3] for d in ctx.regions_evidence(streams, r.sizes, [r.request], bound, 500, ec.FRAG_WIDE, 20, crcs=r.good)] == [1], r
        assert _refused(lambda: ctx.pull_select(streams, r.sizes, [r.request], tile, crcs=r.refuse)) == rc.ERR_CRC, r
        sel = ctx.pull_select(streams, r.sizes, [r.request], tile, crcs=r.good)
        assert sel[0].size == 0 and sel[3].tolist() == [1], r
        assert ctx.regions_fetch(good.streams, good.isize, good.requests, crcs=good.crcs) == good.expect, r
