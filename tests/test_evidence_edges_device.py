"""The evidence kernel (strling_amd/csrc/evidence.hip) on the device over the case table of tests/evidence_cases.py: what the
CPU suite cannot see of it -- the walk through the 4 KiB LDS window at every alignment and over a record longer than the
window, the ballots and ranks at 0, 255, 256, 257 and 4096 records and with no kept record, the row reservation across the
regions of a call, the depth scan and histogram at their clamps, the LDS hash table with two names of one murmur value and
with 4096 equal names -- against spanners() as the oracle restates it.  tests/test_evidence_cases.py proves on the CPU that
every case reaches the edge it is named after (its witness) and runs the per-record rule under sanitizers.

strl_evidence_records takes ONE window, histogram and min_mapq per call, and the table needs a few of each (window 0, 500 and
4095; min_mapq 0 for the placed unmapped mates): "one call" below is one call per such setting, the cases of a setting in the
order given."""
import time

import numpy as np
import pytest

import evidence_cases as ec
from strling_amd import api
from test_evidence_device import _same


def _run(ctx, cases):
    """{case id: (supports, median_depth, expected_spanners, status)}; the cases of one setting share a call, in their order"""
    groups = {}
    for c in cases:
        groups.setdefault((c.window, c.min_mapq, id(c.frag)), []).append(c)
    out = {}
    for (window, min_mapq, _), cs in groups.items():
        got = ctx.evidence_records([c.raw for c in cs], np.array([c.bound for c in cs], api.BOUNDS_DTYPE), window, cs[0].frag, min_mapq)
        out.update({c.id: d for c, d in zip(cs, got)})
    return out, len(groups)


def _bytes(d):
    return d[0].tobytes(), d[1], np.float32(d[2]).view(np.uint32), d[3]


@pytest.fixture(scope="module")
def refs():
    return ec.references()


@pytest.fixture(scope="module")
def table(ctx):
    t0 = time.perf_counter()
    got, n_calls = _run(ctx, ec.answered())
    print(f"the table of {len(ec.answered())} cases in {n_calls} calls: {time.perf_counter() - t0:.3f} s")
    return got


@pytest.mark.gpu
def test_every_case_equals_the_oracle(table, refs):
    """no case of a .. h is passed on, and every one equals spanners(): supports, median, the float32 bits of expected_spanners"""
    cases = ec.answered()
    assert len(table) == len(cases)
    for c in cases:
        d, ref = table[c.id], refs[c.id]
        assert c.witness(ref), c
        assert d[3] == 0, (c, "passed on")
        assert _same(d, ref), (c, d[1:], ref[1:], len(d[0]), len(ref[0]))


@pytest.mark.gpu
def test_shuffled_and_by_family_give_the_same_answers(ctx, table):
    """a region's answer does not depend on its neighbours in the call: the table in a fixed shuffled order, and each family as
    a call of its own, give the bytes the table order gave"""
    cases = list(ec.answered())
    order = np.random.default_rng(20240611).permutation(len(cases))
    assert not np.array_equal(order, np.arange(len(cases)))
    shuffled, _ = _run(ctx, [cases[i] for i in order])
    for c in cases:
        assert shuffled[c.id][3] == 0 and _bytes(shuffled[c.id]) == _bytes(table[c.id]), (c, "shuffled")
    for fam in sorted({c.family for c in cases}):
        alone, _ = _run(ctx, [c for c in cases if c.family == fam])
        assert alone
        for cid, d in alone.items():
            assert d[3] == 0 and _bytes(d) == _bytes(table[cid]), (cid, "family alone")


@pytest.mark.gpu
def test_two_runs_give_identical_bytes(ctx, table):
    again, _ = _run(ctx, ec.answered())
    for cid, d in table.items():
        assert _bytes(again[cid]) == _bytes(d), cid


@pytest.mark.gpu
def test_refused_bytes_are_passed_on_and_their_neighbours_answered(ctx, refs):
    """the inputs of family i (tests/test_evidence_cases.py takes them clean under AddressSanitizer first) between answered
    regions in one call: exactly they give status 2 with no supports; the others equal the oracle"""
    near = [c for c in ec.answered() if (c.window, c.min_mapq) == (500, 20) and c.family in "abegh" and c.rec.n <= 300]
    assert len(near) > 3 * len(ec.refused())
    mixed, k = [], 0
    for c in ec.refused():
        mixed += [near[k], near[k + 1], c]
        k += 2
    mixed += near[k:k + 2]
    assert {(c.window, c.min_mapq, id(c.frag)) for c in mixed} == {(500, 20, id(ec.FRAG_WIDE))}
    got = ctx.evidence_records([c.raw for c in mixed], np.array([c.bound for c in mixed], api.BOUNDS_DTYPE), 500, ec.FRAG_WIDE, 20)
    assert [d[3] for d in got] == [2 if c.refused else 0 for c in mixed]
    for c, d in zip(mixed, got):
        if c.refused:
            assert len(d[0]) == 0 and d[1] == 0 and d[2] == 0, c
        else:
            assert _same(d, refs[c.id]), c


@pytest.mark.gpu
def test_the_same_region_at_sixteen_alignments(ctx, refs):
    """the small region behind fillers of every length mod 16 (valid one-record regions): sixteen identical answers, the oracle's"""
    regions, reached = ec.alignment_regions()
    assert sorted(reached) == list(range(16))
    got = ctx.evidence_records([r[0] for r in regions], np.array([r[1] for r in regions], api.BOUNDS_DTYPE), 500, ec.FRAG_WIDE, 20)
    assert all(d[3] == 0 for d in got)
    copies = [d for d, r in zip(got, regions) if r[2]]
    assert len(copies) == 16
    ref = refs["h-small-region"]
    assert len(ref[0]) >= 2
    for d in copies:
        assert _same(d, ref) and _bytes(d) == _bytes(copies[0])
