"""The device replay of Cache.add (strling_amd/csrc/pair.hip) at its arithmetic and staging edges, against the oracle, exactly.

The inputs and the conditions that keep them from going vacuous are in tests/pair_cases.py; every condition is asserted on the
oracle's output, here in the CPU half and again in the -m gpu half.  CPU: the host twins of the rule functions on the grid, the
crafted batch through the host pairer.  GPU: the same grid through the device functions in one launch per option set, the
crafted batch through the device join / strl_extract / a chunked run, and the staging mechanisms of pair.hip -- in-block replay
(runs of up to 15 items, 16-item halo), pair_long_kernel (16..512 items), the 256-tread LDS emit stage, the probe's flush, the
capacity errors."""
import os
import subprocess
import sys

import numpy as np
import pytest

import pair_cases as pc
from helpers import oracle_words, soft_items_expected, treads_equal
from strling_amd import api

HERE = os.path.dirname(os.path.abspath(__file__))
ZERO_OPTS = (0.8, 40, 0)


def _units_as_treads():
    units = pc.all_units()
    A = np.zeros(len(units), api.TREAD_DTYPE)
    A["repeat"] = units
    return units, A


def _check_canonical(ctx, oracle):
    units, A = _units_as_treads()
    assert len(units) == 5460
    exp = np.array([oracle.canonical_repeat(u.decode()).encode() for u in units], "S6")
    assert 500 < int((exp != A["repeat"]).sum()) < 5460 - 500          # both answers of the comparison, many times
    res, got = api.pair_rules(ctx, 2, A, A.copy(), ZERO_OPTS)
    bad = np.flatnonzero(got["repeat"] != exp)
    assert bad.size == 0, [(units[i], got["repeat"][i], exp[i]) for i in bad[:5]]
    for f in ("tid", "position", "flag", "split", "mapping_quality", "repeat_count", "align_length", "qname_id"):
        assert np.array_equal(got[f], A[f]), f


def _check_rule_grid(ctx):
    g, expect = pc.rule_grid(), pc.rule_expect()
    pc.rule_grid_conditions(g)
    counts = pc.rule_conditions(g, expect)
    print("rule grid:", g.n, "cases;", counts)
    for (op, j), (idx, res, a) in expect.items():
        got_res, got_a = api.pair_rules(ctx, op, g.A[idx], g.B[idx], pc.RULE_OPTS[j], g.bpos[idx])
        bad = np.flatnonzero(got_res != res)
        assert bad.size == 0, (op, pc.RULE_OPTS[j], [(g.A[idx][i], g.B[idx][i], int(g.bpos[idx][i]), int(res[i])) for i in bad[:3]])
        ok, why = treads_equal(got_a, a)
        assert ok, (op, pc.RULE_OPTS[j], why)


# ---- CPU: the host twins and the generators' conditions ------------------------------------------------------------------
def test_canonical_repeat_host_twin_on_every_unit(oracle):
    _check_canonical(None, oracle)


def test_rule_grid_host_twins_equal_the_oracle(oracle):
    """adjust_by / unplaced_pair of host_logic.cpp on ~28 000 cases: return value and every field of A afterwards"""
    _check_rule_grid(None)


@pytest.mark.parametrize("p,q", pc.PQ)
def test_crafted_batch_meets_its_conditions_and_the_host_pairer_equals_the_oracle(oracle, p, q):
    rec, n_tail = pc.crafted_batch()
    exp = pc.crafted_expect(p, q)
    print("crafted batch (p %.1f, min_mapq %d):" % (p, q), rec.n, "records;", pc.crafted_conditions(rec, exp, p, q))
    whole, softd = oracle_words(oracle, rec, None, oracle.make_opts(pc.MEDIAN, p, q))
    items = soft_items_expected(rec, whole, q)
    soft = np.zeros(len(items), api.SOFT_DTYPE)
    for j, (i, side) in enumerate(items):
        soft[j] = ((i << 1) | side, softd[(i, side)][0], softd[(i, side)][1], 0)
    got = api.pair_reads(rec, (p, q, pc.MEDIAN), whole, soft, n_tail)
    ok, why = treads_equal(got, exp)
    assert ok, why


ONE_QNAME = [(15, 14), (16, 16), (400, 400), (512, 512), (513, 512)]        # records under the qname, treads the oracle emits for them


def test_staging_batches_meet_their_conditions(oracle):
    for n, n_treads in ONE_QNAME:
        rec = pc.one_qname(n)
        assert len(pc.hot_expect(rec)) == n_treads + 600
    rec = pc.many_long_runs()
    assert len(pc.hot_expect(rec)) == 70 * 20 and 70 > 64
    rec = pc.hot_pairs(3000)
    assert rec.n == 6000 and len(pc.hot_expect(rec)) == 6000 > 256 * -(-6000 // 512)      # pigeonhole: a block emits more than 256
    rec = pc.seam_batch()
    print("seam batch:", pc.seam_conditions(rec, api.Soa(rec).pair_rows()[1], pc.hot_expect(rec)))


# ---- GPU -----------------------------------------------------------------------------------------------------------------
def _device(ctx, rec, n_tail=0, p=0.8, q=40, **caps):
    """strl_extract_device + strl_treads_fetch: the device join itself, no fallback"""
    ctx.set_opts(p, q, pc.MEDIAN)
    ctx.set_genome(None)
    soa = api.Soa(rec)
    rows, qh = soa.pair_rows()
    ctx.extract_device(soa.c_struct(), api.CPairSoa(rows.ctypes.data, qh.ctypes.data), n_tail, **caps)
    return ctx.treads_fetch()[0]


def _same(got, exp):
    ok, why = treads_equal(got, exp)
    assert ok, why


@pytest.mark.gpu
def test_canonical_repeat_device_on_every_unit(ctx, oracle):
    _check_canonical(ctx, oracle)


@pytest.mark.gpu
def test_rule_grid_device_functions_equal_the_oracle(ctx, oracle):
    """the same grid through adjust_by / unplaced_pair of pair.hip: one launch per rule and option set, one lane per case"""
    _check_rule_grid(ctx)


@pytest.mark.gpu
def test_batched_and_single_rule_entry_points_agree(ctx):
    """strl_pair_rule(ctx, ...) is the batched launch with n = 1"""
    g = pc.rule_grid()
    idx = g.of_opts(4)[:8]
    res, a = api.pair_rules(ctx, 0, g.A[idx], g.B[idx], pc.RULE_OPTS[4], g.bpos[idx])
    for k, i in enumerate(idx):
        r1, a1 = api.pair_rule(ctx, 0, g.A[i], g.B[i], pc.RULE_OPTS[4], int(g.bpos[i]))
        assert r1 == res[k] and all(a1[f] == a[k][f] for f in pc.TREAD_FIELDS)      # (the dtype has padding bytes: field by field)


@pytest.mark.gpu
@pytest.mark.parametrize("p,q", pc.PQ)
def test_crafted_batch_through_the_device_replay(ctx, oracle, p, q):
    """read lengths 150..510, all orientations, mapq around min_mapq, every mate placement, soft clips around 16 bases and 0.9:
    the device join, strl_extract, and a chunked run cut between mates, each against the oracle"""
    rec, n_tail = pc.crafted_batch()
    exp = pc.crafted_expect(p, q)
    pc.crafted_conditions(rec, exp, p, q)
    _same(_device(ctx, rec, n_tail, p, q), exp)
    got, _ = ctx.extract(rec)
    _same(got, exp)
    edges = [0] + pc.cuts_between_mates(rec, n_tail) + [rec.n]
    keep, chunks = [], []
    for a, b in zip(edges[:-1], edges[1:]):
        soa = api.Soa(rec.slice(a, b))
        rows, qh = soa.pair_rows()
        keep.append((soa, rows, qh))
        chunks.append((soa.c_struct(), api.CPairSoa(rows.ctypes.data, qh.ctypes.data)))
    ctx.extract_chunks(chunks, n_tail)
    _same(ctx.treads_fetch()[0], exp)


@pytest.mark.gpu
@pytest.mark.parametrize("n,n_treads", ONE_QNAME)
def test_one_qname_on_n_alternating_records(ctx, oracle, n, n_treads):
    """15: the longest run the in-block replay takes; 16 .. 512: pair_long_kernel, 400 and 512 with more treads than the 256 of
    its LDS stage; 513: reported, and strl_extract repeats the batch on the host"""
    rec = pc.one_qname(n)
    exp = pc.hot_expect(rec)
    assert len(exp) == n_treads + 600
    if n <= 512:
        _same(_device(ctx, rec), exp)
    else:
        with pytest.raises(api.StrlingError, match="share the low 32 bits"):
            _device(ctx, rec)
    got, _ = ctx.extract(rec)
    _same(got, exp)


@pytest.mark.gpu
def test_more_long_runs_than_pair_long_kernel_has_blocks(ctx, oracle):
    rec = pc.many_long_runs()
    exp = pc.hot_expect(rec)
    assert len(exp) == 1400
    _same(_device(ctx, rec), exp)


@pytest.mark.gpu
def test_runs_across_block_seams(ctx, oracle):
    """runs that start in the last lanes of a 512-item block and lie in its halo, one that ends on the seam, a 16-item run over
    a seam; every block emits more than its 256-tread stage holds"""
    rec = pc.seam_batch()
    exp = pc.hot_expect(rec)
    pc.seam_conditions(rec, api.Soa(rec).pair_rows()[1], exp)
    _same(_device(ctx, rec), exp)


@pytest.mark.gpu
def test_capacities_are_reported_and_a_block_passes_its_emit_stage(ctx, oracle):
    """3000 hot pairs: 6000 items over 12 blocks and 6000 treads, so some block emits past its 256-tread LDS stage.  With room
    for 1024 items or 1024 treads strl_treads_fetch reports STRL_ERR_CAPACITY; the same context then runs it with defaults."""
    rec = pc.hot_pairs(3000)
    exp = pc.hot_expect(rec)
    assert rec.n == 6000 and len(exp) == 6000 > 256 * -(-6000 // 512)
    with pytest.raises(api.StrlingError, match=r"error -4: .*item_cap"):
        _device(ctx, rec, item_cap=1024)
    with pytest.raises(api.StrlingError, match=r"error -4: .*tread_cap"):
        _device(ctx, rec, tread_cap=1024)
    _same(_device(ctx, rec), exp)


@pytest.mark.gpu
def test_probe_flushes_mid_stream_with_one_block(oracle, tmp_path):
    """STRL_GRID_P=1: pair_probe_kernel runs as one block, 5056 reads per wave, every one a hit: each wave's 1024-entry stage
    fills and is flushed several times before the final flush.  In a process of its own (the switch is read once)."""
    assert -(-20000 // 4) > 4 * 1024
    script = (
        "import sys, numpy as np\n"
        "sys.path[:0] = [%r, %r]\n"
        "import pair_cases as pc\n"
        "from strling_amd import api\n"
        "rec = pc.hot_pairs(10000)\n"
        "c = api.Context(0); c.set_opts(0.8, 40, pc.MEDIAN); c.set_genome(None)\n"
        "soa = api.Soa(rec); rows, qh = soa.pair_rows()\n"
        "c.extract_device(soa.c_struct(), api.CPairSoa(rows.ctypes.data, qh.ctypes.data), 0)\n"
        "np.save(sys.argv[1], c.treads_fetch()[0])\n"
        "c.close()\n"
    ) % (os.path.dirname(HERE), HERE)
    out = str(tmp_path / "treads.npy")
    subprocess.run([sys.executable, "-c", script, out], check=True, env=dict(os.environ, STRL_GRID_P="1"))
    exp = pc.hot_expect(pc.hot_pairs(10000))
    assert len(exp) == 20000
    _same(np.load(out), exp)
