"""The clustering kernels (strling_amd/csrc/cluster.hip) on the cases of tests/cluster_cases.py, against the oracle: the same
rows, every field, in the same order.  tests/test_cluster_cases.py shows that each case reaches its edge."""
import time

import numpy as np
import pytest

import cluster_cases as cc
from strling_amd import api

pytestmark = pytest.mark.gpu

FIELDS = ("tid", "repeat", "left", "right", "left_most", "right_most", "center_mass", "n_left", "n_right", "n_total")


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


def _api_treads(t):
    at = np.zeros(len(t), api.TREAD_DTYPE)
    for f in at.dtype.names:
        at[f] = t[f]
    return at


def _same_rows(got, exp, what):
    assert len(got) == len(exp), (what, len(got), len(exp))
    for f in FIELDS:
        if not np.array_equal(got[f], exp[f]):
            bad = np.nonzero(got[f] != exp[f])[0]
            j = int(bad[0])
            raise AssertionError(f"{what}: {f} differs in {bad.size} of {len(exp)} rows, first at row {j}: got {got[j]}, expected {exp[j]}")


def _same_unplaced(u, exp_u, what):
    assert [(x["repeat"].decode(), int(x["count"])) for x in u] == exp_u, what


def _run(ctx, oracle, case, members=False, counts=None):
    """cluster `case` in each of its modes -> {mode: rows}"""
    at = _api_treads(case.treads)
    out = {}
    for mode in case.modes:
        what = f"{case.name} mode {mode}"
        exp_b, exp_u = case.expect(oracle, mode)
        b, u, st = ctx.cluster(at, mode, case.window, **case.kw())
        _same_rows(b, exp_b, what)
        if mode == api.MODE_CALL:
            _same_unplaced(u, exp_u, what)
        n_groups, n_clusters = counts[mode] if counts else (case.meta.get("n_groups"), case.meta.get("n_clusters"))
        if n_groups is not None:
            assert st.n_groups == n_groups, what
        if n_clusters is not None:
            assert st.n_clusters == n_clusters, what
        assert st.n_bounds == len(exp_b), what
        if members and mode == api.MODE_CALL:
            off, mem = ctx.cluster_members(len(b))
            exp_m = oracle.cluster_members_call(case.treads, case.window, **case.kw())
            assert len(exp_m) == len(b), what
            assert np.array_equal(mem, np.concatenate(exp_m).astype(np.uint32)), what
            assert np.array_equal(off, np.concatenate([[0], np.cumsum([len(m) for m in exp_m])]).astype(np.uint64)), what
        out[mode] = b
    return out


def _bare(ctx, oracle, case):
    """the same emit_bounds on the bare sorted cluster (strl_bounds_bare) against the oracle's bounds()"""
    t = case.treads[np.argsort(case.treads["position"], kind="stable")]
    row, good = ctx.bounds_bare(t["position"], t["split"], case.max_clip_dist)
    exp = oracle.bounds_of(t, 0, 0, case.max_clip_dist)
    for f in FIELDS[2:]:
        assert int(row[f]) == int(getattr(exp, f)), (case.name, f)
    assert good == (exp.right - exp.left <= 1000), case.name


# ---- a. CountTable growth and slot order on the device ------------------------------------------------------------------
@pytest.mark.parametrize("d", cc.TIE_D)
def test_clip_ties(ctx, oracle, d):
    case = cc.clip_ties(d)
    _run(ctx, oracle, case)
    _bare(ctx, oracle, case)


@pytest.mark.parametrize("variant", ["split", "single"])
@pytest.mark.parametrize("d", [12, 44])
def test_clip_ties_variants(ctx, oracle, d, variant):
    case = cc.clip_ties(d, variant)
    _run(ctx, oracle, case)
    _bare(ctx, oracle, case)


@pytest.mark.parametrize("base", [0, 399, 4_000_000_000])
def test_clip_ties_at_both_ends_of_the_position_range(ctx, oracle, base):
    for d in (12, 44, 343):
        case = cc.clip_ties(d, base=base)
        _run(ctx, oracle, case)
        _bare(ctx, oracle, case)


# ---- b. LDS / global views either side of BK_LIM ---------------------------------------------------------------------
@pytest.mark.parametrize("n,n_trimmed", cc.SIZES)
def test_sizes(ctx, oracle, n, n_trimmed):
    rows = _run(ctx, oracle, cc.sizes(n, n_trimmed), members=True)
    assert all(b["n_total"].tolist() == [n] * 3 for b in rows.values())


# ---- c. the 65535 gate --------------------------------------------------------------------------------------------
def test_gate(ctx, oracle):
    for n in cc.GATE_N:
        rows = _run(ctx, oracle, cc.gate(n))[api.MODE_CALL]
        assert len(rows) == {65534: 1, 65535: 0, 65536: 0, 70000: 2}[n]
    case = cc.gate(65534, api.MODE_MERGE)
    t0 = time.perf_counter()
    exp_b, _ = case.expect(oracle, api.MODE_MERGE)      # has_per_sample_reads of the oracle is quadratic: seconds on the CPU
    t1 = time.perf_counter()
    b, _, st = ctx.cluster(_api_treads(case.treads), api.MODE_MERGE, case.window, **case.kw())
    t2 = time.perf_counter()
    print(f"gate, merge mode, n = 65534: oracle {t1 - t0:.2f} s, device call {t2 - t1:.3f} s")
    _same_rows(b, exp_b, case.name)
    assert b["n_total"].tolist() == [65534] and (st.n_groups, st.n_clusters) == (1, 1)


# ---- d. the per-sample count table of merge mode --------------------------------------------------------------------
@pytest.mark.parametrize("stride", cc.SAMPLE_STRIDE)
@pytest.mark.parametrize("n", cc.SAMPLE_N)
def test_sample_table(ctx, oracle, n, stride):
    assert len(_run(ctx, oracle, cc.sample_table(n, stride))[api.MODE_MERGE]) == 1
    case = cc.sample_table(n, stride, doubled=True)
    assert len(_run(ctx, oracle, case)[api.MODE_MERGE]) == 1
    t = _api_treads(case.treads)
    t["qname_id"][n - 1] = n * stride + 7               # without the doubled id no sample has two reads
    assert len(ctx.cluster(t, api.MODE_MERGE, case.window, **case.kw())[0]) == 0
    assert len(case.expect(oracle, api.MODE_MERGE)[0]) == 1


def test_sample_ids_that_meet_in_32_bits_are_refused(ctx, oracle):
    """The per-sample table keeps 32 bits of qname_id.  Ids 5 and 2^32 + 5 are two samples to the oracle (no row at
    min_support 2); the device must say that it cannot tell them apart, not count them as one.  Call mode never reads the id."""
    case = cc.sample_table(16, 1)
    t = _api_treads(case.treads)
    t["qname_id"][0] = (1 << 32) + int(t["qname_id"][5])
    with pytest.raises(api.StrlingError, match="qname_id"):
        ctx.cluster(t, api.MODE_MERGE, case.window, min_support=2)
    _run(ctx, oracle, cc.sample_table(16, 1, doubled=True))
    ot = case.treads.copy()
    ot["qname_id"] = t["qname_id"]
    exp_b, exp_u = oracle.call_bounds(ot, api.MODE_CALL, case.window, min_support=2)
    b, u, _ = ctx.cluster(t, api.MODE_CALL, case.window, min_support=2)
    _same_rows(b, exp_b, "call mode with a wide qname_id")


# ---- e. seams of heads_kernel / gather_kernel -------------------------------------------------------------------------
@pytest.mark.parametrize("layout,n", cc.SEAM_LAYOUTS)
def test_seams(ctx, oracle, layout, n):
    case = cc.seams(layout, n)
    rows = _run(ctx, oracle, case, members=True)
    assert all(len(b) == case.meta["n_groups"] for b in rows.values())


# ---- f. <= against < in ends_kernel and bounds_filter_kernel ----------------------------------------------------------
@pytest.mark.parametrize("min_support", [1, 2, 3])
def test_gaps(ctx, oracle, min_support):
    case = cc.gaps(11, min_support)
    t = case.treads
    counts = {api.MODE_CALL: cc.count_groups_clusters(t, case.window), api.MODE_MERGE: cc.count_groups_clusters(t[t["tid"] >= 0], case.window)}
    _run(ctx, oracle, case, counts=counts)


# ---- g. tile_scan_kernel ----------------------------------------------------------------------------------------------
def test_many_tiles(ctx, oracle):
    t0 = time.perf_counter()
    case = cc.many_tiles()
    t1 = time.perf_counter()
    exp_b, exp_u = case.expect(oracle, api.MODE_CALL)
    t2 = time.perf_counter()
    b, u, st = ctx.cluster(_api_treads(case.treads), api.MODE_CALL, case.window, **case.kw())
    t3 = time.perf_counter()
    print(f"many_tiles, n = {case.treads.size}: build {t1 - t0:.2f} s, oracle {t2 - t1:.2f} s, device call with the copy of the input {t3 - t2:.2f} s")
    assert len(exp_b) > 100_000
    _same_rows(b, exp_b, case.name)
    _same_unplaced(u, exp_u, case.name)
    assert st.n_groups == case.meta["n_groups"] == np.unique(cc.group_keys(case.treads)).size


# ---- h. one composite sort or two -------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_tid", [131070, 131071])
def test_key_width(ctx, oracle, monkeypatch, max_tid):
    monkeypatch.delenv("STRL_CLUSTER_TWO_SORTS", raising=False)
    rows = _run(ctx, oracle, cc.key_width(max_tid))
    assert len(rows[api.MODE_MERGE]) > 100


# ---- i. the resident entry: folded positions, error flags -------------------------------------------------------------
def _resident(ctx, oracle, case, n_tid=None):
    ctx.set_treads(_api_treads(case.treads))
    b, u, st = ctx.cluster_resident(n_tid or case.meta["n_tid"], case.window, pos_bits=case.meta["pos_bits"], **case.kw())
    exp_b, exp_u = case.expect(oracle, api.MODE_CALL)
    _same_rows(b, exp_b, case.name)
    _same_unplaced(u, exp_u, case.name)
    assert st.n_treads == case.treads.size
    return b


@pytest.mark.parametrize("pos_bits", [22, 24])
def test_folded(ctx, oracle, pos_bits):
    b = _resident(ctx, oracle, cc.folded(pos_bits))
    assert (b["left"] >= (1 << 32) - 64).sum() >= 20


def _still_works(ctx, oracle):
    _run(ctx, oracle, cc.sizes(257, 1))
    _resident(ctx, oracle, cc.folded(22))


def test_error_flags_become_errors_and_the_context_goes_on(ctx, oracle):
    bad = cc.folded_bad(22)
    ctx.set_treads(_api_treads(bad.treads))
    with pytest.raises(api.StrlingError, match="position needs more than 22 bits"):
        ctx.cluster_resident(bad.meta["n_tid"], bad.window, pos_bits=22, **bad.kw())
    _still_works(ctx, oracle)
    for kind in ("letter", "gap"):
        case = cc.bad_unit(kind)
        for mode in case.modes:
            with pytest.raises(api.StrlingError, match="repeat unit is not a NUL-padded ACGT string"):
                ctx.cluster(_api_treads(case.treads), mode, case.window, **case.kw())
            _still_works(ctx, oracle)
    good = cc.folded(22)
    assert int(good.treads["tid"].max()) == 24
    ctx.set_treads(_api_treads(good.treads))
    with pytest.raises(api.StrlingError, match=r"tid is outside \[-1, 24\)"):
        ctx.cluster_resident(24, good.window, pos_bits=22, **good.kw())
    _still_works(ctx, oracle)
