"""Every builder of tests/cluster_cases.py reaches the edge it is named for -- shown with the oracle alone, on any machine.
tests/test_cluster_device.py feeds the same cases to the kernels; a case that silently stopped exercising its edge would
leave that file green and meaningless, so it fails here instead."""
import ctypes as C

import numpy as np
import pytest

import cluster_cases as cc


def _largest(oracle, keys):
    """CountTable[uint32].largest of the oracle -> (key, count, distinct keys)"""
    keys = np.ascontiguousarray(keys, np.uint32)
    k, v, nd = C.c_uint32(0), C.c_int64(0), C.c_int64(0)
    oracle.lib().orc_counttable_largest(keys.ctypes.data, keys.size, 8, C.byref(k), C.byref(v), C.byref(nd))
    return k.value, v.value, nd.value


def _clips(case, kind):
    t = case.treads
    return np.sort(t["position"][t["split"] == kind])


@pytest.fixture(scope="module")
def tie_rows(oracle):
    out = {}
    for d in cc.TIE_D:
        c = cc.clip_ties(d)
        b, _ = c.expect(oracle, cc.MODE_CALL)
        out[d] = (c, b)
    return out


@pytest.mark.parametrize("d", cc.TIE_D[1:])
def test_clip_ties_are_ties_and_the_table_picks_the_row(oracle, tie_rows, d):
    c, b = tie_rows[d]
    assert len(b) == 1 and int(b["n_total"][0]) == 4 * d + 10       # the whole cluster, unsplit
    for kind, field in ((cc.RIGHT, "left"), (cc.LEFT, "right")):     # (left > right after bounds(): the two are swapped)
        keys = _clips(c, kind)
        key, val, distinct = _largest(oracle, keys)
        assert distinct == d and val == 2 and (np.unique(keys, return_counts=True)[1] == val).all()   # d keys tied at the maximum
        assert int(b[field][0]) == key
    assert int(b["n_left"][0]) == int(b["n_right"][0]) == 2 * d      # max_clip_dist filtered nothing
    assert int(b["right"][0]) - int(b["left"][0]) <= 1000


def test_clip_ties_choice_moves_at_every_growth_step_and_only_there(tie_rows):
    off = {d: (int(b["left"][0]) - c.meta["base"], int(b["right"][0]) - c.meta["base"] - 400) for d, (c, b) in tie_rows.items() if d >= 4}
    for a, b, c in cc.TIE_STEPS:
        assert off[a] == off[b], (a, b, off[a], off[b])
        assert off[b][0] != off[c][0] and off[b][1] != off[c][1], (b, c, off[b], off[c])
    inner = sum(all(0 < o < d - 1 for o in lr) for d, lr in off.items())
    assert 2 * inner >= len(off)                                     # neither the smallest nor the largest tied key, in at least half


def test_clip_ties_two_keys_split_the_cluster(oracle, tie_rows):
    """d = 2: each modal position holds 2 / 2 of the distinct count, above one half"""
    assert len(tie_rows[2][1]) == 2


@pytest.mark.parametrize("d", [12, 44])
def test_clip_ties_variants(oracle, d):
    c = cc.clip_ties(d, "split")
    b, _ = c.expect(oracle, cc.MODE_CALL)
    assert len(b) == 2 and int(b["n_total"].sum()) == c.treads.size
    for kind in (cc.RIGHT, cc.LEFT):
        key, val, distinct = _largest(oracle, _clips(c, kind))
        assert val == d + 1 and 2 * val > distinct
    c = cc.clip_ties(d, "single")
    b, _ = c.expect(oracle, cc.MODE_CALL)
    assert len(b) == 1 and int(b["left"][0]) == int(b["center_mass"][0]) and int(b["right"][0]) == int(b["left"][0]) + 1
    assert _largest(oracle, _clips(c, cc.LEFT))[1] == 1


@pytest.mark.parametrize("base", [0, 399, 4_000_000_000])
def test_clip_ties_at_both_ends_of_the_position_range(oracle, base):
    for d in (12, 44, 343):
        c = cc.clip_ties(d, base=base)
        b, _ = c.expect(oracle, cc.MODE_CALL)
        assert len(b) == 1 and int(b["n_total"][0]) == 4 * d + 10
        assert base <= int(b["left"][0]) < base + d and base + 400 <= int(b["right"][0]) < base + 400 + d


@pytest.mark.parametrize("n,n_trimmed", cc.SIZES)
def test_sizes_after_the_trim(oracle, n, n_trimmed):
    c = cc.sizes(n, n_trimmed)
    for mode in c.modes:
        b, _ = c.expect(oracle, mode)
        assert b["n_total"].tolist() == [n] * 3
        assert c.treads.size - int(b["n_total"].sum()) == 3 * n_trimmed      # what the trim removed
    assert cc.count_groups_clusters(c.treads, c.window) == (2, 3)            # the trimmed read was part of its cluster
    for kind in (cc.LEFT, cc.RIGHT):
        assert np.unique(_clips(c, kind)).size >= 3 * 30
    assert {s[0] for s in cc.SIZES} >= {255, 256, 257, 300, 1000, 5000} and (256, 1) in cc.SIZES   # 257 reads before the trim, 256 after


def test_gate(oracle):
    rows = {n: cc.gate(n).expect(oracle, cc.MODE_CALL)[0] for n in cc.GATE_N}
    assert rows[65534]["n_total"].tolist() == [65534]
    assert len(rows[65535]) == 0 and len(rows[65536]) == 0
    assert len(rows[70000]) == 2 and int(rows[70000]["n_total"].astype(np.int64).sum()) == 70000
    assert all(cc.count_groups_clusters(cc.gate(n).treads, cc.WINDOW) == (1, 1) for n in (65534, 70000))


@pytest.mark.parametrize("n", cc.SAMPLE_N)
@pytest.mark.parametrize("stride", cc.SAMPLE_STRIDE)
def test_sample_table(oracle, n, stride):
    c = cc.sample_table(n, stride)
    assert np.unique(c.treads["qname_id"]).size == n
    assert c.expect(oracle, cc.MODE_MERGE)[0]["n_total"].tolist() == [n]
    tl = 16
    while tl < 2 * n:
        tl <<= 1
    if stride == 4096:      # the device table's hash, (id * 0x9E3779B1) mod table size: every id in slot 0
        assert not ((c.treads["qname_id"].astype(np.uint64) * np.uint64(0x9E3779B1)) & np.uint64(tl - 1)).any()
    c = cc.sample_table(n, stride, doubled=True)
    assert c.min_support == 2 and c.expect(oracle, cc.MODE_MERGE)[0]["n_total"].tolist() == [n]
    t = c.treads.copy()
    t["qname_id"][n - 1] = n * stride + 7    # the doubled id removed
    assert len(oracle.call_bounds(t, cc.MODE_MERGE, c.window, **c.kw())[0]) == 0


@pytest.mark.parametrize("layout,n", cc.SEAM_LAYOUTS)
def test_seams(oracle, layout, n):
    c = cc.seams(layout, n)
    order, gkey = cc.sort_key_order(c.treads)
    heads = np.concatenate([[0], np.nonzero(np.diff(gkey[order]))[0] + 1])
    assert heads.tolist() == c.meta["heads"].tolist()
    if layout == "heads":
        assert set(cc.SEAM_HEADS + [c.treads.size - 1]) <= set(heads.tolist())
    if layout == "big":
        assert np.diff(np.append(heads, c.treads.size)).max() == n > 2 * 2048
    for mode in c.modes:
        b, _ = c.expect(oracle, mode)
        assert len(b) == len(heads) == c.meta["n_groups"]                    # one row per group
        if len(b) > 1:
            assert b["tid"].tolist() != sorted(b["tid"].tolist())            # and not in key order


def test_gaps(oracle):
    t = cc.gaps(11, 3).treads
    assert 7000 < t.size < 9500
    assert len(cc.gaps(11, 3).expect(oracle, cc.MODE_CALL)[0]) > 1000
    b1, u1 = cc.gaps(11, 1).expect(oracle, cc.MODE_CALL)
    assert len(b1) > 2000 and len(u1) > 3
    order, gkey = cc.sort_key_order(t)
    pos, gk = t["position"][order].astype(np.int64), gkey[order]
    gap = np.diff(pos)[(np.diff(gk) == 0) & (gk[1:] >> 15 != 0)]
    for g in (cc.WINDOW + 99, cc.WINDOW + 100, cc.WINDOW + 101):
        assert (gap == g).sum() > 300
    assert (t["position"] < cc.WINDOW).sum() > 20          # medians below max_dist: left_most = median - max_dist wraps


def test_many_tiles_shape():
    assert cc.MANY_TILES_N == 4096 * 2048 + 1      # GT_TILE = 2048; the scan runs above 4096 tiles


@pytest.mark.parametrize("max_tid", [131070, 131071])
def test_key_width(oracle, max_tid):
    c = cc.key_width(max_tid)
    assert int(c.treads["tid"].max()) == max_tid and int(c.treads["position"].max()) >= 1 << 31
    assert (max_tid + 1).bit_length() + 15 + 32 == (64 if max_tid == 131070 else 65)
    assert len(c.expect(oracle, cc.MODE_MERGE)[0]) > 100


@pytest.mark.parametrize("pos_bits", [22, 24])
def test_folded(oracle, pos_bits):
    c = cc.folded(pos_bits)
    p = c.treads["position"].astype(np.int64)
    half = 1 << (pos_bits - 1)
    assert ((p < half) | (p >= (1 << 32) - half)).all() and {0, half - 1, (1 << 32) - half, (1 << 32) - 1} <= set(p.tolist())
    b, _ = c.expect(oracle, cc.MODE_CALL)
    assert len(b) > 200 and (b["left"] >= (1 << 32) - 64).sum() >= 20       # rows of wrapped reads: the last of their groups
    p = cc.folded_bad(pos_bits).treads["position"].astype(np.int64)
    assert ((p >= half) & (p < (1 << 32) - half)).sum() == 1
