"""The case list of tests/sort_cases.py, checked on the CPU: the model of a sort pass equals numpy on every case, every named
mistake of the model is caught by a case this file names, every seam / loop / window case is what it claims (computed from
sort.h's constants), and the table region lies inside the scratch for every (n_max, bits, skew) of the list.  The kernels
themselves run in tests/test_sort_edges_device.py.  CPU only."""
import numpy as np
import pytest

import sort_cases as sc

T, CT, CHUNK = sc.T, sc.CT, sc.SORT_CHUNK


def _model_verdict(c, v=None):
    try:
        return sc.verdict(c, sc.model(c, v))
    except sc.ModelFault as f:
        return ["fault: %s" % f]


@pytest.mark.parametrize("name", sc.NAMES)
def test_model_equals_numpy(name):
    assert _model_verdict(sc.case(name)) == []


# the case that catches each mistake (any one would do; these are the narrowest)
CAUGHT_BY = {
    "cut_inclusive": "count_%d" % (T + 1),                  # `below` takes my own chunk's row: every digit starts too late
    "chunk_off_by_one": "count_%d" % CT,                    # tile CHUNK - 1 believes it opens the next chunk
    "full_mask": "window_5_9",                              # the 1-bit second pass reads 8 bits, the adversarial ones among them
    "pad_peers_zero": "ones_small",                         # padding lanes valued 0 and counted: every later digit base moves
    "no_clamp": "dn_%d_of_%d" % (sc.NMAX_A + 1, sc.NMAX_A),  # the decoy behind n_max is sorted to the front
    "lane_rank": "count_%d" % (T - 1),
    "not_zeroed": "scratch_pa5_s0_z0",
}


@pytest.mark.parametrize("variant", sorted(CAUGHT_BY))
def test_variant_is_caught(variant):
    assert variant in sc.VARIANTS
    bad = _model_verdict(sc.case(CAUGHT_BY[variant]), variant)
    print("%s: caught by %s: %s" % (variant, CAUGHT_BY[variant], bad[0] if bad else "NOT CAUGHT"))
    assert bad, "no failure under %s on %s: extend the case list" % (variant, CAUGHT_BY[variant])


def test_every_variant_is_accounted_for():
    assert sorted(list(CAUGHT_BY) + ["pad_peers"]) == sorted(sc.VARIANTS)     # pad_peers: see the test of that name below


def test_dirt_of_an_earlier_stage_is_caught_on_a_clean_scratch():
    """poison 0x00: what the second sort of a chain finds in its chunk tables is the first sort's tables, not the poison"""
    c = sc.case("chain_cluster_clean")
    assert c.poison == 0 and _model_verdict(c, "not_zeroed")


def test_padding_lanes_as_peers_cannot_change_a_result():
    """Counting the padding lanes of the last tile as peers -- in the histogram, in the match and in the counters -- is the one
    listed mistake NO input can show.  The padding lanes follow every real key of their tile, so they never precede a real lane
    in a peer group or in a wave; their key is ~0, whose digit is the largest of every pass, so what they add to a digit total
    moves no other digit's base; and their tile is the last, so no later tile sums its row.  The model agrees on every case,
    the real ~0 keys in a partly filled tile among them.  Only together with ANOTHER padding value can it be seen
    (pad_peers_zero above), which is why the kernel's ~0 matters and the `ones` cases stay."""
    for name in sc.NAMES:
        if name not in sc.BIG:
            assert _model_verdict(sc.case(name), "pad_peers") == [], name
    c = sc.case("ones_small")
    assert c.n_max % T and np.all(c.keys[:c.n_max] == np.uint64(sc.M64))


# ---- every case is what it claims ---------------------------------------------------------------------------------------------
def _unrolled(q, rows):
    """wave q of row_sums enters the loop that keeps 8 rows in flight when it has rows q, q + 4, .. q + 28 below `rows`"""
    return q + 28 < rows


def _tail_rows(q, rows):
    return len(range(q + 32 if _unrolled(q, rows) else q, rows, 4)) if rows > q else 0


def test_constants_are_the_ones_the_cases_were_written_for():
    assert sc.SHARE * sc.WAVES == T and T % sc.WAVE == 0 and CHUNK >= 32 and sc.WAVES == 4
    assert set(sc.COUNTS) >= {1, 63, 64, 65, sc.SHARE - 1, sc.SHARE, sc.SHARE + 1, T - 1, T, T + 1, CT - 1, CT, CT + 1}


def test_tile_row_loop_cases():
    """k tiles + 77 keys: the last tile sums k rows of its own chunk; wave q unrolls at CHUNK - 3 + q rows -- wave 3 never does,
    a chunk has no tile with CHUNK rows before it"""
    seen = {}
    for k in range(CHUNK - 3, CHUNK + 1):
        c = sc.case("count_%d" % (k * T + 77))
        nt = sc.div_up(c.n_max, T)
        assert nt == k + 1 and c.d_n == c.n_max
        rows = max(t % CHUNK for t in range(nt))         # most rows of its own chunk any tile sums
        seen[k] = [q for q in range(sc.WAVES) if _unrolled(q, rows)]
    assert seen == {CHUNK - 3: [0], CHUNK - 2: [0, 1], CHUNK - 1: [0, 1, 2], CHUNK: [0, 1, 2]}
    assert sc.div_up(CHUNK * T + 77, T) == CHUNK + 1       # the last of them opens a second chunk: one tile with no row before it


def test_chunk_row_loop_cases():
    shape = {}
    for nc in sc.NCHUNKS:
        c = sc.case("nchunks_%d" % nc)
        assert sc.tiles_chunks(c.n_max)[1] == nc and sc.tiles_chunks(min(c.d_n, c.n_max))[1] == nc
        assert 9 <= c.stages[0][1] <= 16
        shape[nc] = ([q for q in range(4) if _unrolled(q, nc)], [_tail_rows(q, nc) for q in range(4)])
    assert shape[CHUNK - 4] == ([], [7, 7, 7, 7])                      # no wave unrolled
    assert shape[CHUNK - 3] == ([0], [0, 7, 7, 7])                     # wave 0 only
    assert shape[CHUNK - 1] == ([0, 1, 2], [0, 0, 0, 7])
    assert shape[CHUNK] == ([0, 1, 2, 3], [0, 0, 0, 0])                # all four, empty tails
    assert shape[CHUNK + 1] == ([0, 1, 2, 3], [1, 0, 0, 0])            # unrolled plus a tail row


def test_count_cases_against_n_max():
    assert sorted(sc.case(n).d_n for n in sc.NAMES if n.startswith("dn_") and n.endswith("_of_%d" % sc.NMAX_A)) == \
        [0, 1, sc.NMAX_A - 1, sc.NMAX_A, sc.NMAX_A + 1, 2 ** 32 - 1]
    assert sc.NMAX_A == 2 * T + 77
    for n in sc.NAMES:
        c = sc.case(n) if n not in sc.BIG else None
        if c is not None and c.d_n > c.n_max:
            assert c.cap > c.n_max                          # decoys behind n_max: field 0, they would sort to the front
            lo, bits, _ = c.stages[0]
            assert not sc.field_of(c.keys[c.n_max:], lo, bits).any() and sc.field_of(c.keys[:c.n_max], lo, bits).any()
    c = sc.case("dn_%d_of_70000" % (T + 1))
    assert sc.tiles_chunks(c.n_max) == (sc.div_up(70000, T), 2) and sc.tiles_chunks(c.n_max)[0] > CHUNK
    assert sc.tiles_chunks(c.d_n) == (2, 1)                 # one full tile and one key; one chunk of the launch's two holds data


def test_window_cases():
    w = [sc.case("window_%d_%d" % x).stages[0][:2] for x in sc.WINDOWS]
    assert w == sc.WINDOWS == [(0, 0), (0, 1), (63, 1), (0, 7), (5, 9), (31, 2), (56, 8), (57, 7), (1, 63), (0, 64)]
    assert sc.passes(9) == 2 and 9 - 8 == 1                 # (5, 9): a second pass of one bit
    for lo, bits in sc.WINDOWS:
        c = sc.case("window_%d_%d" % (lo, bits))
        n = c.n_max
        f = sc.field_of(c.keys[:n], lo, bits)
        assert np.unique(f).size < max(n // 2, 2)                       # many ties
        # outside the window the keys hold the DESCENDING index, as far as the bits there go: above the window and below it
        desc = np.uint64(sc.M64) - np.arange(n, dtype=np.uint64)
        hi = lo + bits
        if lo:
            assert np.array_equal(c.keys[:n] & np.uint64((1 << lo) - 1), desc & np.uint64((1 << lo) - 1))
        if hi < 64:
            above = c.keys[:n] >> np.uint64(hi)
            assert np.array_equal(above, desc & np.uint64((1 << (64 - hi)) - 1))
            if (1 << (64 - hi)) > n:
                assert np.all(above[:-1] > above[1:])                      # sorting the whole key would reverse the input
        if bits:
            assert f.min() == 0 and int(f.max()) == (1 << bits) - 1


def test_digit_pattern_cases():
    for size, n in sc.SIZES.items():
        d = lambda p: sc.field_of(sc.case("%s_%s" % (p, size)).keys[:n], 3, 8)
        full = n // sc.WAVE * sc.WAVE
        rounds = lambda f: np.sort(f[:full].reshape(-1, sc.WAVE), axis=1)
        assert np.all(np.diff(rounds(d("distinct64")), axis=1) > 0)       # 64 distinct digits in every wave round
        r = rounds(d("onedigit"))
        assert np.all(r[:, 0] == r[:, -1]) and np.unique(r[:, 0]).size > 32  # one digit per round: lane 63 has 63 peers below it
        assert set(np.unique(d("digits0and255"))) == {0, 255}
        f = d("allbutfirst")
        assert f[0] > f[1] and np.all(f[1:] == f[1])
        f = d("allbutlast")
        assert f[-1] < f[0] and np.all(f[:-1] == f[0])
        f = d("seamrun")
        assert f[T - 1] == f[T] == 9 and (n <= CT or f[CT - 1] == f[CT] == 9)
        for p, v in (("zeros", 0), ("ones", sc.M64)):
            assert np.all(sc.case("%s_%s" % (p, size)).keys[:n] == np.uint64(v))
        assert n % T and n > 2 * T                                          # more than one block, a partly filled last tile
    assert sc.SIZES["seam"] > CT + T


def test_chains_compose_to_one_sort():
    for name in sc.NAMES:
        if name.startswith("chain_"):
            c = sc.case(name)
            lo, bits = c.meta["whole"]
            assert lo == min(s[0] for s in c.stages if s[1]) and lo + bits == max(s[0] + s[1] for s in c.stages)
            k, v, n = sc.reference(c)
            o = np.argsort(sc.field_of(c.keys[:n], lo, bits), kind="stable")
            assert np.array_equal(k, c.keys[:n][o]) and np.array_equal(v, c.vals[:n][o])
    p = [sc.passes(s[1]) for s in sc.case("chain_wide_narrow").stages]
    q = [sc.passes(s[1]) for s in sc.case("chain_narrow_wide").stages]
    assert p[0] > p[1] and q[0] < q[1]                      # the pass count changes: the second sort's tables overlay the first's


def test_scratch_cases():
    got = {(c.poison, c.skew, c.stages[0][2]) for c in (sc.case(n) for n in sc.NAMES if n.startswith("scratch_p"))}
    assert got == {(p, s, z) for p in (0x00, 0xA5, 0xFF) for s in (0, 4, 252) for z in (0, 1)}
    assert all(sc.case(n).delta == 0 for n in sc.NAMES if n != "scratch_short")
    c = sc.case("scratch_short")
    assert c.delta == -1 and c.meta["rc"] == [sc.HIP_INVALID] * len(c.stages) and {s[2] for s in c.stages} == {0, 1}


# ---- the table region, by calculation ----------------------------------------------------------------------------------------
def test_table_region_lies_inside_the_scratch():
    combos = {(n, b, s) for n in sc.LAYOUT_NMAX for b in sc.LAYOUT_BITS for s in range(256)}
    for name in sc.NAMES:
        c = sc.case(name) if name not in sc.BIG else None
        n_max = c.n_max if c else (int(name.split("_")[1]) - 1) * CT + T + 77
        stages, skew = (c.stages, c.skew) if c else ([(5, 12, 0)], 0)
        wide = max(s[1] for s in stages)
        for _, bits, _ in stages:
            combos.add((n_max, bits, skew))
            assert sc.scratch_bytes(n_max, bits) <= sc.scratch_bytes(n_max, wide)      # the widest stage sizes the chain's scratch
    for n_max, bits, skew in sorted(combos):
        off, size = sc.tables_region(skew, n_max, bits)
        if bits == 0:
            assert (off, size) == (-1, 0)
            continue
        have = sc.scratch_bytes(n_max, bits)
        nt, nc = sc.tiles_chunks(n_max)
        assert 0 <= off < 256 and (skew + off) % 256 == 0 and size == sc.passes(bits) * nc * 1024
        assert off + size <= sc.used_end(skew, n_max, bits) <= have, (n_max, bits, skew)
        assert sc.used_end(skew, n_max, bits) - (off + size) == sc.passes(bits) * nt * 1024
