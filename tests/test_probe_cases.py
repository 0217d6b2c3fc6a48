"""The premises of tests/probe_cases.py, on the CPU: its restatement of the Bloom layout equals the header's functions
(tests/emu/bloom_emu.cpp), its inverse of fmix64 is one, and every case is what it says -- the groups the oracle finds hot are the
designed ones, no cold key can pass a bitmap that holds the hot keys (so the expected item count is exact), the last read is hot,
and the `flush` case fills a wave's stage inside its loop under the one-block grid."""
import numpy as np
import pytest

import loop_cases as LC
import probe_cases as PC
from test_bloom_layout import _keys, _patterns, _words, emu  # noqa: F401  (emu: the fixture)


def test_layout_restated(emu):
    assert emu.bloom_emu_k() == PC.K and emu.bloom_emu_word_bits() == PC.WORD_BITS
    m = _keys(5, 50_000)
    for bits in (PC.SMALL_BITS, 1 << 24, 1 << 27):
        assert _words(emu, m, bits - 1).tolist() == [PC.word_of(int(x), bits) for x in m]
    assert _patterns(emu, m).tolist() == [PC.pattern_of(int(x)) for x in m]
    k = PC.key(1023, (0, 31, 32, 63), 12345)
    assert PC.word_of(k) == 1023 and PC.pattern_of(k) == (1 << 0) | (1 << 31) | (1 << 32) | (1 << 63)


def test_fmix64_inverse():
    assert PC.fmix64(1) == 0xb456bcfc34c2cb2c          # MurmurHash3's finalizer
    for m in [0, 1, PC.M64, 0x123456789abcdef0] + [int(x) for x in _keys_plain(6, 1000)]:
        assert PC.fmix64(PC.fmix64_inv(m)) == m and PC.fmix64_inv(PC.fmix64(m)) == m


def _keys_plain(seed, n):
    return np.random.Generator(np.random.Philox(key=[seed, 11])).integers(0, 1 << 64, n, dtype=np.uint64)


@pytest.mark.parametrize("name", PC.ALL)
def test_case_premises(name):
    c, e = PC.case(name), PC.expected(name)
    n = c.rec.n
    assert n <= 131072 and (name[0] != "n" or n == int(name[1:]))
    assert np.array_equal(e["probe_hit"], c.hot_design), "the oracle's hot groups are not the designed ones"
    assert c.hot_design[-1] and len(e["treads"]) > 0
    assert e["n_hot_soft"] > 0 or n < 20
    grp = LC.qname_groups(c.rec)
    m = [PC.fmix64(int(h)) for h in c.qhash]
    assert all(m[i] == m[j] for i, j in zip(range(n - 1), range(1, n)) if grp[i] == grp[j])
    assert len(set(m)) == grp.max() + 1
    bitmap = {}
    for i in np.flatnonzero(c.hot_design):
        bitmap[PC.word_of(m[i])] = bitmap.get(PC.word_of(m[i]), 0) | PC.pattern_of(m[i])
    for i in np.flatnonzero(~c.hot_design):
        p = PC.pattern_of(m[i])
        assert bitmap.get(PC.word_of(m[i]), 0) & p != p, "cold read %d would pass" % i


def test_layout_case_edges():
    c = PC.layout()
    what = [G.what for G in c.groups]
    short = [G for G in c.groups if "short" in G.what]
    hot_bits = {}
    for G in c.groups:
        if G.hot:
            hot_bits.setdefault(G.word, set()).update(G.fields)
    assert len(short) == 7
    for G in short:          # same word as a hot key, exactly one of its bits not set
        assert len(set(G.fields) - hot_bits[G.word]) == 1, G
    assert sum(1 for G in c.groups if G.hot and G.word == 7) == 2
    assert {0, PC.SMALL_WORDS - 1} <= set(hot_bits) and any(G.hot and len(set(G.fields)) == 1 for G in c.groups)
    assert any(G.hot and set(G.fields) == {0, 31, 32, 63} for G in c.groups)
    assert all(G.word not in hot_bits for G in c.groups if "disjoint" in G.what) and "lone" not in what


def test_flush_case_fills_the_stage_inside_the_loop():
    c = PC.flush()
    m = LC.Model()
    waves = m.iterations(c.rec.n, "P", PC.CONFIGS["one"])
    assert len(waves) == 4
    for its in waves:
        assert len(its) >= 4
        before_last = int(c.hot_design[its[0][0]:its[-1][0]].sum())
        assert before_last >= m.PR_STAGE, before_last
    # under the default grid no wave does: what differs between the two runs is the flush
    for its in m.iterations(c.rec.n, "P", None):
        assert int(c.hot_design[its[0][0]:its[-1][1]].sum()) < m.PR_STAGE


@pytest.mark.parametrize("n", PC.SIZES)
def test_sizes_reach_the_clamped_loads(n):
    """under both grids the wave that owns the last read has lanes past its end in its last turn (n is no multiple of 512), or ends
    exactly on a lane boundary (64): both sides of the clamp"""
    m = LC.Model()
    for cfg in (None, PC.CONFIGS["one"]):
        a, b = m.iterations(n, "P", cfg)[-1][-1]
        assert b == n and (b - a) % 512 != 0
