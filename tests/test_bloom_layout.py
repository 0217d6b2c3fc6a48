"""The Bloom bitmap's layout (strling_amd/csrc/bloom_layout.h) on the CPU: tests/emu/bloom_emu.cpp compiles, with plain g++, the
very index functions bloom_set and pair_probe_kernel compile.  Checked: a key's word lies inside the bitmap at its smallest and
largest size, its pattern has between 1 and k bits, and at the benchmark's load fewer unmarked keys pass than under the layout
before (two bits anywhere in the bitmap, restated here)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def emu():
    so = os.path.join(HERE, "emu", "libbloom_emu.so")
    src = os.path.join(HERE, "emu", "bloom_emu.cpp")
    hdr = os.path.join(HERE, "..", "strling_amd", "csrc", "bloom_layout.h")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, src])
    L = C.CDLL(so)
    L.bloom_emu_words.argtypes = [C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p]
    L.bloom_emu_patterns.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p]
    return L


def _words(L, m, mask):
    m = np.ascontiguousarray(m, np.uint64)
    out = np.zeros(m.size, np.uint32)
    L.bloom_emu_words(m.ctypes.data, m.size, mask, out.ctypes.data)
    return out


def _patterns(L, m):
    m = np.ascontiguousarray(m, np.uint64)
    out = np.zeros(m.size, np.uint64)
    L.bloom_emu_patterns(m.ctypes.data, m.size, out.ctypes.data)
    return out


def _popcount(x):
    return np.unpackbits(np.ascontiguousarray(x, np.uint64).view(np.uint8)).reshape(x.size, 64).sum(axis=1)


def _keys(seed, n):
    return np.random.Generator(np.random.Philox(key=[seed, 11])).integers(0, 1 << 64, n, dtype=np.uint64)


@pytest.mark.parametrize("log2_bits", [16, 27])
def test_word_inside_the_bitmap_and_pattern_bits(emu, log2_bits):
    k, wbits = emu.bloom_emu_k(), emu.bloom_emu_word_bits()
    assert wbits == 64 and 1 <= k <= 8
    mask = (1 << log2_bits) - 1
    n_words = (1 << log2_bits) // wbits
    edge = np.array([0, ~0 & (2 ** 64 - 1), mask, mask + 1, (1 << 32) - 1, 1 << 32, 0xffffffff00000000, 0x00ffffff00000000,
                     0x0000003f00000000 | mask], np.uint64)
    m = np.concatenate([edge, _keys(1, 200_000)])
    w = _words(emu, m, mask)
    assert int(w.max()) < n_words
    # every word is reached by a key of the low bits alone: the first and the last included
    assert set(_words(emu, np.arange(n_words, dtype=np.uint64), mask).tolist()) == set(range(n_words))
    pc = _popcount(_patterns(emu, m))
    assert int(pc.min()) >= 1 and int(pc.max()) <= k
    assert int(_popcount(_patterns(emu, edge[:1]))[0]) == 1            # all fields equal: one bit
    assert int(pc[len(edge):].max()) == k                                 # random keys reach k distinct bits
    # the pattern depends on the high half only, the word on the low half only
    assert np.array_equal(_patterns(emu, m), _patterns(emu, m & np.uint64(0xffffffff00000000)))
    assert np.array_equal(w, _words(emu, m & np.uint64(0xffffffff), mask))


def test_fewer_false_positives_than_two_bits_anywhere(emu):
    """1.2e6 marked keys in 2^24 bits (the benchmark's bitmap at about its load), 4e6 probes of unmarked keys, seeded"""
    bits = 1 << 24
    mask = bits - 1
    marked, probes = _keys(2, 1_200_000), _keys(3, 4_000_000)
    # this layout, through the header's functions
    bm = np.zeros(bits // 64, np.uint64)
    np.bitwise_or.at(bm, _words(emu, marked, mask), _patterns(emu, marked))
    pat = _patterns(emu, probes)
    fp_new = float(((bm[_words(emu, probes, mask)] & pat) == pat).mean())
    # the layout before: bit (low half & mask) and bit (high half & mask)
    old = np.zeros(bits, bool)
    b0 = lambda m: (m & np.uint64(0xffffffff)).astype(np.int64) & mask
    b1 = lambda m: (m >> np.uint64(32)).astype(np.int64) & mask
    old[b0(marked)] = True
    old[b1(marked)] = True
    fp_old = float((old[b0(probes)] & old[b1(probes)]).mean())
    # no false negative in either restatement
    mp = _patterns(emu, marked[:1000])
    assert bool(((bm[_words(emu, marked[:1000], mask)] & mp) == mp).all())
    print("false positives at 1.2e6 keys in 2^24 bits: this layout %.4f %%, two bits anywhere %.4f %%" % (100 * fp_new, 100 * fp_old))
    assert 0 < fp_new < fp_old
