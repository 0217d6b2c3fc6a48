"""The scorer's wave-uniform length bounds only skip work: one emulated lane (strling_amd/csrc/score_core.h compiled for the
host by tests/emu/score_bounds_emu.cpp) scored under every legal pair lo <= len <= hi <= 16 NW gives the oracle's words.
CPU only.  The lengths sit on the edges of what the bounds cut: the blocks of four windows of the k = 5, 6 counts (20 / 24
bases), the 16-base words of the recount, the 8-window batches of k <= 4 and the ends of the 160-base class."""
import ctypes as C
import os
import random
import subprocess

import pytest

from strling_amd.records import pack_seq4, unpack_result

HERE = os.path.dirname(os.path.abspath(__file__))
LENGTHS = [0, 1, 4, 5, 6, 19, 20, 21, 23, 24, 25, 29, 30, 31, 95, 96, 100, 149, 150, 151, 160]
P = 0.8


@pytest.fixture(scope="module")
def bemu():
    so = os.path.join(HERE, "emu", "libscore_bounds_emu.so")
    src = os.path.join(HERE, "emu", "score_bounds_emu.cpp")
    csrc = os.path.join(HERE, "..", "strling_amd", "csrc")
    deps = [src, os.path.join(csrc, "score_core.h"), os.path.join(csrc, "score_tables.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, src])
    L = C.CDLL(so)
    L.bemu_set_p.argtypes = [C.c_double]
    L.bemu_score.argtypes = [C.c_void_p] + [C.c_int] * 7 + [C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.bemu_score.restype = C.c_int
    L.bemu_set_p(P)
    return L


def _segment(rng, L):
    """the generator of test_emu_parity.py at a given length: random, k = 1..6 repeats at several purities and phases,
    two-unit mixes, not-ACGT bases"""
    kind = rng.random()
    if kind < 0.25:
        s = "".join(rng.choice("ACGT") for _ in range(L))
    elif kind < 0.8:
        k = rng.randint(1, 6)
        u = "".join(rng.choice("ACGT") for _ in range(k))
        pur = rng.choice([1.0, 0.98, 0.95, 0.9, 0.85, 0.7])
        ph = rng.randint(0, k)
        s = (u * (L // k + 3))[ph:ph + L]
        s = "".join(c if rng.random() < pur else rng.choice("ACGT") for c in s)
    elif kind < 0.9:
        k1, k2 = rng.randint(2, 6), rng.randint(2, 6)
        u1 = "".join(rng.choice("ACGT") for _ in range(k1))
        u2 = "".join(rng.choice("AC") for _ in range(k2))
        cut = rng.randint(0, L)
        s = ((u1 * 200)[:cut] + (u2 * 200))[:L]
    else:
        s = "".join(rng.choice("ACGTNNMR=") for _ in range(L))
    if rng.random() < 0.15 and L > 0:
        s = list(s)
        for _ in range(rng.randint(1, 25)):
            s[rng.randrange(L)] = rng.choice("NNNMRY")
        s = "".join(s)
    return s


def _his(L, cap):
    """len, len + 1, the next multiple of four windows of k = 5 and of k = 6 (and of a 16-base word), the class's length"""
    up = lambda m: (L + m - 1) // m * m
    return sorted({min(h, cap) for h in (L, L + 1, up(20), up(24), up(16), cap)})


def _words(bemu, seq4, s0, n, lo, hi, mode, klass, fused):
    o0, o1 = C.c_uint32(), C.c_uint32()
    assert bemu.bemu_score(seq4.ctypes.data, s0, n, lo, hi, mode, klass, fused, C.byref(o0), C.byref(o1)) == 0, (n, lo, hi)
    return unpack_result(o0.value)[:2], unpack_result(o1.value)[:2]


@pytest.mark.parametrize("L", LENGTHS)
def test_bounds_only_skip_work(bemu, oracle, L):
    rng = random.Random(7000 + L)
    n_runs = 0
    for _ in range(40):
        pre = rng.choice([0, 0, rng.randint(1, 40)])       # the bases of the read in front of the clipped end
        s = _segment(rng, pre + L)
        seg = s[pre:]
        seq4, _, _ = pack_seq4([s])
        exp_soft = (oracle.get_repeat(seg, P - 0.07), oracle.get_repeat(seg, min(P, 0.6)))
        exp_whole = oracle.get_repeat(seg, P)
        for hi in _his(L, 160):
            for lo in (0, L):
                for fused in (0, 1):      # the fused soft-clip launch, and stage A -> hand-over -> stage B
                    assert _words(bemu, seq4, pre, L, lo, hi, 1, 0, fused) == exp_soft, (seg, lo, hi, fused)
                    n_runs += 1
                if pre == 0:              # a whole read: converted straight from the loaded words, threshold row of -p
                    w = _words(bemu, seq4, 0, L, lo, hi, 0, 0, 0)
                    assert w == (exp_whole, exp_whole), (seg, lo, hi)
                    n_runs += 1
    assert n_runs >= 40 * len(_his(L, 160)) * 2 * 2


@pytest.mark.parametrize("klass,cap", [(1, 256), (2, 512)])
def test_long_classes_unchanged(bemu, oracle, klass, cap):
    """NW = 16 and 32 count k = 5, 6 through their hash path; the recount's bound is the only thing they share with the change"""
    rng = random.Random(klass)
    for L in [0, 1, 15, 16, 17, 100, 160, 161, 250, 255, 256] + ([257, 300, 500, 510] if klass == 2 else []):
        for _ in range(6):
            s = _segment(rng, L)
            seq4, _, _ = pack_seq4([s])
            exp = (oracle.get_repeat(s, P - 0.07), oracle.get_repeat(s, min(P, 0.6)))
            for hi in _his(L, cap):
                for lo in (0, L):
                    assert _words(bemu, seq4, 0, L, lo, hi, 1, klass, 0) == exp, (s, lo, hi)


def test_illegal_bounds_are_refused(bemu):
    seq4, _, _ = pack_seq4(["ACGT" * 10])
    o = C.c_uint32()
    for lo, hi in ((41, 160), (0, 39), (0, 161), (-1, 160)):
        assert bemu.bemu_score(seq4.ctypes.data, 0, 40, lo, hi, 1, 0, 1, C.byref(o), C.byref(o)) == -1
