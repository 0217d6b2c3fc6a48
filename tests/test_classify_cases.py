"""The turn arithmetic of classify_kernel on the CPU.  tests/emu/classify_emu.cpp compiles, with plain g++, the functions of
strling_amd/csrc/classify_turn.h that the kernel compiles, and walks every wave's loop in the kernel's order.  Held against the
launch-arithmetic model of tests/loop_cases.py (which reads the kernel's own text): every read is handled exactly once, the turns
are the model's, a turn is full exactly when it and the next one are whole, and nothing a full turn loads (its prefetch included)
or stores lies outside its wave's range.  Then: every device case of tests/classify_cases.py reaches the edge it is named for.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import classify_cases as CC
import loop_cases as LC

HERE = os.path.dirname(os.path.abspath(__file__))
CFGS = {"default": None, "one": CC.CONFIGS["one"], "two": CC.CONFIGS["two"]}       # up to 4096 waves, 4 and 8
N_MAX = 8200


@pytest.fixture(scope="module")
def emu():
    so = os.path.join(HERE, "emu", "libclassify_emu.so")
    src = os.path.join(HERE, "emu", "classify_emu.cpp")
    hdr = os.path.join(HERE, "..", "strling_amd", "csrc", "classify_turn.h")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, src])
    lib = C.CDLL(so)
    lib.classify_emu_turn.restype = C.c_uint32
    lib.classify_emu_ilp.restype = C.c_uint32
    lib.classify_emu_range.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p]
    lib.classify_emu_full.argtypes = [C.c_uint32, C.c_uint32]
    lib.classify_emu_read_offs.argtypes = [C.c_uint32, C.c_void_p]
    lib.classify_emu_walk.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, C.c_void_p, C.c_long, C.c_void_p, C.c_void_p]
    lib.classify_emu_walk.restype = C.c_long
    return lib


@pytest.fixture(scope="module")
def model():
    return LC.Model()


def _launch(m, n, cfg):
    """(waves of the launch, reads per wave) as the host and the kernel's own lines compute them"""
    env = m._env(cfg, "STRL_GRID_C")
    waves = 4 * min(-(-n // m.cl_reads_per_block), env if env > 0 else m.cl_max_blocks)
    return waves, -(-(-(-n // waves)) // m.cl_round) * m.cl_round


def _walk(emu, n, per, waves, vec):
    cap = waves + n // 512 + 8
    turns = np.zeros((cap, 4), np.uint64)
    handled = np.zeros(n, np.uint32)
    acc = np.zeros(6, np.uint64)
    nt = emu.classify_emu_walk(n, per, waves, int(vec), turns.ctypes.data, cap, handled.ctypes.data, acc.ctypes.data)
    assert 0 < nt <= cap
    return turns[:nt].astype(np.int64), handled, acc.astype(np.int64)


def test_constants(emu, model):
    assert emu.classify_emu_ilp() == model.CL_ILP and emu.classify_emu_turn() == 64 * model.CL_ILP
    assert model.cl_round == 256          # a share is a multiple of 256 reads: a column's 16-byte vectors stay aligned from r0 on


@pytest.mark.parametrize("cfg", list(CFGS))
def test_walk_against_the_model(emu, model, cfg):
    """n = 1 .. 8200: the emulation's turns are the model's, every read once, full <=> this turn and the next are whole, bounds"""
    step = 64 * model.CL_ILP
    n_full = 0
    for n in range(1, N_MAX + 1):
        waves, per = _launch(model, n, CFGS[cfg])
        its = model.iterations(n, "C", CFGS[cfg])
        exp = np.array([(w, a, b, int(b - a == step and k + 1 < len(t) and t[k + 1][1] - t[k + 1][0] == step))
                        for w, t in enumerate(its) for k, (a, b) in enumerate(t)], np.int64)
        for vec in (True, False):
            turns, handled, acc = _walk(emu, n, per, waves, vec)
            assert int(handled.min()) == 1 and int(handled.max()) == 1, (n, cfg, vec)
            assert np.array_equal(turns[:, :3], exp[:, :3]), (n, cfg, vec)
            assert acc[3] == 0 and acc[4] == 0, (n, cfg, vec, acc)           # nothing unmasked outside the range, no stale register set
            assert acc[5] == waves - len(its), (n, cfg)                       # the waves without a read return before their first load
            if vec:
                assert np.array_equal(turns[:, 3], exp[:, 3]), (n, cfg)
                assert acc[0] <= n and acc[1] <= n and acc[2] == int(exp[:, 3].sum()), (n, cfg, acc)
                n_full += int(acc[2])
            else:
                assert acc[2] == 0 and not turns[:, 3].any(), (n, cfg)        # the scalar variant has no full turn
        # the range of every wave, the ones that own nothing included
        for gw in (0, len(its) - 1, len(its), waves - 1):
            r = np.zeros(4, np.uint64)
            emu.classify_emu_range(n, per, gw, r.ctypes.data)
            if gw < len(its):
                assert (int(r[0]), int(r[1]), int(r[2])) == (its[gw][0][0], its[gw][-1][1], 1), (n, cfg, gw)
            else:
                assert int(r[2]) == 0 and int(r[3]) == 0, (n, cfg, gw)
    # the sweep met full turns under the small grids; under the default grid a wave owns at most 256 of so few reads
    assert (n_full > 0) == (cfg != "default")


def test_read_offsets_are_the_models_order(emu, model):
    for off in (0, 512, 7680):
        got = np.zeros(64 * model.CL_ILP, np.uint32)
        emu.classify_emu_read_offs(off, got.ctypes.data)
        assert np.array_equal(got.astype(np.int64), model.iteration_order(off, off + 64 * model.CL_ILP, True))
    assert emu.classify_emu_full(0, 1024) == 1 and emu.classify_emu_full(0, 1023) == 0 and emu.classify_emu_full(512, 1535) == 0
    assert emu.classify_emu_full(512, 1536) == 1


def test_large_batch_the_benchmarks_partition(emu, model):
    """2^25 reads under the default grid: 4096 waves of 16 turns, all but the last full; the prefetch of the last full turn ends at r1"""
    n = 1 << 25
    waves, per = _launch(model, n, None)
    assert (waves, per) == (4096, 8192)
    turns, handled, acc = _walk(emu, n, per, waves, True)
    assert int(handled.min()) == 1 and int(handled.max()) == 1
    assert acc[2] == 4096 * 15 and acc[0] == n and acc[1] == n - 512 and acc[3] == 0 and acc[4] == 0 and acc[5] == 0


# ---- the device cases reach their edges (under STRL_GRID_C=1, the partition they are built for) ----------------------------
def _kinds_of_turns(n, cfg="one"):
    return [t[4] for t in CC.turn_kinds(n, CFGS[cfg])]


def test_shapes_reach_their_turns(model):
    one = {n: CC.turn_kinds(n, CFGS["one"]) for n in list(CC.SHAPES_TURNS) + list(CC.SHAPES_SMALL)}
    per_wave = lambda n: [[t[4] for t in one[n] if t[0] == w] for w in range(4)]
    assert per_wave(4096) == [["full", "seam"]] * 4
    assert max(t[3] for t in one[4096] if t[0] == 0 and t[4] == "full") + 512 == 1024          # the prefetch ends exactly at r1
    assert per_wave(4095)[:3] == [["full", "seam"]] * 3 and per_wave(4095)[3] == ["general", "general"] and 4095 % 4 != 0
    assert per_wave(4097)[:3] == [["full", "seam", "behind"]] * 3 and per_wave(4097)[3] == ["general"]
    assert [t[3] - t[2] for t in one[4097] if t[0] == 3] == [257]
    assert [t[3] - t[2] for t in one[4097] if t[0] == 0] == [512, 512, 256]
    assert per_wave(6144) == [["full", "full", "seam"]] * 4
    assert per_wave(7168) == [["full", "full", "seam", "behind"]] * 4 and [t[3] - t[2] for t in one[7168] if t[0] == 0][-1] == 256
    assert per_wave(8192) == [["full", "full", "full", "seam"]] * 4
    assert [len(model.wave_ranges(n, "C", CFGS["one"])) for n in (1, 3, 255, 256, 257, 1021)] == [1, 1, 1, 1, 2, 4]
    for n in CC.SHAPES_SMALL:
        assert set(_kinds_of_turns(n)) == {"general"}
    # eight waves and the default grid: other turns are full, or none
    assert "full" in _kinds_of_turns(8192, "two") and "full" not in _kinds_of_turns(4096, "two")
    assert "full" not in _kinds_of_turns(8192, "default")


FEATURE = {      # kind of records -> what a row of Model.classify_trace shows where the edge is met
    "reload": lambda r: r["window"] == "loaded" and r["turn"] > 0 and not r["fallback"],
    "contig": lambda r: r["contig_changed"] and r["uniform"],
    "dense": lambda r: r["fallback"] and r["uniform"] and r.get("starts_in_span", 0) > 8,
    "backwards": lambda r: r.get("below", False) and r["window"] == "loaded",
    "keep_all": lambda r: r["flushed"] and r["cnt_after"] >= 512,
    "keep_none": lambda r: r["any"] and r["cnt_after"] == 0,
}


@pytest.mark.parametrize("kind", CC.KINDS)
def test_kinds_reach_full_turns_the_seam_and_the_turn_behind(model, kind):
    """each kind of records meets its edge INSIDE a full turn, on the first general turn behind one, and in the turn behind that
    (shapes 4097 and 7168 have one); two full turns in a row both meet it (6144, 8192)"""
    reached = {}
    for n in CC.SHAPES_TURNS:
        c = CC.case(kind, n)
        e = CC.expected(c.name)
        kinds = {(t[0], t[1]): t[4] for t in CC.turn_kinds(n, CFGS["one"])}
        rows = model.classify_trace(c, CFGS["one"], ~e["skipped"])
        hit = [kinds[(r["wave"], r["turn"])] for r in rows if FEATURE[kind](r)]
        reached[n] = {k: hit.count(k) for k in ("full", "seam", "behind", "general")}
        full_rows = [r for r in rows if kinds[(r["wave"], r["turn"])] == "full"]
        if kind in ("dense", "keep_all", "keep_none"):
            # in every turn of every wave (keep_all: every whole turn; a ragged one stages fewer than CL_STAGE reads)
            assert all(FEATURE[kind](r) for r in rows if kind != "keep_all" or r["end"] - r["base"] == 512), (kind, n)
        elif kind in ("reload", "contig", "backwards") and n in (6144, 7168, 8192):
            assert all(FEATURE[kind](r) for r in full_rows if r["turn"] > 0), (kind, n)   # in every full turn but a wave's first
        assert reached[n]["seam"] >= 3, (kind, n, reached[n])
    assert all(reached[n]["full"] >= 4 for n in (6144, 7168, 8192)), reached
    # (the turn behind the seam is half a turn in both shapes: now and then the seam's window still holds it)
    # keep_all: that half turn stages 256 reads, which the flush behind the loop writes
    assert kind == "keep_all" or (reached[4097]["behind"] >= 1 and reached[7168]["behind"] >= 1), reached
    if kind in ("dense", "keep_all", "keep_none"):
        assert all(reached[n]["full"] >= 3 for n in CC.SHAPES_TURNS), reached


def test_a_kept_reads_word_is_never_zero():
    """what lets `whole` and n_scored stand for the queued ids (tests/classify_cases.py), and: every kind keeps and skips as named"""
    for name in CC.ALL:
        c, e = CC.by_name(name), CC.expected(name)
        kept = ~e["skipped"]
        assert (e["whole"][kept] != 0).all(), name
        if c.kind == "keep_all":
            assert kept.all(), name
        elif c.kind == "keep_none":
            assert not kept.any(), name
        elif c.n >= 4095:
            assert 0 < int(kept.sum()) < c.n, name
