"""The rule of strl_assign_reads_loci_device (strling_amd/csrc/assign_core.h: given loci take their reads) on the CPU: the bodies
of its kernels are compiled for the host (tests/emu/assign_emu.cpp, a stand-alone program built with AddressSanitizer and UBSan,
64 threads and a barrier for a wave) and run over the edge tables and over drawn tables; what they give is compared with the
host function, api.assign_reads_loci.  CPU only."""
import os
import subprocess

import numpy as np
import pytest

from strling_amd import api
import assign_cases as AC

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "emu", "assign_emu.cpp")
CSRC = os.path.join(HERE, "..", "strling_amd", "csrc")
FLAGS = ["-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-pthread"]


@pytest.fixture(scope="module")
def emu():
    out = os.path.join(HERE, "emu", "assign_build")
    exe = os.path.join(out, "assign_emu")
    deps = [SRC, os.path.join(CSRC, "assign_core.h"), os.path.join(HERE, "..", "include", "strling_amd.h")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(d) for d in deps):
        os.makedirs(out, exist_ok=True)
        subprocess.check_call(["g++"] + FLAGS + ["-o", exe, SRC])
    return exe


def run_emu(emu, tmp_path, t, lo, mode, two_sorts=0):
    unit = lambda u: bytes(u).decode() or "-"
    lines = [f"{mode} {len(t)} {len(lo)} {two_sorts}"]
    lines += [f"{int(r['tid'])} {int(r['position'])} {int(r['split'])} {unit(r['repeat'])}" for r in t]
    lines += [f"{int(b['tid'])} {int(b['left_most'])} {int(b['right_most'])} {unit(b['repeat'])}" for b in lo["b"]]
    p = tmp_path / "case.txt"
    p.write_text("\n".join(lines) + "\n")
    r = subprocess.run([emu, str(p)], capture_output=True, text=True)
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
    assert r.returncode == 0, (r.returncode, r.stderr)
    out = r.stdout.splitlines()
    if out[0].startswith("err"):
        return int(out[0].split()[1]), None, None, None
    stat = tuple(int(x) for x in out[0].split()[1:])
    loci = []
    for ln in out[1:1 + len(lo)]:
        head, _, tail = ln.partition(":")
        w = head.split()
        loci.append((int(w[2]), int(w[3]), int(w[4]), [int(x) for x in tail.split()]))
    marks = [int(x) for x in out[1 + len(lo)].split()[1:]]
    return 0, stat, loci, marks


def check(emu, tmp_path, t, lo, mode, two_sorts=0):
    err, stat, loci, marks = run_emu(emu, tmp_path, t, lo, mode, two_sorts)
    assert err == 0
    wt, wl, wa = api.assign_reads_loci(t, lo, mode)
    for j, (tot, left, right, idx) in enumerate(loci):
        b = wl["b"][j]
        assert (tot & 0xFFFF, left & 0xFFFF, right & 0xFFFF) == (int(b["n_total"]), int(b["n_left"]), int(b["n_right"])), j
        assert idx == wa[j].tolist() and tot == len(idx), j
    want_marks = np.flatnonzero((wt["split"] == AC.TAKEN) & (t["split"] != AC.TAKEN)).tolist()
    assert marks == want_marks
    assert stat[1] == len(want_marks) - sum(len(x) for x in wa)      # what was lost
    return stat, loci, marks


@pytest.mark.parametrize("mode", [api.MODE_MERGE, api.MODE_CALL])
@pytest.mark.parametrize("name", sorted(AC.edge_tables()))
def test_edge_tables(emu, tmp_path, name, mode):
    rows, loci = AC.edge_tables()[name]
    check(emu, tmp_path, AC.treads_of(rows), AC.loci_of(loci), mode)


def test_edge_tables_say_what_their_names_say(emu, tmp_path):
    E = AC.edge_tables()
    run = lambda name, mode=api.MODE_CALL: check(emu, tmp_path, AC.treads_of(E[name][0]), AC.loci_of(E[name][1]), mode)
    stat, loci, marks = run("empty_range_loses_the_read_behind")
    assert loci[0][0] == 0 and marks == [1] and stat == (1, 1)
    stat, loci, marks = run("range_at_the_end_of_its_group")
    assert loci[0][3] == [2] and marks == [2] and stat == (1, 0)
    stat, loci, marks = run("right_most_below_left_most")
    assert [l[0] for l in loci] == [0, 0] and marks == [1, 2]        # the first loses 300, the second 200: both ranges are empty
    stat, loci, marks = run("equal_positions_keep_input_order")
    assert loci[0][3] == [9, 0, 1, 4, 5, 6, 7, 8] and marks == [0, 1, 3, 4, 5, 6, 7, 8, 9]     # 499, the 500s as they came; 600 is lost
    stat, loci, marks = run("the_same_locus_twice")
    assert [l[0] for l in loci] == [7, 0, 0] and stat == (1, 3)       # 104 .. 110, then 111, 112 and 113 are lost one by one
    a = run("overlapping_loci_a_b")[1]
    b = run("overlapping_loci_b_a")[1]
    assert sorted(a[0][3] + a[1][3]) != sorted(b[0][3] + b[1][3])     # the orders differ in what the pair receives
    stat, loci, marks = run("units_A_AA_AAAAAA_are_three_groups")
    assert stat[0] == 3 and loci[3][0] == 0
    stat, loci, marks = run("unplaced_treads", api.MODE_MERGE)
    assert loci[0][0] == 0 and loci[2][0] == 0 and loci[1][0] == 2
    stat, loci, marks = run("unplaced_treads", api.MODE_CALL)
    assert loci[0][0] == 2 and loci[2][0] == 1


@pytest.mark.parametrize("seed", range(12))
def test_drawn_tables(emu, tmp_path, seed):
    t, lo = AC.random_table(seed, n_max=600, loci_max=60)
    check(emu, tmp_path, t, lo, seed % 2, two_sorts=(seed // 2) % 2)


def test_widths_around_the_wave(emu, tmp_path):
    rows, loci = AC.widths_table([63, 64, 65, 129])
    check(emu, tmp_path, AC.treads_of(rows), AC.loci_of(loci), api.MODE_CALL)


def test_bad_treads_are_named(emu, tmp_path):
    lo = AC.loci_of([(0, 1, 10, b"AC")])
    assert run_emu(emu, tmp_path, AC.treads_of([(0, 5, 3, b"AC"), (0, 6, 3, b"AN")]), lo, 1)[0] == 1
    assert run_emu(emu, tmp_path, AC.treads_of([(0, 5, 3, b"AC"), (-2, 6, 3, b"AC")]), lo, 1)[0] == 2
    assert run_emu(emu, tmp_path, AC.treads_of([(0, 5, 255, b"AX")]), lo, 0)[0] == 1       # a taken one is checked too
