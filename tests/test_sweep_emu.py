"""The rule of `call --sweep` (strling_amd/csrc/sweep_core.h: which records of a chunk answer which bound, and which bounds fall
on a seam) on the CPU: the bodies of the keys, tiles and ranges kernels are compiled for the host (tests/emu/sweep_emu.cpp, a
stand-alone program built with AddressSanitizer and UBSan, threads and a barrier for a workgroup) and run over record tables
drawn here, cut into chunks; what they decide is compared with a restatement of the rule in a few lines of Python.  CPU only."""
import os
import random
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "emu", "sweep_emu.cpp")
CSRC = os.path.join(HERE, "..", "strling_amd", "csrc")
FLAGS = ["-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-pthread"]
REF_OPS = (0, 2, 3, 7, 8)          # CIGAR operations that consume the reference: M D N = X


@pytest.fixture(scope="module")
def emu():
    out = os.path.join(HERE, "emu", "sweep_build")
    exe = os.path.join(out, "sweep_emu")
    deps = [SRC, os.path.join(CSRC, "sweep_core.h"), os.path.join(CSRC, "bam_rec.h")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(d) for d in deps):
        os.makedirs(out, exist_ok=True)
        subprocess.check_call(["g++"] + FLAGS + ["-o", exe, SRC])
    return exe


def rec_end(r):
    tid, pos, flag, cig = r
    rl = 0 if flag & 4 else sum(n for n, op in cig if op in REF_OPS)
    return pos + (rl or 1)


def rule(chunks, bounds):
    """the rule as the issue states it: {bound: (chunk, i0, i1, status)} and the carry that leaves every chunk"""
    carry, res, carries = None, {}, []
    for k, recs in enumerate(chunks):
        pm, run = [], carry                                  # running maximum of end within a reference, seeded with the carry
        for r in recs:
            run = (r[0], max(rec_end(r), run[1]) if run and run[0] == r[0] else rec_end(r))
            pm.append(run[1])
        for j, (t, beg, end) in enumerate(bounds):
            if j in res:
                continue
            i1 = next((i for i, r in enumerate(recs) if (r[0] & 0xffffffff) > t or (r[0] == t and r[1] >= end)), len(recs))
            if i1 == len(recs) and k + 1 < len(chunks):
                continue
            seam = carry is not None and carry[0] == t and carry[1] > beg
            i0 = next((i for i in range(i1) if recs[i][0] == t and pm[i] > beg), i1)
            res[j] = (k, i0, i1, int(seam))
        carry = run
        carries.append(carry)
    return res, carries


def run_emu(emu, tmp_path, n_ref, chunks, bounds):
    lines = [f"{n_ref} {len(bounds)} {len(chunks)}"] + [f"{t} {b} {e}" for t, b, e in bounds]
    for k, recs in enumerate(chunks):
        lines.append(f"{len(recs)} {int(k + 1 == len(chunks))}")
        for tid, pos, flag, cig in recs:
            lines.append(" ".join([str(tid), str(pos), str(flag), str(len(cig))] + [f"{n} {op}" for n, op in cig]))
    p = tmp_path / "case.txt"
    p.write_text("\n".join(lines) + "\n")
    r = subprocess.run([emu, str(p)], capture_output=True, text=True)
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
    assert r.returncode == 0, (r.returncode, r.stderr)
    res, carries, errs, k = {}, [], [], -1
    for ln in r.stdout.splitlines():
        w = ln.split()
        if w[0] == "chunk":
            k = int(w[1])
            carries.append((int(w[3]), int(w[4])))
            errs.append((int(w[6]), int(w[8])))
        else:
            assert int(w[1]) not in res, "a bound decided twice"
            res[int(w[1])] = (k, int(w[2]), int(w[3]), int(w[4]))
    return res, carries, errs


def draw_records(rng, n, tids, span=20000, long_every=7, tail=0):
    """n placed records on the references `tids`, sorted; every long_every-th one has a deletion or an N skip of thousands of
    bases, some are placed-unmapped or have no CIGAR; `tail` unplaced records behind them"""
    recs = []
    for i in range(n):
        tid, pos = rng.choice(tids), rng.randrange(span)
        kind = rng.randrange(12)
        if kind == 0:
            flag, cig = 4, [(100, 0)]                          # placed-unmapped: ends at pos + 1 whatever its CIGAR says
        elif kind == 1:
            flag, cig = 0, []                                   # no CIGAR
        elif i % long_every == 0:
            flag, cig = 0, [(30, 0), (rng.randrange(1000, 9000), rng.choice((2, 3))), (70, 0)]
        else:
            flag, cig = rng.choice((0, 16, 256, 2048)), [(5, 4), (rng.randrange(20, 150), 0), (3, 1)]
        recs.append((tid, pos, flag, cig))
    recs.sort(key=lambda r: (r[0], r[1]))
    return recs + [(-1, -1, 4, [])] * tail


def cut(recs, sizes):
    out, at = [], 0
    for s in sizes:
        out.append(recs[at:at + s])
        at += s
    if at < len(recs) or not out:
        out.append(recs[at:])
    return out


def draw_bounds(rng, n, tids, span=20000, window=500):
    """queries [max(0, left - window), right + window): some clamped to 0, some identical, many overlapping"""
    b = []
    for _ in range(n):
        left = rng.randrange(-200, span + 2000)
        left = max(0, left)
        right = left + rng.randrange(0, 60)
        b.append((rng.choice(tids), max(0, left - window), right + window))
    b += b[:max(1, n // 8)]                                     # identical ones
    return sorted(b, key=lambda x: (x[0], x[1]))


def check(emu, tmp_path, n_ref, chunks, bounds):
    want, want_carry = rule(chunks, bounds)
    got, carries, errs = run_emu(emu, tmp_path, n_ref, chunks, bounds)
    assert all(e == (-1, -1) for e in errs), errs
    for k, recs in enumerate(chunks):                           # (an empty chunk leaves the carry as it came)
        assert carries[k] == (want_carry[k] if want_carry[k] is not None else (-2, -2 ** 31)), (k, carries[k], want_carry[k])
    assert got == want
    assert len(got) == len(bounds)                              # the last chunk closes every bound
    return got


@pytest.mark.parametrize("seed", range(6))
def test_random_tables(emu, tmp_path, seed):
    """several references in a chunk, references without records (1 and 4), long deletions / skips, seams everywhere"""
    rng = random.Random(seed)
    recs = draw_records(rng, 700, (0, 2, 3, 5), tail=rng.choice((0, 9)))
    sizes = [rng.choice((1, 2, 40, 256, 257, 300)) for _ in range(5)]
    bounds = draw_bounds(rng, 60, (0, 1, 2, 3, 4, 5))
    got = check(emu, tmp_path, 6, cut(recs, sizes), bounds)
    assert {s for _, _, _, s in got.values()} == {0, 1}         # both answers occur


def test_one_chunk_has_no_seam(emu, tmp_path):
    rng = random.Random(11)
    recs = draw_records(rng, 600, (0, 1), tail=5)
    got = check(emu, tmp_path, 2, [recs], draw_bounds(rng, 50, (0, 1)))
    assert all(s == 0 for _, _, _, s in got.values())


def test_prefix_maximum_is_not_the_previous_end(emu, tmp_path):
    """one record with a 5000-base skip far to the left: i0 of a bound behind many short records is that record"""
    recs = [(0, 100, 0, [(10, 0), (5000, 3), (10, 0)])] + [(0, 200 + 10 * i, 0, [(50, 0)]) for i in range(300)]
    bounds = [(0, 4000, 4600), (0, 5200, 5400), (0, 0, 90), (0, 0, 101)]
    bounds.sort(key=lambda x: (x[0], x[1]))
    got = check(emu, tmp_path, 1, [recs], bounds)
    by = {bounds[j]: v for j, v in got.items()}
    assert by[(0, 4000, 4600)][1:3] == (0, 301)                 # the skip reaches to 5120: the long record opens the range
    assert by[(0, 5200, 5400)][1:3] == (301, 301)               # nothing reaches 5200: empty, and still a range
    assert by[(0, 0, 90)][1:3] == (0, 0) and by[(0, 0, 101)][1:3] == (0, 1)
    # the same table cut behind the long record: the carry (0, 5120) makes the first bound a seam, not the second
    got = check(emu, tmp_path, 1, [recs[:1], recs[1:]], bounds)
    by = {bounds[j]: v for j, v in got.items()}
    assert by[(0, 4000, 4600)][3] == 1 and by[(0, 5200, 5400)][3] == 0


def test_single_record_chunks_and_end_of_file(emu, tmp_path):
    """chunks of one record; a bound behind every record is closed only by the file's end, one on a later reference too"""
    recs = [(1, 10 * i, 0, [(8, 0)]) for i in range(5)]
    bounds = [(0, 0, 50), (1, 0, 25), (1, 20, 1000), (1, 500, 1000), (2, 0, 100)]
    got = check(emu, tmp_path, 3, [[r] for r in recs], bounds)
    assert got[0] == (0, 0, 0, 0)                               # reference 0 has no records: decided by the first record of 1
    assert got[1] == (3, 0, 0, 1)                               # pos 30 >= 25 closes it in chunk 3; the carry (1, 28) > 0: a seam
    assert got[2][0] == 4 and got[2][3] == 1                    # closed by the end of the file, records in earlier chunks
    assert got[3] == (4, 1, 1, 0)                               # nothing reaches 500: empty
    assert got[4] == (4, 1, 1, 0)                               # a reference behind the last record


def test_reference_change_at_a_chunks_first_record(emu, tmp_path):
    recs = [(0, 100 + i, 0, [(50, 0)]) for i in range(256)] + [(1, 5 + i, 0, [(50, 0)]) for i in range(256)]
    bounds = [(0, 300, 900), (1, 0, 40), (1, 0, 2000)]
    got = check(emu, tmp_path, 2, [recs[:256], recs[256:]], bounds)
    assert got[0] == (1, 0, 0, 1)                               # its records lie in chunk 0, its end passes in chunk 1
    assert got[1] == (1, 0, 35, 0)                              # the carry belongs to reference 0
    assert got[2] == (1, 0, 256, 0)


def test_unsorted_and_foreign_reference_are_named(emu, tmp_path):
    recs = [(0, 10, 0, [(5, 0)]), (0, 30, 0, [(5, 0)]), (0, 20, 0, [(5, 0)]), (1, 5, 0, [(5, 0)]), (0, 50, 0, [(5, 0)]), (7, 1, 0, [(5, 0)])]
    _, _, errs = run_emu(emu, tmp_path, 2, [recs[:2], recs[2:]], [(0, 0, 100)])
    assert errs[0] == (-1, -1) and errs[1] == (2, 5)            # the first record of chunk 1 is compared with the last of chunk 0
    _, _, errs = run_emu(emu, tmp_path, 2, [[(-1, -1, 4, [])], [(0, 5, 0, [(5, 0)])]], [])
    assert errs[1][0] == 1                                      # a placed record behind an unplaced one
