"""The evidence kernel's per-record rule (strling_amd/csrc/evidence_core.h) on the CPU, over the case table of
tests/evidence_cases.py: every case's witness holds on the oracle's spanners(); the host path (strl_spanners) equals the oracle
byte for byte; and the rule itself -- the header test, the keep test with its depth slots, the row fill, compiled for the host
in tests/emu/evidence_emu.cpp, a stand-alone program built with AddressSanitizer and UBSan -- gives rows that equal, field by
field, what the oracle's own functions give.  The refused inputs of family i give status 2 and a clean exit.  What stays in
evidence.hip (the LDS window, ballots and ranks, the scan, the hash table) is the business of
tests/test_evidence_edges_device.py.  CPU only."""
import os
import struct
import subprocess

import numpy as np
import pytest

import evidence_cases as ec
from strling_amd import api

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "emu", "evidence_emu.cpp")
CSRC = os.path.join(HERE, "..", "strling_amd", "csrc")
FLAGS = ["-O1", "-g", "-std=c++17", "-fsanitize=address,undefined"]
EV_OVERLAP, EV_PAIR = 1, 2
ROW_FIELDS = ("ord", "name_id", "hash", "prob", "start", "stop", "isize", "flags", "type", "repeat_count", "cigar_ins", "cigar_del")
FAMILIES = "abcdefgh"


@pytest.fixture(scope="module")
def emu():
    out = os.path.join(HERE, "emu", "evidence_build")
    exe = os.path.join(out, "evidence_emu")
    deps = [SRC] + [os.path.join(CSRC, h) for h in ("evidence_core.h", "bam_rec.h", "nim_tables.h")] + [os.path.join(HERE, "..", "include", "strling_amd.h")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(d) for d in deps):
        os.makedirs(out, exist_ok=True)
        subprocess.check_call(["g++"] + FLAGS + ["-o", exe, SRC])
    return exe


def run_emu(emu, tmp_path, tables, regions):
    """tables: float32[4096] arrays; regions: (raw, bound, window, min_mapq, table index) -> [(status, median, [row dict])]"""
    blob = bytearray(struct.pack("<I", len(tables)))
    for t in tables:
        assert t.dtype == np.float32 and t.size == 4096
        blob += t.tobytes()
    blob += struct.pack("<I", len(regions))
    for raw, b, window, min_mapq, table in regions:
        blob += struct.pack("<iIIiII8sQ", window, min_mapq, table, int(b["tid"]), int(b["left"]), int(b["right"]), bytes(b["repeat"]), len(raw))
        blob += raw
    p = tmp_path / "regions.bin"
    p.write_bytes(bytes(blob))
    r = subprocess.run([emu, str(p)], capture_output=True, text=True)
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.returncode == 0, (r.returncode, r.stderr[-4000:])
    out = []
    for ln in r.stdout.splitlines():
        w = ln.split()
        if w[0] == "region":
            assert int(w[1]) == len(out)
            out.append((int(w[3]), int(w[5]), []))
        else:
            out[-1][2].append(dict(zip(ROW_FIELDS, (int(x) for x in w[1:]))))
    assert len(out) == len(regions)
    return out


def expected_rows(c, ref, cd):
    """the rows of a case from the oracle's functions: the keep set, name_id and EV_PAIR restated from collect.nim:138-141,157-158"""
    rec, b = c.rec, c.bound
    left, right, wl, wr = int(b["left"]), int(b["right"]), int(b["left"]) - c.window, int(b["right"]) + c.window
    beg, end = max(0, wl), wr
    by_rec = {int(s["rec"]): s for s in ref[0] if s["type"] != 0}
    rows, first = [], {}
    for i in range(rec.n):
        start, stop, flag = int(rec.pos[i]), ec.rec_stop(rec, i), int(rec.flag[i])
        if int(rec.tid[i]) != int(b["tid"]) or not (start < end and stop > beg) or flag & (0x100 | 0x400 | 0x800) or int(rec.mapq[i]) < c.min_mapq:
            continue
        name = bytes(rec.qname(i))
        k = len(rows)
        s = by_rec.get(i)
        flags = (EV_OVERLAP if s is not None else 0) | (EV_PAIR if int(rec.tid[i]) == int(rec.mtid[i]) and abs(int(rec.isize[i])) <= 5000 else 0)
        prob = np.float32(ec.probability(cd, start, stop, flag & 0x10, left, right))
        rows.append(dict(ord=i, name_id=first.setdefault(name, k), hash=ec.nim_hash(name), prob=int(prob.view(np.uint32)), start=start, stop=stop,
                         isize=int(rec.isize[i]), flags=flags, type=int(s["type"]) if s is not None else 0,
                         repeat_count=int(s["repeat_count"]) if s is not None else 0, cigar_ins=int(s["cigar_ins"]) if s is not None else 0,
                         cigar_del=int(s["cigar_del"]) if s is not None else 0))
    assert set(by_rec) <= {r["ord"] for r in rows}
    return rows


@pytest.fixture(scope="module")
def refs():
    return ec.references()


def test_the_table_holds_every_family_and_stays_inside_the_capacity_rule():
    cases = ec.answered()
    assert {c.family for c in cases} == set(FAMILIES) and {c.family for c in ec.refused()} == {"i"}
    assert len({c.id for c in cases + ec.refused()}) == len(cases) + len(ec.refused())
    for c in cases:
        assert c.rec.n <= ec.MAX_RECORDS and 1 <= int(c.bound["right"]) - int(c.bound["left"]) + 2 * c.window <= ec.MAX_SPAN, c
    x, y = ec.COLLIDING
    assert x != y and ec.nim_hash(x) == ec.nim_hash(y) == 0x14a79bc7
    _, reached = ec.alignment_regions()
    assert sorted(reached) == list(range(16))


@pytest.mark.parametrize("family", FAMILIES)
def test_witnesses_hold_on_the_oracle(refs, family):
    """a case whose witness fails is a broken case: it does not reach the edge it is named after"""
    cases = [c for c in ec.answered() if c.family == family]
    assert cases
    for c in cases:
        assert c.witness is not None and c.witness(refs[c.id]), (c, refs[c.id][1:], [tuple(s) for s in refs[c.id][0][:8]])


@pytest.mark.parametrize("family", FAMILIES)
def test_host_path_equals_the_oracle(refs, family):
    """strl_spanners against the oracle: the support bytes, the median, the float32 bits of expected_spanners"""
    for c in ec.answered():
        if c.family != family:
            continue
        got, ref = api.spanners(c.rec, c.bound, c.window, c.frag, c.min_mapq), refs[c.id]
        assert got[0].tobytes() == np.ascontiguousarray(ref[0]).tobytes(), c
        assert got[1] == ref[1] and np.float32(got[2]).view(np.uint32) == np.float32(ref[2]).view(np.uint32), (c, got[1:], ref[1:])


def test_emulated_rows_equal_the_oracle_field_by_field(emu, refs, tmp_path):
    """the whole table in one run of the emulation, under AddressSanitizer and UBSan"""
    cases = ec.answered()
    frags = []
    for c in cases:
        if not any(c.frag is f for f in frags):
            frags.append(c.frag)
    tables = [ec.cumulative(f) for f in frags]
    which = [next(t for t, f in enumerate(frags) if c.frag is f) for c in cases]
    got = run_emu(emu, tmp_path, tables, [(c.raw, c.bound, c.window, c.min_mapq, t) for c, t in zip(cases, which)])
    n_rows = 0
    for c, t, (status, median, rows) in zip(cases, which, got):
        ref = refs[c.id]
        assert status == 0, c
        assert median == ref[1], (c, median, ref[1])
        want = expected_rows(c, ref, tables[t])
        assert len(rows) == len(want), (c, len(rows), len(want))
        for a, b in zip(rows, want):
            assert a == b, (c, a, b)
        n_rows += len(rows)
    assert n_rows > 3 * ec.MAX_RECORDS


def test_emulated_probability_at_the_table_s_last_entry(emu, tmp_path):
    """family d again with a table whose last entry is not 1 (evidence_cases.synthetic_cd): dist = 4095 is taken, 4096 is not --
    with a cumulative table both give zero"""
    syn = ec.synthetic_cd()
    cases = [c for c in ec.answered() if c.family == "d"]
    got = run_emu(emu, tmp_path, [syn], [(c.raw, c.bound, c.window, c.min_mapq, 0) for c in cases])
    at_edge = 0
    for c, (status, _, rows) in zip(cases, got):
        assert status == 0 and len(rows) == c.rec.n
        left, right = int(c.bound["left"]), int(c.bound["right"])
        for i, row in enumerate(rows):
            p = np.float32(ec.probability(syn, int(c.rec.pos[i]), ec.rec_stop(c.rec, i), int(c.rec.flag[i]) & 0x10, left, right))
            assert row["prob"] == int(p.view(np.uint32)), (c, i, row, p)
            at_edge += p == np.float32(1.0) - syn[4095]
    assert at_edge == 2                                       # one forward and one reverse read exactly at 4095


def test_refused_bytes_give_status_2_and_a_clean_exit(emu, refs, tmp_path):
    """the inputs the kernel is written to refuse, between answered neighbours: exactly they give status 2 and no rows, and the
    neighbours' answers are those they have alone.  (These go to the device only because this test takes them clean.)"""
    cd = [ec.cumulative(ec.FRAG_WIDE)]
    near = [c for c in ec.answered() if c.id in ("h-small-region", "b-ins-del-300", "a-count-300-wraps")]
    assert len(near) == 3
    mixed = []
    for k, c in enumerate(ec.refused()):
        mixed += [near[k % 3], c]
    mixed.append(near[0])
    got = run_emu(emu, tmp_path, cd, [(c.raw, c.bound, c.window, c.min_mapq, 0) for c in mixed])
    for c, (status, median, rows) in zip(mixed, got):
        if c.refused:
            assert status == 2 and not rows and median == 0, c
        else:
            assert status == 0 and median == refs[c.id][1] and rows == expected_rows(c, refs[c.id], cd[0]), c
    # the capacity rule of the bound itself: one base beyond the span limit, and exactly at it
    c = near[0]
    wide, at = ec.bound(0, 1000, 1000 + ec.MAX_SPAN - 2 * 500 + 1, "AC"), ec.bound(0, 1000, 1000 + ec.MAX_SPAN - 2 * 500, "AC")
    got = run_emu(emu, tmp_path, cd, [(c.raw, wide, 500, 20, 0), (c.raw, at, 500, 20, 0)])
    assert [g[0] for g in got] == [2, 0]
