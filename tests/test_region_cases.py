"""The case table of tests/region_cases.py on the CPU: every case reaches the edge it is named for (its witness, over the
model's trace), nothing the rule looks at lies outside the request's bytes, the layout of the copy, the CRC dealing of
crc32_kernel restated in Python against zlib.crc32 at every size and flipped bit of the CRC table, which case tells each
deliberate break of the kernels apart (the break applied to the model), and the host's stand-in for the walk
(cli/region_feed.cpp: region_walk) against the model, through a stand-alone program (tests/emu/region_walk_driver.cpp) built
with AddressSanitizer and UBSan.  tests/test_regions_edges_device.py sends the same calls to the device."""
import os
import struct
import subprocess
import zlib
from concurrent.futures import ThreadPoolExecutor

import pytest

import region_cases as rc

HERE = os.path.dirname(os.path.abspath(__file__))
CLI = os.path.join(HERE, "..", "strling_amd", "csrc", "cli")
SOURCES = [os.path.join(HERE, "emu", "region_walk_driver.cpp")] + [os.path.join(CLI, s) for s in (
    "region_feed.cpp", "bam_reader.cpp", "fast_inflate.cpp", "cram_reader.cpp", "cram_codecs.cpp")]
FLAGS = ["-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-I" + CLI]
WALK_CALLS = ("w", "k", "s", "e", "b", "m")

# the edges the table must hold, by family: a case that is renamed or lost fails here
WANTED = {
    "w": [f"start-mod16-{j}" for j in range(16)] + ["header-crosses-by-1", "header-crosses-by-35", "header-crosses-by-0", "cigar-crosses-header-inside",
                                                    "need-4080", "need-4081", "record-longer-than-window", "record-over-three-blocks", "cigar-65535", "last-window-cut"],
    "k": ["reach-is-beg-minus-1", "reach-is-beg", "clips-and-insertions-reach", "clips-and-insertions-short", "unmapped-flag-cigar-short", "no-cigar-kept",
          "no-cigar-dropped", "short-record-behind-kept", "beg-negative", "nothing-reaches-beg"],
    "s": ["pos-is-end-minus-1", "pos-is-end", "next-reference", "unplaced-tail", "first-record-stops", "tid-of-another-reference"],
    "e": ["ends-behind-a-record", "ends-1-into-a-header", "ends-35-into-a-header", "ends-inside-a-body", "last-blocks-of-the-call"],
    "b": ["in-block-is-isize-two-blocks", "in-block-is-isize-one-block", "empty-blocks-inside-and-last", "one-byte-blocks", "same-blocks-first",
          "same-blocks-second", "later-first-block-odd-uoff"],
    "m": ["block-size-31", "block-size-2-to-28-plus-1", "cigar-ends-with-record", "cigar-leaves-record-by-4", "cigar-65535-leaves-record"],
}


def test_the_table_holds_every_named_edge():
    ids = [c.id for call in rc.calls() for c in call.cases]
    assert len(ids) == len(set(ids))
    for fam, names in WANTED.items():
        assert [c.name for c in rc.call(fam).cases] == names, fam
    c = [x.name for x in rc.call("c").cases]
    assert c == [f"start-mod16-{j}" for j in range(16)] + [f"length-mod16-{j}" for j in range(16)] + ["empty-between", "more-than-256-pieces"]
    assert len(rc.call("c-grid").cases) == rc.COPY_GRID + 4


@pytest.mark.parametrize("name", [c.name for c in rc.calls()])
def test_every_witness_holds(name):
    call = rc.call(name)
    for c, t in zip(call.cases, call.traces):
        assert c.witness(t, call), (c, t.status, t.keep, t.stop, t.end, t.wins, t.paths[-3:])
        # a request is what the header says it is, and the rule never looks outside its bytes
        fb, nb, in_block = c.req[:3]
        assert nb >= 1 and fb + nb <= len(call.blocks) and in_block <= call.isize[fb], c
        assert t.max_read <= t.lim <= call.tot, c
        assert all(w1 <= (call.tot + 64) & ~15 for _, w1, *_ in t.wins), c
        if t.status == 0:
            assert t.base <= t.p0 <= t.keep <= t.stop <= t.lim - 36, c


def test_the_three_cigar_ways_and_both_reloads_are_reached():
    ways = {p[1] for call in rc.calls() for t in call.traces for p in t.paths}
    whys = {w[2] for call in rc.calls() for t in call.traces for w in t.wins}
    assert ways == {"lds", "global", "malformed"} and whys == {"header", "cigar"}
    ends = {(t.status, t.end) for call in rc.calls() for t in call.traces}
    assert ends == {(0, "ref"), (0, "pos"), (1, "lim-header"), (1, "lim-body"), (1, "bad-size")}


@pytest.mark.parametrize("name", [c.name for c in rc.calls()])
def test_the_layout_of_the_copy(name):
    """16-aligned plus the source's offset mod 16 for a non-empty piece, none overlapping, the capacity the header promises"""
    call = rc.call(name)
    at = 0
    for rg, off, ln in zip(call.ranges, call.out_off, call.out_len):
        if ln:
            assert off % 16 == rg[0] % 16 and at <= off < at + 31 and ln == rg[1] - rg[0]
            at = off + ln
        else:
            assert off == at
    assert at == call.needed <= sum(sum(call.isize[q[0]:q[0] + q[1]]) + 32 for q in call.requests)
    out = rc.copied(call)
    assert all(out[o:o + n] == e[0] for o, n, e in zip(call.out_off, call.out_len, call.expect))
    if name == "c":
        kept = [(rg[0] % 16, (rg[1] - rg[0]) % 16) for rg in call.ranges if rg and rg[1] > rg[0]]
        assert {k[0] for k in kept} == set(range(16)) == {k[1] for k in kept}


# ---- the breaks a wrong kernel would have, applied to the model ----------------------------------------------------------------
def _answers(call, mut=None):
    return [(t.status, t.keep, t.stop) for t in (call.traces if mut is None else [rc.walk(call, q, mut) for q in call.requests])]


@pytest.mark.parametrize("mut,teller", [("end_gt", "s-pos-is-end"), ("beg_ge", "k-reach-is-beg-minus-1"), ("no_empty_keep", "k-nothing-reaches-beg")])
def test_a_broken_rule_is_told_apart(mut, teller):
    """`pos > end` for `pos >= end`, `>= beg` for `> beg`, no empty range at stop: each changes the answer of the case named"""
    told = [c.id for name in WALK_CALLS for call in [rc.call(name)] for c, a, b in zip(call.cases, _answers(call), _answers(call, mut)) if a != b]
    assert teller in told, (mut, told)


@pytest.mark.parametrize("mut,teller", [("no_cigar_reload", "w-cigar-crosses-header-inside"), ("reload_lt", "w-need-4080")])
def test_a_lost_reload_changes_no_answer(mut, teller):
    """without the second load, or with `<` for `<=` at 4096 - 16, the CIGAR is read from global memory instead of the window:
    the case named takes the other way, and no case of the table gets another answer -- no test of bytes can tell these two"""
    call = rc.call("w")
    moved = [c.id for c, t, q in zip(call.cases, call.traces, call.requests) if [p[1] for p in rc.walk(call, q, mut).paths] != [p[1] for p in t.paths]]
    assert teller in moved, (mut, moved)
    for name in WALK_CALLS:
        assert _answers(rc.call(name), mut) == _answers(rc.call(name)), name


def test_a_copy_without_its_grid_loop_is_told_apart():
    call = rc.call("c-grid")
    whole, cut = rc.copied(call), rc.copied(call, grid_loop=False)
    first = call.out_off[rc.COPY_GRID]
    assert whole[:first] == cut[:first] and all(call.out_len[rc.COPY_GRID:]) and not any(cut[first:]) and whole[first:] != cut[first:]


# ---- the CRC -------------------------------------------------------------------------------------------------------------------
def test_the_crc_table_holds_every_size_and_position():
    rows = rc.crc_rows()
    assert len({r.name for r in rows}) == len(rows) >= 170
    single = [r for r in rows if len(r.blocks) == 1 and not r.name.startswith("size260-lane")]
    assert sorted({r.sizes[0] for r in single}) == sorted(rc.CRC_SIZES)
    for n in rc.CRC_SIZES:
        at = {r.at for r in single if r.sizes[0] == n}
        if n:
            assert {0, n - 1} | {a for a in (n - 2, n - 3, n - 4, n // 2) if a >= 0} <= at
        if n > 256:
            assert 256 in at and at & {252, 253, 254, 255}
    lanes = [r for r in rows if r.name.startswith("size260-lane")]
    assert [r.at // 4 for r in lanes] == list(range(64)) and len({r.bit for r in lanes}) == 8
    nine = [r for r in rows if len(r.blocks) == 9]
    assert [r.bad for r in nine] == list(range(9)) and 0 in nine[0].sizes[1:-1] and {sum(nine[0].sizes[:k]) % 4 for k in range(9)} == {0, 1, 2, 3}
    for r in rows:
        assert r.refuse[r.bad] != r.good[r.bad] and r.refuse[:r.bad] + r.refuse[r.bad + 1:] == r.good[:r.bad] + r.good[r.bad + 1:]
        assert r.request[2] == r.sizes[0] and all(zlib.decompress(s, -15) == b for s, b in zip(r.streams, r.blocks))
        if r.blocks[r.bad]:
            assert len(r.twin) == len(r.blocks[r.bad]) and sum(bin(a ^ b).count("1") for a, b in zip(r.twin, r.blocks[r.bad])) == 1


def test_the_dealing_of_the_crc_equals_zlib():
    """lane j takes dwords j, j + 64, ...; every block and every one-bit twin of the table, and every size up to 600"""
    for r in rc.crc_rows():
        for d in set(r.blocks) | {r.twin}:
            assert rc.crc_dealt(d) == zlib.crc32(d), (r, len(d))
        assert not rc.crc_verdict(r, r.good) and rc.crc_verdict(r, r.refuse), r
    d = rc.crc_rows()[-1].blocks[6]
    for n in range(600):
        assert rc.crc_dealt(d[:n]) == zlib.crc32(d[:n]), n


@pytest.mark.parametrize("mut,tellers", [("drop_lane63", ["size260-lane63", "size256-byte252"]), ("drop_tail", ["size259-byte258", "size1-byte0", "size65535-byte65534"]),
                                        ("expect_blockidx", ["nine-blocks-bad1", "nine-blocks-bad8"])])
def test_a_broken_crc_is_told_apart(mut, tellers):
    """the kernel without lane 63, without the tail bytes, or comparing with expect[workgroup]: the rows named get another
    verdict than the rule's -- the twin accepted, or the block itself refused"""
    rows = {r.name: r for r in rc.crc_rows()}
    for name in tellers:
        r = rows[name]
        assert not rc.crc_verdict(r, r.refuse, mut) or rc.crc_verdict(r, r.good, mut), (mut, name)


# ---- the host's stand-in ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver():
    out = os.path.join(HERE, "emu", "region_walk_build")
    exe = os.path.join(out, "region_walk_driver")
    deps = SOURCES + [os.path.join(CLI, h) for h in os.listdir(CLI) if h.endswith(".h")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(d) for d in deps):
        os.makedirs(out, exist_ok=True)
        objs = [os.path.join(out, os.path.basename(s)[:-4] + ".o") for s in SOURCES]
        with ThreadPoolExecutor(len(SOURCES)) as ex:
            list(ex.map(lambda so: subprocess.check_call(["g++"] + FLAGS + ["-c", so[0], "-o", so[1]]), zip(SOURCES, objs)))
        subprocess.check_call(["g++"] + FLAGS + ["-o", exe] + objs + ["-lz", "-lpthread"])
    return exe


@pytest.mark.parametrize("name", WALK_CALLS)
def test_the_stand_in_equals_the_model(driver, name, tmp_path):
    """region_walk over each request's run of bytes, in a vector of exactly that size: stopped = status 0, and then keep and stop"""
    call = rc.call(name)
    path = str(tmp_path / f"{name}.in")
    with open(path, "wb") as f:
        f.write(struct.pack("<QQ", len(call.u), len(call.requests)) + call.u)
        for q, t in zip(call.requests, call.traces):
            f.write(struct.pack("<QQQiiii", t.base, t.lim, q[2], q[3], q[4], q[5], 0))
    r = subprocess.run([driver, path], capture_output=True, text=True)
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
    assert r.returncode == 0, (r.returncode, r.stderr)
    got = [tuple(int(x) for x in line.split()) for line in r.stdout.splitlines()]
    assert len(got) == len(call.cases)
    for c, t, g in zip(call.cases, call.traces, got):
        assert g[0] == (t.status == 0), (c, g)
        if t.status == 0:
            assert g[1:] == (t.keep - t.base, t.stop - t.base), (c, g, t.keep - t.base, t.stop - t.base)
