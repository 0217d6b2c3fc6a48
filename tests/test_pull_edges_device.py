"""The kernels behind `strling pull` (strling_amd/csrc/pull.hip: pull_select_kernel, pull_keys_kernel + pull_count_kernel,
pull_mate_kernel + pull_mate_rows_kernel, pull_copy_kernel) on the device over the calls of tests/pull_cases.py: the status of
every tile and window, tile_rows, every row field by field (hash, count, found and l_name among them) and the bytes gathered for
it, against the plain-Python model -- exact equality, one call per family; and the same edges as one file through `strling pull`
itself, with a second file whose window of status 2 the host answers.  tests/test_pull_cases.py proves on the CPU that every case reaches the edge it is named for, that nothing sent here is
read outside its buffer, and which case tells which break of a kernel apart."""
import time

import numpy as np
import pytest

import evidence_cases as ec
import pull_cases as pc
from strling_amd import api, bamio
from test_pull import check_output, parse_bam, pull_expected, run_pull
from test_pull_device import _stats

SELECT = [c.name for c in pc.calls() if c.kind == "select" and c.name != "c-grid"]
MATES = [c.name for c in pc.calls() if c.kind == "mates"]


def _send(ctx, call):
    """-> (status, tile_rows or None, rows as tuples, the gathered bytes)"""
    if call.kind == "select":
        rows, tile_rows, data, st, _ = ctx.pull_select(call.streams, call.isize, call.requests, np.array([c.tile for c in call.cases], api.PULL_TILE_DTYPE), crcs=call.crcs)
        return st.tolist(), [int(x) for x in tile_rows], rows.tolist(), data
    rows, data, st, _ = ctx.pull_mates(call.streams, call.isize, call.requests, call.win_off, np.array(call.reqs, api.PULL_REQ_DTYPE), call.names, crcs=call.crcs)
    return st.tolist(), None, rows.tolist(), data


def _equal(call, got):
    A = call.answer
    status, tile_rows, rows, data = got
    assert tuple(api.PULL_ROW_DTYPE.names) == pc.ROW_FIELDS
    for c, t in zip(call.cases, A["traces"]):
        assert c.witness(t, call) is True, c
    assert status == A["status"], [(c, g, e) for c, g, e in zip(call.cases, status, A["status"]) if g != e]
    cut = A["tile_rows"] if call.kind == "select" else call.win_off
    mine = tile_rows if call.kind == "select" else cut
    assert len(mine) == len(cut)
    for c, a, b, ga, gb in zip(call.cases, cut, cut[1:], mine, mine[1:]):
        assert gb - ga == b - a, (c, "rows", gb - ga, b - a)
        for k in range(b - a):
            g, e = rows[ga + k], A["rows"][a + k]
            assert g[1:] == e[1:], (c, k, dict(zip(pc.ROW_FIELDS, g)), dict(zip(pc.ROW_FIELDS, e)))
            if g[9]:
                src = A["src"][a + k][0]
                assert data[g[0]:g[0] + g[5]] == call.u[src:src + g[5]], (c, k, "bytes")
    assert mine == cut and rows == A["rows"] and len(data) == len(A["data"])
    # a tile or window the device passes on has no rows / no answers, and nothing is gathered for it
    for c, s, a, b in zip(call.cases, status, cut, cut[1:]):
        if s:
            assert a == b if call.kind == "select" else all(r == pc.ZERO_ROW for r in rows[a:b]), c


@pytest.fixture(scope="module")
def answers(ctx):
    t0 = time.perf_counter()
    out = {c.name: _send(ctx, c) for c in pc.calls() if c.name != "c-grid"}
    print(f"{sum(len(c.cases) for c in pc.calls() if c.name != 'c-grid')} cases in {len(out)} calls: {time.perf_counter() - t0:.3f} s")
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", SELECT)
def test_every_tile_equals_the_model(answers, name):
    _equal(pc.call(name), answers[name])


@pytest.mark.gpu
@pytest.mark.parametrize("name", MATES)
def test_every_window_equals_the_model(answers, name):
    _equal(pc.call(name), answers[name])


@pytest.mark.gpu
def test_status_2_leaves_the_other_tiles_and_windows_alone(answers):
    """bytes that do not parse: status 2 without rows for the tile (1 where the walk in front of pull refuses the block_size
    itself), all of a window's rows zero although pull_mate_kernel had folded answers of the first batch, and the good tiles
    and windows of the same call answered in full"""
    for name in ("m", "mm"):
        call = pc.call(name)
        status, tile_rows, rows, data = answers[name]
        assert status == [1, 1, 0, 2, 2, 0, 2, 2, 0] == call.answer["status"]
        cut = tile_rows if name == "m" else call.win_off
        good = [k for k, s in enumerate(status) if s == 0]
        assert all(cut[k + 1] - cut[k] == 4 and all(r[9] == 1 for r in rows[cut[k]:cut[k + 1]]) for k in good)
        assert sum(r[9] for r in rows) == 12 and len(data) == len(call.answer["data"])
    folded = [t.folded for t in pc.call("mm").answer["traces"]]
    assert folded == [0, 0, 0, 0, 2, 0, 0, 2, 0]


@pytest.mark.gpu
def test_the_copy_of_8200_rows():
    """the grid loop's second turn, on a context of its own: its out buffer has never held these bytes"""
    call = pc.call("c-grid")
    assert len(call.answer["rows"]) > pc.COPY_ROWS
    own = api.Context(0)
    try:
        _equal(call, _send(own, call))
    finally:
        own.close()


@pytest.mark.gpu
def test_two_runs_give_the_same_rows(ctx, answers):
    for name in ("t", "hm"):
        again = _send(ctx, pc.call(name))
        assert again[:3] == answers[name][:3]


@pytest.mark.gpu
def test_the_edges_through_the_command(tmp_path):
    """`strling pull` over a file that holds the tiles of 0, 1, 255, 256, 257 and 512 records, the alternating lanes and the names
    with one hash: the device's output == the restatement of extract_region.nim == the host path's output"""
    recs, regions, args = pc.cli_records()
    bam = str(tmp_path / "in.bam")
    hdr = bamio.write_bam(bam, ec.batch(recs), block=1500)
    header, parsed, _ = parse_bam(bam)
    assert len(parsed) == len(recs)
    exp, kept, missing, requests = pull_expected(header, parsed, len(ec.TARGETS), regions)
    per_window = [sum(1 for r in parsed if r.tid == 0 and r.pos >> 14 == w) for w in range(8)]
    assert per_window[:7] == [0, 1, 255, 256, 257, 512, 700] and requests > 256 and len(missing) > 256
    K = pc.colliding()
    names = [r.qname for r in kept]
    assert all(names.count(n) == 1 for n in K["same"][0] + K["mixed"][0]) and all(names.count(n) == 2 for n in K["same"][1])
    out_d, out_h = str(tmp_path / "dev.bam"), str(tmp_path / "host.bam")
    d = run_pull(["-v", "-o", out_d, bam] + args)
    assert d.returncode == 0, d.stderr
    S = _stats(d.stderr)
    print(S)
    assert S["tiles"] == 8 and S["device_tiles"] == 8 and S["host_tiles"] == 0 and S["device_counts"] is True, S
    # the index cannot bound a window without a later window of its reference behind it; the last mates' window here is 40 and
    # filler_end lies in window 60, so every window is bounded and none is left to the host
    assert max(r.mpos >> 14 for r in kept if r.mtid == 0) == 40 and S["device_windows"] == S["windows"] and S["host_windows"] == 0, S
    assert S["kept"] == len(kept) and S["requests"] == requests, S
    got = check_output(out_d, exp, len(hdr.rstrip("\n").split("\n")))
    assert [l[len("skipping pair. mate not found for "):].encode() for l in d.stderr.split("\n") if l.startswith("skipping pair")] == missing
    out_names = [r.qname for r in got]
    assert all(out_names.count(n) == 2 for n in K["same"][0] + K["mixed"][0] + tuple(K["home1023"][:3]))
    h = run_pull(["-o", out_h, bam] + args, mode="host")
    assert h.returncode == 0, h.stderr
    assert open(out_d, "rb").read() == open(out_h, "rb").read()


@pytest.mark.gpu
def test_a_window_of_status_2_falls_back_to_the_host(tmp_path):
    """`strling pull` over pull_cases.cli_fallback_records: the window of A's and B's mates holds a record that does not parse
    behind both mates -- status 2 on the device, and the host, which stops at the last answer, finds both; C's mate's window is
    the device's.  The output == the restatement == the host path's output"""
    bam = str(tmp_path / "in.bam")
    hdr, regions, args, bad = pc.write_cli_fallback(bam)
    header, parsed, _ = parse_bam(bam)
    exp, kept, missing, requests = pull_expected(header, parsed, len(ec.TARGETS), regions)
    assert [r.qname for r in kept] == [b"A", b"B", b"C"] and not missing
    out_d, out_h = str(tmp_path / "dev.bam"), str(tmp_path / "host.bam")
    d = run_pull(["-v", "-o", out_d, bam] + args)
    assert d.returncode == 0, d.stderr
    S = _stats(d.stderr)
    print(S)
    assert S["device_tiles"] == 1 and S["host_tiles"] == 0 and S["requests"] == 3 and S["mates"] == 3, S
    assert S["windows"] == 2 and S["device_windows"] == 1 and S["host_windows"] == 1 and "1 of 2 mate windows searched on the host" in d.stderr, S
    got = check_output(out_d, exp, len(hdr.rstrip("\n").split("\n")))
    assert sorted(r.qname for r in got) == [b"A", b"A", b"B", b"B", b"C", b"C"]
    h = run_pull(["-o", out_h, bam] + args, mode="host")
    assert h.returncode == 0, h.stderr
    assert open(out_d, "rb").read() == open(out_h, "rb").read()
