"""The case table of tests/pull_cases.py on the CPU: every case reaches the edge it is named for (its witness, over the model's
trace), the colliding names are collisions of Nim's murmur as tests/test_pull.py restates it, which case tells each deliberate
break of the kernels apart (the break applied to the model; the breaks that change no answer are shown to change none), and
the host twins (csrc/pull_logic.cpp: strl_pull_select_host, _counts_host, _mates_host) against the model, through a stand-alone
program (tests/emu/pull_logic_driver.cpp) built with AddressSanitizer and UBSan.  tests/test_pull_edges_device.py sends the same
calls to the device."""
import os
import shutil
import struct
import subprocess

import pytest

import pull_cases as pc
from test_pull import _murmur, check_output, parse_bam, pull_expected, run_pull

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "strling_amd", "csrc")
SOURCES = [os.path.join(HERE, "emu", "pull_logic_driver.cpp"), os.path.join(CSRC, "pull_logic.cpp")]
ERR_FORMAT = -6

_M = [x for k, b in enumerate(pc.BAD) for x in (f"{b}-first-record", f"{b}-second-batch", f"good-tile-{k}")]
# the edges the table must hold, by call: a case that is renamed or lost fails here
WANTED = {
    "t": [f"records-{n}" for n in (0, 1, 255, 256, 257, 512)] + ["wave0-empty-wave3-full", "alternating-three-batches", "first-batch-empty"],
    "w": [f"tile-start-mod16-{j}" for j in range(16)] + [f"header-ends-{d}-behind-w1" for d in (0, 1, 35)] + ["record-longer-than-window"],
    "k": ["the-region", "own-range", "stop-leaves-32-bits", "another-reference"],
    "h": ["same-length", "different-lengths", "interleaved-A-B-A-B-A", "empty-name-l0-and-l1"],
    "hm": ["both-ask-in-one-window", "the-other-name-alone", "chain-wraps-1023-to-0", "forty-at-one-home", "same-name-both-read1-bits"],
    "q": ["requests-256", "requests-257", "requests-512", "first-match-two-waves", "first-match-two-batches", "rule-edges", "another-reference-ends-the-window"],
    "m": _M,
    "mm": _M,
    "c": ["alignments-tails-and-sizes"],
    "c-grid": ["more-rows-than-the-grid"],
}
NAMES = [c.name for c in pc.calls()]


def test_the_table_holds_every_named_edge():
    assert NAMES == list(WANTED)
    ids = [(call.name, c.id) for call in pc.calls() for c in call.cases]
    assert len(ids) == len(set(ids))
    for name, names in WANTED.items():
        assert [c.name for c in pc.call(name).cases] == names, name
    assert {c.family for call in pc.calls() for c in call.cases} == set("twkhqmc")


@pytest.mark.parametrize("name", NAMES)
def test_every_witness_holds(name):
    call = pc.call(name)
    readable = (call.tot + 64) & ~15
    for c, t in zip(call.cases, call.answer["traces"]):
        assert c.witness(t, call) is True, (c, t.status, t.batches[:4], t.wins[:4], [r[:3] for r in t.rounds])
        fb, nb, in_block = c.req[:3]
        assert nb >= 1 and fb + nb <= len(call.blocks) and in_block <= call.isize[fb], c
        # nothing the kernels load lies outside the call's readable bytes: the windows, the records, the names
        assert all(w0 % 16 == 0 and w1 <= readable for w0, w1, *_ in t.wins), c
        assert t.s0 <= t.s1 <= call.tot and all(t.s0 <= r.p and r.p + 4 + r.bs <= t.s1 for r in t.recs), c
    assert call.tot < 1_000_000


def test_the_names_with_one_hash():
    """found at import over 2^20 names of 8 and of 9 bytes; each checked against the murmur of tests/test_pull.py"""
    K = pc.colliding()
    assert len(K["same"]) >= 50 and len(K["mixed"]) >= 100 and len(K["home1023"]) >= 500 and len(K["home512"]) >= 500
    for a, b in K["same"] + K["mixed"]:
        assert a != b and _murmur(a) == _murmur(b) == pc.murmur(a) == pc.murmur(b), (a, b)
    assert all((len(a), len(b)) == (8, 8) for a, b in K["same"]) and all((len(a), len(b)) == (8, 9) for a, b in K["mixed"])
    for n in K["home1023"][:50]:
        assert (_murmur(n) * 0x9E3779B1 & 0xFFFFFFFF) >> 22 == 1023 == pc.home(pc.murmur(n)), n
    for n in (b"", b"x", b"ab", b"abc", b"abcd", b"L" * 254):
        assert pc.murmur(n) == _murmur(n), n


def test_the_shapes_the_issue_names():
    """taken over all traces: the batch sizes, the rounds, the gather's alignments"""
    tr = [t for call in pc.calls() for t in call.answer["traces"]]
    assert {0, 1, 255, 256} <= {b[0] for t in tr for b in t.batches}
    assert {256, 1} <= {r[0] for t in tr for r in t.rounds} and max(len(t.rounds) for t in tr) == 2
    q = pc.call("q")
    t257 = q.answer["traces"][[c.name for c in q.cases].index("requests-257")]
    assert len(t257.rounds) == 2 and len(t257.batches) == 2          # rounds and batches interact
    assert {t.status for t in tr} == {0, 1, 2}
    c = pc.call("c")
    assert {r[0] % 16 for r in c.answer["src"]} == set(range(16)) and all(a[0] % 16 == b[0] % 16 for a, b in zip(c.answer["src"], c.answer["rows"]))
    assert len(pc.call("c-grid").answer["rows"]) > pc.COPY_ROWS


# ---- the breaks a wrong kernel would have, applied to the model ------------------------------------------------------------------
def _per_case(call, ans):
    """a case's answer: its status and its rows (off = the record's place in the call), each with the bytes gathered for it"""
    rows = [s + (ans["data"][r[0]:r[0] + r[5]] if r[9] else b"",) for s, r in zip(ans["src"], ans["rows"])]
    cut = ans["tile_rows"] if call.kind == "select" else call.win_off
    return [(s, rows[a:b]) for s, a, b in zip(ans["status"], cut, cut[1:])]


def _told(mut):
    return [f"{call.name}:{c.id}" for call in pc.calls() for c, a, b in zip(call.cases, _per_case(call, call.answer), _per_case(call, call.model(mut))) if a != b]


TELLERS = {
    "no_running": ["t:t-records-257", "t:t-records-512", "t:t-alternating-three-batches", "c-grid:c-more-rows-than-the-grid"],
    "wcnt_wrong_wave": ["t:t-wave0-empty-wave3-full", "t:t-alternating-three-batches", "t:t-records-255"],
    "no_wrap": ["hm:h-chain-wraps-1023-to-0"],
    "first_hash": ["hm:h-both-ask-in-one-window", "hm:h-same-name-both-read1-bits"],
    "max": ["q:q-first-match-two-waves", "q:q-first-match-two-batches", "q:q-requests-257"],
    "ge": ["k:k-the-region", "q:q-rule-edges"],
    "end_le": ["k:k-the-region", "q:q-rule-edges"],
    "l_name": ["h:h-empty-name-l0-and-l1"],
    "no_grid_loop": ["c-grid:c-more-rows-than-the-grid"],
    "no_head": ["c:c-alignments-tails-and-sizes", "w:w-tile-start-mod16-1", "w:w-tile-start-mod16-15"],
}


@pytest.mark.parametrize("mut", list(TELLERS))
def test_a_broken_kernel_is_told_apart(mut):
    """the prefix without `running`, wcnt[] of the wrong wave, no wrap at slot 1023, the probe stopped at the first equal hash,
    max for min, >= for > at beg and <= for < at end in the two interval tests, l_read_name for the name's length, the copy without its grid loop or its
    head bytes: each changes the answer of the cases named"""
    told = _told(mut)
    assert set(TELLERS[mut]) <= set(told), (mut, told)
    # and what passes by construction: a first batch without kept rows needs no running count; 16-aligned records have no head
    if mut == "no_running":
        assert "t:t-first-batch-empty" not in told and "t:t-records-256" not in told
    if mut == "no_head":
        assert "w:w-tile-start-mod16-0" in told          # (only its first record is aligned)
    if mut in ("ge", "end_le"):
        assert set(told) == set(TELLERS[mut])


def test_every_break_of_the_model_is_listed():
    assert set(pc.MUTATIONS) == set(TELLERS) | {"win_lt", "no_len"}


def test_a_reload_one_byte_early_changes_no_answer():
    """`<` for `<=` at the window's end: a header that ends with the window is loaded once more, from global memory that holds
    the same bytes; the case named takes the other way and no case of the table gets another answer -- no test of bytes can
    tell this break apart, on the CPU or on the device"""
    moved = [f"{call.name}:{c.id}" for call in pc.calls() for c, a, b in zip(call.cases, call.answer["traces"], call.model("win_lt")["traces"]) if a.wins != b.wins]
    assert "w:w-header-ends-0-behind-w1" in moved and "w:w-header-ends-1-behind-w1" not in moved
    assert _told("win_lt") == []


def test_the_mate_rule_s_length_compare_decides_no_case():
    """pull_mate_kernel compares the names' lengths behind the hashes and in front of the bytes.  Without it a record would meet a
    request of the same hash whose name begins with the record's: among the names with one hash found here (8 bytes against 8,
    8 against 9) none is the beginning of the other, so no case of the table gets another answer -- the compare is not covered"""
    K = pc.colliding()
    assert not any(b.startswith(a) for a, b in K["same"] + K["mixed"])
    assert _told("no_len") == []


# ---- the host twins ------------------------------------------------------------------------------------------------------------------
def _rocm_include():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    return os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "include")


@pytest.fixture(scope="module")
def driver():
    """pull_logic.cpp and the driver under ASan and UBSan; common.h includes the HIP runtime's header, so plain g++ gets its path"""
    out = os.path.join(HERE, "emu", "pull_logic_build")
    exe = os.path.join(out, "pull_logic_driver")
    deps = SOURCES + [os.path.join(CSRC, h) for h in ("common.h", "nim_tables.h", "pull_rec.h")] + [os.path.join(HERE, "..", "include", "strling_amd.h")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(d) for d in deps):
        os.makedirs(out, exist_ok=True)
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-D__HIP_PLATFORM_AMD__", "-I" + _rocm_include(), "-o", exe] + SOURCES)
    return exe


def _run(driver, call, items, kind, tmp_path):
    path = str(tmp_path / f"{call.name}.in")
    names = call.names if kind else b""
    with open(path, "wb") as f:
        f.write(struct.pack("<QQQQ", len(call.u), len(items), kind, len(names)) + call.u + names + b"".join(items))
    r = subprocess.run([driver, path], capture_output=True, text=True)
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
    assert r.returncode == 0, (r.returncode, r.stderr)
    return [line.split() for line in r.stdout.splitlines()]


def _bytes_of(t):
    """the bytes the host reads for a tile or window: [s0, s1), or with status 1 what the request's blocks hold from its start"""
    return (t.walk.p0, t.walk.lim) if t.status == 1 else (t.s0, t.s1)


@pytest.mark.parametrize("name", [c.name for c in pc.calls() if c.kind == "select"])
def test_the_host_select_and_counts_equal_the_model(driver, name, tmp_path):
    """strl_pull_select_host over every tile's bytes, in a vector of exactly their size, and strl_pull_counts_host over all rows:
    status 0 = STRL_OK with the model's rows, field by field; status 1 and 2 = STRL_ERR_FORMAT"""
    call = pc.call(name)
    A = call.answer
    items = [struct.pack("<QQiiiiii", *_bytes_of(t), *c.tile, 0) for c, t in zip(call.cases, A["traces"])]
    out = _run(driver, call, items, 0, tmp_path)
    heads = out[:len(items)]
    for c, t, h, a, b in zip(call.cases, A["traces"], heads, A["tile_rows"], A["tile_rows"][1:]):
        assert h[0] == "T" and int(h[1]) == (0 if t.status == 0 else ERR_FORMAT) and int(h[2]) == b - a, (c, h, t.status, b - a)
    assert out[len(items)] == ["C", "0"]
    got = [tuple(int(x) for x in line) for line in out[len(items) + 1:]]
    assert got == A["src"]


@pytest.mark.parametrize("name", [c.name for c in pc.calls() if c.kind == "mates"])
def test_the_host_mates_equal_the_model(driver, name, tmp_path):
    call = pc.call(name)
    A = call.answer
    items = []
    for w, (c, t) in enumerate(zip(call.cases, A["traces"])):
        reqs = call.reqs[call.win_off[w]:call.win_off[w + 1]]
        items.append(struct.pack("<QQiI", *_bytes_of(t), c.req[3], len(reqs)) + b"".join(struct.pack("<IiiIHBB", *q) for q in reqs))
    out = _run(driver, call, items, 1, tmp_path)
    at = 0
    for w, (c, t) in enumerate(zip(call.cases, A["traces"])):
        n = call.win_off[w + 1] - call.win_off[w]
        assert out[at][0] == "W" and int(out[at][1]) == (0 if t.status == 0 else ERR_FORMAT), (c, out[at], t.status)
        if t.status == 0:
            got = [tuple(int(x) for x in line) for line in out[at + 1:at + 1 + n]]
            assert got == A["src"][call.win_off[w]:call.win_off[w + 1]], c
        at += 1 + n
    assert at == len(out)


# ---- status 2 in the command ---------------------------------------------------------------------------------------------------------
def test_the_file_whose_window_only_the_host_can_answer(tmp_path):
    """pull_cases.cli_fallback_records: the bad record does not parse for pl_plausible, lies inside the bytes of A's and B's
    window behind both mates and in front of the record that ends the query -- so pl_walk meets it (status 2) and
    strl_pull_mates_host, which stops when every request is answered, does not; the host path's output is the restatement's.
    tests/test_pull_edges_device.py sends the file down the device path"""
    bam = str(tmp_path / "in.bam")
    hdr, regions, args, bad = pc.write_cli_fallback(bam)
    header, parsed, _ = parse_bam(bam)
    u = b"".join(r.raw for r in parsed)
    at = {r.qname + (b"'" if r.flag & 0x80 else b""): (k, sum(len(x.raw) for x in parsed[:k])) for k, r in enumerate(parsed)}
    k, p = at[bad + b"'"]
    assert len(parsed[k].raw) == 36 + len(bad) + 1 + 4 and not pc.plausible(u, p, len(u) - p)
    assert all(pc.plausible(u, q, len(u) - q) for j, q in at.values() if j != k)
    exp, kept, missing, requests = pull_expected(header, parsed, 2, regions)
    assert [r.qname for r in kept] == [b"A", b"B", b"C"] and requests == 3 and not missing
    beg, end = min(r.mpos - 1 for r in kept[:2]), max(r.mpos + 1 for r in kept[:2])          # the window's query
    assert beg >> 14 == (kept[1].mpos - 1) >> 14 == 20 and (kept[2].mpos - 1) >> 14 == 25
    assert at[b"A'"][0] < at[b"B'"][0] < k < at[b"C'"][0] and beg <= parsed[k].pos < end <= parsed[k + 1].pos
    h = run_pull(["-o", str(tmp_path / "host.bam"), bam] + args, mode="host")
    assert h.returncode == 0, h.stderr
    check_output(str(tmp_path / "host.bam"), exp, len(hdr.rstrip("\n").split("\n")))
