"""The dense mode of the BGZF compressor (strling_amd/csrc/deflate_core.h: DflDense) on the CPU, through the host twin
(api.bgzf_deflate_host(mode="dense")).  The references are never the code under test: zlib for validity and size, and for the
tokens a Python model of the rule written here from its statement -- chain(p) = the earlier positions with p's 4-byte hash within
W, nearest first, the first D of them; match(p) = the longest common prefix among them, the nearest of equal ones, at least 4;
the parse takes the literal where match(pos + 1) is strictly longer than match(pos).  tests/test_deflate_dense_device.py runs
the same inputs through the kernel and compares byte for byte with the twin."""
import functools
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

import deflate_cases as D
from strling_amd import api
from test_deflate_cases import _token_list
from test_pull import sample  # noqa: F401  (the fixture)

HERE = os.path.dirname(os.path.abspath(__file__))
DEPTH, WINDOW, RING, BATCH = 16, 16128, 16384, 256      # the rule's constants; RING and BATCH only shape inputs


# ---- the model -----------------------------------------------------------------------------------------------------------------
def hash4(b, p):
    return ((int.from_bytes(b[p:p + 4], "little") * 2654435761) & 0xFFFFFFFF) >> 20


def _prefix(b, q, p, maxl):
    x = int.from_bytes(b[q:q + maxl], "little") ^ int.from_bytes(b[p:p + maxl], "little")
    return maxl if not x else ((x & -x).bit_length() - 1) // 8


def model_matches(b):
    """match(p) for every position: (length, distance) or None"""
    n, seen, out = len(b), {}, [None] * len(b)
    for p in range(n - 3):
        chain = seen.setdefault(hash4(b, p), [])
        best, dist, maxl = 3, 0, min(258, n - p)
        for q in chain[:-DEPTH - 1:-1]:                      # the D nearest, nearest first
            if p - q > WINDOW:
                break
            l = _prefix(b, q, p, maxl)
            if l > best:
                best, dist = l, p - q
        if dist:
            out[p] = (best, dist)
        chain.append(p)
    return out


def model_tokens(b):
    m, pos, toks = model_matches(b), 0, []
    while pos < len(b):
        c = m[pos]
        if c and pos + 1 < len(b) and m[pos + 1] and m[pos + 1][0] > c[0]:
            c = None
        toks.append(c)
        pos += c[0] if c else 1
    return toks


# ---- the inputs ------------------------------------------------------------------------------------------------------------------
class _Filler:
    """bytes in which no 4 bytes occur twice, over all the pieces handed out: a counter in the first two of every four bytes.
    The third byte is >= 0xF0 and the fourth 0xE1: no letter, so a filler never continues a match of the letters around it"""

    def __init__(self):
        self.k = 0

    def __call__(self, n):
        out = bytearray()
        while len(out) < n:
            out += struct.pack("<HBB", self.k, 0xF0 | (self.k & 7), 0xE1)
            self.k += 1
        return bytes(out[:n])


def _colliding_grams(target, count):
    """`count` different 4-grams of letters-free bytes with target's hash, none equal to it"""
    v = np.arange(1 << 22, dtype=np.uint64)
    grams = (v & 0xFF) | 0x80 | ((v >> 8 & 0x7F) | 0x80) << 8 | ((v >> 15 & 0x7F) | 0x80) << 16 | np.uint64(0xD7) << 24
    h = ((grams * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)) >> np.uint64(20)
    hit = np.unique(grams[h == hash4(target, 0)])
    res = [int(g).to_bytes(4, "little") for g in hit if int(g).to_bytes(4, "little") != target][:count]
    assert len(res) == count and all(hash4(g, 0) == hash4(target, 0) for g in res)
    return res


def _pad_to_lane(prefix, lane, f):
    """prefix + filler so that the next byte lies on `lane` of a batch of 256 positions"""
    return prefix + f((lane - len(prefix)) % BATCH)


@functools.lru_cache(maxsize=None)
def token_cases():
    """-> {name: (data, what the model's tokens must show: a function of (tokens, positions) -> bool)}; one block each"""
    r = np.random.default_rng(23)
    rnd = lambda n: bytes(r.integers(0, 256, n, dtype=np.uint8))
    text = lambda n: bytes(r.choice(np.frombuffer(b"ACGTN", np.uint8), n))
    f = _Filler()
    c = {}
    c["abcd_from_byte_0"] = (b"abcd" * 100, lambda toks, at: toks[:5] == [None] * 4 + [(258, 4)] and at[4] == 4)
    c["zeros_from_byte_0"] = (b"\0" * 1000, lambda toks, at: toks == [None, (258, 1), (258, 1), (258, 1), (225, 1)])
    # a 4-gram D + 1 or D + 2 times: the long match is the D-th nearest (found) or the (D + 1)-th (not found: the nearest, of 4
    # bytes, loses to the 43 bytes the next position finds on a chain of its own).  A byte of its own in front of and behind every
    # occurrence, so that no match begins before one or goes on behind one
    tail = b"t" + rnd(39)
    sep = lambda i: bytes([0xA0 + i])
    found = lambda toks, at, w: any(t and t[0] == 44 for t in toks) == w and (w or _follows(toks, [None, (43, _dist(toks, 43))]))
    for name, middle in (("depth_reaches_the_dth", DEPTH - 1), ("depth_stops_before_the_dth_plus_1", DEPTH)):
        d = f(64) + sep(30) + b"WXYZ" + tail + f(16)
        for i in range(middle):
            d += sep(i) + b"WXYZ" + sep(i) + f(12)
        d += sep(31) + b"WXYZ" + tail + f(16)
        c[name] = (d, lambda toks, at, w=(middle == DEPTH - 1): found(toks, at, w))
    # colliding 4-grams use depth up: D - 1 of them leave room for the true match, D do not
    for name, k in (("collisions_leave_room", DEPTH - 1), ("collisions_use_the_depth_up", DEPTH)):
        d = f(64) + sep(30) + b"WXYZ" + tail + f(16)
        for g in _colliding_grams(b"WXYZ", k):
            d += g + f(12)
        d += sep(31) + b"WXYZ" + tail + f(16)
        c[name] = (d, lambda toks, at, w=(k == DEPTH - 1): found(toks, at, w))
    x = rnd(20)
    d = f(40) + x + f(31) + x + f(17) + x + f(8)
    c["equal_lengths_nearest_wins"] = (d, lambda toks, at: (20, 37) in toks and (20, 51) in toks and (20, 88) not in toks)
    piece = rnd(100)
    c["distance_window"] = (piece + text(WINDOW - 100) + piece + text(50), lambda toks, at: any(t and t[1] == WINDOW for t in toks))
    c["distance_window_plus_1"] = (piece + text(WINDOW + 1 - 100) + piece + text(50), lambda toks, at: all(not t or t[1] <= WINDOW for t in toks))
    # longer than 2 W, the piece at positions that share a slot of the ring (RING apart) and once more 5000 before the last
    d = bytearray(text(2 * RING + 1000))
    for at_ in (100, 100 + RING, 100 + 2 * RING - 5000, 100 + 2 * RING):
        d[at_:at_ + 100] = piece
    c["ring_slots_shared"] = (bytes(d), lambda toks, at: len(toks) > 0 and any(t and t[1] == 5000 and t[0] >= 90 for t in toks))
    # lazy: the next match strictly longer (literal, then the longer one); equally long (the first is taken).  Every planted string
    # has a byte of its own in front and behind, as above
    marks = iter(list(range(0x80, 0xA0)) + list(range(0xC0, 0xE0)))
    own = lambda s_: bytes([next(marks)]) + s_ + bytes([next(marks)])
    tok_at = lambda toks, at, pos: toks[at.index(pos)] if pos in at else "no token starts here"

    def lazy(first, second, last, lane=None):
        d = f(24) + own(first) + f(24) + own(second) + f(24)
        if lane is not None:
            d += f((lane - 1 - len(d)) % BATCH)
        pos = len(d) + 1
        return d + own(last) + f(16), pos, pos - (d.index(second) if second[0] == last[0] else d.index(first))

    for name, lane in (("lazy_next_longer", None), ("lazy_next_longer_on_the_last_lane", 255)):
        d, pos, dist = lazy(b"BCDEFGHIJK", b"ABCDE", b"ABCDEFGHIJK", lane)
        dist = pos + 1 - d.index(b"BCDEFGHIJK")
        c[name] = (d, lambda toks, at, pos=pos, dist=dist, lane=lane: tok_at(toks, at, pos) is None and tok_at(toks, at, pos + 1) == (10, dist) and (lane is None or pos % BATCH == lane))
    for name, lane in (("lazy_next_equal", None), ("lazy_next_equal_on_the_last_lane", 255)):
        d, pos, dist = lazy(b"BCDEFG", b"ABCDEF", b"ABCDEFG", lane)
        c[name] = (d, lambda toks, at, pos=pos, dist=dist, lane=lane: tok_at(toks, at, pos) == (6, dist) and tok_at(toks, at, pos + 6) is None and (lane is None or pos % BATCH == lane))
    # lazy at the block's end: pos + 1 has fewer than four bytes left (no match there), and pos + 1 with an equal match
    d = f(40) + own(b"WXYZ") + f(40) + bytes([next(marks)]) + b"WXYZ"
    c["lazy_at_the_last_four"] = (d, lambda toks, at, dist=len(d) - 4 - 41: toks[-2:] == [None, (4, dist)])
    d = f(40) + own(b"VWXYQ") + f(40) + own(b"WXYZ") + f(40) + bytes([next(marks)]) + b"VWXYZ"
    c["lazy_at_the_last_five"] = (d, lambda toks, at, dist=len(d) - 5 - 41: toks[-3:] == [None, (4, dist), None])
    d = f(40) + own(piece[:50]) + f(40) + bytes([next(marks)]) + piece[:30]
    c["match_cut_at_the_end"] = (d, lambda toks, at, dist=len(d) - 30 - 41: toks[-2:] == [None, (30, dist)])
    return c


def _dist(toks, length):
    return next((t[1] for t in toks if t and t[0] == length), 0)


def _follows(toks, pair):
    return any(toks[i:i + 2] == pair for i in range(len(toks) - 1))


def _positions(toks):
    at, pos = [], 0
    for t in toks:
        at.append(pos)
        pos += t[0] if t else 1
    return at


TOKEN_CASES = list(token_cases())
SHORT = {f"n{n}": b"ACGTN"[:n] if n < 5 else b"ACGTA" for n in (1, 3, 4, 5)}


@functools.lru_cache(maxsize=None)
def small_blocks():
    """600 blocks of 256 bytes, every odd one a copy of its predecessor"""
    r = np.random.default_rng(29)
    out = bytearray()
    for _ in range(300):
        t = bytes(r.choice(np.frombuffer(b"ACGT", np.uint8), 256))
        out += t + t
    return bytes(out)


WORST = {"zeros_full_block": b"\0" * D.BLK, "period4_full_block": b"abcd" * (D.BLK // 4)}


@functools.lru_cache(maxsize=None)
def dense_inputs():
    """every input of the dense tests that goes through twin and kernel alike -> tuple of (name, data, block_bytes)"""
    c = [(name, data, block) for name, data, block in D.cases()]
    c += [(name, token_cases()[name][0], D.BLK) for name in TOKEN_CASES]
    c += [(name, data, D.BLK) for name, data in SHORT.items()]
    c += [(name, data, D.BLK) for name, data in WORST.items()]
    c.append(("small_blocks", small_blocks(), 256))
    return tuple(c)


INPUTS = {name: (data, block) for name, data, block in dense_inputs()}


@pytest.fixture(scope="module")
def twin():
    return {name: api.bgzf_deflate_host(data, block, mode="dense") for name, (data, block) in INPUTS.items()}


# ---- validity ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(INPUTS))
def test_members_are_valid(twin, name):
    data, block = INPUTS[name]
    D.check_members(data, block, *twin[name])


# ---- tokens ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", TOKEN_CASES)
def test_tokens_are_the_model_s(twin, name):
    data, shows = token_cases()[name]
    want = model_tokens(data)
    assert shows(want, _positions(want)), "the input does not reach what it was made for"
    out, csize, stored = twin[name]
    assert csize.size == 1 and stored == 0
    assert _token_list(out) == want


@pytest.mark.parametrize("name", list(SHORT))
def test_the_shortest_inputs(twin, name):
    """n = 1, 3, 4, 5: nothing to match (at n = 5 two positions with four bytes left, of different bytes); 31 bytes more than the
    input, stored, since a dynamic header alone is longer"""
    data = SHORT[name]
    assert model_tokens(data) == [None] * len(data)
    out, csize, stored = twin[name]
    assert stored == 1 and len(out) == len(data) + 31


@pytest.mark.parametrize("name", list(WORST))
def test_worst_case_chains(twin, name):
    """one chain of 65 k entries (zeros) or four (period 4): valid (test_members_are_valid), and the size of 254 longest matches --
    with at most 15 + 15 bits a match and a header of at most 100 bytes that is below 1100 bytes"""
    out, csize, stored = twin[name]
    assert stored == 0 and len(out) < 1100
    toks = _token_list(out)
    period, matches = 1 if name.startswith("zeros") else 4, [t for t in toks if t]
    assert toks[:period] == [None] * period and all(t == (258, period) for t in matches[:-1]) and len(matches) in (253, 254) and toks.count(None) < period + 4


def test_identical_blocks_give_identical_members(twin):
    out, csize, _ = twin["two_identical_blocks"]
    a, b = D.members_of(out, csize)
    assert a == b


def test_no_state_survives_from_block_to_block(twin):
    """600 blocks in one call, one work area: every odd block's member is its predecessor's, every member's tokens are the model's
    of that block alone, and no distance reaches in front of the block"""
    out, csize, stored = twin["small_blocks"]
    data = small_blocks()
    members = D.members_of(out, csize)
    assert len(members) == 600 and stored == 0
    for k in range(0, 600, 2):
        assert members[k] == members[k + 1], k
        toks = _token_list(members[k])
        assert toks == model_tokens(data[k * 256:(k + 1) * 256]), k
        assert all(t is None or t[1] <= at for t, at in zip(toks, _positions(toks)))


# ---- size --------------------------------------------------------------------------------------------------------------------
def test_size_against_zlib_level_5():
    """the DEFLATE payloads of the 19 blocks of a BAM's payload are at most zlib level 5's over the same cuts.
    Measured: dense twin 422 731 bytes = 0.8608 x level 1 (491 095), 0.9723 x level 5 (434 752), 0.9988 x level 6 (423 233);
    the fast mode gives 487 593"""
    p = D.fixture_payload()
    out, csize, stored = api.bgzf_deflate_host(p, mode="dense")
    assert csize.size == 19 and stored == 0
    mine = int(csize.sum()) - 26 * csize.size
    level = {}
    for lv in (1, 5, 6):
        level[lv] = 0
        for o in range(0, len(p), D.BLK):
            c = zlib.compressobj(lv, zlib.DEFLATED, -15)
            level[lv] += len(c.compress(p[o:o + D.BLK]) + c.flush())
    print(f"deflate payload bytes: dense twin {mine}; zlib level 1 {level[1]} ({mine / level[1]:.4f} x), level 5 {level[5]} ({mine / level[5]:.4f} x), "
          f"level 6 {level[6]} ({mine / level[6]:.4f} x)")
    assert mine <= level[5]
    D.check_members(p, D.BLK, out, csize, stored)


# ---- the fast mode, refusals ---------------------------------------------------------------------------------------------------
def test_the_fast_mode_is_the_call_without_a_mode():
    for name, data, block in D.cases() + (("fixture", D.fixture_payload(), D.BLK),):
        a, b = api.bgzf_deflate_host(data, block), api.bgzf_deflate_host(data, block, mode="fast")
        assert a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2] == b[2], name
    a, b = api.bgzf_deflate_host(D.fixture_payload()), api.bgzf_deflate_host(D.fixture_payload(), mode="dense")
    assert len(b[0]) < len(a[0])


def test_refusals():
    data = D.fixture_payload()[:100_000]
    need = D.bound(len(data), D.BLK)
    out = np.full(need + 64, 0xA5, np.uint8)
    got, csize, stored = api.bgzf_deflate_host(data, D.BLK, out=out, mode="dense")
    assert len(got) < len(data) and (out[len(got):] == 0xA5).all(), "nothing is written behind the output"
    out[:] = 0xA5
    with pytest.raises(api.StrlingError) as e:
        api.bgzf_deflate_host(data, D.BLK, out=out[:need - 1], mode="dense")
    assert e.value.code == -4 and (out == 0xA5).all()                   # STRL_ERR_CAPACITY
    for block in (0, 0xFF01):
        with pytest.raises(api.StrlingError) as e:
            api.bgzf_deflate_host(data, block, out=out, mode="dense")
        assert e.value.code == -3 and (out == 0xA5).all()               # STRL_ERR_ARG
    for mode in (2, -1, 256):                                           # neither STRL_DEFLATE_FAST nor STRL_DEFLATE_DENSE
        with pytest.raises(api.StrlingError) as e:
            api.bgzf_deflate_host(data, D.BLK, out=out, mode=mode)
        assert e.value.code == -3 and (out == 0xA5).all() and "mode" in str(e.value)
    with pytest.raises(ValueError):
        api.bgzf_deflate_host(data, D.BLK, mode="densest")


# ---- the commands on the host path ---------------------------------------------------------------------------------------------
def _json_of(stderr, command):
    import json
    import re
    m = re.search(r"\[strling\] %s: (\{.*\})" % command, stderr) if command == "pull" else re.search(r"(\{.*\})\s*$", stderr.strip())
    assert m, stderr
    return json.loads(m.group(1))


def test_pull_deflate_dense_on_the_host_path(sample, tmp_path):  # noqa: F811
    from test_pull import bgzf_payload, run_pull
    regions = ["chrA", "chr:B:1-60000"]
    files = {}
    for form in ("host", "device", "dense"):
        out = str(tmp_path / f"{form}.bam")
        r = run_pull(["-v", "-o", out, sample["bam"]] + regions + [f"--deflate={form}"], mode="host")
        assert r.returncode == 0, r.stderr
        files[form] = (out, open(out, "rb").read(), r)
    want = bgzf_payload(files["host"][0], max_block=0xFF00)
    assert bgzf_payload(files["dense"][0], max_block=0xFF00) == want
    members, csize, stored = api.bgzf_deflate_host(want, mode="dense")
    assert files["dense"][1] == members + D.EOF_BLOCK
    assert len(files["dense"][1]) < len(files["device"][1])
    s = _json_of(files["dense"][2].stderr, "pull")
    assert s["deflate"] == "core-host-dense" and s["deflate_stored_blocks"] == stored and s["deflate_kernel_ms"] == 0
    r = run_pull(["-o", str(tmp_path / "bad.bam"), sample["bam"], "chrA", "--deflate=nonsense"], mode="host")
    assert r.returncode != 0 and "--deflate must be" in r.stderr and "dense" in r.stderr and "Usage:" in r.stderr
    assert "--deflate=host|device|dense" in run_pull(["--help"]).stdout


def test_sort_deflate_dense_on_the_host_path(tmp_path, tmp_path_factory):
    import gzip

    import sort_index_cases as X
    from strling_amd import build
    src = X.case_dir(tmp_path_factory)["bins_of_every_level"]
    env = dict(os.environ, STRL_SORT="host")
    files = {}
    for form in ("host", "device", "dense"):
        out = str(tmp_path / f"{form}.bam")
        r = subprocess.run([build.CLI, "sort", "--write-index", "-v", f"--deflate={form}", "-o", out, src], capture_output=True, text=True, env=env)
        assert r.returncode == 0, r.stderr
        files[form] = (out, r)
    stream = gzip.decompress(open(files["host"][0], "rb").read())
    assert gzip.decompress(open(files["dense"][0], "rb").read()) == stream
    assert open(files["dense"][0], "rb").read() == api.bgzf_deflate_host(stream, mode="dense")[0] + D.EOF_BLOCK
    assert os.path.getsize(files["dense"][0]) < os.path.getsize(files["device"][0])
    assert _json_of(files["dense"][1].stderr, "sort")["deflate"] == "core-host-dense"
    # (`strling bamindex` needs a device: its bytes for this file are compared in tests/test_deflate_dense_device.py; here the
    # index against the Python writer's for the file, as tests/test_sort_index.py compares the fast mode's)
    assert X.index_structure(files["dense"][0] + ".bai", files["dense"][0], "bai") == X.reference_index(files["dense"][0], "bai")
    r = subprocess.run([build.CLI, "sort", "--deflate=nonsense", "-o", str(tmp_path / "bad.bam"), src], capture_output=True, text=True, env=env)
    assert r.returncode != 0 and "--deflate must be" in r.stderr and "dense" in r.stderr and not os.path.exists(tmp_path / "bad.bam")
    assert "--deflate=host|device|dense" in subprocess.run([build.CLI, "sort", "--help"], capture_output=True, text=True).stdout


# ---- the twin as a stand-alone program under the sanitizers -----------------------------------------------------------------------
def test_standalone_program_under_asan_and_ubsan():
    """tests/emu/deflate_dense_main.cpp: the dense twin, and the lanes' side of the rule on one thread, in buffers exact to the byte"""
    out = os.path.join(HERE, "emu", "deflate_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "deflate_dense_main")
    src = os.path.join(HERE, "emu", "deflate_dense_main.cpp")
    core = os.path.join(HERE, "..", "strling_amd", "csrc", "deflate_core.h")
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(f) for f in (src, core)):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, src, "-lz"])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "all cases passed" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
