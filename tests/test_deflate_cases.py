"""The BGZF compressor's rule (strling_amd/csrc/deflate_core.h) on the CPU: the host twin (api.bgzf_deflate_host) over the inputs
of tests/deflate_cases.py -- every member valid on its own and the shapes the inputs were made for really reached --, the
code-length routine alone through tests/emu/deflate_emu.cpp, the refusals, and the size against zlib level 1 on a BAM's payload.
tests/test_deflate_device.py runs the same inputs through the kernel and compares byte for byte."""
import ctypes as C
import os
import subprocess
import zlib
from fractions import Fraction

import numpy as np
import pytest

import deflate_cases as D
from strling_amd import api

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = {name: (data, block) for name, data, block in D.cases()}


@pytest.fixture(scope="module")
def twin():
    return {name: api.bgzf_deflate_host(data, block) for name, (data, block) in CASES.items()}


@pytest.fixture(scope="module")
def emu():
    so = os.path.join(HERE, "emu", "libdeflate_emu.so")
    src = os.path.join(HERE, "emu", "deflate_emu.cpp")
    core = os.path.join(HERE, "..", "strling_amd", "csrc", "deflate_core.h")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in (src, core)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, src])
    L = C.CDLL(so)
    L.emu_code_lengths.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
    L.emu_deflate_host.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.c_void_p, C.POINTER(C.c_uint32)]
    return L


# ---- validity ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_members_are_valid(twin, name):
    data, block = CASES[name]
    D.check_members(data, block, *twin[name])


def test_no_input_gives_no_member(twin):
    out, csize, stored = twin["len0"]
    assert out == b"" and csize.size == 0 and stored == 0


def test_the_emu_build_of_the_core_writes_the_library_s_bytes(emu, twin):
    """the g++ build of the header the code-length test below goes through is the rule the library runs"""
    for name in ("full_block_plus1", "fibonacci_literals", "zeros"):
        data, block = CASES[name]
        src = np.frombuffer(data, np.uint8)
        out = np.zeros(D.bound(len(data), block), np.uint8)
        nb, st = C.c_uint64(0), C.c_uint32(0)
        assert emu.emu_deflate_host(src.ctypes.data, src.size, block, out.ctypes.data, out.size, C.byref(nb), None, C.byref(st)) == 0
        assert out[:nb.value].tobytes() == twin[name][0] and st.value == twin[name][2]


# ---- the inputs reach what they were made for ----------------------------------------------------------------------------------
def _only_member(twin, name):
    out, csize, stored = twin[name]
    assert csize.size == 1
    return out


def _tokens(member):
    """(number of literals, [(length, distance)]) of a member's dynamic block"""
    toks = _token_list(member)
    return sum(1 for t in toks if t is None), [t for t in toks if t is not None]


def _token_list(member):
    """the tokens of a member's dynamic block in order, decoded here: None for a literal, (length, distance) for a match"""
    hlit, hdist, ll, dl = D.dynamic_header(member)
    bits = int.from_bytes(member[18:-8], "little")

    def table(lengths):
        code, tab = 0, {}
        for ln in range(1, 16):
            for s, l in enumerate(lengths):
                if l == ln:
                    tab[(ln, code)] = s
                    code += 1
            code <<= 1
        return tab

    # where the header ends: read it again, counting
    at = [0]

    def take(n):
        v = (bits >> at[0]) & ((1 << n) - 1)
        at[0] += n
        return v

    def symbol(tab):
        code = 0
        for ln in range(1, 16):
            code = code << 1 | take(1)
            if (ln, code) in tab:
                return tab[(ln, code)]
        raise AssertionError("no code")

    take(3); take(5); take(5)
    hclen = take(4) + 4
    cl = [0] * 19
    for i in range(hclen):
        cl[(16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)[i]] = take(3)
    ct, n = table(cl), 0
    while n < hlit + hdist:
        s = symbol(ct)
        n += 1 if s < 16 else 3 + take(2) if s == 16 else 3 + take(3) if s == 17 else 11 + take(7)
    lt, dt = table(ll), table(dl)
    LB = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
    LE = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
    DB = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
    DE = [0, 0, 0, 0] + [e for e in range(1, 14) for _ in (0, 1)]
    toks = []
    while True:
        s = symbol(lt)
        if s == 256:
            return toks
        if s < 256:
            toks.append(None)
            continue
        length = LB[s - 257] + take(LE[s - 257])
        d = symbol(dt)
        toks.append((length, DB[d] + take(DE[d])))


def test_zeros_use_the_longest_match(twin):
    """a run: the first batch is literals (nothing is inserted before its lookups), then 258-byte matches.  A position sees the
    last position of the batch before its own, so the distances along a long run differ (1, 3, 5, ...)"""
    lits, matches = _tokens(_only_member(twin, "zeros"))
    assert lits == 256 and matches and all(l == 258 for l, _ in matches[:-1]) and lits + sum(l for l, _ in matches) == D.BLK
    assert all(1 <= d <= 256 for _, d in matches)


def test_a_single_distance_code_is_sent_with_one_bit(twin):
    """300 zero bytes: one match, at distance 1; RFC 1951 3.2.7's one-code distance tree"""
    m = _only_member(twin, "zeros300")
    hlit, hdist, ll, dl = D.dynamic_header(m)
    assert hdist == 1 and dl == [1]
    assert _tokens(m) == (256, [(44, 1)])


@pytest.mark.parametrize("name", ["one_literal", "no_repeated_4gram"])
def test_no_distance_code(twin, name):
    m = _only_member(twin, name)
    assert D.block_type(m) == 2
    hlit, hdist, ll, dl = D.dynamic_header(m)
    assert hdist == 1 and dl == [0], "HDIST = 1 and that one code has zero bits"
    if name == "one_literal":
        assert sorted(s for s, l in enumerate(ll) if l) == [ord("Q"), 256] and ll[ord("Q")] == ll[256] == 1
    assert _tokens(m) == (len(CASES[name][0]), [])


def test_fibonacci_literals(twin):
    """bytes whose counts are 1, 1, 2, 3, 5, ...: a plain Huffman tree of the BYTES is deeper than 15.  Eighteen letters cannot
    fill 4180 positions without repeating 4-grams, so the parse turns part of them into matches and the counts the code is made
    from are flatter; what is sent is a complete code of at most 15 bits either way.  (The limit itself is reached in
    test_code_lengths_of_fibonacci_counts.)"""
    data = CASES["fibonacci_literals"][0]
    counts = sorted(np.bincount(np.frombuffer(data, np.uint8))[65:].tolist() + [1])
    depth = 0
    while len(counts) > 1:
        counts = sorted([counts[0] + counts[1]] + counts[2:])
        depth += 1
    assert depth > 15
    _, _, ll, dl = D.dynamic_header(_only_member(twin, "fibonacci_literals"))
    assert max(ll) <= 15 and sum(Fraction(1, 1 << l) for l in ll if l) == 1
    assert max(dl) <= 15 and sum(Fraction(1, 1 << l) for l in dl if l) == 1


def test_random_bytes_are_stored(twin):
    out, csize, stored = twin["random"]
    assert stored == 1 and D.block_type(out) == 0 and len(out) == D.BLK + 31 <= 65536


def test_matches_cross_batches(twin):
    """the 600-byte pattern: tokens that start in one batch of 256 positions and end in a later one, covering its first position"""
    pos, covering = 0, 0
    for t in _token_list(_only_member(twin, "pattern600")):
        n = 1 if t is None else t[0]
        if t is not None:
            assert t[1] % 600 == 0
            covering += (pos + n - 1) // 256 > pos // 256
        pos += n
    assert pos == 20_000 and covering >= 20_000 // 258 - 8, "nearly every token is a longest match, and 258 > 256"


def test_the_distance_limit(twin):
    for name, reach in (("dist32768", True), ("dist32769", False)):
        _, matches = _tokens(_only_member(twin, name))
        far = [m for m in matches if m[1] > 32000]
        assert max(d for _, d in matches) <= 32768
        if reach:
            assert far and all(d == 32768 for _, d in far) and sum(l for l, _ in far) >= 1000 - 256 - 4
        else:
            assert not far


def test_a_match_stops_at_the_block_s_end(twin):
    """the copy's source goes on behind the bytes that match; the match is cut where the block ends"""
    last = _token_list(_only_member(twin, "match_to_the_end"))[-1]
    assert last is not None and last[1] == 1300 and 4 <= last[0] <= 600 - 2 * 258, "the rest of the 600 bytes behind two longest matches"
    assert _token_list(_only_member(twin, "match_to_the_end_short"))[-1] == (5, 500)


def test_identical_blocks_give_identical_members(twin):
    out, csize, _ = twin["two_identical_blocks"]
    a, b = D.members_of(out, csize)
    assert a == b


# ---- the code-length routine -------------------------------------------------------------------------------------------------
def _lengths(emu, freq, limit):
    f = np.asarray(freq, np.uint32)
    out = np.full(f.size, 0xEE, np.uint8)
    assert emu.emu_code_lengths(f.ctypes.data, f.size, limit, out.ctypes.data) == 0
    return out.tolist()


def _fib(n, cap=60000):
    f = [1, 1]
    while len(f) < n:
        f.append(min(f[-1] + f[-2], cap))               # (a block has at most 0xFF00 + 1 symbols: the counts stop growing there)
    return f[:n]


@pytest.mark.parametrize("nsym,limit", [(286, 15), (30, 15), (19, 7)])
def test_code_lengths_of_fibonacci_counts(emu, nsym, limit):
    for freq in (_fib(nsym), _fib(nsym)[::-1], [f if k % 3 else 0 for k, f in enumerate(_fib(nsym))], [1] * nsym, [0] * (nsym - 2) + [5, 7]):
        ln = _lengths(emu, freq, limit)
        assert max(ln) <= limit
        assert all((l == 0) == (f == 0) for l, f in zip(ln, freq)), "no code for a symbol that does not occur, one for each that does"
        assert sum(Fraction(1, 1 << l) for l in ln if l) == 1, "a complete code"
        # never a longer code for the more frequent of two symbols
        used = sorted((f, -l) for f, l in zip(freq, ln) if f)
        assert all(a[1] <= b[1] for a, b in zip(used, used[1:]) if a[0] < b[0])
    # where the limit does not bind, the lengths are Huffman's: the cost equals the optimum
    freq = [3, 1, 4, 1, 5, 9, 2, 6, 5, 3, 5, 8, 9, 7, 9, 3, 2, 3, 8][:nsym]
    ln = _lengths(emu, freq + [0] * (nsym - len(freq)), limit)
    heap, cost = sorted(freq), 0
    while len(heap) > 1:
        s = heap[0] + heap[1]
        cost += s
        heap = sorted([s] + heap[2:])
    assert sum(f * l for f, l in zip(freq, ln)) == cost


@pytest.mark.parametrize("nsym,limit", [(286, 15), (30, 15), (19, 7)])
def test_code_lengths_of_one_and_of_no_symbol(emu, nsym, limit):
    """RFC 1951 3.2.7: one distance code is sent with one bit, not zero; no code at all is one code of zero bits"""
    assert _lengths(emu, [0] * nsym, limit) == [0] * nsym
    for s in (0, nsym // 2, nsym - 1):
        assert _lengths(emu, [9 if k == s else 0 for k in range(nsym)], limit) == [1 if k == s else 0 for k in range(nsym)]


def test_code_lengths_are_deterministic_in_their_ties(emu):
    """equal counts: the symbol order decides, and the same call gives the same lengths"""
    freq = [2, 2, 2, 1, 1, 1, 1, 4, 4]
    a = _lengths(emu, freq, 15)
    assert a == _lengths(emu, freq, 15) and sum(Fraction(1, 1 << l) for l in a) == 1


# ---- refusals and buffers ------------------------------------------------------------------------------------------------------
def test_nothing_is_written_behind_the_output():
    data = D.fixture_payload()[:100_000]
    out = np.full(D.bound(len(data), D.BLK) + 64, 0xA5, np.uint8)
    got, csize, stored = api.bgzf_deflate_host(data, D.BLK, out=out)
    assert len(got) < len(data) and (out[len(got):] == 0xA5).all()
    D.check_members(data, D.BLK, got, csize, stored)


def test_refusals():
    data = D.fixture_payload()[:100_000]
    need = D.bound(len(data), D.BLK)
    assert api.bgzf_deflate_bound(len(data), D.BLK) == need == len(data) + 2 * 31
    out = np.full(need, 0xA5, np.uint8)
    with pytest.raises(api.StrlingError) as e:
        api.bgzf_deflate_host(data, D.BLK, out=out[:need - 1])
    assert e.value.code == -4 and (out == 0xA5).all()                   # STRL_ERR_CAPACITY
    for block in (0, 0xFF01):
        with pytest.raises(api.StrlingError) as e:
            api.bgzf_deflate_host(data, block, out=out)
        assert e.value.code == -3 and (out == 0xA5).all()               # STRL_ERR_ARG


# ---- the twin as a stand-alone program under the sanitizers -----------------------------------------------------------------------
def test_standalone_program_under_asan_and_ubsan():
    """tests/emu/deflate_cases_main.cpp: the same shapes in buffers exact to the byte, every member through zlib"""
    out = os.path.join(HERE, "emu", "deflate_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "deflate_cases_main")
    src = os.path.join(HERE, "emu", "deflate_cases_main.cpp")
    core = os.path.join(HERE, "..", "strling_amd", "csrc", "deflate_core.h")
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(f) for f in (src, core)):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, src, "-lz"])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "all cases passed" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ---- size --------------------------------------------------------------------------------------------------------------------
def test_size_against_zlib_level_1():
    """a compressor that stores everything, or parses badly, does not pass: the DEFLATE payloads of the 19 blocks of a BAM's
    payload are at most 1.10 x zlib level 1's over the same cuts (measured: 0.993 x; level 6 is 0.862 x level 1)"""
    p = D.fixture_payload()
    assert len(p) == 1_190_664
    out, csize, stored = api.bgzf_deflate_host(p)
    assert csize.size == 19 and stored == 0
    mine = int(csize.sum()) - 26 * csize.size
    level1 = 0
    for o in range(0, len(p), D.BLK):
        c = zlib.compressobj(1, zlib.DEFLATED, -15)
        level1 += len(c.compress(p[o:o + D.BLK]) + c.flush())
    print(f"deflate payload bytes: twin {mine}, zlib level 1 {level1}, ratio {mine / level1:.4f}")
    assert mine <= 1.10 * level1
    D.check_members(p, D.BLK, out, csize, stored)
