"""Inputs of the BGZF compressor's tests (strling_amd/csrc/deflate_core.h) and the checks every output must pass; shared by
tests/test_deflate_cases.py (the host twin) and tests/test_deflate_device.py (the kernel).  The inputs are the smallest shapes at
which the rule can go wrong: lengths around a batch of 256 positions and around a block, matches across batches, at the distance
limit and at the block's end, one or no distance code, literal counts that make a Huffman tree deeper than 15."""
import functools
import gzip
import struct
import zlib

import numpy as np

BLK = 0xFF00
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def bound(n, block):
    return (n // block) * (block + 31) + ((n % block + 31) if n % block else 0)


def _rng(seed):
    return np.random.default_rng(seed)


def _no_repeated_4gram(n):
    """n bytes in which no 4 bytes occur twice: a counter in the first two of every four bytes"""
    out = bytearray()
    k = 0
    while len(out) < n:
        out += struct.pack("<HBB", k, 0xF0 | (k & 7), 0xE1)
        k += 1
    out = bytes(out[:n])
    grams = [out[i:i + 4] for i in range(len(out) - 3)]
    assert len(set(grams)) == len(grams)
    return out


def _fibonacci_literals():
    """literal counts 1, 1, 2, 3, 5, ...: 4180 bytes over 18 symbols; a plain Huffman tree of them is 17 deep"""
    f, out = [1, 1], bytearray()
    while sum(f) < 4180:
        f.append(f[-1] + f[-2])
    for s, c in enumerate(f):
        out += bytes([65 + s]) * c
    perm = _rng(5).permutation(len(out))                    # spread, so that few 4-grams repeat and the literals stay literals
    return bytes(np.frombuffer(bytes(out), np.uint8)[perm])


@functools.lru_cache(maxsize=None)
def cases():
    """-> tuple of (name, data, block_bytes)"""
    r = _rng(11)
    rnd = lambda n: bytes(r.integers(0, 256, n, dtype=np.uint8))
    text = lambda n: bytes(r.choice(np.frombuffer(b"ACGTN", np.uint8), n))
    c = []
    for n in (0, 1, 3, 4, 5):
        c.append((f"len{n}", text(n), BLK))
    for b in (1, 255, 256, 257):
        c.append((f"block{b}_exact", text(b), b))
        c.append((f"block{b}_plus1", text(b + 1), b))
        c.append((f"block{b}_five", (b"GATTACA" * 200)[:5 * b], b))
    seq = text(BLK + 1)
    c.append(("full_block", seq[:BLK], BLK))
    c.append(("full_block_plus1", seq, BLK))
    c.append(("zeros", b"\0" * BLK, BLK))                                   # 258-byte matches
    c.append(("zeros300", b"\0" * 300, BLK))                                # one match behind the first batch: a single distance code
    c.append(("one_literal", b"Q" * 200, BLK))                              # inside the first batch: no match, no distance code
    c.append(("no_repeated_4gram", _no_repeated_4gram(300), BLK))           # lookups that all miss: no distance code
    c.append(("random", rnd(BLK), BLK))                                     # stored
    c.append(("pattern600", (rnd(600) * 40)[:20_000], BLK))                 # matches from one batch into later ones
    piece = rnd(1000)
    c.append(("dist32768", piece + text(32768 - 1000) + piece + text(100), BLK))
    c.append(("dist32769", piece + text(32769 - 1000) + piece + text(100), BLK))
    c.append(("match_to_the_end", text(700) + piece + text(300) + piece[:600], BLK))   # the copy ends with the block
    c.append(("match_to_the_end_short", text(300) + piece[:400] + text(100) + piece[:5], BLK))
    two = text(3000) + piece
    c.append(("two_identical_blocks", two + two, len(two)))
    c.append(("fibonacci_literals", _fibonacci_literals(), BLK))
    return tuple(c)


def members_of(out, csize):
    res, at = [], 0
    for s in csize:
        res.append(out[at:at + int(s)])
        at += int(s)
    assert at == len(out)
    return res


def block_type(member):
    return (member[18] >> 1) & 3


def check_members(data, block, out, csize, n_stored):
    """every member on its own: header, BSIZE, the DEFLATE block alone gives the slice back, CRC-32, ISIZE; then the file through gzip"""
    n_blocks = (len(data) + block - 1) // block
    assert len(csize) == n_blocks and int(np.sum(csize, dtype=np.uint64)) == len(out)
    stored = 0
    for k, m in enumerate(members_of(out, csize)):
        want = data[k * block:(k + 1) * block]
        assert len(m) <= 65536 and len(m) <= len(want) + 31
        assert m[:16] == bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 66, 67, 2, 0])
        assert struct.unpack_from("<H", m, 16)[0] == len(m) - 1, "BSIZE"
        assert m[18] & 1 == 1 and block_type(m) in (0, 2), "one final block, stored or dynamic"
        d = zlib.decompressobj(-15)
        got = d.decompress(m[18:-8])
        assert d.eof and d.unused_data == b"" and got == want, f"member {k}"
        assert struct.unpack_from("<II", m, len(m) - 8) == (zlib.crc32(want) & 0xFFFFFFFF, len(want)), "CRC-32 / ISIZE"
        if block_type(m) == 0:
            stored += 1
            assert len(m) == len(want) + 31
        else:
            assert len(m) < len(want) + 31, "a dynamic block that is no smaller than the stored one"
    assert stored == n_stored
    assert gzip.decompress(out + EOF_BLOCK) == data


def dynamic_header(member):
    """(HLIT, HDIST, literal/length code lengths, distance code lengths) of a member's dynamic block, read bit by bit"""
    bits = int.from_bytes(member[18:-8], "little")
    at = 0

    def take(n):
        nonlocal at
        v = (bits >> at) & ((1 << n) - 1)
        at += n
        return v

    def decoder(lengths):
        code, tab = 0, {}
        for ln in range(1, 16):
            for s, l in enumerate(lengths):
                if l == ln:
                    tab[(ln, code)] = s
                    code += 1
            code <<= 1
        return tab

    def symbol(tab):
        code = 0
        for ln in range(1, 16):
            code = code << 1 | take(1)
            if (ln, code) in tab:
                return tab[(ln, code)]
        raise AssertionError("no code")

    assert take(1) == 1 and take(2) == 2
    hlit, hdist, hclen = take(5) + 257, take(5) + 1, take(4) + 4
    cl = [0] * 19
    for i in range(hclen):
        cl[(16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)[i]] = take(3)
    tab, lens = decoder(cl), []
    while len(lens) < hlit + hdist:
        s = symbol(tab)
        if s < 16:
            lens.append(s)
        elif s == 16:
            lens += [lens[-1]] * (3 + take(2))
        elif s == 17:
            lens += [0] * (3 + take(3))
        else:
            lens += [0] * (11 + take(7))
    assert len(lens) == hlit + hdist
    return hlit, hdist, lens[:hlit], lens[hlit:]


@functools.lru_cache(maxsize=None)
def fixture_payload():
    """a BAM's payload: 1 190 664 bytes, 19 blocks of 0xFF00"""
    from strling_amd import bamio, synth
    rec, _ = synth.synth_wgs(2000, seed=7, n_contigs=2, contig_len=20000, hot_loci=4)
    return bytes(bamio.serialize_records(rec, quals=True, aux=True, seed=3)[0])
