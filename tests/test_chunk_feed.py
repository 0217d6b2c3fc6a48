"""The host side of every device pass over a BAM (strling_amd/csrc/cli/chunk_feed.cpp: stage_chunk, the read-ahead ring, the
fragment-length accumulator) on its own: a stand-alone program (tests/emu/chunk_feed_driver.cpp) built with AddressSanitizer and
UBSan stages whole files chunk by chunk into malloc'ed buffers of exactly the size the callers allocate, and what it staged is
compared with Python's own reading of the file.  CPU only."""
import os
import struct
import subprocess
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from strling_amd import bamio, synth

HERE = os.path.dirname(os.path.abspath(__file__))
CLI = os.path.join(HERE, "..", "strling_amd", "csrc", "cli")
SOURCES = [os.path.join(HERE, "emu", "chunk_feed_driver.cpp")] + [os.path.join(CLI, s) for s in (
    "chunk_feed.cpp", "bgzf_feed.cpp", "bam_reader.cpp", "fast_inflate.cpp", "cram_reader.cpp", "cram_codecs.cpp")]
FLAGS = ["-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-I" + CLI]
BLOCK = 1200            # inflated bytes per BGZF block: a few thousand records make a few hundred blocks


@pytest.fixture(scope="module")
def driver():
    out = os.path.join(HERE, "emu", "chunk_feed_build")
    exe = os.path.join(out, "chunk_feed_driver")
    deps = SOURCES + [os.path.join(CLI, h) for h in os.listdir(CLI) if h.endswith(".h")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(d) for d in deps):
        os.makedirs(out, exist_ok=True)
        objs = [os.path.join(out, os.path.basename(s)[:-4] + ".o") for s in SOURCES]
        with ThreadPoolExecutor(len(SOURCES)) as ex:
            list(ex.map(lambda so: subprocess.check_call(["g++"] + FLAGS + ["-c", so[0], "-o", so[1]]), zip(SOURCES, objs)))
        subprocess.check_call(["g++"] + FLAGS + ["-o", exe] + objs + ["-lz", "-lpthread"])
    return exe


def run(driver, *args, ok=(0,)):
    r = subprocess.run([driver] + [str(a) for a in args], capture_output=True, text=True)
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
    assert r.returncode in ok, (r.returncode, r.stderr)
    return r


def blocks_of(path):
    """[(file offset, gzip header bytes, inflated bytes)] of every BGZF block of the file, empty ones included"""
    raw = open(path, "rb").read()
    out, o = [], 0
    while o < len(raw):
        xlen = struct.unpack_from("<H", raw, o + 10)[0]
        bsize = struct.unpack_from("<H", raw, o + 16)[0] + 1
        out.append((o, 12 + xlen, zlib.decompress(raw[o + 12 + xlen:o + bsize - 8], -15)))
        o += bsize
    return raw, out


def first_record(infl):
    l_text, = struct.unpack_from("<i", infl, 4)
    q = 8 + l_text
    n_ref, = struct.unpack_from("<i", infl, q)
    q += 4
    for _ in range(n_ref):
        q += 8 + struct.unpack_from("<i", infl, q)[0]
    return q


def read_dump(path):
    """chunks of the driver's dump: dicts of nb, lo, hi, last, short_read, blocks = [(boff, coff, clen, isz, crc, inflated)]"""
    d = open(path, "rb").read()
    chunks, o = [], 0
    while o < len(d):
        nb, lo, hi, last, short = struct.unpack_from("<5q", d, o)
        o += 40
        blocks = []
        for _ in range(max(nb, 0)):
            boff, coff, clen, isz, crc, got = struct.unpack_from("<QQIIII", d, o)
            o += 32
            blocks.append((boff, coff, clen, isz, crc, d[o:o + got]))
            o += got
        chunks.append(dict(nb=nb, lo=lo, hi=hi, last=last, short_read=short, blocks=blocks))
    return chunks


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """plain: ends in the empty block only; holes: the same with empty blocks spliced in mid-file, two of them side by side
    (bamio's writer makes no empty block but the last, so the test splices them in itself; that file has no index)"""
    d = tmp_path_factory.mktemp("chunk_feed")
    rec, _ = synth.synth_wgs(3000, seed=5, contig_len=300_000)
    plain = str(d / "plain.bam")
    bamio.write_bam(plain, rec, block=BLOCK)
    raw, blocks = blocks_of(plain)
    assert 300 < len(blocks) < 3000 and blocks[-1][2] == b"" and all(b[2] for b in blocks[:-1])
    holes = str(d / "holes.bam")
    cuts = [blocks[len(blocks) // 3][0], blocks[len(blocks) // 2][0]]
    with open(holes, "wb") as f:
        f.write(raw[:cuts[0]] + bamio._EOF + raw[cuts[0]:cuts[1]] + bamio._EOF * 2 + raw[cuts[1]:])
    return dict(dir=d, plain=plain, holes=holes)


def check_staged(path, chunks, max_blocks, max_bytes):
    raw, blocks = blocks_of(path)
    assert chunks[-1]["nb"] == 0 and all(c["nb"] > 0 for c in chunks[:-1])
    assert not any(c["short_read"] for c in chunks)
    staged = [b for c in chunks for b in c["blocks"]]
    start = next(k for k, b in enumerate(blocks) if b[0] == staged[0][0])          # the block the feed starts at
    q = first_record(b"".join(b[2] for b in blocks))
    before = sum(len(b[2]) for b in blocks[:start])
    assert before <= q < before + len(blocks[start][2])                           # ... is the one the first record is in
    assert b"".join(b[5] for b in staged) == b"".join(b[2] for b in blocks[start:])
    assert len(staged) == sum(1 for b in blocks[start:] if b[2])                  # every non-empty block once, no empty one
    hdr = {b[0]: b[1] for b in blocks}
    for c in chunks[:-1]:
        assert c["nb"] <= max_blocks and c["hi"] - c["lo"] <= max_bytes
        assert c["hi"] == c["blocks"][-1][0] + hdr[c["blocks"][-1][0]] + c["blocks"][-1][2]      # the last payload's end: CRC-32 and ISIZE follow
        for boff, coff, clen, isz, crc, infl in c["blocks"]:
            assert crc == zlib.crc32(infl) and isz == len(infl)
            assert raw[boff:boff + 2] == b"\x1f\x8b" and boff + hdr[boff] == c["lo"] + coff
    return staged


@pytest.mark.parametrize("which", ["plain", "holes"])
@pytest.mark.parametrize("max_blocks,max_bytes", [(1, 1 << 20), (2, 1 << 20), (3, 1 << 20), (7, 1 << 20), (100000, 1 << 20), (100000, 4000)])
def test_staged_chunks_are_the_file(driver, files, which, max_blocks, max_bytes):
    path, d = files[which], files["dir"]
    dumps = []
    for ahead in (1, 0):
        out = str(d / f"{which}.{max_blocks}.{max_bytes}.{ahead}.dump")
        run(driver, "stage", path, max_blocks, max_bytes, ahead, out)
        dumps.append(open(out, "rb").read())
    assert dumps[0] == dumps[1]                                  # the read-ahead thread changes nothing
    chunks = read_dump(out)
    check_staged(path, chunks, max_blocks, max_bytes)
    if max_bytes < 1 << 20:                                      # the byte cap, not the block cap, ended the chunks
        assert len(chunks) > 10 and max(c["nb"] for c in chunks) > 1 and all(c["nb"] < max_blocks for c in chunks)
    elif max_blocks > 1000:
        assert len(chunks) == 2
    else:
        assert all(c["nb"] == max_blocks for c in chunks[:-2])


@pytest.mark.parametrize("max_blocks", [1, 5, 100000])
def test_two_shares_tile_the_records(driver, files, max_blocks):
    path, d = files["plain"], files["dir"]
    outs = [str(d / f"share{k}.{max_blocks}.dump") for k in (0, 1)]
    r = run(driver, "shares", path, max_blocks, 1 << 20, *outs)
    words = r.stdout.split()
    first_off, cut_uoff, trim0, trim1 = int(words[1]), int(words[3]), int(words[5]), int(words[6])
    shares = [read_dump(o) for o in outs]
    for chunks in shares:
        assert [c["last"] for c in chunks[:-1]] == [0] * (len(chunks) - 2) + [1]      # `last` on exactly the final chunk
        assert not any(c["short_read"] for c in chunks) and all(c["nb"] <= max_blocks for c in chunks)
    a, b = (b"".join(blk[5] for c in chunks for blk in c["blocks"]) for chunks in shares)
    _, blocks = blocks_of(path)
    infl = b"".join(blk[2] for blk in blocks)
    assert trim1 == 0 and (trim0 > 0) == (cut_uoff > 0)
    assert a[first_off:len(a) - trim0] + b[cut_uoff:] == infl[first_record(infl):]


def test_a_truncated_file_is_reported(driver, files):
    raw, blocks = blocks_of(files["plain"])
    mid = blocks[len(blocks) // 2]
    path = str(files["dir"] / "cut.bam")
    with open(path, "wb") as f:
        f.write(raw[:mid[0] + mid[1] + 7])                         # in the middle of a block's payload
    for max_blocks in (1, 7, 100000):
        out = str(files["dir"] / f"cut.{max_blocks}.dump")
        run(driver, "stage", path, max_blocks, 1 << 20, 1, out)
        chunks = read_dump(out)
        assert chunks[-1]["nb"] < 0 or chunks[-1]["short_read"], chunks[-1]
        assert all(c["nb"] > 0 and not c["short_read"] for c in chunks[:-1])


def frag_model(flag, isize):
    """fragment_length_distribution, utils.nim:86-111"""
    ok = np.flatnonzero(((flag & 0x2) != 0) & ((flag & 0x900) == 0) & (isize >= 0) & (isize <= 4095))
    late = ok[ok >= 100000][:2000001]                 # the count stops behind the 2 000 001st
    hist = np.bincount(isize[late], minlength=4096)
    if hist.sum() == 0:
        hist = np.bincount(isize[ok[ok < 100000]], minlength=4096)
    looked = int(late[-1]) + 1 if len(late) == 2000001 else len(flag)
    return hist.astype(np.uint32), looked


@pytest.mark.parametrize("n,all_eligible", [(60000, False), (100000, True), (100001, True), (2800000, False)])
def test_fragment_length_accumulator(driver, tmp_path, n, all_eligible):
    rng = np.random.default_rng(n)
    flag = rng.choice(np.array([0x63, 0x93, 0x43, 0x163, 0x863, 0x1], np.uint32), n, p=[0.45, 0.45, 0.04, 0.02, 0.02, 0.02])
    isize = rng.integers(-300, 4400, n).astype(np.int32)
    if all_eligible:
        flag[:] = 0x63
        isize = np.abs(isize) % 4096
    isize = isize.astype(np.int32)
    rec = np.empty((n, 2), np.uint32)
    rec[:, 0] = flag
    rec[:, 1] = isize.view(np.uint32)
    src, out = str(tmp_path / "rec.bin"), str(tmp_path / "frag.bin")
    rec.tofile(src)
    r = run(driver, "frag", src, out)
    want, looked = frag_model(flag, isize)
    assert (np.fromfile(out, np.uint32) == want).all()
    assert int(r.stdout.split()[1]) == looked
    fell_back = "using first reads in fragment_length_distribution calculation as there were not enough" in r.stderr
    assert fell_back == (n <= 100000) and want.sum() > 0
    if n > 2100000:
        assert looked < n                                  # stopped early
