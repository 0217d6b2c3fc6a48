"""The host side of every region read (strling_amd/csrc/cli/region_feed.cpp: the block planner, the layout of the block tables,
the read of the compressed runs, the host's stand-in for the device's walk) on its own: a stand-alone program
(tests/emu/region_feed_driver.cpp) built with AddressSanitizer and UBSan plans regions, lays them all out in one RegionBlocks and
reads them into a malloc'ed buffer of exactly the size `strling call` allocates at the least, and what it laid out is compared
with Python's own reading of the file.  CPU only."""
import bisect
import os
import shutil
import struct
import subprocess
import zlib
from concurrent.futures import ThreadPoolExecutor

import pytest

from strling_amd import bamio, synth

HERE = os.path.dirname(os.path.abspath(__file__))
CLI = os.path.join(HERE, "..", "strling_amd", "csrc", "cli")
SOURCES = [os.path.join(HERE, "emu", "region_feed_driver.cpp")] + [os.path.join(CLI, s) for s in (
    "region_feed.cpp", "bam_reader.cpp", "fast_inflate.cpp", "cram_reader.cpp", "cram_codecs.cpp")]
FLAGS = ["-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-I" + CLI]
CONTIG = 11 * 16384 + 6500     # the reads end ~5000 bases short of it: the last 16 KiB window holds a few blocks of them
EMPTY_TID = 3           # a reference without records, behind the three that have some


@pytest.fixture(scope="module")
def driver():
    out = os.path.join(HERE, "emu", "region_feed_build")
    exe = os.path.join(out, "region_feed_driver")
    deps = SOURCES + [os.path.join(CLI, h) for h in os.listdir(CLI) if h.endswith(".h")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(d) for d in deps):
        os.makedirs(out, exist_ok=True)
        objs = [os.path.join(out, os.path.basename(s)[:-4] + ".o") for s in SOURCES]
        with ThreadPoolExecutor(len(SOURCES)) as ex:
            list(ex.map(lambda so: subprocess.check_call(["g++"] + FLAGS + ["-c", so[0], "-o", so[1]]), zip(SOURCES, objs)))
        subprocess.check_call(["g++"] + FLAGS + ["-o", exe] + objs + ["-lz", "-lpthread"])
    return exe


class Scan:
    """Python's own reading of a BAM: its BGZF blocks [(file offset, gzip header bytes, block bytes, inflated bytes)], empty ones
    included, and of the inflated stream the records [(tid, pos, end, name, flag)] and their offsets"""
    def __init__(self, path):
        self.path = path
        self.raw = raw = open(path, "rb").read()
        self.blocks, o = [], 0
        while o < len(raw):
            xlen = struct.unpack_from("<H", raw, o + 10)[0]
            bsize = struct.unpack_from("<H", raw, o + 16)[0] + 1
            self.blocks.append((o, 12 + xlen, bsize, zlib.decompress(raw[o + 12 + xlen:o + bsize - 8], -15)))
            o += bsize
        self.at = {b[0]: k for k, b in enumerate(self.blocks)}
        self.ustart = [0]                                      # offset of block k in the inflated stream
        for b in self.blocks:
            self.ustart.append(self.ustart[-1] + len(b[3]))
        infl = b"".join(b[3] for b in self.blocks)
        q = 8 + struct.unpack_from("<i", infl, 4)[0]
        n_ref, = struct.unpack_from("<i", infl, q)
        q += 4
        for _ in range(n_ref):
            q += 8 + struct.unpack_from("<i", infl, q)[0]
        self.records, self.rec_off = records_of(infl[q:], q)
        self.rec_off.append(len(infl))


def records_of(b, base=0):
    """BAM records back to back -> [(tid, pos, end, name, flag)], [offset]; end by the rule of `strling _region`"""
    out, offs, p = [], [], 0
    while p < len(b):
        bs, tid, pos, l_name, _mapq, _bin, n_cig, flag = struct.unpack_from("<iiiBBHHH", b, p)
        cig = struct.unpack_from(f"<{n_cig}I", b, p + 36 + l_name)
        rl = 0 if flag & 4 else sum(c >> 4 for c in cig if (c & 15) in (0, 2, 3, 7, 8))
        out.append((tid, pos, pos + (rl or 1), b[p + 36:p + 36 + l_name - 1], flag))
        offs.append(base + p)
        p += 4 + bs
    assert p == len(b)
    return out, offs


def write_indexed(path, rec, block):
    bamio.write_bam(path, rec, block=block)
    return Scan(path)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """plain: three references with records and one without; its block size is chosen so that the first record of some 16 KiB
    window starts a block (the index offset of a region there has in_block 0).  holes: the same with empty blocks spliced in
    mid-file, two of them side by side, and the index written for the new block offsets.  tiny: two short references in blocks of 48
    inflated bytes, several thousand to a 16 KiB window."""
    d = tmp_path_factory.mktemp("region_feed")
    rec, _ = synth.synth_wgs(3000, seed=5, n_contigs=3, contig_len=CONTIG, unmapped_frac=0)     # (no tail: the file ends soon behind the last window)
    rec.targets = list(rec.targets) + [("empty", 50_000)]
    S = write_indexed(str(d / "probe.bam"), rec, 1200)
    first = {}                                                 # (tid, window) -> offset of the first record overlapping it
    for (tid, pos, end, _, _), off in zip(S.records, S.rec_off):
        for w in range(pos >> 14, ((end - 1) >> 14) + 1):
            first.setdefault((tid, w), off)
    block, aligned = next((b, tw) for b in range(900, 2000) for tw, off in sorted(first.items()) if off % b == 0 and 0 < tw[1] < 10)
    plain = write_indexed(str(d / "plain.bam"), rec, block)
    assert 200 < len(plain.blocks) < 3000 and plain.blocks[-1][3] == b"" and all(b[3] for b in plain.blocks[:-1])
    # holes: empty blocks in front of data blocks k0 and k1 (both inside reference 1), the index for the new block offsets
    mid = sorted({bisect.bisect_right(plain.ustart, off) - 1 for r, off in zip(plain.records, plain.rec_off) if r[0] == 1 and 90_000 < r[1] < 110_000})
    k0, k1 = mid[2], mid[5]
    cuts = [plain.blocks[k0][0], plain.blocks[k1][0]]
    holes_path = str(d / "holes.bam")
    with open(holes_path, "wb") as f:
        f.write(plain.raw[:cuts[0]] + bamio._EOF + plain.raw[cuts[0]:cuts[1]] + bamio._EOF * 2 + plain.raw[cuts[1]:])
    shift = lambda o: o + 28 * (o >= cuts[0]) + 56 * (o >= cuts[1])
    bamio.write_bai(holes_path + ".bai", rec, plain.rec_off, [shift(b[0]) for b in plain.blocks], block)
    holes = Scan(holes_path)
    assert [r[:2] for r in holes.records] == [r[:2] for r in plain.records] and sum(1 for b in holes.blocks if not b[3]) == 4
    small, _ = synth.synth_wgs(2400, seed=6, n_contigs=2, contig_len=40_000)
    tiny = write_indexed(str(d / "tiny.bam"), small, 48)
    return dict(dir=d, plain=plain, holes=holes, tiny=tiny, aligned=aligned)


def run(driver, path, more, regions, out):
    r = subprocess.run([driver, path, str(more), out] + [f"{t}:{b}:{e}" for t, b, e in regions], capture_output=True, text=True)
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
    assert r.returncode == 0, (r.returncode, r.stderr)
    d = open(out, "rb").read()
    n_regions, n_blocks, comp_bytes, inflated, read_ok = struct.unpack_from("<5q", d, 0)
    o = 40
    rows = [struct.unpack_from("<QIII", d, o + 20 * k) for k in range(n_blocks)]
    o += 20 * n_blocks
    comp = d[o:o + comp_bytes]
    o += comp_bytes
    out_regions = []
    for reg in regions:
        ok, c_beg, c_end, plan_blocks = struct.unpack_from("<4q", d, o)
        o += 32
        R = dict(region=reg, ok=ok, c_beg=c_beg, c_end=c_end, plan_blocks=plan_blocks)
        if ok:
            R.update(zip(("first_block", "n_blocks", "in_block", "file_off", "len", "at", "bad", "stopped", "keep", "stop", "u_size"), struct.unpack_from("<11q", d, o)))
            o += 88
            if R["stopped"]:
                R["bytes"] = d[o:o + R["stop"] - R["keep"]]
                o += len(R["bytes"])
        out_regions.append(R)
    assert o == len(d) and n_regions == len(regions) and read_ok == 1
    return dict(rows=rows, comp=comp, comp_bytes=comp_bytes, inflated=inflated, regions=out_regions)


def check_layout(S, D):
    """the tables and the buffer against the file; returns the planned regions"""
    rows, comp, planned = D["rows"], D["comp"], [R for R in D["regions"] if R["ok"]]
    assert len(comp) == D["comp_bytes"] and D["inflated"] == sum(r[2] for r in rows)
    for coff, clen, isize, crc in rows:                        # every slice is a raw deflate stream of isize bytes with that CRC
        assert coff + clen <= len(comp)
        infl = zlib.decompress(comp[coff:coff + clen], -15)
        assert len(infl) == isize and zlib.crc32(infl) == crc
    at, nb = 0, 0
    for R in planned:                                          # runs in the order added: 16-byte aligned, none overlapping
        assert R["at"] == at and at % 16 == 0 and R["first_block"] == nb and R["n_blocks"] == R["plan_blocks"] > 0
        assert R["first_block"] + R["n_blocks"] <= len(rows) and R["in_block"] <= rows[R["first_block"]][2]
        assert R["file_off"] == R["c_beg"] and R["len"] == R["c_end"] - R["c_beg"]
        assert comp[at:at + R["len"]] == S.raw[R["c_beg"]:R["c_end"]]
        k, o = S.at[R["c_beg"]], 0                             # the run is whole file blocks, from the one the index offset is in
        for coff, clen, isize, crc in rows[nb:nb + R["n_blocks"]]:
            boff, hdr, bsize, infl = S.blocks[k]
            assert coff == at + o + hdr and clen == bsize - hdr - 8 and isize == len(infl)
            k, o = k + 1, o + bsize
        assert o == R["len"] and S.ustart[S.at[R["c_beg"]]] + R["in_block"] in S.rec_off      # ... at a record's start
        at, nb = at + (R["len"] + 15) // 16 * 16, nb + R["n_blocks"]
    assert at == D["comp_bytes"] and nb == len(rows)
    return planned


def check_walk(S, R):
    tid, beg, end = R["region"]
    assert R["bad"] == 0 and R["stopped"] == 1, R["region"]
    got = [r for r in records_of(R["bytes"])[0] if r[0] == tid and r[1] < end and r[2] > beg]
    assert got == [r for r in S.records if r[0] == tid and r[1] < end and r[2] > beg], R["region"]
    return got


def test_regions_of_one_layout(driver, files):
    S, (atid, aw) = files["plain"], files["aligned"]
    regions = [(atid, (aw << 14) + 10, (aw << 14) + 900),                       # its index offset starts a block
               (0, 0, 500), (1, 16_300, 16_400), (1, 150_000, 150_001), (0, 100_000, 140_000), (2, 0, 1), (1, 16_000, 33_000),
               (1, 30_000, 40_000), (1, 40_000, 50_000),                       # neighbours: the boundary's blocks are in both runs
               (1, 40_000, 50_000),                                             # ... and the same blocks once more
               (EMPTY_TID, 100, 5000),                                          # a reference without records
               (2, CONTIG - 3000, CONTIG + 500)]                                # the index has no later window: the host reader's
    regions += [(t, a, a + 700) for t in range(3) for a in range(5_000, 150_000, 23_000)]       # more than one group of 16
    D = run(driver, S.path, 1, regions, str(files["dir"] / "plain.dump"))
    planned = check_layout(S, D)
    assert [R["ok"] for R in D["regions"][10:12]] == [0, 0] and len(planned) == len(regions) - 2 > 16
    assert planned[0]["in_block"] == 0 and sum(1 for R in planned if R["in_block"] > 0) > 16
    a, b, c = D["regions"][7:10]
    assert a["c_beg"] < b["c_beg"] < a["c_end"] and (b["c_beg"], b["c_end"]) == (c["c_beg"], c["c_end"]) and b["at"] != c["at"]
    assert sum(len(check_walk(S, R)) for R in planned) > 500


def test_a_run_that_ends_with_the_file(driver, files):
    S = files["plain"]
    D = run(driver, S.path, 8, [(2, 170_000, 175_000), (1, 16_300, 16_400)], str(files["dir"] / "tail.dump"))
    last, other = check_layout(S, D)
    assert last["c_end"] == len(S.raw) and D["rows"][last["n_blocks"] - 1][1:3] == (2, 0)      # up to and with the EOF block
    assert other["c_end"] < len(S.raw)
    assert check_walk(S, last)
    check_walk(S, other)


def test_empty_blocks_inside_a_run(driver, files):
    S = files["holes"]
    D = run(driver, S.path, 1, [(1, 85_000, 115_000), (1, 99_000, 101_000), (0, 100_000, 140_000)], str(files["dir"] / "holes.dump"))
    planned = check_layout(S, D)
    assert len(planned) == 3
    rows = D["rows"][planned[0]["first_block"]:][:planned[0]["n_blocks"]]
    assert [r[1:3] for r in rows].count((2, 0)) == 3 and rows[0][2] > 0 and rows[-1][2] > 0
    assert all(check_walk(S, R) for R in planned)


def test_the_block_cap(driver, files):
    S = files["tiny"]
    region = (0, 100, 200)
    want = [r for r in S.records if r[0] == 0 and r[1] < 200 and r[2] > 100]
    # the file really holds more than 4096 and fewer than 32768 blocks from the window's first record to the next window's
    nxt = next(off for r, off in zip(S.records, S.rec_off) if r[0] == 0 and r[2] > 16384)
    n_run = sum(1 for k in range(len(S.blocks)) if S.ustart[k + 1] > S.rec_off[0] and S.ustart[k] <= nxt)
    assert 4096 < n_run < 32768 - 16 and want
    D = run(driver, S.path, 1, [region], str(files["dir"] / "cap1.dump"))
    assert D["regions"][0]["plan_blocks"] == 4096
    for R in check_layout(S, D):                               # not planned, or cut at the cap before the query's end
        assert not R["stopped"]
    D = run(driver, S.path, 8, [region], str(files["dir"] / "cap8.dump"))
    R, = check_layout(S, D)
    assert n_run <= R["n_blocks"] <= n_run + 16 and check_walk(S, R) == want


@pytest.mark.parametrize("damage", ["header", "truncated"])
def test_a_damaged_run_is_not_planned(driver, files, damage):
    S, d = files["plain"], files["dir"]
    regions = [(0, 100_000, 101_000), (1, 50_000, 52_000)]
    good = run(driver, S.path, 1, regions, str(d / "good.dump"))["regions"]
    k = S.at[good[1]["c_beg"]] + 2                             # the third block of the second region's run
    assert good[1]["plan_blocks"] > 3 and good[0]["c_end"] < good[1]["c_beg"]
    boff, hdr = S.blocks[k][:2]
    path = str(d / f"{damage}.bam")
    with open(path, "wb") as f:
        f.write(S.raw[:boff] + b"\0" + S.raw[boff + 1:] if damage == "header" else S.raw[:boff + hdr + 5])
    shutil.copy(S.path + ".bai", path + ".bai")
    D = run(driver, path, 1, regions, str(d / f"{damage}.dump"))
    planned = check_layout(S, D)                               # (the first region's run lies in front of the damage)
    assert [R["ok"] for R in D["regions"]] == [1, 0] and len(planned) == 1 and check_walk(S, planned[0])
