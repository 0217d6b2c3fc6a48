"""`strling pull` on the host path (STRL_PULL=host; csrc/pull_logic.cpp and the CLI's BAM writer) against a Python restatement of
extract_region.nim: the region forms, the merge of regions, the mate search on a reference and in the unplaced tail, the order
with refID == -1 first, and the output file checked block by block.  The restatement below reads the input BAM with zlib alone;
tests/test_pull_device.py shares it."""
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

from strling_amd import api, bamio, build, synth
from strling_amd.records import RecordBatch

CLI = build.CLI
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
INT32_MAX = 2**31 - 1


# ---- reading a BAM with zlib: every BGZF block inflated, its CRC-32 and ISIZE checked, the EOF block last -----------------------
def bgzf_payload(path, max_block=None):
    data = open(path, "rb").read()
    assert data.endswith(EOF_BLOCK), "no EOF block at the end"
    out, at = bytearray(), 0
    while at < len(data):
        assert data[at:at + 4] == b"\x1f\x8b\x08\x04" and data[at + 12:at + 16] == b"BC\x02\x00", f"not a BGZF block at {at}"
        bsize = struct.unpack_from("<H", data, at + 16)[0] + 1
        raw = zlib.decompress(data[at + 18:at + bsize - 8], -15)
        crc, isize = struct.unpack_from("<II", data, at + bsize - 8)
        assert zlib.crc32(raw) & 0xFFFFFFFF == crc and len(raw) == isize, f"CRC-32 / ISIZE of the block at {at}"
        if max_block is not None:
            assert isize <= max_block
        out += raw
        at += bsize
    assert at == len(data)
    return bytes(out)


class Rec:
    __slots__ = ("raw", "tid", "pos", "flag", "mtid", "mpos", "qname", "end", "u_off")

    def __init__(self, buf, at):
        bs, self.tid, self.pos, l_name, _, _, n_cig, self.flag, _, self.mtid, self.mpos = struct.unpack_from("<iiiBBHHHiii", buf, at)
        self.raw = buf[at:at + 4 + bs]
        self.u_off = at
        self.qname = buf[at + 36:at + 36 + l_name - 1]
        rl = 0
        if not self.flag & 4:
            for c in struct.unpack_from(f"<{n_cig}I", buf, at + 36 + l_name):
                if c & 15 in (0, 2, 3, 7, 8):
                    rl += c >> 4
        self.end = self.pos + (rl or 1)                        # bam_endpos


def parse_bam(path):
    """-> (header bytes, [Rec] in file order, reference names)"""
    u = bgzf_payload(path)
    assert u[:4] == b"BAM\1"
    l_text = struct.unpack_from("<i", u, 4)[0]
    at = 8 + l_text
    n_ref = struct.unpack_from("<i", u, at)[0]
    at += 4
    names = []
    for _ in range(n_ref):
        ln = struct.unpack_from("<i", u, at)[0]
        names.append(u[at + 4:at + 4 + ln - 1].decode())
        at += 8 + ln
    header, recs = u[:at], []
    while at < len(u):
        recs.append(Rec(u, at))
        at += len(recs[-1].raw)
    return header, recs, names


# ---- extract_region.nim, restated --------------------------------------------------------------------------------------------
def merge_regions(regions):
    out = []
    for tid, beg, end in sorted(regions):
        if out and out[-1][0] == tid and beg <= out[-1][2]:
            out[-1][2] = max(out[-1][2], end)
        else:
            out.append([tid, beg, end])
    return [tuple(r) for r in out]


def overlaps(r, tid, beg, end):
    return r.tid == tid and r.pos < end and r.end > beg       # htslib's iterator filter


def pull_expected(header, recs, n_ref, regions):
    """regions = [(tid, beg, end)], 0-based half-open -> (the output's inflated bytes, kept records, [qname of every request
    without a mate], requests)"""
    kept = [r for tid, beg, end in merge_regions(regions) for r in recs if overlaps(r, tid, beg, end) and not r.flag & 0x900]      # :46-48
    counts = {}
    for r in kept:
        counts[r.qname] = counts.get(r.qname, 0) + 1                                                                                # :50
    placed = [i for i, r in enumerate(recs) if r.tid >= 0]
    tail = recs[placed[-1] + 1:] if placed else recs
    mates, missing, requests = [], [], 0
    for r in kept:
        if counts[r.qname] == 2:                                                                                                    # :57
            continue
        requests += 1
        if r.mtid == -1:                                                                                                            # :8-9
            cand = tail
        elif 0 <= r.mtid < n_ref and r.mpos + 1 > max(0, r.mpos - 1):                                                               # :15
            cand = [o for o in recs if overlaps(o, r.mtid, max(0, r.mpos - 1), r.mpos + 1)]
        else:
            cand = []
        for o in cand:
            if not o.flag & 0x900 and (o.flag & 0x40) != (r.flag & 0x40) and o.qname == r.qname:                                   # :10-12, :16-18
                mates.append(o)
                break
        else:
            missing.append(r.qname)                                                                                                 # :20
    out = sorted(kept + mates, key=lambda r: (r.tid, r.pos))                                                                        # :63-68 (stable)
    return header + b"".join(r.raw for r in out), kept, missing, requests


# ---- hand-made records -------------------------------------------------------------------------------------------------------
class Recs:
    """a list of records to edit by hand; build() sorts them by (reference, position) with the unplaced ones last and packs them"""

    def __init__(self, targets):
        self.targets, self.rows = targets, []

    def add(self, qname, flag, tid, pos, mtid, mpos, cigar="50M", seq=None, mapq=60, isize=0):
        if seq is None:
            n = sum(int(c) >> 4 for c in _cig(cigar) if (int(c) & 15) in (0, 1, 4, 7, 8))
            seq = "ACGT" * (n // 4) + "ACGT"[:n % 4]
        self.rows.append((tid, pos, mtid, mpos, flag, mapq, cigar, seq, qname, isize))

    def add_synth(self, n_pairs, seed, keep=lambda tid, pos: True, **kw):
        rec, _ = synth.synth_wgs(n_pairs, seed=seed, n_contigs=len(self.targets), contig_len=min(l for _, l in self.targets) - 1000, **kw)
        for i in range(rec.n):
            if rec.tid[i] >= 0 and not keep(int(rec.tid[i]), int(rec.pos[i])):
                continue
            c0, c1 = int(rec.cigar_off[i]), int(rec.cigar_off[i + 1])
            self.rows.append((int(rec.tid[i]), int(rec.pos[i]), int(rec.mtid[i]), int(rec.mpos[i]), int(rec.flag[i]), int(rec.mapq[i]),
                              [int(c) for c in rec.cigar[c0:c1]], rec.sequence(i), b"s%d_" % seed + rec.qname(i), int(rec.isize[i])))

    def build(self):
        rows = sorted(self.rows, key=lambda r: (r[0] if r[0] >= 0 else 1 << 40, r[1]))
        c = list(zip(*rows))
        return RecordBatch.from_fields(c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7], c[8], isize=c[9], targets=self.targets)


def _cig(c):
    from strling_amd.records import encode_cigar
    return encode_cigar(c) if isinstance(c, str) else c


def run_pull(args, mode=None, **kw):
    env = dict(os.environ)
    env.pop("STRL_PULL", None)
    if mode:
        env["STRL_PULL"] = mode
    return subprocess.run([CLI, "pull"] + args, capture_output=True, text=True, env=env, **kw)


def check_output(path, expected, n_header_lines):
    """the three checks of the output: blocks (CRC-32, ISIZE, <= 0xFF00 bytes each, the EOF block), the bytes, the read back"""
    got = bgzf_payload(path, max_block=0xFF00)
    assert got == expected, f"{len(got)} bytes, {len(expected)} expected"
    r = subprocess.run([CLI, "_dump", path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    _, recs, _ = parse_payload(expected)
    assert len([l for l in r.stdout.split("\n") if l]) == n_header_lines + len(recs)
    return recs


def parse_payload(u):
    l_text = struct.unpack_from("<i", u, 4)[0]
    at = 8 + l_text
    n_ref = struct.unpack_from("<i", u, at)[0]
    at += 4
    for _ in range(n_ref):
        at += 8 + struct.unpack_from("<i", u, at)[0]
    header, recs = u[:at], []
    while at < len(u):
        recs.append(Rec(u, at))
        at += len(recs[-1].raw)
    return header, recs, n_ref


TARGETS = [("chrA", 70_000), ("chr:B", 70_000), ("chrA:100-200", 70_000)]


@pytest.fixture(scope="module")
def sample(tmp_path_factory):
    d = tmp_path_factory.mktemp("pull")
    R = Recs(TARGETS)
    R.add_synth(400, seed=31)
    # a pair whose mate is unplaced and sits in the tail, behind a supplementary copy and a record with the same 0x40 bit (rule 4)
    R.add("tailpair", 0x49, 0, 30_000, -1, -1)
    R.add("tailpair", 0x845, -1, -1, 0, 30_000, cigar="", seq="ACGTACGT")
    R.add("tailpair", 0x45, -1, -1, 0, 30_000, cigar="", seq="ACGTACGTAC")
    R.add("tailpair", 0x85, -1, -1, 0, 30_000, cigar="", seq="ACGTACGTACGT")
    R.add("tailpair", 0x85, -1, -1, 0, 30_000, cigar="", seq="ACGT")
    R.add("notail", 0x49, 0, 30_010, -1, -1)               # asks the tail and finds nothing
    R.add("zzz_unplaced_pair", 0x4d, -1, -1, -1, -1, cigar="", seq="ACGT")
    rec = R.build()
    bam = str(d / "in.bam")
    hdr = bamio.write_bam(bam, rec, block=3000)
    header, recs, names = parse_bam(bam)
    assert names == [t[0] for t in TARGETS] and len(recs) == rec.n
    # the same records without the unplaced tail
    placed = Recs(TARGETS)
    placed.rows = [r for r in R.rows if r[0] >= 0]
    bam2 = str(d / "placed.bam")
    bamio.write_bam(bam2, placed.build(), block=3000)
    return dict(dir=d, bam=bam, bam2=bam2, header=header, recs=recs, n_hdr=len(hdr.rstrip("\n").split("\n")))


def _pull_and_check(sample, args, regions, bam=None, tag="o"):
    out = str(sample["dir"] / f"{tag}.bam")
    bam = bam or sample["bam"]
    r = run_pull(["-o", out, bam] + args, mode="host")
    assert r.returncode == 0, r.stderr
    header, recs, names = (sample["header"], sample["recs"], None) if bam == sample["bam"] else parse_bam(bam)
    exp, kept, missing, _ = pull_expected(header, recs, len(TARGETS), regions)
    got = check_output(out, exp, sample["n_hdr"])
    assert f"extracted {len(kept)} alignments. now checking for mates" in r.stderr
    assert [l[len("skipping pair. mate not found for "):].encode() for l in r.stderr.split("\n") if l.startswith("skipping pair")] == missing
    return got, kept, missing, r


@pytest.mark.parametrize("region,expect", [("chrA", (0, 0, INT32_MAX)), ("chrA:20001", (0, 20_000, INT32_MAX)), ("chrA:20,001-31,000", (0, 20_000, 31_000)),
                                           ("chrA:1-1", (0, 0, 1))], ids=["name", "name-beg", "name-beg-end-commas", "first-base"])
def test_region_forms(sample, region, expect):
    got, kept, _, _ = _pull_and_check(sample, [region], [expect])
    assert region != "chrA" or len(kept) > 200


def test_reference_names_with_colons(sample):
    """a string that is a reference's name as a whole is that reference; otherwise the part behind the last colon is the range"""
    _, kept, _, _ = _pull_and_check(sample, ["chr:B"], [(1, 0, INT32_MAX)], tag="a")
    assert kept and all(r.tid == 1 for r in kept)
    _pull_and_check(sample, ["chr:B:10001-20000"], [(1, 10_000, 20_000)], tag="b")
    _, kept, _, _ = _pull_and_check(sample, ["chrA:100-200"], [(2, 0, INT32_MAX)], tag="c")
    assert kept and all(r.tid == 2 for r in kept)
    _pull_and_check(sample, ["chrA:100-200:100-200"], [(2, 99, 200)], tag="d")


def test_unknown_reference_is_an_error(sample):
    r = run_pull(["-o", str(sample["dir"] / "x.bam"), sample["bam"], "chrQ:1-100"], mode="host")
    assert r.returncode == 1 and "chrQ" in r.stderr
    r = run_pull(["-o", str(sample["dir"] / "x.bam"), sample["bam"]], mode="host")
    assert r.returncode == 1 and "no region" in r.stderr


def test_bed_rows_are_merged(sample):
    """-L rows that overlap and touch give what the merged regions, written out by hand, give: no record twice"""
    bed = str(sample["dir"] / "r.bed")
    with open(bed, "w") as f:
        f.write("# rows\nchr:B\t5000\t9000\nchrA\t22000\t26000\nchrA\t20000\t23000\nchrA\t26000\t27000\nchrA\t40000\t41000\n")
    rows = [(1, 5000, 9000), (0, 22_000, 26_000), (0, 20_000, 23_000), (0, 26_000, 27_000), (0, 40_000, 41_000)]
    assert merge_regions(rows) == [(0, 20_000, 27_000), (0, 40_000, 41_000), (1, 5000, 9000)]
    _, kept, _, _ = _pull_and_check(sample, ["-L", bed], rows, tag="bed")
    assert len(set(id(r) for r in kept)) == len(kept) > 20
    _pull_and_check(sample, ["chrA:20001-27000", "chr:B:5001-9000", "chrA:40001-41000"], rows, tag="hand")
    assert open(sample["dir"] / "bed.bam", "rb").read() == open(sample["dir"] / "hand.bam", "rb").read()
    # positional regions and -L rows together
    _pull_and_check(sample, ["-L", bed, "chrA:26500-30000"], rows + [(0, 26_499, 30_000)], tag="both")


def test_region_without_records(sample):
    R = Recs(TARGETS)
    R.add("a", 0x41, 0, 100, 0, 300)
    R.add("a", 0x81, 0, 300, 0, 100)
    bam = str(sample["dir"] / "sparse.bam")
    bamio.write_bam(bam, R.build())
    for k, region in enumerate(["chrA:5000-6000", "chr:B", "chrA:151-300"]):
        out = str(sample["dir"] / f"empty{k}.bam")
        r = run_pull(["-o", out, bam, region], mode="host")
        assert r.returncode == 0, r.stderr
        header, _, _ = parse_bam(bam)
        assert bgzf_payload(out) == header and "extracted 0 alignments" in r.stderr
        assert subprocess.run([CLI, "_dump", out], capture_output=True).returncode == 0


def test_region_to_the_last_record_of_a_file_without_a_tail(sample):
    _, recs, _ = parse_bam(sample["bam2"])
    assert recs[-1].tid == 2
    last = recs[-1]
    got, kept, _, _ = _pull_and_check(sample, [f"chrA:100-200:{last.pos - 500}"], [(2, last.pos - 501, INT32_MAX)], bam=sample["bam2"], tag="last")
    assert kept[-1].raw == last.raw
    # ... and a request for an unplaced mate in a file that has no tail: not found
    _, _, missing, _ = _pull_and_check(sample, ["chrA:30001-30020"], [(0, 30_000, 30_020)], bam=sample["bam2"], tag="notail")
    assert b"tailpair" in missing and b"notail" in missing


def test_unplaced_mates_come_from_the_tail_and_sort_first(sample):
    """rule 4: the first record of the tail with the name, another 0x40 bit and neither 0x100 nor 0x800; refID == -1 sorts first"""
    got, kept, missing, _ = _pull_and_check(sample, ["chrA:30001-30020"], [(0, 30_000, 30_020)], tag="tail")
    assert missing == [b"notail"]
    assert got[0].tid == -1 and got[0].qname == b"tailpair" and got[0].flag == 0x85 and len(got[0].raw) == 4 + 32 + 9 + 6 + 12
    assert [r.tid for r in got] == sorted(r.tid for r in got) and len(got) == len(kept) + 1


def test_cram_is_refused(sample):
    cram = str(sample["dir"] / "x.cram")
    with open(cram, "wb") as f:
        f.write(b"CRAM\x03\x00" + b"\0" * 64)
    r = run_pull(["-o", str(sample["dir"] / "x.bam"), cram, "chrA"], mode="host")
    assert r.returncode == 1 and "CRAM" in r.stderr and "qualities" in r.stderr
    # -f is accepted, and ignored for a BAM
    _pull_and_check(sample, ["-f", "ref.fa", "chrA:20001-21000"], [(0, 20_000, 21_000)], tag="fasta")


def test_pull_region_is_still_refused_and_points_here():
    r = subprocess.run([CLI, "pull_region", "x", "y"], capture_output=True, text=True)
    assert r.returncode == 1 and "not part of this build" in r.stderr and "use `strling pull`" in r.stderr
    r = subprocess.run([CLI], capture_output=True, text=True)
    assert "  pull " in r.stdout


# ---- the host entry points, directly -------------------------------------------------------------------------------------------
def _murmur(b):
    """Nim's hash of a string (MurmurHash3_x86_32, seed 0: lib/pure/hashes.nim)"""
    M = 0xFFFFFFFF
    rotl = lambda x, r: ((x << r) | (x >> (32 - r))) & M      # noqa: E731
    h, n = 0, len(b) // 4 * 4
    for i in range(0, n, 4):
        k = struct.unpack_from("<I", b, i)[0]
        k = rotl(k * 0xcc9e2d51 & M, 15) * 0x1b873593 & M
        h = (rotl(h ^ k, 13) * 5 + 0xe6546b64) & M
    k = 0
    for x in reversed(b[n:]):
        k = (k << 8) | x
    h ^= rotl(k * 0xcc9e2d51 & M, 15) * 0x1b873593 & M
    h ^= len(b)
    h ^= h >> 16
    h = h * 0x85ebca6b & M
    h ^= h >> 13
    h = h * 0xc2b2ae35 & M
    return h ^ (h >> 16)


def test_pull_order_is_stable_and_signed():
    """strl_pull_order: (tid, pos) as signed integers -- refID -1 in front of 0, pos -1 in front of 0 -- and ties in input order"""
    rng = np.random.default_rng(5)
    rows = np.zeros(3000, api.PULL_ROW_DTYPE)
    rows["tid"] = rng.integers(-1, 3, rows.size)
    rows["pos"] = rng.choice([-1, 0, 1, 7, 2**31 - 1], rows.size)
    order = api.pull_order(rows)
    want = sorted(range(rows.size), key=lambda i: (int(rows["tid"][i]), int(rows["pos"][i])))
    assert order.tolist() == want and rows["tid"][order[0]] == -1 and rows["pos"][order[0]] == -1
    assert api.pull_order(rows[:0]).size == 0


def test_host_select_counts_and_mates_equal_the_restatement(sample):
    """strl_pull_select_host / _counts_host / _mates_host over the raw records of the sample, against the restatement"""
    recs = sample["recs"]
    raw = b"".join(r.raw for r in recs)
    off = np.concatenate([[0], np.cumsum([len(r.raw) for r in recs])])
    tile = np.array([(0, 20_000, 31_000, 25_000, 29_000)], api.PULL_TILE_DTYPE)
    rows = api.pull_select_host(raw, tile)
    want = [i for i, r in enumerate(recs) if overlaps(r, 0, 20_000, 31_000) and not r.flag & 0x900 and 25_000 <= r.pos < 29_000]
    assert want and rows["off"].tolist() == [int(off[i]) for i in want]
    assert rows["hash"].tolist() == [_murmur(recs[i].qname) for i in want] and rows["size"].tolist() == [len(recs[i].raw) for i in want]
    # counts over all primary records of the file: by the names' bytes
    every = api.pull_select_host(raw, np.array([(0, 0, INT32_MAX, -2**31, INT32_MAX)], api.PULL_TILE_DTYPE))
    prim = [r for r in recs if r.tid == 0 and not r.flag & 0x900]
    counts = {}
    for r in prim:
        counts[r.qname] = counts.get(r.qname, 0) + 1
    assert api.pull_counts_host(raw, every)["count"].tolist() == [counts[r.qname] for r in prim] and max(counts.values()) >= 2
    # the tail search of rule 4 (no interval) and a search with an interval
    ask = next(r for r in recs if r.qname == b"tailpair" and r.tid == 0)
    placed = [i for i, r in enumerate(recs) if r.tid >= 0]
    t0 = int(off[placed[-1] + 1])
    reqs = np.array([(_murmur(b"tailpair"), 0, 0, 0, ask.flag, 8, 0), (_murmur(b"notail"), 0, 0, 8, 0x49, 6, 0)], api.PULL_REQ_DTYPE)
    got = api.pull_mates_host(raw[t0:], reqs, b"tailpairnotail", use_interval=False)
    assert got["found"].tolist() == [1, 0] and got["flag"][0] == 0x85 and got["size"][0] == 4 + 32 + 9 + 6 + 12
    pair = next(r for r in prim if counts[r.qname] == 2 and r.mtid == 0 and r.mpos > r.pos)
    reqs = np.array([(_murmur(pair.qname), max(0, pair.mpos - 1), pair.mpos + 1, 0, pair.flag, len(pair.qname), 0),
                     (_murmur(pair.qname), pair.mpos + 5000, pair.mpos + 5002, 0, pair.flag, len(pair.qname), 0)], api.PULL_REQ_DTYPE)
    got = api.pull_mates_host(raw, reqs, pair.qname, tid=0)
    mate = next(r for r in prim if r.qname == pair.qname and r is not pair)
    assert got["found"].tolist() == [1, 0] and int(got["off"][0]) == int(off[recs.index(mate)]) and got["pos"][0] == pair.mpos
