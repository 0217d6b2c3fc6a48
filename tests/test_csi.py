"""CSI indexes (CSIv1) without a device: bamio.write_csi against a brute-force model, and the readers -- region reads, the record
count, the shares' cuts, host `pull` -- with only a .csi beside the BAM, contigs longer than 2^29 included.

Indexes are compared as structures: every virtual offset becomes an offset of the inflated stream (a walk of the BGZF headers).
tests/test_csi_device.py shares the helpers and the files below.
"""
import os
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest

from strling_amd import bamio, build, synth
from strling_amd.records import RecordBatch

CLI = build.CLI
P29, P30 = 1 << 29, 1 << 30
HUGE_LEN = P30 + 300_000
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def _run(args, **kw):
    return subprocess.run([CLI] + args, capture_output=True, text=True, **kw)


# ---- the tests' own readers ----------------------------------------------------------------------------------------------------
def _block_starts(path):
    """file offset of every BGZF block (empty ones and the end of the file too) -> offset of its first byte in the inflated stream"""
    raw = open(path, "rb").read()
    at, o, u = {}, 0, 0
    while o < len(raw):
        at[o] = u
        bsize = struct.unpack_from("<H", raw, o + 16)[0] + 1
        u += struct.unpack_from("<I", raw, o + bsize - 4)[0]
        o += bsize
    at[o] = u
    return at


def _bgzf_inflate(raw):
    out, o = bytearray(), 0
    while o < len(raw):
        assert raw[o:o + 4] == b"\x1f\x8b\x08\x04" and raw[o + 12:o + 16] == b"BC\x02\x00", o
        bsize = struct.unpack_from("<H", raw, o + 16)[0] + 1
        piece = zlib.decompress(raw[o + 18:o + bsize - 8], -15)
        crc, isize = struct.unpack_from("<II", raw, o + bsize - 8)
        assert zlib.crc32(piece) & 0xFFFFFFFF == crc and len(piece) == isize and isize <= 0xFF00
        out += piece
        o += bsize
    return bytes(out)


def _csi_file_payload(path):
    """the payload of a .csi FILE as samtools writes one: BGZF blocks, the EOF block last"""
    raw = open(path, "rb").read()
    assert raw.endswith(EOF_BLOCK)
    return _bgzf_inflate(raw)


def _meta_bin(depth):
    return ((1 << 3 * (depth + 1)) - 1) // 7 + 1


def _csi_abs(d, at):
    """CSI payload -> (min_shift, depth, [bins] per reference, n_no_coor); bins[b] = (loffset, chunks), offsets of the inflated
    stream (loffset 0 stays None), chunks ascending with chunks that touch merged; bins[pseudo-bin] = (None, [[first, end], [n_mapped, n_unmapped]])"""
    assert d[:4] == b"CSI\1"
    m, depth, l_aux, n_ref = struct.unpack_from("<iiii", d, 4)
    assert l_aux == 0
    o = 20
    ab = lambda v: at[v >> 16] + (v & 0xffff)
    refs = []
    for _ in range(n_ref):
        n_bin = struct.unpack_from("<i", d, o)[0]; o += 4
        bins, order = {}, []
        for _ in range(n_bin):
            b, loff, nc = struct.unpack_from("<IQi", d, o); o += 16
            order.append(b)
            assert b not in bins
            if b == _meta_bin(depth):
                v0, v1, n_map, n_unm = struct.unpack_from("<QQQQ", d, o); o += 32
                assert nc == 2 and loff == 0
                bins[b] = (None, [[ab(v0), ab(v1)], [n_map, n_unm]])
                continue
            ch = []
            for _ in range(nc):
                v0, v1 = struct.unpack_from("<QQ", d, o); o += 16
                assert ab(v0) < ab(v1)
                if ch and ch[-1][1] == ab(v0):
                    ch[-1][1] = ab(v1)
                else:
                    assert not ch or ch[-1][1] < ab(v0)
                    ch.append([ab(v0), ab(v1)])
            assert nc > 0 and b < _meta_bin(depth) - 1
            bins[b] = (ab(loff) if loff else None, ch)
        plain = [b for b in order if b != _meta_bin(depth)]
        assert plain == sorted(plain) and (_meta_bin(depth) not in order or order[-1] == _meta_bin(depth))
        refs.append(bins)
    no_coor = struct.unpack_from("<Q", d, o)[0]; o += 8
    assert o == len(d)
    return m, depth, refs, no_coor


def _bai_abs(d, at):
    """.bai -> ([(bins, lin)] per reference, n_no_coor) in the same terms (bins[b] = chunks; lin[w] = offset or None)"""
    assert d[:4] == b"BAI\1"
    n_ref = struct.unpack_from("<i", d, 4)[0]
    o = 8
    ab = lambda v: at[v >> 16] + (v & 0xffff)
    refs = []
    for _ in range(n_ref):
        n_bin = struct.unpack_from("<i", d, o)[0]; o += 4
        bins = {}
        for _ in range(n_bin):
            b, nc = struct.unpack_from("<Ii", d, o); o += 8
            raw = [struct.unpack_from("<QQ", d, o + 16 * k) for k in range(nc)]; o += 16 * nc
            if b == 37450:
                bins[b] = [[ab(raw[0][0]), ab(raw[0][1])], list(raw[1])]
                continue
            ch = []
            for v0, v1 in raw:
                if ch and ch[-1][1] == ab(v0):
                    ch[-1][1] = ab(v1)
                else:
                    ch.append([ab(v0), ab(v1)])
            bins[b] = ch
        n_intv = struct.unpack_from("<i", d, o)[0]; o += 4
        lin = [ab(v) if v else None for v in struct.unpack_from(f"<{n_intv}Q", d, o)]; o += 8 * n_intv
        refs.append((bins, lin))
    return refs, struct.unpack_from("<Q", d, o)[0]


def _reg2bin(beg, end, m, depth):
    """CSIv1 specification, section 3"""
    end -= 1
    s, t = m, ((1 << depth * 3) - 1) // 7
    l = depth
    while l > 0:
        if beg >> s == end >> s:
            return t + (beg >> s)
        l -= 1
        s += 3
        t -= 1 << l * 3
    return 0


def _bin_first_window(b, depth):
    l = 0
    while l < depth and b >= ((1 << 3 * (l + 1)) - 1) // 7:
        l += 1
    return (b - ((1 << 3 * l) - 1) // 7) << 3 * (depth - l)


def _layout(rec, text):
    """offsets of the records in the inflated stream (off[n] = its end) and their ends on the reference, from the arrays alone"""
    o = 12 + len(text.encode()) + sum(9 + len(n.encode()) for n, _ in rec.targets)
    off = [o]
    for i in range(rec.n):
        l_seq = int(rec.l_seq[i])
        o += 36 + len(rec.qname(i)) + 1 + 4 * (int(rec.cigar_off[i + 1]) - int(rec.cigar_off[i])) + (l_seq + 1) // 2 + l_seq
        off.append(o)
    stop = np.array([int(rec.pos[i]) + bamio._ref_len(rec, i) for i in range(rec.n)], np.int64)
    return off, stop


def _backfilled(want):
    """window -> offset of the first record that overlaps it; an empty window takes the next filled one's; None behind the last"""
    keys = sorted(want)

    def at(w):
        import bisect
        k = bisect.bisect_left(keys, w)
        return want[keys[k]] if k < len(keys) else None
    return at


def _check_model(parsed, rec, off, stop, scheme=None):
    """the properties of a CSI index, from the record arrays alone"""
    m, depth, refs, no_coor = parsed
    if scheme is not None:
        assert (m, depth) == scheme
    edges = set(off)
    n_ref = len(rec.targets)
    assert len(refs) == n_ref
    want_lin = [dict() for _ in range(n_ref)]
    counted = 0
    for i in range(rec.n):
        t = int(rec.tid[i])
        if t < 0:
            continue
        b = _reg2bin(int(rec.pos[i]), int(stop[i]), m, depth)
        assert b in refs[t], (i, b)
        assert sum(1 for c in refs[t][b][1] if c[0] <= off[i] and off[i + 1] <= c[1]) == 1, (i, b)       # in exactly one chunk of its bin
        for w in range(int(rec.pos[i]) >> m, ((int(stop[i]) - 1) >> m) + 1):
            want_lin[t][w] = min(want_lin[t].get(w, off[i]), off[i])
    for t, bins in enumerate(refs):
        fill = _backfilled(want_lin[t])
        for b, (loff, ch) in bins.items():
            if b == _meta_bin(depth):
                counted += sum(ch[1])
                continue
            for c in ch:
                assert c[0] in edges and c[1] in edges, (t, b, c)
            assert loff == fill(_bin_first_window(b, depth)), (t, b)
        sel = rec.tid == t
        if sel.any():
            idx = np.nonzero(sel)[0]
            assert bins[_meta_bin(depth)] == (None, [[off[idx[0]], off[idx[-1] + 1]], [int((sel & ((rec.flag & 4) == 0)).sum()), int((sel & ((rec.flag & 4) != 0)).sum())]])
        else:
            assert not bins
    assert no_coor == int((rec.tid < 0).sum()) and counted + no_coor == rec.n


# ---- the files -------------------------------------------------------------------------------------------------------------------
def _rows(rows, targets):
    """rows of (tid, pos, cigar, flag), sorted here; every record is its own mate's position"""
    rows = sorted((r for r in rows if r[0] >= 0), key=lambda r: (r[0], r[1])) + [r for r in rows if r[0] < 0]
    n = len(rows)
    return RecordBatch.from_fields([r[0] for r in rows], [r[1] for r in rows], [r[0] for r in rows], [r[1] for r in rows], [r[3] for r in rows], [60] * n,
                                   [r[2] for r in rows], ["ACGT" * 25] * n, [f"r{i}" for i in range(n)], [0] * n, targets)


def _huge():
    """a contig of 2^30 + 300 000 bases: records at its start, on both sides of 2^29 and one across it, around 2^30, one with a
    200 kb N skip, a placed-unmapped mate, a read on the second contig that hangs over its end, two unplaced reads.  seed 61"""
    rng = np.random.default_rng(61)
    rows = [(0, int(p), "100M", 0x1) for p in rng.integers(0, 400_000, 150)]
    rows += [(0, int(p), "60M5D40M", 0x1) for p in rng.integers(P29 - 100_000, P29 + 150_000, 150)] + [(0, P29 - 50, "100M", 0x1)]
    rows += [(0, int(p), "100M", 0x1) for p in rng.integers(P30 - 60_000, P30 + 60_000, 100)] + [(0, HUGE_LEN - 100, "100M", 0x1)]
    rows += [(0, 50_000, "50M200000N50M", 0x1)]
    rows += [(1, 10, "100M", 0x1 | 0x8), (1, 10, "*", 0x1 | 0x4), (1, 20_000, "30S70M", 0x1), (1, 18 * 16384 - 12, "100M", 0x1)]
    rows += [(-1, -1, "*", 0x1 | 0x4 | 0x8)] * 2
    return _rows(rows, [("huge", HUGE_LEN), ("c2", 18 * 16384)])


def _humanlike():
    return synth.synth_wgs(2500, seed=31, n_contigs=3, contig_len=200_000)[0]


def _empty_contig():
    rec = synth.synth_wgs(1500, seed=35, n_contigs=3, contig_len=100_000)[0]
    tid, mtid = rec.tid.copy(), rec.mtid.copy()
    tid[rec.tid == 2] = 3
    mtid[rec.mtid == 2] = 3
    t = rec.targets
    return RecordBatch(tid, rec.pos, mtid, rec.mpos, rec.flag, rec.mapq, rec.cigar_off, rec.cigar, rec.seq_off, rec.l_seq, rec.seq4, rec.qname_off, rec.qnames,
                       rec.isize, [t[0], t[1], ("empty", 123_456), t[2]])


def _header_only():
    t = synth.synth_wgs(10, seed=36, n_contigs=2, contig_len=50_000)[0].targets
    return RecordBatch.from_fields([], [], [], [], [], [], [], [], [], targets=t)


def _depth0():
    rng = np.random.default_rng(62)
    return _rows([(0, int(p), "100M", 0x1) for p in rng.integers(0, 9_800, 200)] + [(-1, -1, "*", 0x1 | 0x4 | 0x8)], [("tiny", 10_000)])


# name -> (records, BGZF block size of the BAM, blocks per push, (min_shift, depth as asked: None = the rule), the scheme that gives)
FILES = {
    "huge_small_blocks": (_huge, 2500, 1, (14, None), (14, 6)),
    "huge": (_huge, 0xFF00, 16384, (14, None), (14, 6)),
    "humanlike": (_humanlike, 0xFF00, 16384, (14, None), (14, 2)),
    "humanlike_as_bai": (_humanlike, 0xFF00, 16384, (14, 5), (14, 5)),
    "m12": (_humanlike, 0xFF00, 16384, (12, None), (12, 2)),
    "depth0": (_depth0, 0xFF00, 16384, (14, 0), (14, 0)),
    "empty_contig": (_empty_contig, 0xFF00, 16384, (14, None), (14, 1)),
    "header_only": (_header_only, 0xFF00, 16384, (14, None), (14, 1)),
}
_RECS = {}


def make_file(d, name, index="csi"):
    """the BAM of a case in directory d, with the Python writer's .csi (index="csi"), its .bai ("bai") or nothing (None) beside it"""
    make, block, per_push, asked, scheme = FILES[name]
    if make not in _RECS:
        _RECS[make] = make()
    rec = _RECS[make]
    bam = os.path.join(str(d), f"{name}.bam")
    text = bamio.write_bam(bam, rec, block=block, index=(index == "bai"))
    at = _block_starts(bam)
    off, stop = _layout(rec, text)
    if index == "csi":
        bamio.write_csi(bam + ".csi", rec, off, sorted(at), block, min_shift=asked[0], depth=asked[1])
    return dict(rec=rec, bam=bam, text=text, at=at, off=off, stop=stop, block=block, per_push=per_push, asked=asked, scheme=scheme)


@pytest.fixture(scope="module")
def made(tmp_path_factory):
    d = tmp_path_factory.mktemp("csi")
    return {name: make_file(d, name) for name in FILES}


def huge_regions():
    rng = np.random.default_rng(63)
    regions = [(0, P29 + 10_000, P29 + 12_000), (0, P30 - 1000, P30 + 1000), (0, P30 + 50_000, P30 + 70_000),      # wholly beyond 2^29
               (0, P29 - 1000, P29 + 1000),                                                                    # spanning it
               (0, 10_000_000, 10_100_000), (0, P29 + 2_000_000, P29 + 2_000_100),                             # the empty stretches between the clusters
               (0, HUGE_LEN - 1, HUGE_LEN),                                                                    # the contig's last base
               (0, 0, 500), (0, 249_000, 251_000), (1, 0, 100), (1, 18 * 16384 - 1, 18 * 16384 + 50)]
    regions += [(0, int(a), int(a) + int(rng.integers(1, 3000))) for a in rng.integers(0, 400_000, 6)]
    regions += [(0, int(a), int(a) + int(rng.integers(1, 3000))) for a in rng.integers(P29 - 100_000, P29 + 150_000, 8)]
    regions += [(0, int(a), int(a) + int(rng.integers(1, 3000))) for a in rng.integers(P30 - 60_000, P30 + 60_000, 6)]
    return regions


HUMANLIKE_REGIONS = [(0, 0, 500), (2, 199_000, 200_500), (1, 16_300, 16_400), (1, 150_000, 150_001), (0, 100_000, 140_000), (2, 0, 1)]


def regions_match(f, regions):
    rec, stop = f["rec"], f["stop"]
    nonempty = 0
    for tid, beg, end in regions:
        r = _run(["_region", f["bam"], str(tid), str(beg), str(end)])
        assert r.returncode == 0, r.stderr
        got = [tuple(l.split("\t")) for l in r.stdout.splitlines()]
        sel = np.nonzero((rec.tid == tid) & (rec.pos < end) & (stop > beg))[0]
        assert got == [(rec.qname(i).decode(), str(int(rec.pos[i])), str(int(rec.flag[i]))) for i in sel], (tid, beg, end)
        nonempty += len(sel) > 0
    return nonempty


# ---- `strling pull`, restated (extract_region.nim) ---------------------------------------------------------------------------------
class _Rec:
    def __init__(self, buf, at):
        bs, self.tid, self.pos, l_name, _, _, n_cig, self.flag, _, self.mtid, self.mpos = struct.unpack_from("<iiiBBHHHiii", buf, at)
        self.raw = buf[at:at + 4 + bs]
        self.qname = buf[at + 36:at + 36 + l_name - 1]
        rl = 0
        if not self.flag & 4:
            rl = sum(c >> 4 for c in struct.unpack_from(f"<{n_cig}I", buf, at + 36 + l_name) if c & 15 in (0, 2, 3, 7, 8))
        self.end = self.pos + (rl or 1)


def _parse_bam(path):
    u = _bgzf_inflate(open(path, "rb").read())
    at = 8 + struct.unpack_from("<i", u, 4)[0]
    n_ref = struct.unpack_from("<i", u, at)[0]
    at += 4
    for _ in range(n_ref):
        at += 8 + struct.unpack_from("<i", u, at)[0]
    header, recs = u[:at], []
    while at < len(u):
        recs.append(_Rec(u, at))
        at += len(recs[-1].raw)
    return header, recs, n_ref


def pull_expected(path, regions):
    """the inflated bytes `strling pull` writes for the (merged, sorted) regions [(tid, beg, end)]"""
    header, recs, n_ref = _parse_bam(path)
    over = lambda r, tid, beg, end: r.tid == tid and r.pos < end and r.end > beg
    kept = [r for tid, beg, end in regions for r in recs if over(r, tid, beg, end) and not r.flag & 0x900]
    counts = {}
    for r in kept:
        counts[r.qname] = counts.get(r.qname, 0) + 1
    placed = [i for i, r in enumerate(recs) if r.tid >= 0]
    tail = recs[placed[-1] + 1:] if placed else recs
    mates = []
    for r in kept:
        if counts[r.qname] == 2:
            continue
        if r.mtid == -1:
            cand = tail
        elif 0 <= r.mtid < n_ref and r.mpos + 1 > max(0, r.mpos - 1):
            cand = [o for o in recs if over(o, r.mtid, max(0, r.mpos - 1), r.mpos + 1)]
        else:
            cand = []
        for o in cand:
            if not o.flag & 0x900 and (o.flag & 0x40) != (r.flag & 0x40) and o.qname == r.qname:
                mates.append(o)
                break
    return header + b"".join(r.raw for r in sorted(kept + mates, key=lambda r: (r.tid, r.pos))), len(kept)


def run_pull(args, mode):
    env = dict(os.environ)
    env.pop("STRL_PULL", None)
    if mode:
        env["STRL_PULL"] = mode
    return subprocess.run([CLI, "pull"] + args, capture_output=True, text=True, env=env)


# ---- the Python writer against the model -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(FILES))
def test_the_model_accepts_the_python_writer(made, name):
    f = made[name]
    parsed = _csi_abs(_csi_file_payload(f["bam"] + ".csi"), f["at"])
    _check_model(parsed, f["rec"], f["off"], f["stop"], f["scheme"])
    bins = parsed[2]
    if name.startswith("huge"):
        first6 = ((1 << 18) - 1) // 7                                       # the first bin of the deepest level of (14, 6)
        assert 0 in bins[0] and any(b >= first6 + (P29 >> 14) for b in bins[0]) and any(b >= first6 + (P30 >> 14) for b in bins[0])
        assert bins[0][0][0] is not None                                   # bin 0 holds the record across 2^29; its loffset is the file's first record
    if name == "depth0":
        assert sorted(bins[0]) == [0, 2]
    if name == "empty_contig":
        assert bins[2] == {}


def test_scheme_14_5_is_the_bai(made, tmp_path):
    """the two serializers against each other: bins, chunks and pseudo-bins of the (14, 5) CSI are the .bai's, every loffset is the
    .bai's linear index, empty windows taking the next filled one's value, at the bin's first window"""
    f = made["humanlike_as_bai"]
    m, depth, refs, no_coor = _csi_abs(_csi_file_payload(f["bam"] + ".csi"), f["at"])
    b = make_file(tmp_path, "humanlike_as_bai", index="bai")
    assert b["at"] == f["at"]
    bai, bai_no_coor = _bai_abs(open(b["bam"] + ".bai", "rb").read(), b["at"])
    assert (m, depth) == (14, 5) and no_coor == bai_no_coor and len(refs) == len(bai)
    for bins, (bbins, lin) in zip(refs, bai):
        assert {k: v[1] for k, v in bins.items()} == bbins
        fill = _backfilled({w: v for w, v in enumerate(lin) if v is not None})
        for k, (loff, _) in bins.items():
            if k != 37450:
                assert loff == fill(_bin_first_window(k, 5)), k


# ---- the readers, with only the .csi beside the file ---------------------------------------------------------------------------------
def test_region_reads_through_the_csi(made):
    regions = huge_regions()
    assert len(regions) >= 25
    assert regions_match(made["huge"], regions) >= 18
    assert regions_match(made["huge_small_blocks"], regions[:12]) >= 6
    assert regions_match(made["humanlike"], HUMANLIKE_REGIONS) >= 4
    assert regions_match(made["m12"], HUMANLIKE_REGIONS) >= 4            # anchors in the middle of a 16 KiB window
    assert not os.path.exists(made["huge"]["bam"] + ".bai")


@pytest.mark.parametrize("name", ["huge", "humanlike", "m12", "header_only"])
def test_indexed_records_and_shares(made, name):
    f = made[name]
    r = _run(["_indexed_records", f["bam"]])
    assert r.returncode == 0 and r.stdout.strip() == str(f["rec"].n), (r.stdout, r.stderr)
    if name == "header_only":
        return
    r = _run(["_shares", f["bam"], "2"])
    assert r.returncode == 0, r.stderr
    rows = [l.split("\t") for l in r.stdout.strip().split("\n")]
    assert int(rows[0][1]) == 2 and len(rows) == 3, r.stdout
    starts = set(f["off"][:-1])
    for row in rows[1:]:
        assert row[0] == "share" and row[2] != "error", row
        assert f["at"][int(row[2])] + int(row[3]) in starts, "a cut that is not a record start"


def test_host_pull_humanlike_csi_equals_bai(made, tmp_path):
    f = made["humanlike"]
    b = make_file(tmp_path, "humanlike", index="bai")
    out_c, out_b = str(tmp_path / "c.bam"), str(tmp_path / "b.bam")
    region = [f"{f['rec'].targets[0][0]}:90001-130000"]
    rc, rb = run_pull(["-o", out_c, f["bam"]] + region, "host"), run_pull(["-o", out_b, b["bam"]] + region, "host")
    assert rc.returncode == 0 and rb.returncode == 0, (rc.stderr, rb.stderr)
    assert open(out_c, "rb").read() == open(out_b, "rb").read()
    exp, n_kept = pull_expected(f["bam"], [(0, 90_000, 130_000)])
    assert n_kept > 50 and _bgzf_inflate(open(out_c, "rb").read()) == exp


def test_host_pull_beyond_2p29(made, tmp_path):
    f = made["huge"]
    out = str(tmp_path / "o.bam")
    r = run_pull(["-o", out, f["bam"], f"huge:{P29 + 1}-{P29 + 100_000}"], "host")
    assert r.returncode == 0, r.stderr
    exp, n_kept = pull_expected(f["bam"], [(0, P29, P29 + 100_000)])
    assert n_kept > 30 and _bgzf_inflate(open(out, "rb").read()) == exp


def test_a_bai_wins_over_a_corrupt_csi(tmp_path):
    f = make_file(tmp_path, "humanlike", index="bai")
    open(f["bam"] + ".csi", "wb").write(b"not an index at all")
    assert regions_match(f, HUMANLIKE_REGIONS) >= 4
    r = _run(["_indexed_records", f["bam"]])
    assert r.returncode == 0 and r.stdout.strip() == str(f["rec"].n)


def test_small_bgzf_blocks_without_eof_block(made, tmp_path):
    f = made["huge"]
    bam = str(tmp_path / "h.bam")
    shutil.copy(f["bam"], bam)
    bamio.write_csi(bam + ".csi", f["rec"], f["off"], sorted(f["at"]), f["block"], bgzf_block=512)
    raw = open(bam + ".csi", "rb").read()
    assert raw.endswith(EOF_BLOCK) and raw.count(b"\x1f\x8b\x08\x04") >= 5
    open(bam + ".csi", "wb").write(raw[:-len(EOF_BLOCK)])
    assert _bgzf_inflate(raw[:-len(EOF_BLOCK)]) == _csi_file_payload(f["bam"] + ".csi")
    assert regions_match(dict(f, bam=bam), huge_regions()[:10]) >= 6
    r = _run(["_indexed_records", bam])
    assert r.returncode == 0 and r.stdout.strip() == str(f["rec"].n)


@pytest.mark.parametrize("what", ["truncated", "wrong_magic", "n_bin", "depth_40", "not_bgzf", "min_shift_3"])
def test_corrupt_csi(made, tmp_path, what):
    f = made["humanlike"]
    bam = str(tmp_path / "x.bam")
    shutil.copy(f["bam"], bam)
    p = bytearray(_csi_file_payload(f["bam"] + ".csi"))
    if what == "truncated":
        p = p[:len(p) // 2]
    elif what == "wrong_magic":
        p[:4] = b"CSJ\1"
    elif what == "n_bin":
        struct.pack_into("<i", p, 20, 0x7000_0000)                         # the first reference's n_bin
    elif what == "depth_40":
        struct.pack_into("<i", p, 8, 40)
    elif what == "min_shift_3":
        struct.pack_into("<i", p, 4, 3)
    raw = bamio.bgzf_bytes(bytes(p))
    if what == "not_bgzf":
        raw = bytes(p)
    open(bam + ".csi", "wb").write(raw)
    r = _run(["_region", bam, "0", "0", "500"])
    assert r.returncode == 1 and "corrupt .csi index" in r.stderr, (r.returncode, r.stderr)
    assert _run(["_indexed_records", bam]).stdout.strip() == "unknown"


def test_no_index_message(tmp_path):
    f = make_file(tmp_path, "depth0", index=None)
    r = _run(["_region", f["bam"], "0", "0", "500"])
    assert r.returncode == 1 and f"no .bai index next to {f['bam']}" in r.stderr and "(nor a .csi)" in r.stderr, r.stderr


def test_usage():
    h = _run(["bamindex"])
    assert h.returncode == 0 and "--csi" in h.stdout and "--min-shift" in h.stdout
    for args in (["bamindex", "-m", "12", "x.bam"], ["bamindex", "--csi", "-m", "7", "x.bam"], ["bamindex", "--csi", "-m", "25", "x.bam"],
                 ["extract", "--write-index", "-m", "12", "x.bam", "x.bin"], ["extract", "--csi", "x.bam", "x.bin"]):
        r = _run(args)
        assert r.returncode == 1 and "Usage:" in r.stderr, (args, r.stderr)
    assert "--csi" in _run(["extract"]).stdout


def test_write_bam_index_csi(tmp_path):
    rec = _RECS.get(_depth0) or _depth0()
    bam = str(tmp_path / "w.bam")
    bamio.write_bam(bam, rec, index="csi")
    assert os.path.exists(bam + ".csi") and not os.path.exists(bam + ".bai")
    m, depth, refs, no_coor = _csi_abs(_csi_file_payload(bam + ".csi"), _block_starts(bam))
    assert (m, depth) == (14, 0) and sorted(refs[0]) == [0, 2] and no_coor == 1
    with pytest.raises(ValueError):
        bamio.write_bam(bam, rec, index="tbi")
