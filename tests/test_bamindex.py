"""`strling bamindex` / strl_bamindex_*: the .bai built on the device behind the front end's record scan.

Compared as structures, never as bytes: every virtual offset is turned into an offset of the inflated stream (a walk of the
BGZF headers), so a chunk that ends at the end of a block may name (that block, isize) or (the next block, 0).
  1. against the index the Python writer (bamio.write_bai) wrote for the same records;
  2. against a brute-force model made from the record arrays alone (a mistake shared with write_bai would pass 1);
  3. by use: region reads, the record count and `extract --gpus 2` with only the device-built index beside the file;
  4. `strling call --make-index`;
  5. refusals: unsorted, pos >= 2^29, a flipped payload byte, a CRAM.
"""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from strling_amd import bamio, build, synth
from strling_amd.records import RecordBatch

CLI = build.CLI
META_BIN = 37450


def _run(args, **kw):
    return subprocess.run([CLI] + args, capture_output=True, text=True, **kw)


# ---- the test's own readers ---------------------------------------------------------------------------------------------
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


def _bai_abs(d, at):
    """bytes of a .bai -> ([(bins, lin)] per reference, n_no_coor), every virtual offset an offset of the inflated stream;
    bins[b] = ascending chunk list with chunks that touch merged, bins[37450] = [[first, end], [n_mapped, n_unmapped]]"""
    assert d[:4] == b"BAI\1"
    n_ref = struct.unpack_from("<i", d, 4)[0]
    o = 8
    refs = []
    ab = lambda v: at[v >> 16] + (v & 0xffff)
    for _ in range(n_ref):
        n_bin = struct.unpack_from("<i", d, o)[0]; o += 4
        bins, order = {}, []
        for _ in range(n_bin):
            b, nc = struct.unpack_from("<Ii", d, o); o += 8
            order.append(b)
            if b == META_BIN:
                v0, v1, n_map, n_unm = struct.unpack_from("<QQQQ", d, o); o += 32
                assert nc == 2
                bins[b] = [[ab(v0), ab(v1)], [n_map, n_unm]]
                continue
            ch = []
            for _ in range(nc):
                v0, v1 = struct.unpack_from("<QQ", d, o); o += 16
                assert ab(v0) < ab(v1)
                if ch and ch[-1][1] == ab(v0):
                    ch[-1][1] = ab(v1)
                else:
                    assert not ch or ch[-1][1] < ab(v0)                # ascending and disjoint
                    ch.append([ab(v0), ab(v1)])
            assert nc > 0 and b not in bins
            bins[b] = ch
        plain = [b for b in order if b != META_BIN]
        assert plain == sorted(plain) and (META_BIN not in order or order[-1] == META_BIN)   # bins ascending, the pseudo-bin last
        n_intv = struct.unpack_from("<i", d, o)[0]; o += 4
        lin = [ab(v) if v else None for v in struct.unpack_from(f"<{n_intv}Q", d, o)]; o += 8 * n_intv
        refs.append((bins, lin))
    no_coor = struct.unpack_from("<Q", d, o)[0]; o += 8
    assert o == len(d)
    return refs, no_coor


def _reg2bin(beg, end):
    """SAM specification section 5.3"""
    end -= 1
    for shift, first in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return first + (beg >> shift)
    return 0


def _layout(rec, text):
    """offsets of the records in the inflated stream (rec_off[n] = its end) and their ends on the reference, from the arrays alone"""
    o = 12 + len(text.encode()) + sum(9 + len(n.encode()) for n, _ in rec.targets)
    off = [o]
    for i in range(rec.n):
        l_seq = int(rec.l_seq[i])
        o += 36 + len(rec.qname(i)) + 1 + 4 * (int(rec.cigar_off[i + 1]) - int(rec.cigar_off[i])) + (l_seq + 1) // 2 + l_seq
        off.append(o)
    stop = np.array([int(rec.pos[i]) + bamio._ref_len(rec, i) for i in range(rec.n)], np.int64)
    return off, stop


def _check_model(refs, no_coor, rec, off, stop):
    """the properties of an index, from the record arrays alone"""
    edges = set(off)
    n_ref = len(rec.targets)
    assert len(refs) == n_ref
    want_lin = [dict() for _ in range(n_ref)]
    counted = 0
    for i in range(rec.n):
        t = int(rec.tid[i])
        if t < 0:
            continue
        bins, _ = refs[t]
        b = _reg2bin(int(rec.pos[i]), int(stop[i]))
        assert b in bins, (i, b)
        assert sum(1 for c in bins[b] if c[0] <= off[i] and off[i + 1] <= c[1]) == 1, (i, b)
        for w in range(int(rec.pos[i]) >> 14, ((int(stop[i]) - 1) >> 14) + 1):
            want_lin[t][w] = min(want_lin[t].get(w, off[i]), off[i])
    for t, (bins, lin) in enumerate(refs):
        for b, ch in bins.items():
            if b == META_BIN:
                counted += sum(ch[1])
                continue
            for c in ch:
                assert c[0] in edges and c[1] in edges, (t, b, c)
        sel = rec.tid == t
        if sel.any():
            idx = np.nonzero(sel)[0]
            assert bins[META_BIN] == [[off[idx[0]], off[idx[-1] + 1]], [int((sel & ((rec.flag & 4) == 0)).sum()), int((sel & ((rec.flag & 4) != 0)).sum())]]
        else:
            assert not bins and not lin
        n_intv = max(want_lin[t]) + 1 if want_lin[t] else 0
        assert lin == [want_lin[t].get(w) for w in range(n_intv)], t
    assert no_coor == int((rec.tid < 0).sum()) and counted + no_coor == rec.n


# ---- the files -------------------------------------------------------------------------------------------------------------
def _with_empty_contig(rec):
    """three contigs with reads and one, in the middle, without"""
    tid, mtid = rec.tid.copy(), rec.mtid.copy()
    tid[rec.tid == 2] = 3
    mtid[rec.mtid == 2] = 3
    t = rec.targets
    return RecordBatch(tid, rec.pos, mtid, rec.mpos, rec.flag, rec.mapq, rec.cigar_off, rec.cigar, rec.seq_off, rec.l_seq, rec.seq4, rec.qname_off, rec.qnames,
                       rec.isize, [t[0], t[1], ("empty", 123_456), t[2]])


def _long_contig():
    """a contig longer than 2^26 with records on both sides of that boundary and one across it (bin 0), a record with a 200 kb N
    skip (a higher-level bin, many windows), a placed-unmapped mate, a second contig whose last read reaches past l_ref into a window of its own, two unplaced reads.  seed 41"""
    rng = np.random.default_rng(41)
    M = 1 << 26
    rows = [(0, 1000, "100M", 0x1), (0, 50_000, "50M200000N50M", 0x1), (0, M - 5000, "100M", 0x1), (0, M - 50, "100M", 0x1), (0, M + 1000, "100M", 0x1)]
    rows += [(0, int(p), "100M", 0x1) for p in rng.integers(0, 400_000, 150)] + [(0, int(p), "60M5D40M", 0x1) for p in rng.integers(M - 100_000, M + 150_000, 150)]
    rows += [(1, 10, "100M", 0x1 | 0x8), (1, 10, "*", 0x1 | 0x4), (1, 20_000, "30S70M", 0x1), (1, 18 * 16384 - 12, "100M", 0x1)]   # the last hangs over the contig's end
    rows.sort(key=lambda r: (r[0], r[1]))
    rows += [(-1, -1, "*", 0x1 | 0x4 | 0x8)] * 2
    n = len(rows)
    seq = "ACGT" * 25
    return RecordBatch.from_fields([r[0] for r in rows], [r[1] for r in rows], [r[0] for r in rows], [r[1] for r in rows], [r[3] for r in rows], [60] * n,
                                   [r[2] for r in rows], [seq] * n, [f"r{i}" for i in range(n)], [0] * n, [("big", M + 200_000), ("c2", 18 * 16384)])


# name -> (records, BGZF block size, level, blocks per push); the synthetic-data seed is the one given to synth_wgs
def _case(name):
    if name == "three_contigs":          # placed-unmapped mates (flag 0x4 with a position) and a tail of unplaced reads come with synth_wgs
        return synth.synth_wgs(2500, seed=31, n_contigs=3, contig_len=200_000)[0], 0xFF00, 1, 16384
    if name == "one_contig_level6":
        return synth.synth_wgs(2000, seed=32, n_contigs=1, contig_len=300_000, interchrom_frac=0.0)[0], 20011, 6, 16384
    if name == "small_blocks_small_pushes":   # records straddle several blocks, runs and records straddle pushes
        return synth.synth_wgs(2000, seed=33, n_contigs=3, contig_len=150_000)[0], 2500, 1, 7
    if name == "pushes_of_one_block":
        return synth.synth_wgs(600, seed=34, n_contigs=2, contig_len=40_000)[0], 20011, 6, 1
    if name == "empty_contig":
        return _with_empty_contig(synth.synth_wgs(1500, seed=35, n_contigs=3, contig_len=100_000)[0]), 0xFF00, 6, 16384
    if name == "header_only":
        t = synth.synth_wgs(10, seed=36, n_contigs=2, contig_len=50_000)[0].targets
        return RecordBatch.from_fields([], [], [], [], [], [], [], [], [], targets=t), 0xFF00, 1, 16384
    if name == "long_contig":
        return _long_contig(), 2500, 1, 1
    raise KeyError(name)


CASES = ["three_contigs", "one_contig_level6", "small_blocks_small_pushes", "pushes_of_one_block", "empty_contig", "header_only", "long_contig"]


@pytest.fixture(scope="module")
def built(tmp_path_factory, ctx):
    """every case once: the file, the Python writer's index, the device-built index (api) -- shared by the tests below"""
    d = tmp_path_factory.mktemp("bamindex")
    out = {}
    for name in CASES:
        rec, block, level, per_push = _case(name)
        bam = str(d / f"{name}.bam")
        text = bamio.write_bam(bam, rec, level=level, block=block, index=True)
        got, info = ctx.bamindex(bam, chunk_blocks=per_push)
        out[name] = dict(rec=rec, bam=bam, text=text, bai=got, info=info, at=_block_starts(bam))
    return out


# ---- CPU -------------------------------------------------------------------------------------------------------------------
def test_bamindex_usage():
    r = _run(["bamindex"])
    assert r.returncode == 0 and "strling bamindex" in r.stdout and "--output" in r.stdout
    top = _run([])
    assert "bamindex" in top.stdout and "extract" in top.stdout


def test_region_seed_has_enough_nonempty_regions(tmp_path):
    """the regions test 3 uses, read through the Python-written index: more than 15 are non-empty, and they are what the model says"""
    rec, _, regions, stop = _region_sample()
    bam = str(tmp_path / "r.bam")
    bamio.write_bam(bam, rec)
    assert _regions_match(bam, rec, regions, stop) > 15


@pytest.mark.parametrize("name", CASES)
def test_the_model_accepts_the_python_writer(tmp_path, name):
    """the brute-force model and the parser on an index that does not come from the device"""
    rec, block, level, _ = _case(name)
    bam = str(tmp_path / "m.bam")
    text = bamio.write_bam(bam, rec, level=level, block=block)
    refs, no_coor = _bai_abs(open(bam + ".bai", "rb").read(), _block_starts(bam))
    off, stop = _layout(rec, text)
    _check_model(refs, no_coor, rec, off, stop)
    if name == "long_contig":
        assert 0 in refs[0][0] and 73 in refs[0][0] and len(refs[0][1]) > 4096


def _region_sample():
    rec, g = synth.synth_wgs(5000, seed=3, n_contigs=3, contig_len=200_000)
    stop = np.array([int(rec.pos[i]) + bamio._ref_len(rec, i) for i in range(rec.n)])
    rng = np.random.default_rng(1)
    regions = [(0, 0, 500), (2, 199_000, 200_500), (1, 16_300, 16_400), (1, 150_000, 150_001), (0, 100_000, 140_000), (2, 0, 1)]
    regions += [(int(rng.integers(0, 3)), int(a), int(a) + int(rng.integers(1, 3000))) for a in rng.integers(0, 199_000, 20)]
    return rec, g, regions, stop


def _regions_match(bam, rec, regions, stop):
    nonempty = 0
    for tid, beg, end in regions:
        r = _run(["_region", bam, str(tid), str(beg), str(end)])
        assert r.returncode == 0, r.stderr
        got = [tuple(l.split("\t")) for l in r.stdout.splitlines()]
        sel = np.nonzero((rec.tid == tid) & (rec.pos < end) & (stop > beg))[0]
        assert got == [(rec.qname(i).decode(), str(int(rec.pos[i])), str(int(rec.flag[i]))) for i in sel], (tid, beg, end)
        nonempty += len(sel) > 0
    return nonempty


# ---- GPU -------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_device_index_equals_the_python_writers(built, name):
    b = built[name]
    (ia, nca), (ib, ncb) = _bai_abs(b["bai"], b["at"]), _bai_abs(open(b["bam"] + ".bai", "rb").read(), b["at"])
    assert len(ia) == len(ib) == len(b["rec"].targets)
    for t, ((bins_a, lin_a), (bins_b, lin_b)) in enumerate(zip(ia, ib)):
        assert bins_a == bins_b, t                   # bins, their chunk lists, the pseudo-bin's four numbers
        assert lin_a == lin_b, t
    assert nca == ncb == int((b["rec"].tid < 0).sum())
    assert b["info"]["n_records"] == b["rec"].n and b["info"]["n_no_coor"] == nca
    assert b["info"]["n_chunks"] <= b["info"]["n_runs"] <= max(1, b["rec"].n)


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_device_index_meets_the_model(built, name):
    b = built[name]
    refs, no_coor = _bai_abs(b["bai"], b["at"])
    off, stop = _layout(b["rec"], b["text"])
    _check_model(refs, no_coor, b["rec"], off, stop)
    if name == "long_contig":
        bins, lin = refs[0]
        assert 0 in bins and 73 in bins and len(lin) > 4096            # across 2^26: bin 0; the N skip: a 1 Mb bin; windows on both sides
        assert all(lin[w] is not None for w in range(50_000 >> 14, (250_100 - 1 >> 14) + 1))
        assert len(refs[1][1]) == 19                                     # l_ref = 18 windows, the last read hangs into the 19th
    if name == "empty_contig":
        assert refs[2] == ({}, [])


@pytest.mark.gpu
def test_cli_small_pushes_equal_one_push(built, tmp_path):
    """`strling bamindex -o` with STRL_CHUNK_BLOCKS forced small: runs and records straddle pushes; the same index as one push"""
    b = built["small_blocks_small_pushes"]
    outs = []
    for k, blocks in enumerate(("3", "4096")):
        out = str(tmp_path / f"o{k}.bai")
        r = _run(["bamindex", "-v", "-o", out, b["bam"]], env=dict(os.environ, STRL_CHUNK_BLOCKS=blocks))
        assert r.returncode == 0 and "records" in r.stderr, r.stderr
        outs.append(_bai_abs(open(out, "rb").read(), b["at"]))
        assert sorted(os.listdir(tmp_path)) == [f"o{j}.bai" for j in range(k + 1)]        # no temporary file stays
    assert outs[0] == outs[1] == _bai_abs(b["bai"], b["at"])


@pytest.mark.gpu
def test_the_index_works(tmp_path):
    """only the device-built .bai beside the file: region reads, the record count, `extract --gpus 2` cut into shares"""
    rec, g, regions, stop = _region_sample()
    bam, bed = str(tmp_path / "r.bam"), str(tmp_path / "ref.str")
    bamio.write_bam(bam, rec, index=False)
    bamio.write_genome_bed(bed, g, rec.targets)
    r = _run(["bamindex", bam])
    assert r.returncode == 0 and os.path.exists(bam + ".bai"), r.stderr
    assert _regions_match(bam, rec, regions, stop) > 15
    r = _run(["_indexed_records", bam])
    assert r.returncode == 0 and r.stdout.strip() == str(rec.n)
    one, two = str(tmp_path / "one.bin"), str(tmp_path / "two.bin")
    r1 = _run(["extract", "-g", bed, "-v", bam, one])
    r2 = _run(["extract", "-g", bed, "-v", "--gpus", "2", bam, two])
    assert r1.returncode == 0 and r2.returncode == 0, (r1.stderr, r2.stderr)
    assert "in turn" not in r2.stderr and "a contiguous share of the file each" in r2.stderr, r2.stderr
    assert open(one, "rb").read() == open(two, "rb").read()


@pytest.mark.gpu
def test_call_make_index(tmp_path):
    rec, g = synth.synth_wgs(1500, seed=2, n_contigs=2, contig_len=30_000)
    bam, bed, binp = str(tmp_path / "s.bam"), str(tmp_path / "ref.str"), str(tmp_path / "s.bin")
    bamio.write_bam(bam, rec)
    bamio.write_genome_bed(bed, g, rec.targets)
    assert _run(["extract", "-g", bed, bam, binp]).returncode == 0
    r = _run(["call", "-o", str(tmp_path / "py"), bam, binp])
    assert r.returncode == 0, r.stderr
    os.remove(bam + ".bai")
    r = _run(["call", "-v", "--make-index", "-o", str(tmp_path / "dev"), bam, binp])
    assert r.returncode == 0 and "--make-index" in r.stderr, r.stderr
    assert os.path.exists(bam + ".bai")
    outs = sorted(f[2:] for f in os.listdir(tmp_path) if f.startswith("py"))
    assert len(outs) == 3 and outs == sorted(f[3:] for f in os.listdir(tmp_path) if f.startswith("dev")), os.listdir(tmp_path)
    for f in outs:
        assert open(tmp_path / ("py" + f), "rb").read() == open(tmp_path / ("dev" + f), "rb").read(), f
    # a directory that cannot be written to: the reason, no index
    ro = tmp_path / "ro"
    ro.mkdir()
    shutil.copy(bam, ro / "s.bam")
    os.chmod(ro, 0o555)
    try:
        if not os.access(ro, os.W_OK):                  # (root writes anywhere)
            r = _run(["call", "--make-index", "-o", str(tmp_path / "ro_out"), str(ro / "s.bam"), binp])
            assert r.returncode == 1 and "cannot write" in r.stderr and "Permission denied" in r.stderr, r.stderr
    finally:
        os.chmod(ro, 0o755)


def _tiny(rows, targets):
    n = len(rows)
    return RecordBatch.from_fields([r[0] for r in rows], [r[1] for r in rows], [r[0] for r in rows], [r[1] for r in rows], [0x1] * n, [60] * n, ["50M"] * n, ["ACGTA" * 10] * n,
                                   [f"q{i}" for i in range(n)], [0] * n, targets)


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["shuffled", "tid_goes_back", "placed_behind_unplaced", "pos_2p29", "end_2p29", "far_past_l_ref", "flipped_byte", "cram"])
def test_refusals(tmp_path, what):
    """exit 1 with a message that names the cause, no signal, no partial output"""
    bam = str(tmp_path / "x.bam")
    if what == "shuffled":
        rec, _ = synth.synth_wgs(800, seed=37, n_contigs=2, contig_len=60_000)
        order = np.random.default_rng(37).permutation(rec.n)[:300]
        bamio.write_bam(bam, _tiny([(int(rec.tid[i]), int(rec.pos[i])) for i in order], rec.targets), index=False)
        want = "not coordinate sorted"
    elif what == "tid_goes_back":
        bamio.write_bam(bam, _tiny([(0, 100), (1, 5), (0, 200)], [("a", 1000), ("b", 1000)]), index=False)
        want = "not coordinate sorted: record 2 "
    elif what == "placed_behind_unplaced":
        bamio.write_bam(bam, _tiny([(0, 100), (-1, -1), (0, 200)], [("a", 1000)]), index=False)
        want = "not coordinate sorted: record 2 "
    elif what == "pos_2p29":
        bamio.write_bam(bam, _tiny([(0, 100), (0, (1 << 29) + 5)], [("huge", 1 << 30)]), index=False)
        want = "2^29"
    elif what == "end_2p29":
        bamio.write_bam(bam, _tiny([(0, 100), (0, (1 << 29) - 20)], [("huge", 1 << 30)]), index=False)
        want = "CSI"
    elif what == "far_past_l_ref":
        bamio.write_bam(bam, _tiny([(0, 100), (0, 5_000_000)], [("short", 1000)]), index=False)
        want = "past the end of its reference"
    elif what == "flipped_byte":
        rec, _ = synth.synth_wgs(800, seed=38, n_contigs=2, contig_len=60_000)
        bamio.write_bam(bam, rec, index=False, level=6)
        raw = bytearray(open(bam, "rb").read())
        first = struct.unpack_from("<H", raw, 16)[0] + 1              # a payload byte in the middle of the second block
        second = struct.unpack_from("<H", raw, first + 16)[0] + 1
        raw[first + 18 + (second - 26) // 2] ^= 0x40
        open(bam, "wb").write(raw)
        want = "BGZF block"
    else:
        open(bam, "wb").write(b"CRAM\x03\x00" + bytes(64))
        want = ".crai"
    r = _run(["bamindex", bam])
    assert r.returncode == 1, (r.returncode, r.stderr)
    assert want in r.stderr, r.stderr
    assert os.listdir(tmp_path) == ["x.bam"]
