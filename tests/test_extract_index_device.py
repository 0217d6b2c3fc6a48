"""strl_front_index_*: the .bai built inside `strling extract`'s own pass over the BAM, through api.py.

The reference is the index strl_bamindex_* builds of the same file fed the same pushes, compared BYTE FOR BYTE.  Across
different push sizes the comparison is byte for byte as well: `bamindex` of the parent commit was checked first and gives the same
bytes for pushes of 1, 3, 7 and all blocks of each file used here (bai_voff names the last block that starts at or in front of
a byte, however the blocks were grouped into pushes, and the end of a push is the next block's offset).
test_push_size_does_not_change_the_bytes asserts that premise of `bamindex` again before it asks it of the new builder.
The extraction must not notice the builder: treads and names with the index on equal those with it off.
"""
import struct

import numpy as np
import pytest

from strling_amd import api, bamio, synth
from strling_amd.records import RecordBatch

pytestmark = pytest.mark.gpu

STRL_ERR_ARG = -3
FIELDS = ("tid", "position", "repeat", "flag", "split", "mapping_quality", "repeat_count", "align_length", "qname_id")


def _with(rec, tid=None, pos=None, mtid=None, targets=None):
    return RecordBatch(rec.tid if tid is None else tid, rec.pos if pos is None else pos, rec.mtid if mtid is None else mtid, rec.mpos, rec.flag, rec.mapq,
                       rec.cigar_off, rec.cigar, rec.seq_off, rec.l_seq, rec.seq4, rec.qname_off, rec.qnames, rec.isize, rec.targets if targets is None else targets)


def _from_rows(rows, targets):
    """rows of (tid, pos, cigar, flag); the sequence is as long as the CIGAR's query"""
    n = len(rows)
    qlen = lambda c: 1 if c == "*" else sum(int(x[:-1]) for x in __import__("re").findall(r"\d+[MIS=X]", c)) or 1
    return RecordBatch.from_fields([r[0] for r in rows], [r[1] for r in rows], [r[0] for r in rows], [r[1] for r in rows], [r[3] for r in rows], [60] * n,
                                   [r[2] for r in rows], [("ACGT" * 64)[:qlen(r[2])] for r in rows], [f"r{i}" for i in range(n)], [0] * n, targets)


def _wgs():
    """a few thousand records on three contigs with reads and one, in the middle, without; placed-unmapped mates and a tail of
    unplaced reads come with synth_wgs.  seed 51"""
    rec = synth.synth_wgs(1500, seed=51, n_contigs=3, contig_len=200_000)[0]
    tid, mtid = rec.tid.copy(), rec.mtid.copy()
    tid[rec.tid == 2] = 3
    mtid[rec.mtid == 2] = 3
    t = rec.targets
    assert ((rec.flag & 4) != 0)[rec.tid >= 0].any() and (rec.tid < 0).any()
    return _with(rec, tid=tid, mtid=mtid, targets=[t[0], t[1], ("empty", 123_456), t[2]])


def _long():
    """a contig longer than 2^26 with records on both sides of that position and one across it, a record with a 200 kb N skip, a
    placed-unmapped mate, a read that hangs over the end of its contig, two unplaced reads.  seed 52"""
    rng = np.random.default_rng(52)
    M = 1 << 26
    rows = [(0, 1000, "100M", 0x1), (0, 50_000, "50M200000N50M", 0x1), (0, M - 5000, "100M", 0x1), (0, M - 50, "100M", 0x1), (0, M + 1000, "100M", 0x1)]
    rows += [(0, int(p), "100M", 0x1) for p in rng.integers(0, 400_000, 150)] + [(0, int(p), "60M5D40M", 0x1) for p in rng.integers(M - 100_000, M + 150_000, 150)]
    rows += [(1, 10, "100M", 0x1 | 0x8), (1, 10, "*", 0x1 | 0x4), (1, 20_000, "30S70M", 0x1), (1, 18 * 16384 - 12, "100M", 0x1)]
    rows.sort(key=lambda r: (r[0], r[1]))
    rows += [(-1, -1, "*", 0x1 | 0x4 | 0x8)] * 2
    return _from_rows(rows, [("big", M + 200_000), ("c2", 18 * 16384)])


def _header_only():
    t = synth.synth_wgs(10, seed=53, n_contigs=2, contig_len=50_000)[0].targets
    return RecordBatch.from_fields([], [], [], [], [], [], [], [], [], targets=t)


def _alternating(n=4000):
    """every record starts a run: all at one position, alternately inside a 16 KiB window (bin 4681) and across its end (bin 585)"""
    p = 16384 - 10
    rows = [(0, p, "5M" if i % 2 == 0 else "50M", 0x1) for i in range(n)] + [(-1, -1, "*", 0x1 | 0x4 | 0x8)] * 2
    return _from_rows(rows, [("c", 100_000)])


FILES = {"wgs_big_blocks": (_wgs, 0xFF00), "wgs_small_blocks": (_wgs, 2500), "long": (_long, 2500), "header_only": (_header_only, 0xFF00),
         "alternating": (_alternating, 2500)}
# (file, blocks per push)
CASES = [("wgs_big_blocks", 1), ("wgs_big_blocks", 3), ("wgs_big_blocks", 7), ("wgs_small_blocks", 1), ("wgs_small_blocks", 3), ("wgs_small_blocks", 7),
         ("long", 1), ("long", 7), ("header_only", 3)]


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("extract_index")
    out = {}
    for name, (make, block) in FILES.items():
        rec = make()
        bam = str(d / f"{name}.bam")
        bamio.write_bam(bam, rec, block=block, index=False)
        out[name] = dict(rec=rec, bam=bam)
    return out


def _prepare(ctx):
    ctx.set_opts(0.8, 40, 350)
    ctx.set_genome(None)


@pytest.fixture(scope="module")
def runs(files, ctx):
    """every (file, push size) once: the index of `bamindex`, the extraction alone, the extraction with the index -- shared below"""
    _prepare(ctx)
    out = {}
    for name, per_push in CASES + [("alternating", 1)]:
        bam = files[name]["bam"]
        ref, ref_info = ctx.bamindex(bam, chunk_blocks=per_push)
        plain = ctx.extract_bam_device(bam, chunk_blocks=per_push)
        res, bai, info, refused = ctx.extract_bam_device_indexed(bam, chunk_blocks=per_push, runs0=64 if name == "alternating" else 0)
        out[(name, per_push)] = dict(ref=ref, ref_info=ref_info, plain=plain, res=res, bai=bai, info=info, refused=refused)
    return out


def _same_extraction(a, b):
    for f in FIELDS:
        assert np.array_equal(a["treads"][f], b["treads"][f]), f
    assert a["qnames"] == b["qnames"]
    assert np.array_equal(a["fragwords"], b["fragwords"]) and a["n_records"] == b["n_records"] and a["n_tail"] == b["n_tail"]


def test_the_entry_points_exist(ctx):
    for f in ("strl_front_index_begin", "strl_front_index_blocks", "strl_front_index_finish"):
        assert hasattr(ctx.L, f)


@pytest.mark.parametrize("name,per_push", CASES)
def test_index_of_the_pass_equals_bamindex_bytes(files, runs, name, per_push):
    r = runs[(name, per_push)]
    assert r["refused"] is None, r["refused"]
    assert r["bai"] == r["ref"]
    assert r["info"] == r["ref_info"]
    rec = files[name]["rec"]
    assert r["info"]["n_records"] == rec.n and r["info"]["n_no_coor"] == int((rec.tid < 0).sum())
    if name == "long":      # the shapes are there: bin 0 across 2^26, a 1 Mb bin for the N skip, windows on both sides of 2^26
        n_bin = struct.unpack_from("<i", r["bai"], 8)[0]
        bins, o = [], 12
        for _ in range(n_bin):
            b, nc = struct.unpack_from("<Ii", r["bai"], o)
            bins.append(b)
            o += 8 + 16 * nc
        assert 0 in bins and 73 in bins and struct.unpack_from("<i", r["bai"], o)[0] > 4096
    if name == "header_only":
        assert r["bai"] == b"BAI\1" + struct.pack("<i", 2) + bytes(16) + bytes(8)


@pytest.mark.parametrize("name", ["wgs_big_blocks", "wgs_small_blocks", "long"])
def test_push_size_does_not_change_the_bytes(runs, name):
    """`bamindex` gives the same bytes for pushes of 1, 3 and 7 blocks (the premise, asserted first), so the index of the pass must
    as well -- byte identity, not a comparison of structures"""
    sizes = [p for n, p in CASES if n == name]
    for p in sizes[1:]:
        assert runs[(name, p)]["ref"] == runs[(name, sizes[0])]["ref"], p
        assert runs[(name, p)]["bai"] == runs[(name, sizes[0])]["bai"], p


@pytest.mark.parametrize("name,per_push", CASES)
def test_the_extraction_is_untouched(runs, name, per_push):
    r = runs[(name, per_push)]
    _same_extraction(r["res"], r["plain"])
    if name.startswith("wgs"):
        assert len(r["plain"]["treads"]) > 10


def test_table_growth(files, runs):
    """4000 records that each start a run, pushes of one 2500-byte block, a table of 64 runs at first: it grows many times, ahead of
    the counts the host has seen"""
    r = runs[("alternating", 1)]
    rec = files["alternating"]["rec"]
    assert r["refused"] is None, r["refused"]
    assert len(r["plain"]["chunks"]) > 50
    assert r["bai"] == r["ref"]
    assert r["info"]["n_runs"] == r["ref_info"]["n_runs"] == 4000 + 1 and rec.n == 4002
    _same_extraction(r["res"], r["plain"])


def _refusal_case(what):
    rec = synth.synth_wgs(1500, seed=54, n_contigs=1, contig_len=300_000, interchrom_frac=0.0, unmapped_frac=0.0)[0]
    assert (rec.tid == 0).all()
    pos = rec.pos.copy()
    if what == "unsorted_in_the_first_push":
        k = next(i for i in range(3, 20) if pos[i - 1] > 0)
        pos[k] = pos[k - 1] - 1                      # only record k lies behind a record of a later position
        return _with(rec, pos=pos), k, "not coordinate sorted: record %d " % k
    pos[rec.n - 1] = (1 << 29) + 5
    return _with(rec, pos=pos, targets=[("huge", 1 << 30)]), rec.n - 1, "record %d lies at or reaches past position 2^29" % (rec.n - 1)


@pytest.mark.parametrize("what", ["unsorted_in_the_first_push", "pos_2p29_in_the_last_push"])
def test_late_refusals(ctx, tmp_path, what):
    """the refusal is seen a chunk late or at the end; strl_front_index_finish gives bamindex's code and message, ordinal included"""
    rec, k, want = _refusal_case(what)
    bam = str(tmp_path / "x.bam")
    bamio.write_bam(bam, rec, block=2500, index=False)
    _prepare(ctx)
    with pytest.raises(api.StrlingError) as e:
        ctx.bamindex(bam, chunk_blocks=3)
    plain = ctx.extract_bam_device(bam, chunk_blocks=3)
    assert len(plain["chunks"]) > 50
    res, bai, info, refused = ctx.extract_bam_device_indexed(bam, chunk_blocks=3)
    assert bai is None and refused is not None
    assert str(e.value) == f"strling_amd error {refused[0]}: {refused[1]}"
    assert want in refused[1]
    _same_extraction(res, plain)
    assert len(plain["treads"]) > 10


def test_begin_without_front_begin(ctx):
    l_ref = np.array([1000], np.int32)
    c = api.Context(0)
    try:
        assert c.L.strl_front_index_begin(c.h, l_ref.ctypes.data, 0) == STRL_ERR_ARG
        assert "without strl_front_begin" in c.L.strl_last_error().decode()
    finally:
        c.close()
    # ... and on a context whose extraction has finished
    assert ctx.L.strl_front_index_begin(ctx.h, l_ref.ctypes.data, 0) == STRL_ERR_ARG


def test_a_push_without_its_offsets_ends_the_index(files, runs, ctx):
    _prepare(ctx)
    bam = files["wgs_small_blocks"]["bam"]
    res, bai, info, refused = ctx.extract_bam_device_indexed(bam, chunk_blocks=7, no_offsets_at=4)
    assert bai is None and refused is not None and refused[0] == STRL_ERR_ARG and "without its block offsets" in refused[1]
    _same_extraction(res, runs[("wgs_small_blocks", 7)]["plain"])
