"""Inputs for `strling sort --write-index` beyond tests/sort_bam_cases.py, and the readers its tests share: what the sort cases never
reach of an index -- records and streams that end on a member boundary, a header longer than a member, an N skip across dozens
of windows, bins of every level with a bin that is left and revisited, a reference without records between two with, records
that are all unplaced, placed-unmapped records.  Same form as sort_bam_cases.cases(): (name, RecordBatch, header text or None), a
few thousand short records at most, shuffled (the sort has work to do).

The reference of the index is never the code under test: bamio.write_bai / bamio.csi_payload over the records parsed from the
OUTPUT file by this module, with the record offsets and the member offsets of this module's own BGZF walk."""
import gzip
import os
import struct
import tempfile
import types

import numpy as np

import sort_bam_cases as S
from strling_amd import bamio
from strling_amd.records import RecordBatch

BLK = S.BLK
META_BIN = 37450


def _batch(rows, tg, seed=0):
    """rows of (tid, pos, flag, cigar string): shuffled, distinct names, the sequence as long as the CIGAR's query"""
    from strling_amd.records import encode_cigar
    rng = np.random.default_rng(seed)
    rows = [rows[i] for i in rng.permutation(len(rows))]
    seqs = []
    for _, _, _, c in rows:
        q = sum(op >> 4 for op in encode_cigar(c) if (op & 15) in (0, 1, 4, 7, 8)) if c != "*" else 30
        seqs.append("ACGT" * (q // 4) + "ACGT"[:q % 4])
    n = len(rows)
    return RecordBatch.from_fields([r[0] for r in rows], [r[1] for r in rows], [r[0] for r in rows], [max(r[1], 0) for r in rows], [r[2] for r in rows], [30] * n,
                                   [r[3] for r in rows], seqs, [f"r{i:06d}" for i in range(n)], isize=[0] * n, targets=tg)


def _sq(tg):
    return "".join(f"@SQ\tSN:{n}\tLN:{l}\n" for n, l in tg)


def _sorted_layout(rec, text):
    """(bytes of the output's header, [bytes of each record in sorted order]) of the case, from the reference of the sort"""
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "x.bam")
        S.write_case(p, rec, text)
        stream = S.reference_stream(p)[0]
    lens = [len(r) for r in S.split_stream(stream)[3]]
    return len(stream) - sum(lens), lens


def _padded(rec, tg, edge):
    """a header whose @CO line is padded until edge(header bytes, record lengths) -> a stream offset lands on a multiple of 0xFF00"""
    base = "@HD\tVN:1.6\tSO:unsorted\n" + _sq(tg) + "@CO\t"
    hdr, lens = _sorted_layout(rec, base + "\n")
    return base + "x" * ((-edge(hdr, lens)) % BLK) + "\n"


def cases():
    out = []
    tg3 = S.targets(3)
    # a record ends exactly on a member boundary: the next begins at (member k + 1, 0); and a stream that does: its end is (EOF block, 0)
    t, p, f = S._shuffled(1500, 3, 41)
    rec = S.batch(t, p, f, tg3, seed=41)
    out.append(("record_ends_on_member_boundary", rec, _padded(rec, tg3, lambda h, l: h + sum(l[:len(l) // 2]))))
    t, p, f = S._shuffled(1500, 3, 42)
    rec = S.batch(t, p, f, tg3, seed=42)
    out.append(("stream_ends_on_member_boundary", rec, _padded(rec, tg3, lambda h, l: h + sum(l))))
    # a header longer than a member: the first record starts in member >= 1
    t, p, f = S._shuffled(400, 3, 43)
    out.append(("header_longer_than_a_member", S.batch(t, p, f, tg3, seed=43), "@HD\tVN:1.6\n" + _sq(tg3) + "@CO\t" + "long " * 14000 + "\n"))
    # an N skip across dozens of 16 KiB windows, among short records on both sides of it
    big = [("big", 1 << 28), ("empty", 50_000), ("c2", 300_000)]
    rng = np.random.default_rng(44)
    rows = [(0, int(x), 0, "40M") for x in rng.integers(0, 900_000, 300)] + [(0, 100_000, 0, "20M600000N20M"), (0, 100_000, 16, "30M"), (0, 400_000, 0, "10M1000N10M")]
    out.append(("n_skip_across_windows", _batch(rows, big, seed=44), None))
    # bins of every level (a .bai's: 16 Kb, 128 Kb, 1 Mb, 8 Mb, 64 Mb, bin 0), and small bin / large bin / small bin: the 16 Kb bin
    # of position 20 000 is left for a 1 Mb bin and entered again; a reference without records between two with
    M = 1 << 26
    rows = [(0, 20_000, 0, "30M"), (0, 20_001, 0, "30M"), (0, 20_002, 0, "20M200000N20M"), (0, 20_003, 0, "30M"), (0, 20_004, 16, "30M"),
            (0, 16_380, 0, "30M"),                       # across a 16 Kb edge: 128 Kb bin
            (0, (1 << 17) - 10, 0, "30M"),               # across a 128 Kb edge: 1 Mb bin
            (0, (1 << 20) - 10, 0, "30M"),               # 8 Mb bin
            (0, (1 << 23) - 10, 0, "30M"),               # 64 Mb bin
            (0, M - 10, 0, "30M"),                       # bin 0
            (0, M + 5000, 0, "30M"), (0, 3 * M + 77, 0, "25M2D25M")]
    rows += [(0, int(x), int(s) * 16, "35M") for x, s in zip(rng.integers(0, 2_000_000, 1200), rng.integers(0, 2, 1200))]
    rows += [(2, int(x), 0, "35M") for x in rng.integers(0, 290_000, 300)] + [(-1, -1, 4, "*")] * 5
    out.append(("bins_of_every_level", _batch(rows, big, seed=45), None))
    # all records unplaced, with references in the header
    out.append(("all_unplaced", _batch([(-1, -1, 4, "*")] * 300, tg3, seed=46), None))
    # placed-unmapped records (flag 4, the mate's reference and position): counted in the pseudo-bin
    rows = [(int(a), int(b), 4 if i % 3 == 0 else 0, "*" if i % 3 == 0 else "30M") for i, (a, b) in enumerate(zip(rng.integers(0, 3, 600), rng.integers(0, 500, 600)))]
    out.append(("placed_unmapped", _batch(rows, tg3, seed=47), None))
    return out


def all_cases():
    """the sort's cases and this module's"""
    return S.cases() + cases()


# of the sort's cases exactly these are refused (tests assert the set): a negative position on a placed record; a 2^31 - 1 contig
REFUSED = {"placed_unmapped_and_pos_minus1", "pos_2p31_minus_2"}
SEAM_ENV = dict(STRL_CHUNK_BLOCKS="1", STRL_SORT_SLAB_MB="0.15", STRL_SORT_PIECE_KB="1")


def case_dir(tmp_path_factory):
    d = tmp_path_factory.mktemp("sort_index_cases")
    paths = {}
    for name, rec, text in all_cases():
        paths[name] = os.path.join(str(d), name + ".bam")
        S.write_case(paths[name], rec, text)
    return paths


# ---- the test's own readers of the output ---------------------------------------------------------------------------------------------
def walk(path):
    """the file's own BGZF walk -> (file offset of every member, the EOF block's last; inflated stream; {file offset: stream offset})"""
    data = open(path, "rb").read()
    offs, at, o, u, raw = [], {}, 0, 0, []
    while o < len(data):
        bsize = struct.unpack_from("<H", data, o + 16)[0] + 1
        isize = struct.unpack_from("<I", data, o + bsize - 4)[0]
        offs.append(o)
        at[o] = u
        u += isize
        o += bsize
    at[o] = u
    assert data[offs[-1]:] == S.EOF_BLOCK
    return offs, gzip.decompress(data), at


def records_view(stream):
    """what bamio.write_bai / csi_payload read of a RecordBatch, from the bytes of the output's records; rec_off[n + 1]"""
    l_text = struct.unpack_from("<i", stream, 4)[0]
    at = 8 + l_text
    n_ref = struct.unpack_from("<i", stream, at)[0]
    at += 4
    targets = []
    for _ in range(n_ref):
        ln = struct.unpack_from("<i", stream, at)[0]
        targets.append((stream[at + 4:at + 4 + ln - 1].decode(), struct.unpack_from("<i", stream, at + 4 + ln)[0]))
        at += 8 + ln
    tid, pos, flag, cig_off, cig, rec_off = [], [], [], [0], [], []
    while at < len(stream):
        rec_off.append(at)
        bs, t, p, l_name = struct.unpack_from("<iiiB", stream, at)
        n_cig, fl = struct.unpack_from("<HH", stream, at + 16)
        tid.append(t); pos.append(p); flag.append(fl)
        cig.extend(struct.unpack_from(f"<{n_cig}I", stream, at + 36 + l_name))
        cig_off.append(len(cig))
        at += 4 + bs
    rec_off.append(at)
    assert at == len(stream)
    v = types.SimpleNamespace(n=len(tid), tid=np.array(tid, np.int64), pos=np.array(pos, np.int64), flag=np.array(flag, np.int64), cigar_off=np.array(cig_off, np.int64),
                              cigar=np.array(cig, np.uint32), targets=targets)
    return v, rec_off


def bai_abs(d, at):
    """bytes of a .bai -> ([(bins, lin)] per reference, n_no_coor), every virtual offset an offset of the inflated stream (so a chunk
    that ends at the end of a block may name (that block, isize) or (the next block, 0)); bins[b] = ascending chunk list with chunks
    that touch merged, bins[37450] = [[first, end], [n_mapped, n_unmapped]].  tests/test_bamindex.py's _bai_abs"""
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


def csi_abs(d, at):
    """the uncompressed bytes of a CSI index -> (min_shift, depth, [bins] per reference, n_no_coor) in the manner of bai_abs;
    bins[b] = (loffset as a stream offset or None, chunk list), the pseudo-bin's = (None, [[first, end], [n_mapped, n_unmapped]])"""
    assert d[:4] == b"CSI\1"
    m, depth, l_aux, n_ref = struct.unpack_from("<iiii", d, 4)
    assert l_aux == 0
    meta = ((1 << 3 * (depth + 1)) - 1) // 7 + 1
    o = 20
    ab = lambda v: at[v >> 16] + (v & 0xffff)
    refs = []
    for _ in range(n_ref):
        n_bin = struct.unpack_from("<i", d, o)[0]; o += 4
        bins, order = {}, []
        for _ in range(n_bin):
            b, loff, nc = struct.unpack_from("<IQi", d, o); o += 16
            order.append(b)
            if b == meta:
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
            assert nc > 0 and b not in bins
            bins[b] = (ab(loff) if loff else None, ch)
        plain = [b for b in order if b != meta]
        assert plain == sorted(plain) and (meta not in order or order[-1] == meta)
        refs.append(bins)
    no_coor = struct.unpack_from("<Q", d, o)[0]; o += 8
    assert o == len(d)
    return m, depth, refs, no_coor


def reference_index(bam, kind):
    """reference 1 for the sorted file at `bam`: kind = "bai" | ("csi", min_shift) -> the structure (bai_abs / csi_abs) of what the
    Python writer gives for the file's records, the file's own record offsets and member offsets"""
    offs, stream, at = walk(bam)
    view, rec_off = records_view(stream)
    if kind == "bai":
        with tempfile.TemporaryDirectory() as d:
            p = os.path.join(d, "ref.bai")
            bamio.write_bai(p, view, rec_off, offs, BLK)
            return bai_abs(open(p, "rb").read(), at)
    return csi_abs(bamio.csi_payload(view, rec_off, offs, BLK, min_shift=kind[1]), at)


def index_structure(path, bam, kind):
    """the index file at `path` beside the sorted `bam`, as reference_index gives its reference"""
    _, _, at = walk(bam)
    data = open(path, "rb").read()
    return bai_abs(data, at) if kind == "bai" else csi_abs(gzip.decompress(data), at)
