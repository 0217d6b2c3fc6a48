"""`call --sweep` on the device (strl_sweep_*, csrc/sweep.hip) through api.Context.sweep: the evidence of every bound from one
pass over a BAM written with 1500-byte BGZF blocks.  A status-0 bound equals strl_evidence_records on exactly the bytes of
records [i0, i1) -- Python restates the rule (tests/test_sweep_emu.py checks that restatement against the kernels' bodies on the
CPU) -- and equals the oracle's spanners() in everything but `rec`; with chunks of 1, 2 and 3 blocks exactly the bounds whose
deciding chunk gets a carried-in maximum above `beg` are seams; the capacity edge; reference changes; placed-unmapped and
zero-length records; empty references; bounds behind the last placed record; order; two runs; the error returns."""
import struct

import numpy as np
import pytest

import test_evidence_device as ted
from strling_amd import api, bamio, synth
from strling_amd.records import RecordBatch

BLOCK = 1500
REF_OPS = (0, 2, 3, 7, 8)


def _ends(rec):
    """bam_endpos with Rec::stop's rule: one base behind pos for an unmapped record and for one whose CIGAR consumes no reference"""
    ops, ln = rec.cigar & 0xF, (rec.cigar >> 4).astype(np.int64)
    w = np.where(np.isin(ops, REF_OPS), ln, 0).astype(np.float64)
    rl = np.bincount(np.repeat(np.arange(rec.n), np.diff(rec.cigar_off).astype(np.int64)), weights=w, minlength=rec.n).astype(np.int64)
    rl[(rec.flag & 4) != 0] = 0
    return rec.pos.astype(np.int64) + np.where(rl > 0, rl, 1)


class _File:
    """a batch written as a BAM, and where its records fall when the file is pushed `chunk_blocks` blocks at a time"""

    def __init__(self, rec, path, **kw):
        self.rec, self.path = rec, path
        bamio.write_bam(path, rec, block=BLOCK, index=False, **kw)
        self.L = ted._Layout(rec)
        self.end = _ends(rec)
        pos = np.where(rec.tid >= 0, rec.pos, 0).astype(np.int64)                 # (the unplaced records are in no order among themselves)
        self.key = np.where(rec.tid >= 0, rec.tid, 0x7FFFFFFF).astype(np.int64) << 32 | (pos + (1 << 31))       # unplaced: behind every reference
        assert np.all(np.diff(self.key) >= 0)
        B = api.Context._bam_blocks(path)
        isz = np.array([b[2] for b in B["blocks"]], np.int64)
        self.b0, self.ustart = B["b0"], np.concatenate([[0], np.cumsum(isz)])
        self.hdr = int(self.ustart[-1]) - len(self.L.raw)

    def chunk_starts(self, chunk_blocks):
        """index of the first record that completes in each chunk (a record belongs to the chunk its last byte lies in)"""
        nblk = self.ustart.size - 1
        ends = [int(self.ustart[min(nblk, s0 + chunk_blocks)]) for s0 in range(self.b0, nblk, chunk_blocks)]
        rec_end = self.hdr + self.L.off[1:]
        return [0] + [int(np.searchsorted(rec_end, e, side="right")) for e in ends[:-1]]

    def rule(self, bounds, window, chunk_blocks):
        """[(i0, i1, status)] by the rule, in global record indices"""
        rec, n = self.rec, self.rec.n
        starts = np.array(self.chunk_starts(chunk_blocks))
        out = []
        for b in bounds:
            t, beg, end = int(b["tid"]), max(0, int(b["left"]) - window), int(b["right"]) + window
            i1 = int(np.searchsorted(self.key, (t << 32) | (end + (1 << 31)), side="left"))
            c0 = int(starts[np.searchsorted(starts, i1, side="right") - 1]) if i1 < n else int(starts[-1])
            mine = np.flatnonzero(rec.tid[:i1] == t)
            before = mine[mine < c0]
            seam = before.size > 0 and int(rec.tid[c0 - 1]) == t and int(self.end[before].max()) > beg
            reach = mine[np.maximum.accumulate(self.end[mine]) > beg] if mine.size else mine
            i0 = int(reach[0]) if reach.size else i1
            out.append((i0, i1, int(seam)))
        return out


def _bounds_for(rec, window, seed, n=150):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        tid = int(rng.integers(0, len(rec.targets)))
        clen = rec.targets[tid][1]
        width = int(rng.integers(0, 41)) if rng.random() < 0.6 else int(rng.integers(0, 1001))
        left = int(rng.integers(0, max(1, clen - width)))
        out.append(ted._bound(tid, left, left + width, "".join("ACGT"[c] for c in rng.integers(0, 4, size=int(rng.integers(1, 7))))))
    for tid, (_, clen) in enumerate(rec.targets):              # clamped to 0, at the end of the contig, identical and overlapping ones
        out += [ted._bound(tid, 0, 30, "AC"), ted._bound(tid, 5, 900, "CAG"), ted._bound(tid, clen - 40, clen, "A"), ted._bound(tid, clen - 40, clen, "A"),
                ted._bound(tid, clen // 2, clen // 2 + 10, "AAGGGC"), ted._bound(tid, clen // 2 + 3, clen // 2 + 20, "AC")]
    return np.array(out, api.BOUNDS_DTYPE)


def _with_empty_contigs(rec):
    """the batch with a reference without records in the middle (tid 1) and one at the end"""
    tid = np.where(rec.tid >= 1, rec.tid + 1, rec.tid).astype(np.int32)
    mtid = np.where(rec.mtid >= 1, rec.mtid + 1, rec.mtid).astype(np.int32)
    tg = list(rec.targets)
    tg = tg[:1] + [("empty1", 9000)] + tg[1:] + [("empty2", 7000)]
    return RecordBatch(tid, rec.pos, mtid, rec.mpos, rec.flag, rec.mapq, rec.cigar_off, rec.cigar, rec.seq_off, rec.l_seq, rec.seq4, rec.qname_off, rec.qnames,
                       rec.isize, tg)


def _no_rec(sup):
    s = np.array(sup, copy=True)
    s["rec"] = 0
    return s.tobytes()


def _equal(a, b):
    return a[3] == b[3] and a[0].tobytes() == b[0].tobytes() and a[1] == b[1] and np.float32(a[2]).view(np.uint32) == np.float32(b[2]).view(np.uint32)


@pytest.fixture(scope="module", params=["p99", 25], ids=["window-p99", "window-25"])
def sample(request, tmp_path_factory, ctx, oracle):
    """~3000 records on three references with records and two without, the unmapped tail behind them; the one-chunk answer.
    With the window `call` takes (the fragment lengths' 99th percentile, 637 here) a query spans more records than three
    1500-byte blocks hold, so every bound with records is a seam; a window of 25 leaves answered bounds with records too."""
    rec, _ = synth.synth_wgs(1500, seed=21, n_contigs=3, contig_len=20_000, unmapped_frac=0.02, indel_frac=0.05)
    rec = _with_empty_contigs(rec)
    assert int((rec.tid < 0).sum()) > 0
    F = _File(rec, str(tmp_path_factory.mktemp("sweep") / "s.bam"))
    frag = synth.frag_hist(rec)
    window = oracle.median(frag, 0.99) if request.param == "p99" else request.param
    bounds = _bounds_for(rec, window, seed=3)
    whole, info = ctx.sweep(F.path, bounds, window, frag, 20, chunk_blocks=1 << 20)
    return dict(F=F, frag=frag, window=window, bounds=bounds, whole=whole, info=info)


@pytest.mark.gpu
def test_whole_file_as_one_chunk(ctx, oracle, sample):
    F, frag, window, bounds, whole, info = (sample[k] for k in ("F", "frag", "window", "bounds", "whole", "info"))
    want = F.rule(bounds, window, 1 << 20)
    assert info["n_chunks"] == 1 and info["n_records"] == F.rec.n and info["n_answered"] == len(bounds) and info["n_seam"] == 0
    ref = ctx.evidence_records([F.L.bytes_of(i0, i1) for i0, i1, _ in want], bounds, window, frag, 20)
    n_sup, empty = 0, 0
    for k, (b, (i0, i1, st), d, r) in enumerate(zip(bounds, want, whole, ref)):
        assert st == 0 and d[3] == 0, (k, b)
        assert _equal(d, r), (k, b, i0, i1)                                     # field for field, `rec` counted from i0
        a_, b_ = F.L.region(int(b["tid"]), max(0, int(b["left"]) - window), int(b["right"]) + window)
        o = oracle.spanners(F.rec.slice(a_, b_), b, window, frag, 20)          # htslib's query, as the evidence tests cut it
        assert _no_rec(d[0]) == _no_rec(o[0]) and d[1] == o[1] and np.float32(d[2]).view(np.uint32) == np.float32(o[2]).view(np.uint32), (k, b)
        n_sup += len(d[0])
        empty += i0 == i1
    assert n_sup > 500 and empty >= 10                                          # the empty references' bounds among them: zero bytes, answered


@pytest.mark.gpu
@pytest.mark.parametrize("chunk_blocks", [1, 2, 3])
def test_seams_are_exactly_the_predicate(ctx, sample, chunk_blocks):
    F, frag, window, bounds, whole = (sample[k] for k in ("F", "frag", "window", "bounds", "whole"))
    want = F.rule(bounds, window, chunk_blocks)
    got, info = ctx.sweep(F.path, bounds, window, frag, 20, chunk_blocks=chunk_blocks)
    assert info["n_chunks"] == len(F.chunk_starts(chunk_blocks)) > 100 // chunk_blocks
    assert [d[3] for d in got] == [st for _, _, st in want]
    n_seam = sum(st for _, _, st in want)
    assert 10 <= n_seam <= len(bounds) - 10 and info["n_seam"] == n_seam and info["n_answered"] == len(bounds) - n_seam
    n_sup = 0
    for k, (d, w) in enumerate(zip(got, whole)):
        if d[3] == 0:
            assert _equal(d, w), k
            n_sup += len(d[0])
        else:
            assert len(d[0]) == 0
    assert window > 100 or n_sup > 0                                            # answered bounds that have records


@pytest.mark.gpu
def test_reverse_order_and_two_runs(ctx, sample):
    F, frag, window, bounds, whole = (sample[k] for k in ("F", "frag", "window", "bounds", "whole"))
    rev, _ = ctx.sweep(F.path, bounds[::-1], window, frag, 20, chunk_blocks=1 << 20)
    again, _ = ctx.sweep(F.path, bounds, window, frag, 20, chunk_blocks=1 << 20)
    for k in range(len(bounds)):
        assert _equal(rev[len(bounds) - 1 - k], whole[k]) and _equal(again[k], whole[k]), k


def _pile_file(tmp_path, n_records, name, lead=None):
    """the first n_records records of a pile at one locus (behind `lead`, a batch of records further left)"""
    rec = ted._pile(2049)
    rec = ted._take(rec, np.arange(n_records))
    if lead is not None:
        both = [lead, rec]
        cig = [list(r.cigar[int(r.cigar_off[i]):int(r.cigar_off[i + 1])]) for r in both for i in range(r.n)]
        rec = RecordBatch.from_fields(np.concatenate([r.tid for r in both]), np.concatenate([r.pos for r in both]), np.concatenate([r.mtid for r in both]),
                                      np.concatenate([r.mpos for r in both]), np.concatenate([r.flag for r in both]), np.concatenate([r.mapq for r in both]), cig,
                                      [r.sequence(i) for r in both for i in range(r.n)], [r.qname(i) for r in both for i in range(r.n)],
                                      isize=np.concatenate([r.isize for r in both]), targets=rec.targets)
    return _File(rec, str(tmp_path / name))


def _long_skip(pos=10):
    """one record far to the left whose N skip carries it to 1010 + : it overlaps every window around the pile"""
    return RecordBatch.from_fields(np.zeros(1, np.int32), np.array([pos], np.int32), np.full(1, -1, np.int32), np.full(1, -1, np.int32), np.zeros(1, np.uint16),
                                   np.full(1, 60, np.uint8), ["10M1000N90M"], ["ACGT" * 25], [b"skip"], isize=np.zeros(1, np.int32), targets=[("chr1", 100_000)])


@pytest.mark.gpu
def test_the_capacity_edge(ctx, oracle, tmp_path):
    frag = synth.frag_hist(ted._pile(2049))
    frag[250:450] += 3
    window = oracle.median(frag, 0.99)
    b = np.array([ted._bound(0, 1120, 1130, "AC")], api.BOUNDS_DTYPE)
    for n, lead, status in ((4096, None, 0), (4097, None, 2), (4096, _long_skip(), 2), (1000, _long_skip(), 0)):
        F = _pile_file(tmp_path, n, f"p{n}{lead is not None}.bam", lead)
        (i0, i1, st), = F.rule(b, window, 1 << 20)
        assert (i0, i1, st) == (0, F.rec.n, 0)                                  # the long record pulls i0 back to itself
        (d,), _ = ctx.sweep(F.path, b, window, frag, 20, chunk_blocks=1 << 20)
        assert d[3] == status, (n, lead is not None)
        if status == 0:
            o = oracle.spanners(F.rec, b[0], window, frag, 20)
            assert _no_rec(d[0]) == _no_rec(o[0]) and d[1] == o[1] and np.float32(d[2]).view(np.uint32) == np.float32(o[2]).view(np.uint32)
            assert len(d[0]) > 50
        else:
            assert len(d[0]) == 0


@pytest.mark.gpu
def test_reference_change_unmapped_and_zero_length_records(ctx, oracle, tmp_path):
    """a window with a placed-unmapped record and one without a CIGAR in it; the reference changes inside a chunk and (blocks of
    the size of the first reference's records) at a chunk's first record; bounds behind the last placed record with the unmapped
    tail behind them"""
    n = 40
    seq = "ACGTTGCA" * 12 + "ACGT"
    tid = np.array([0] * n + [1] * n + [-1] * 6, np.int32)
    pos = np.concatenate([200 + 7 * np.arange(n), 150 + 7 * np.arange(n), np.full(6, -1)]).astype(np.int32)
    flag = np.array(([0, 16] * (n // 2)) * 2 + [4] * 6, np.uint16)
    cig = [[(100 << 4)] for _ in range(2 * n)] + [[] for _ in range(6)]
    flag[10], flag[n + 12] = 4, 4                                               # placed-unmapped
    cig[14], cig[n + 15] = [], []                                               # mapped, no CIGAR
    mapq = np.where(tid >= 0, 60, 0).astype(np.uint8)
    rec = RecordBatch.from_fields(tid, pos, np.full(tid.size, -1, np.int32), np.full(tid.size, -1, np.int32), flag, mapq, cig, [seq] * tid.size,
                                  [b"q%d" % i for i in range(tid.size)], isize=np.zeros(tid.size, np.int32), targets=[("chr1", 5000), ("chr2", 5000), ("chr3", 5000)])
    for pad in range(0, 1600, 53):                                              # (the header's length moves the block boundaries over the records)
        F = _File(rec, str(tmp_path / "t.bam"), header_text=bamio.sam_header(rec.targets) + "@CO\t" + "x" * pad + "\n")
        if n in F.chunk_starts(1):
            break
    assert n in F.chunk_starts(1) and n not in F.chunk_starts(1 << 20)
    frag = synth.frag_hist(ted._pile(300))
    window = 150
    bounds = np.array([ted._bound(0, 280, 300, "AC"), ted._bound(1, 240, 260, "CA"), ted._bound(0, 900, 910, "A"), ted._bound(1, 2000, 2010, "AC"),
                       ted._bound(2, 100, 200, "AC"), ted._bound(0, 0, 10, "ACG")], api.BOUNDS_DTYPE)
    whole, _ = ctx.sweep(F.path, bounds, window, frag, 0, chunk_blocks=1 << 20)
    want = F.rule(bounds, window, 1 << 20)
    ref = ctx.evidence_records([F.L.bytes_of(i0, i1) for i0, i1, _ in want], bounds, window, frag, 0)
    for k, (b, d, r) in enumerate(zip(bounds, whole, ref)):
        a_, b_ = F.L.region(int(b["tid"]), max(0, int(b["left"]) - window), int(b["right"]) + window)
        o = oracle.spanners(rec.slice(a_, b_), b, window, frag, 0)
        assert d[3] == 0 and _equal(d, r), k
        assert _no_rec(d[0]) == _no_rec(o[0]) and d[1] == o[1] and np.float32(d[2]).view(np.uint32) == np.float32(o[2]).view(np.uint32), k
    assert len(whole[0][0]) > 5 and len(whole[1][0]) > 5 and [len(whole[k][0]) for k in (2, 3, 4)] == [0, 0, 0]
    # every cut of the file: the reference change comes to lie inside a chunk and at a chunk's first record
    cuts = set()
    for cb in range(1, 9):
        starts = F.chunk_starts(cb)
        cuts |= set(starts)
        want = F.rule(bounds, window, cb)
        got, _ = ctx.sweep(F.path, bounds, window, frag, 0, chunk_blocks=cb)
        assert [d[3] for d in got] == [st for _, _, st in want], cb
        assert all(_equal(d, w) for d, w in zip(got, whole) if d[3] == 0), cb
    assert n in cuts and len(cuts) > 10, sorted(cuts)


def _shuffled(tmp_path):
    rec, _ = synth.synth_wgs(300, seed=8, n_contigs=2, contig_len=20_000)
    idx = np.arange(rec.n)
    idx[[200, 260]] = idx[[260, 200]]
    bad = ted._take(rec, idx)
    assert bad.tid[200] == bad.tid[260] == 0 and bad.pos[200] > bad.pos[201]
    p = str(tmp_path / "u.bam")
    bamio.write_bam(p, bad, block=BLOCK, index=False)
    return rec, p


@pytest.mark.gpu
def test_error_returns_and_the_context_goes_on(ctx, oracle, tmp_path):
    rec, unsorted = _shuffled(tmp_path)
    frag = synth.frag_hist(rec)
    window = oracle.median(frag, 0.99)
    b = np.array([ted._bound(0, 5000, 5010, "AC")], api.BOUNDS_DTYPE)
    for cb in (1 << 20, 2):
        with pytest.raises(api.StrlingError, match=r"error -6: the BAM is not coordinate sorted: record 201 "):
            ctx.sweep(unsorted, b, window, frag, 20, chunk_blocks=cb)
    # a block whose CRC-32 is not its bytes'
    good = str(tmp_path / "g.bam")
    bamio.write_bam(good, rec, block=BLOCK, index=False)
    raw = bytearray(open(good, "rb").read())
    o = 0
    for _ in range(20):
        o += struct.unpack_from("<H", raw, o + 16)[0] + 1
    bsize = struct.unpack_from("<H", raw, o + 16)[0] + 1
    raw[o + bsize - 8] ^= 1
    crc = str(tmp_path / "c.bam")
    open(crc, "wb").write(raw)
    with pytest.raises(api.StrlingError, match=r"error -8"):
        ctx.sweep(crc, b, window, frag, 20, chunk_blocks=4)
    with pytest.raises(api.StrlingError, match=r"error -3"):
        ctx.sweep(good, np.array([ted._bound(0, 50, 40, "AC")], api.BOUNDS_DTYPE), window, frag, 20)
    (d,), info = ctx.sweep(good, b, window, frag, 20, chunk_blocks=4)           # the context goes on
    a_, b_ = ted._Layout(rec).region(0, 5000 - window, 5010 + window)
    o = oracle.spanners(rec.slice(a_, b_), b[0], window, frag, 20)
    assert d[3] in (0, 1) and info["n_records"] == rec.n
    (d,), _ = ctx.sweep(good, b, window, frag, 20, chunk_blocks=1 << 20)
    assert d[3] == 0 and _no_rec(d[0]) == _no_rec(o[0]) and d[1] == o[1]
