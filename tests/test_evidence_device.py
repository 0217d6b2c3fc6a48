"""`strling call`'s per-bound evidence on the device (strl_evidence_records / strl_regions_evidence, csrc/evidence.hip) against
spanners() as the oracle restates it (collect.nim:130-182) and as the host path computes it (strl_spanners): every field of
every Support, median_depth, and expected_spanners as float32 bits; the capacity rule (status 2); the fused form over a BAM's
BGZF blocks; the CLI with the evidence on the device against the CLI with it on the host."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from strling_amd import api, bamio, build, synth
from strling_amd.records import RecordBatch

CLI = build.CLI
MAX_RECORDS, MAX_SPAN = 4096, 9190          # what the device path must take (1000 + 2 * 4095)


# ---- the records of a batch as BAM bytes, and the byte range a region query returns -------------------------------------
class _Layout:
    def __init__(self, rec):
        self.rec = rec
        self.raw = bytes(bamio._raw_records(rec, 0, rec.n))
        ncig = np.diff(rec.cigar_off).astype(np.int64)
        qlen = np.diff(rec.qname_off.astype(np.int64))
        l_seq = rec.l_seq.astype(np.int64)
        size = 4 + 32 + qlen + 1 + 4 * ncig + (l_seq + 1) // 2 + l_seq
        self.off = np.concatenate([[0], np.cumsum(size)])
        assert int(self.off[-1]) == len(self.raw)
        span = np.bincount(np.repeat(np.arange(rec.n), ncig), weights=(rec.cigar >> 4).astype(np.float64), minlength=rec.n).astype(np.int64)
        self.ub = rec.pos.astype(np.int64) + 1 + span       # the walk's upper bound of bam_endpos (every operation counted)
        self.tid_range = {}
        for t in np.unique(rec.tid):
            ix = np.flatnonzero(rec.tid == t)
            assert ix[-1] - ix[0] + 1 == ix.size
            self.tid_range[int(t)] = (int(ix[0]), int(ix[-1]) + 1)

    def region(self, tid, beg, end):
        """records [a, b): from the first record of `tid` that may reach past `beg` up to the first at or behind `end`
        (strl_regions_fetch's rule, as tests/test_regions_device.py walks it)"""
        t0, t1 = self.tid_range.get(int(tid), (0, 0))
        pos = self.rec.pos[t0:t1]
        b = t0 + int(np.searchsorted(pos, end, side="left"))
        cand = np.flatnonzero(self.ub[t0:b] > beg)
        a = t0 + int(cand[0]) if cand.size else b
        return a, b

    def bytes_of(self, a, b):
        return self.raw[int(self.off[a]):int(self.off[b])]


def _bound(tid, left, right, unit):
    b = np.zeros(1, api.BOUNDS_DTYPE)
    b["tid"], b["left"], b["right"], b["repeat"] = tid, left, right, unit
    return b[0]


def _tract_units(rec, g):
    """[(tid, start, stop, unit)] of the genome's STR tracts that reads with a periodic sequence lie on: the unit those reads
    carry over the tract"""
    out = []
    for t in range(g.iv_off.size - 1):
        for v in range(int(g.iv_off[t]), int(g.iv_off[t + 1])):
            s, e = int(g.iv_start[v]), int(g.iv_stop[v])
            ix = np.flatnonzero((rec.tid == t) & (rec.pos >= s - 100) & (rec.pos <= s) & (np.diff(rec.cigar_off) == 1))[:6]
            for i in ix:
                seq = rec.sequence(int(i))
                q = s - int(rec.pos[i]) + 2
                body = seq[q:min(len(seq), q + (e - s) - 2)]
                if len(body) < 24:
                    continue
                for k in range(1, 7):
                    if sum(body[j] == body[j + k] for j in range(len(body) - k)) >= 0.85 * (len(body) - k) and set(body[:k]) <= set("ACGT"):
                        out.append((t, s, e, body[:k]))
                        break
                else:
                    continue
                break
    return out


def _random_bounds(rec, g, seed, n_random=220, per_tract=30):
    rng = np.random.default_rng(seed)
    bounds = []
    for _ in range(n_random):
        tid = int(rng.integers(0, len(rec.targets)))
        clen = rec.targets[tid][1]
        width = int(rng.integers(0, 41)) if rng.random() < 0.5 else int(rng.integers(0, 1001))
        left = int(rng.integers(0, clen - width))
        unit = "".join("ACGT"[c] for c in rng.integers(0, 4, size=int(rng.integers(1, 7))))
        bounds.append(_bound(tid, left, left + width, unit))
    for tid, (_, clen) in enumerate(rec.targets):             # at the contig's start and end
        for width in (0, 3, 40, 700):
            bounds.append(_bound(tid, 0, width, "AC"))
            bounds.append(_bound(tid, int(rng.integers(0, 6)), int(rng.integers(6, 900)), "CAG"))
            bounds.append(_bound(tid, clen - width, clen, "A"))
            bounds.append(_bound(tid, clen - width - int(rng.integers(1, 200)), clen - int(rng.integers(0, 2)), "AAGGGC"))
    tracts = _tract_units(rec, g)
    for (tid, s, e, unit) in tracts:                          # the genome's own units, on their tracts: narrow bounds that reads span
        for _ in range(per_tract):
            left = s + int(rng.integers(-20, max(1, min(60, e - s))))
            width = int(rng.integers(0, 50)) if rng.random() < 0.8 else int(rng.integers(0, 1001))
            k = len(unit)
            rot = int(rng.integers(0, k))
            bounds.append(_bound(tid, max(0, left), max(0, left) + width, unit[rot:] + unit[:rot]))
    return bounds, len(tracts)


def _oracle_bounds(oracle, rec, g, frag):
    med = oracle.median(frag)
    t = oracle.extract(rec, g, oracle.make_opts(med, 0.8, 40))
    b, _ = oracle.call_bounds(t, 1, oracle.median(frag, 0.99), min_support=3, max_clip_dist=int(0.5 * med))
    return [np.frombuffer(x.tobytes(), api.BOUNDS_DTYPE)[0] for x in b]


def _same(dev, ref):
    """a device answer (supports, median_depth, expected_spanners, status) against spanners()' (supports, median, expected)"""
    return (dev[3] == 0 and dev[0].tobytes() == np.ascontiguousarray(ref[0]).tobytes() and dev[1] == ref[1]
            and np.float32(dev[2]).view(np.uint32) == np.float32(ref[2]).view(np.uint32))


SAMPLES = [(dict(n_pairs=6000, seed=5, n_contigs=2, contig_len=30_000), 40), (dict(n_pairs=6000, seed=6, n_contigs=2, contig_len=30_000), 0),
           (dict(n_pairs=6000, seed=7, n_contigs=2, contig_len=30_000), 20), (dict(n_pairs=200_000, seed=9, n_contigs=4, contig_len=1_000_000), 20)]


@pytest.mark.gpu
@pytest.mark.parametrize("kw,min_mapq", SAMPLES, ids=["seed5-q40", "seed6-q0", "seed7-q20", "seed9-large"])
def test_evidence_records_equal_spanners(ctx, oracle, kw, min_mapq):
    """1. parity per region, 2. none of these regions is passed on, 5. two runs give identical bytes"""
    kw = dict(kw)
    rec, g = synth.synth_wgs(kw.pop("n_pairs"), **kw)
    frag = synth.frag_hist(rec)
    window = oracle.median(frag, 0.99)
    L = _Layout(rec)
    clustered = _oracle_bounds(oracle, rec, g, frag)
    rnd, n_tracts = _random_bounds(rec, g, seed=1000 + kw["seed"])
    assert len(rnd) >= 300 and n_tracts >= 1
    bounds = clustered + rnd
    cuts = []
    for b in bounds:
        wl, wr = int(b["left"]) - window, int(b["right"]) + window
        cuts.append(L.region(int(b["tid"]), max(0, wl), wr))
    # the capacity rule, counted here: every region of this test lies inside it
    n_rec = [b_ - a_ for a_, b_ in cuts]
    spans = [int(b["right"]) - int(b["left"]) + 2 * window for b in bounds]
    print(f"{len(clustered)} clustered + {len(rnd)} random bounds; records per region <= {max(n_rec)}, depth span <= {max(spans)}, window {window}")
    assert max(n_rec) <= MAX_RECORDS and max(spans) <= MAX_SPAN
    regions = [L.bytes_of(a_, b_) for a_, b_ in cuts]
    barr = np.array(bounds, api.BOUNDS_DTYPE)
    got = ctx.evidence_records(regions, barr, window, frag, min_mapq)
    again = ctx.evidence_records(regions, barr, window, frag, min_mapq)
    types, n_ins, n_del, n_counted, n_frag_exp = set(), 0, 0, 0, 0
    small = rec.n < 50_000
    for k, (b, (a_, b_), d) in enumerate(zip(bounds, cuts, got)):
        sub = rec.slice(a_, b_)
        ref = oracle.spanners(sub, b, window, frag, min_mapq)
        assert d[3] == 0, (k, b, "passed on")
        assert _same(d, ref), (k, b, d[1:], ref[1:], len(d[0]), len(ref[0]))
        if small:
            assert _same(d, api.spanners(sub, b, window, frag, min_mapq)), (k, b)
        e = again[k]
        assert d[0].tobytes() == e[0].tobytes() and d[1:] == e[1:], (k, "two runs differ")
        types |= set(d[0]["type"].tolist())
        sp = d[0][d[0]["type"] == 1]
        n_ins += int((sp["cigar_ins"] > 0).sum())
        n_del += int((sp["cigar_del"] > 0).sum())
        n_counted += int((sp["repeat_count"] > 0).sum())
        n_frag_exp += d[2] > 0
    print(f"support types {sorted(types)}, spanning reads with insertions {n_ins}, deletions {n_del}, with a unit count {n_counted}, bounds with expected spanners {n_frag_exp}")
    assert types == {0, 1, 2} and n_ins > 0 and n_del > 0 and n_counted > 0 and n_frag_exp > 0


def _pile(n_pairs, at=1000, read_len=100, frag_len=300):
    """n_pairs pairs at one locus, coordinate sorted"""
    rng = np.random.default_rng(77)
    p1 = at + np.arange(n_pairs) // 12
    pos = np.concatenate([p1, p1 + frag_len - read_len])
    order = np.argsort(pos, kind="stable")
    first = order < n_pairs
    n = 2 * n_pairs
    qn = [b"p%d" % (i % n_pairs) for i in order]
    flag = np.where(first, 0x1 | 0x2 | 0x40 | 0x20, 0x1 | 0x2 | 0x80 | 0x10).astype(np.uint16)
    mpos = np.where(first, pos[order] + frag_len - read_len, pos[order] - (frag_len - read_len))
    seqs = ["".join("ACGT"[c] for c in rng.integers(0, 4, size=read_len)) for _ in range(8)]
    return RecordBatch.from_fields(np.zeros(n, np.int32), pos[order], np.zeros(n, np.int32), mpos, flag, np.full(n, 60, np.uint8), ["%dM" % read_len] * n,
                                   [seqs[i % 8] for i in range(n)], qn, isize=np.where(first, frag_len, -frag_len), targets=[("chr1", 100_000)])


@pytest.mark.gpu
def test_status_2_beyond_the_capacity_rule(ctx, oracle):
    """a region of more than 4096 records and a bound wider than the span limit are passed on -- exactly those: their
    neighbours in the same call, the region of exactly 4096 records and the bound exactly at the limit among them, are answered"""
    rec = _pile(2100)
    assert rec.n == 4200
    frag = synth.frag_hist(rec)
    frag[250:450] += 3
    window = oracle.median(frag, 0.99)
    L = _Layout(rec)
    narrow = _bound(0, 1120, 1130, "AC")
    at_limit = _bound(0, 5000, 5000 + MAX_SPAN - 2 * window, "A")
    too_wide = _bound(0, 5000, 5000 + MAX_SPAN - 2 * window + 1, "A")
    cases = [(narrow, (0, 600)), (narrow, (0, rec.n)), (narrow, (0, MAX_RECORDS)), (too_wide, (0, 300)), (at_limit, (0, 300)), (narrow, (100, 900))]
    got = ctx.evidence_records([L.bytes_of(a, b) for _, (a, b) in cases], np.array([b for b, _ in cases], api.BOUNDS_DTYPE), window, frag, 20)
    assert [d[3] for d in got] == [0, 2, 0, 2, 0, 0]
    for (b, (a_, b_)), d in zip(cases, got):
        if d[3] == 0:
            assert _same(d, oracle.spanners(rec.slice(a_, b_), b, window, frag, 20)), (b, a_, b_)
        else:
            assert len(d[0]) == 0
    assert len(got[0][0]) > 50


# ---- the fused form ------------------------------------------------------------------------------------------------------
def _blocks(path):
    """[(raw DEFLATE payload, ISIZE, CRC32)] of every BGZF block"""
    raw = open(path, "rb").read()
    out, o = [], 0
    while o < len(raw):
        xlen = struct.unpack_from("<H", raw, o + 10)[0]
        bsize = struct.unpack_from("<H", raw, o + 16)[0] + 1
        crc, isz = struct.unpack_from("<II", raw, o + bsize - 8)
        out.append((raw[o + 12 + xlen:o + bsize - 8], isz, crc))
        o += bsize
    return out


def _parse(raw, targets):
    """block_size-prefixed BAM records -> RecordBatch"""
    f = {k: [] for k in ("tid", "pos", "mtid", "mpos", "flag", "mapq", "l_seq", "isize")}
    cig, cig_off, qn, qoff, seq, seq_off = [], [0], bytearray(), [0], bytearray(), []
    at = 0
    while at < len(raw):
        bs, tid, pos, l_name, mapq, _, n_cig, flag, l_seq, mtid, mpos, tlen = struct.unpack_from("<iiiBBHHHiiii", raw, at)
        o = at + 36
        qn += raw[o:o + l_name - 1]
        qoff.append(len(qn))
        o += l_name
        cig.extend(struct.unpack_from(f"<{n_cig}I", raw, o))
        cig_off.append(len(cig))
        o += 4 * n_cig
        seq += b"\0" * (-len(seq) % 16)
        seq_off.append(len(seq))
        seq += raw[o:o + (l_seq + 1) // 2]
        for k, v in zip(f, (tid, pos, mtid, mpos, flag, mapq, l_seq, tlen)):
            f[k].append(v)
        at += 4 + bs
    return RecordBatch(np.array(f["tid"], np.int32), np.array(f["pos"], np.int32), np.array(f["mtid"], np.int32), np.array(f["mpos"], np.int32),
                       np.array(f["flag"], np.uint16), np.array(f["mapq"], np.uint8), np.array(cig_off, np.uint32), np.array(cig, np.uint32),
                       np.array(seq_off, np.uint64), np.array(f["l_seq"], np.int32), np.frombuffer(bytes(seq) + b"\0" * 32, np.uint8), np.array(qoff, np.uint64),
                       bytes(qn), np.array(f["isize"], np.int32), targets)


@pytest.mark.gpu
@pytest.mark.parametrize("block", [0xFF00, 1500])
def test_regions_evidence_equals_fetch_then_spanners(ctx, oracle, block, tmp_path):
    """3. inflate -> CRC -> walk -> evidence in one call = regions_fetch followed by strl_spanners per region"""
    rec, g = synth.synth_wgs(3000, seed=12, n_contigs=2, contig_len=20_000)
    bam = str(tmp_path / "r.bam")
    bamio.write_bam(bam, rec, block=block)
    blks = _blocks(bam)
    frag = synth.frag_hist(rec)
    window = oracle.median(frag, 0.99)
    L = _Layout(rec)
    # where record i sits in the inflated stream: behind the header
    hdr = sum(b[1] for b in blks) - len(L.raw)
    ustart = np.concatenate([[0], np.cumsum([b[1] for b in blks])])
    rng = np.random.default_rng(4)
    bounds, regions = [], []
    for _ in range(80):
        tid = int(rng.integers(0, 2))
        width = int(rng.integers(0, 200))
        left = int(rng.integers(0, 20_000 - width))
        b = _bound(tid, left, left + width, "ACGT"[int(rng.integers(0, 4))] + "C")
        beg, end = max(0, left - window), left + width + window
        a_, _ = L.region(tid, beg, end)
        k = max(L.tid_range[tid][0], a_ - int(rng.integers(0, 40)))       # the walk starts at or before the first record that can overlap
        o = hdr + int(L.off[k])
        fb = int(np.searchsorted(ustart, o, side="right") - 1)
        nb = int(rng.integers(1, min(len(blks) - fb, 600 if block == 1500 else 24) + 1))
        bounds.append(b)
        regions.append((fb, nb, o - int(ustart[fb]), tid, beg, end))
    streams, sizes, crcs = [b[0] for b in blks], [b[1] for b in blks], [b[2] for b in blks]
    barr = np.array(bounds, api.BOUNDS_DTYPE)
    fetched = ctx.regions_fetch(streams, sizes, regions, crcs=crcs)
    got = ctx.regions_evidence(streams, sizes, regions, barr, window, frag, 20, crcs=crcs)
    n0 = 0
    for b, (raw, st), d in zip(bounds, fetched, got):
        assert d[3] == st, (b, d[3], st)
        if st:
            continue
        n0 += 1
        assert _same(d, api.spanners(_parse(raw, rec.targets), b, window, frag, 20)), b
    assert n0 >= 20 and sum(1 for _, st in fetched if st == 1) >= 1
    bad = list(crcs)
    bad[regions[0][0]] ^= 1
    with pytest.raises(api.StrlingError):
        ctx.regions_evidence(streams, sizes, regions[:1], barr[:1], window, frag, 20, crcs=bad)


# ---- the CLI -------------------------------------------------------------------------------------------------------------
def _run(args, env=None):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([CLI] + args, capture_output=True, text=True, env=e)


def _take(rec, idx):
    """the records idx (with repeats) as a batch"""
    idx = np.asarray(idx)
    cig = [rec.cigar[int(rec.cigar_off[i]):int(rec.cigar_off[i + 1])] for i in idx]
    cig_off = np.concatenate([[0], np.cumsum([c.size for c in cig])]).astype(np.uint32)
    qn = [rec.qname(int(i)) for i in idx]
    qoff = np.concatenate([[0], np.cumsum([len(q) for q in qn])]).astype(np.uint64)
    seq, seq_off = bytearray(), []
    for i in idx:
        seq += b"\0" * (-len(seq) % 16)
        seq_off.append(len(seq))
        o = int(rec.seq_off[i])
        seq += bytes(rec.seq4[o:o + (int(rec.l_seq[i]) + 1) // 2])
    return RecordBatch(rec.tid[idx], rec.pos[idx], rec.mtid[idx], rec.mpos[idx], rec.flag[idx], rec.mapq[idx], cig_off, np.concatenate(cig).astype(np.uint32),
                       np.array(seq_off, np.uint64), rec.l_seq[idx], np.frombuffer(bytes(seq) + b"\0" * 32, np.uint8), qoff, b"".join(qn), rec.isize[idx], rec.targets)


def _call(prefix, bam, binp, extra, env):
    r = _run(["call", "-v", "-m", "3", "-o", prefix] + extra + [bam, binp], env)
    assert r.returncode == 0, r.stderr
    m = re.search(r"regions through the device (\d+), on the host (\d+)", r.stderr)
    e = re.search(r"computed on the device (\d+), passed on to the host \(.*?\) (\d+), evidence kernels ([0-9.]+) s", r.stderr)
    assert m and e, r.stderr
    return [open(prefix + s).read() for s in ("-bounds.txt", "-genotype.txt", "-unplaced.txt")], int(m.group(1)), int(m.group(2)), int(e.group(1)), int(e.group(2)), r.stderr


@pytest.mark.gpu
def test_call_device_evidence_equals_host_evidence(tmp_path):
    """4. the three files of `strling call` with the evidence on the device (STRL_CALL_EVIDENCE=device: the device path is opt-in
    until it has been measured) = with STRL_CALL_EVIDENCE=host = the default, on the input of
    test_call_device_regions_equal_host_regions; then with -l loci on a copy of that input that piles more than 4096 records
    onto one locus: that locus is passed on (status 2) and the files stay identical.  A locus wider than the span limit is in
    the list too: `call` drops a locus wider than 1000 bases before any evidence is collected ("large bounds ... skipping",
    what the reference does), so it reaches neither path -- with a window of at most 4095 no locus `call` works on can exceed
    the span limit, and the passing on by span is covered by test_status_2_beyond_the_capacity_rule."""
    rec, g = synth.synth_wgs(12000, seed=31, n_contigs=2, contig_len=100_000)
    bam, bed, binp = str(tmp_path / "s.bam"), str(tmp_path / "ref.str"), str(tmp_path / "s.bin")
    bamio.write_bam(bam, rec, block=0xFF00, level=6)
    bamio.write_genome_bed(bed, g, rec.targets)
    r = _run(["extract", "-g", bed, bam, binp])
    assert r.returncode == 0, r.stderr
    dev = _call(str(tmp_path / "dev"), bam, binp, [], {"STRL_CALL_EVIDENCE": "device"})
    host = _call(str(tmp_path / "host"), bam, binp, [], {"STRL_CALL_EVIDENCE": "host"})
    default = _call(str(tmp_path / "default"), bam, binp, [], {})
    assert dev[0] == host[0] == default[0]
    assert dev[0][0].count("\n") >= 4
    assert dev[1] >= 3 and dev[3] >= 3 and dev[3] == dev[1] and dev[4] == 0 and host[3] == 0
    # a pile of records on one locus
    lo, hi = np.searchsorted(rec.pos[rec.tid == 0], [50_000, 50_300])
    reps = np.ones(rec.n, np.int64)
    reps[lo:hi] = MAX_RECORDS // max(1, hi - lo) + 2
    deep = _take(rec, np.repeat(np.arange(rec.n), reps))
    assert int(reps[lo:hi].sum()) > MAX_RECORDS
    bam2, bin2, loci = str(tmp_path / "d.bam"), str(tmp_path / "d.bin"), str(tmp_path / "loci.bed")
    bamio.write_bam(bam2, deep, block=0xFF00, level=6)
    r = _run(["extract", "-g", bed, bam2, bin2])
    assert r.returncode == 0, r.stderr
    open(loci, "w").write("chr1\t50100\t50140\tAC\tpile\nchr1\t20000\t20030\tCAG\tplain\nchr2\t70000\t70600\tA\tbroad\nchr2\t10000\t25000\tAC\ttoo_wide\nchr2\t40000\t40002\tAAGGGC\n")
    dev = _call(str(tmp_path / "ddev"), bam2, bin2, ["-l", loci], {"STRL_CALL_EVIDENCE": "device"})
    host = _call(str(tmp_path / "dhost"), bam2, bin2, ["-l", loci], {"STRL_CALL_EVIDENCE": "host"})
    assert dev[0] == host[0]
    assert "too_wide" not in dev[0][0] and "large bounds: chr2:10000-25000 skipping" in dev[5]
    assert dev[3] >= 3 and dev[4] >= 1, dev[5]
