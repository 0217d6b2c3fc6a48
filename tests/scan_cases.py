"""Inputs that put the device record scan (strling_amd/csrc/front.hip: rec_guess / rec_walk / rec_link / rec_parse) where a guess
is wrong, a record is longer than a segment, and a chunk seam falls on a chosen byte -- plus a pure-Python MODEL of the scan.

Plain builders, no GPU code.  A case is a RecordBatch, the keyword arguments bamio.write_bam turns it into files with, and the
chunk sizes it is pushed with.  The model restates, from front.hip's header comment and the SAM specification (section 4.2),
what the scan must find per chunk; it reads nothing but the file.  Conditions on the model alone (tests/test_scan_cases.py,
on any machine) show that every case reaches the edge it is named for; tests/test_scan_device.py feeds the same files to the
kernels.

The model, per chunk of `chunk_blocks` BGZF blocks:
  truth    the record offsets, by following block_size from the first record;
  layout   the chunk's own bytes start on a segment boundary (the room in front of them is 64 segments); in front of them lies
           the carry = every byte behind the last complete record of all earlier chunks; start0 = -len(carry), s0 = the
           segment of start0, end = the end of the chunk's bytes;
  guess    for every segment above s0: the lowest offset o in it, o + 36 <= end, from which four records in a row are plausible
           -- if the data ends before the fourth, one is enough;
  wrong    segments that hold a true record start (one whose 36 fixed bytes lie in front of `end`: a start behind that is not
           this chunk's to find, it is where the carry begins) and whose guess is not the first of them;
  stray    segments without such a start that still have a guess;
  clean    neither.
Segment numbers are the device's: the chunk's first own byte is in segment 64.
"""
import bisect
import functools
import struct
import zlib

import numpy as np

from strling_amd import bamio, synth
from strling_amd.records import RecordBatch

SEG = 16384
CARRY_SEGS = 64
CARRY_MAX = SEG * CARRY_SEGS
BLOCK = 2 * SEG              # BGZF block size of the decoy cases: segment boundaries are multiples of 16384 of the inflated stream, whatever the chunk size
FAR = 1 << 22                # a block_size that leaves every file here (at most ~2 MB) and is still plausible (<= 2^26)


# ---- the model ------------------------------------------------------------------------------------------------------------
def inflate(path):
    """-> (the inflated stream, isize of every non-empty BGZF block)"""
    raw = open(path, "rb").read()
    parts, isz, o = [], [], 0
    while o < len(raw):
        xlen = struct.unpack_from("<H", raw, o + 10)[0]
        bsize = struct.unpack_from("<H", raw, o + 16)[0] + 1
        data = zlib.decompress(raw[o + 12 + xlen:o + bsize - 8], -15)
        assert len(data) == struct.unpack_from("<I", raw, o + bsize - 4)[0]
        if data:
            parts.append(data)
            isz.append(len(data))
        o += bsize
    return b"".join(parts), isz


def bam_header(stream):
    """-> (n_ref, offset of the first record)"""
    assert stream[:4] == b"BAM\1"
    l_text = struct.unpack_from("<i", stream, 4)[0]
    n_ref = struct.unpack_from("<i", stream, 8 + l_text)[0]
    o = 12 + l_text
    for _ in range(n_ref):
        o += 8 + struct.unpack_from("<i", stream, o)[0]
    return n_ref, o


def truth(stream, first):
    """offsets of the complete records + the offset behind the last of them"""
    offs, o = [], first
    while o + 4 <= len(stream):
        nxt = o + 4 + struct.unpack_from("<I", stream, o)[0]
        if nxt > len(stream):
            break
        offs.append(o)
        o = nxt
    return offs + [o]


def plausible(stream, o, end, n_ref):
    """the record a plausible header at o (o + 36 <= end) announces ends where? None: not plausible"""
    bs, ref, pos, l_name, _, _, n_cigar, _, l_seq, nref, npos, _ = struct.unpack_from("<IiiBBHHHiiii", stream, o)
    if not 32 <= bs <= 1 << 26 or l_seq < 0 or l_name < 1:
        return None
    if not (-1 <= ref < n_ref and -1 <= nref < n_ref) or pos < -1 or npos < -1:
        return None
    if 32 + l_name + 4 * n_cigar + (l_seq + 1) // 2 + l_seq > bs:
        return None
    nul = o + 36 + l_name - 1
    if nul < end and stream[nul] != 0:
        return None
    if any(not 33 <= c <= 126 for c in stream[o + 36:min(nul, end)]):
        return None
    return o + 4 + bs


def chain_of_four(stream, o, end, n_ref):
    n_ok = 0
    while n_ok < 4:
        if o + 36 > end:
            return n_ok >= 1
        o = plausible(stream, o, end, n_ref)
        if o is None:
            return False
        n_ok += 1
    return True


def _candidates(stream, n_ref):
    """offsets whose fixed fields alone do not rule a record out (a sieve in numpy in front of plausible(), which decides)"""
    d = np.frombuffer(stream, np.uint8).astype(np.int64)
    n = d.size - 35
    if n <= 0:
        return np.zeros(0, np.int64)

    def i32(k):
        v = d[k:k + n] | (d[k + 1:k + 1 + n] << 8) | (d[k + 2:k + 2 + n] << 16) | (d[k + 3:k + 3 + n] << 24)
        return np.where(v >= 1 << 31, v - (1 << 32), v)
    bs, ref, pos, l_seq, nref, npos = i32(0), i32(4), i32(8), i32(20), i32(24), i32(28)
    ok = (bs >= 32) & (bs <= 1 << 26) & (ref >= -1) & (ref < n_ref) & (nref >= -1) & (nref < n_ref) & (pos >= -1) & (npos >= -1) & (l_seq >= 0) & (d[12:12 + n] >= 1)
    return np.flatnonzero(ok)


def scan_model(path, chunk_blocks):
    """-> list of per-chunk dicts: base, end, start0 (offsets of the inflated stream), carry (its length; 0 in the first chunk),
    n_records (records that END in the chunk), n_seg, s0, wrong / stray (lists of segment numbers), clean, no_start (segments above
    s0 in which no record starts at all), guess {segment: offset}, n_chunks_left"""
    stream, isz = inflate(path)
    n_ref, first = bam_header(stream)
    offs = truth(stream, first)
    starts = list(offs[:-1]) + ([offs[-1]] if offs[-1] < len(stream) else [])        # (a file cut inside a record: that record starts too)
    ends = offs[1:]
    cand = _candidates(stream, n_ref)
    cum = [0]
    for n in isz:
        cum.append(cum[-1] + n)
    b0 = bisect.bisect_right(cum, first) - 1
    chunks, p = [], first
    for k in range(b0, len(isz), chunk_blocks):
        base, end = cum[k], cum[min(k + chunk_blocks, len(isz))]
        start0 = p
        seg_of = lambda o: (o - base) // SEG + CARRY_SEGS
        done = ends[bisect.bisect_right(ends, p):bisect.bisect_right(ends, end)]
        s0, last = seg_of(start0), seg_of(end - 1)
        wrong, stray, no_start, guess = [], [], [], {}
        for s in range(s0 + 1, last + 1):
            lo = base + (s - CARRY_SEGS) * SEG
            hi = min(lo + SEG, end)
            g = None
            for o in cand[np.searchsorted(cand, lo):np.searchsorted(cand, hi)]:
                if o + 36 <= end and chain_of_four(stream, int(o), end, n_ref):
                    g = int(o)
                    break
            here = starts[bisect.bisect_left(starts, lo):bisect.bisect_left(starts, hi)]
            mine = [o for o in here if o + 36 <= end]
            if g is not None:
                guess[s] = g
            if mine and g != mine[0]:
                wrong.append(s)
            if not mine and g is not None:
                stray.append(s)
            if not here:
                no_start.append(s)
        chunks.append(dict(base=base, end=end, start0=start0, carry=base - start0 if chunks else 0, n_records=len(done), n_seg=last + 1, s0=s0, wrong=wrong,
                           stray=stray, clean=not wrong and not stray, no_start=no_start, guess=guess))
        if done:
            p = done[-1]
    return chunks


def model_line(name, label, chunk_blocks, chunks):
    """one line per file and chunk size: what a reader needs to see that the case reached its edge"""
    w, s = sum(len(c["wrong"]) for c in chunks), sum(len(c["stray"]) for c in chunks)
    return (f"{name}/{label} chunk_blocks={chunk_blocks}: {len(chunks)} chunks, records {sum(c['n_records'] for c in chunks)}, wrong {w}, stray {s}, "
            f"segments without a start {sum(len(c['no_start']) for c in chunks)}, longest carry {max(c['carry'] for c in chunks)}, "
            f"chunks without a record {sum(c['n_records'] == 0 for c in chunks)}")


# ---- records --------------------------------------------------------------------------------------------------------------
def base_records(n_pairs, seed, str_frac=0.08, contig_len=60_000):
    """a small coordinate-sorted batch with enough STR reads for the extraction to have something to say.
    Contigs shorter than 65536: two bytes in front of a record of contig 0 whose pos is 65536 .. 131071 (and whose mate is on contig
    0 too) the bytes read as a plausible header -- block_size = the real one << 16 | two quality bytes, about 17 MB; l_read_name =
    the third byte of pos = 1, its NUL the third byte of tlen -- and in a file of less than 17 MB that one header is all the guess
    rule asks for.  Case (n) keeps such records; every other case stays clear of them, so that its control is clean."""
    return synth.synth_wgs(n_pairs, seed=seed, n_contigs=3, contig_len=contig_len, str_frac=str_frac)


def _rows_of(rec):
    isz = rec.isize if rec.isize is not None else np.zeros(rec.n, np.int32)
    return [dict(tid=int(rec.tid[i]), pos=int(rec.pos[i]), mtid=int(rec.mtid[i]), mpos=int(rec.mpos[i]), flag=int(rec.flag[i]), mapq=int(rec.mapq[i]),
                 cigar=[int(c) for c in rec.cigar[int(rec.cigar_off[i]):int(rec.cigar_off[i + 1])]], seq=rec.sequence(i), qname=rec.qname(i), isize=int(isz[i]))
            for i in range(rec.n)]


def _batch(rows, targets):
    """rows in coordinate order (stable; the unplaced ones last)"""
    rows = sorted(rows, key=lambda r: (r["tid"] < 0, r["tid"], r["pos"]))
    col = lambda k: [r[k] for r in rows]
    return RecordBatch.from_fields(col("tid"), col("pos"), col("mtid"), col("mpos"), col("flag"), col("mapq"), col("cigar"), col("seq"), col("qname"), col("isize"), targets)


# ---- the layout of a file, before it is written -----------------------------------------------------------------------------
def header_bytes(rec, text):
    return 12 + len(text.encode()) + sum(9 + len(n.encode()) for n, _ in rec.targets)


def layout(rec, text, extra):
    """-> (off[n + 1]: where every record starts, aux[n]: where the DATA of an XD:B:C array behind record i's qualities would start)"""
    o, off, aux = header_bytes(rec, text), [], []
    for i in range(rec.n):
        l_seq = int(rec.l_seq[i])
        fixed = 36 + len(rec.qname(i)) + 1 + 4 * (int(rec.cigar_off[i + 1]) - int(rec.cigar_off[i])) + (l_seq + 1) // 2 + l_seq
        off.append(o)
        aux.append(o + fixed + 8)
        o += fixed + len(extra.get(i, b""))
    return off + [o], aux


def aux_array(data):
    """a well-formed XD:B:C array"""
    return b"XDBC" + struct.pack("<I", len(data)) + bytes(data)


class Builder:
    """aux arrays that put chosen bytes at chosen offsets of the inflated stream.  Carriers are chosen front to back: an array
    moves everything behind it."""

    def __init__(self, rec, text=None):
        self.rec, self.text = rec, text if text is not None else bamio.sam_header(rec.targets)
        self.extra, self.marks = {}, []          # marks: (record, offset in the array's data, length) of every payload

    def carrier(self, at):
        _, aux = layout(self.rec, self.text, self.extra)
        i = bisect.bisect_right(aux, at) - 1
        assert i >= 0 and i not in self.extra and all(j < i for j in self.extra), (at, i)
        return i, at - aux[i]

    def put(self, at, payload, tail=0):
        """payload at stream offset `at`, in the last record whose array can begin in front of it; `tail` zero bytes behind -> the record"""
        i, pad = self.carrier(at)
        self.extra[i] = aux_array(bytes(pad) + payload + bytes(tail))
        self.marks.append((i, pad, len(payload)))
        return i

    def more(self, i, at, payload):
        """another payload inside record i's array (which must reach that far)"""
        _, aux = layout(self.rec, self.text, self.extra)
        k = at - aux[i]
        data = bytearray(self.extra[i][8:])
        assert 0 <= k and k + len(payload) <= len(data) and not any(data[k:k + len(payload)])
        data[k:k + len(payload)] = payload
        self.extra[i] = aux_array(data)
        self.marks.append((i, k, len(payload)))

    def end_at(self, at):
        """a record made to END at stream offset `at` (zeros in its array) -> the record"""
        i, pad = self.carrier(at)
        self.extra[i] = aux_array(bytes(pad))
        return i

    def offsets(self):
        return layout(self.rec, self.text, self.extra)[0]

    def zeroed(self):
        """the same arrays with every payload zeroed: the control"""
        out = {i: bytearray(e) for i, e in self.extra.items()}
        for i, k, n in self.marks:
            out[i][8 + k:8 + k + n] = bytes(n)
        return {i: bytes(e) for i, e in out.items()}


def fake_header(block_size, name=b"dcy"):
    """36 fixed bytes + name that pass for a record: 40 bytes with the default name"""
    return struct.pack("<IiiBBHHHiiii", block_size, 0, 0, len(name) + 1, 0, 4680, 0, 0, 0, -1, -1, 0) + name + b"\0"


def decoy_chain(sizes=(36, 36, 36, 36)):
    """fake headers back to back: block_size 36 leads to the next one; whatever the last one says leads where the case wants"""
    return b"".join(fake_header(s) for s in sizes)


def uniform_cuts(total, step=BLOCK, cuts=()):
    """`cuts` + one every `step` bytes where they are further apart than a BGZF block may be"""
    out, prev = [], 0
    for c in sorted(set(cuts)) + [total]:
        while c - prev > step:
            prev += step
            out.append(prev)
        if c < total and c > prev:
            out.append(c)
            prev = c
    return out


# ---- the cases ------------------------------------------------------------------------------------------------------------
class Variant:
    """one file of a case: write_bam's keyword arguments, the chunk sizes it is pushed with, the file it is the control of"""

    def __init__(self, label, chunk_blocks, control_of=None, **kw):
        self.label, self.chunk_blocks, self.control_of, self.kw = label, tuple(chunk_blocks), control_of, kw

    @property
    def indexable(self):
        return "cuts" not in self.kw


class Case:
    def __init__(self, name, rec, genome, variants, **meta):
        self.name, self.rec, self.genome, self.variants, self.meta = name, rec, genome, {v.label: v for v in variants}, meta

    def write(self, path, label, index=False):
        """-> the header text"""
        return bamio.write_bam(path, self.rec, index=index, **self.variants[label].kw)


def _decoy_case(name, seed, segs, chunk_blocks, chain, n_pairs=800):
    """chains at the start of stream segments `segs`, each in the array of the record that reaches into that segment, 64 zero bytes
    behind it, the segment's first true record behind those"""
    rec, g = base_records(n_pairs, seed)
    b = Builder(rec)
    placed = [(b.put(s * SEG, chain, tail=64), s * SEG) for s in segs]
    return rec, g, b, placed


@functools.lru_cache(maxsize=None)
def case_a():
    rec, g, b, placed = _decoy_case("a", 101, (3, 7, 12, 17), (16384, 3), decoy_chain())
    return Case("a", rec, g, [Variant("decoy", (16384, 3), block=BLOCK, extra=b.extra), Variant("control", (16384, 3), control_of="decoy", block=BLOCK, extra=b.zeroed())],
                decoys=[at for _, at in placed])


@functools.lru_cache(maxsize=None)
def case_b():
    """the fourth header's block_size lands on a true record start two segments on: the chain rejoins the truth"""
    rec, g, b, placed = _decoy_case("b", 102, (4, 9, 15), (16384, 3), decoy_chain())
    off = b.offsets()
    for i, at in placed:
        target = off[bisect.bisect_left(off, at + 2 * SEG + 5000)]
        k = [m for m in b.marks if m[0] == i][0][1]
        data = bytearray(b.extra[i][8:])
        data[k + 120:k + 124] = struct.pack("<I", target - (at + 120) - 4)
        b.extra[i] = aux_array(data)
    return Case("b", rec, g, [Variant("decoy", (16384, 3), block=BLOCK, extra=b.extra), Variant("control", (16384, 3), control_of="decoy", block=BLOCK, extra=b.zeroed())],
                decoys=[at for _, at in placed])


@functools.lru_cache(maxsize=None)
def case_c():
    """the second header's block_size points past the end of the data: a second chain that stops, in front of the true one's stop"""
    rec, g, b, placed = _decoy_case("c", 103, (4, 10), (3, 16384), decoy_chain((36, FAR)))
    return Case("c", rec, g, [Variant("decoy", (3, 16384), block=BLOCK, extra=b.extra), Variant("control", (3, 16384), control_of="decoy", block=BLOCK, extra=b.zeroed())],
                decoys=[at for _, at in placed], stops=[at + 40 for _, at in placed])


LONG_AUX = 40_000


def _long_record(seed, at_seg, decoy_segs, n_pairs=700):
    """a record whose array begins at stream segment at_seg and holds 40 KB from there: segments at_seg and at_seg + 1 have no
    record start; chains at the start of decoy_segs and one in the middle of the first"""
    rec, g = base_records(n_pairs, seed)
    b = Builder(rec)
    i = b.put(at_seg * SEG, b"", tail=LONG_AUX)
    for s in decoy_segs:
        b.more(i, s * SEG, decoy_chain())
    if decoy_segs:
        b.more(i, decoy_segs[0] * SEG + 8000, decoy_chain())
    return rec, g, b, i


@functools.lru_cache(maxsize=None)
def case_d():
    rec, g, b, i = _long_record(104, 5, (5, 6))
    return Case("d", rec, g, [Variant("plain", (16384, 5), control_of="decoy", block=BLOCK, extra=b.zeroed()), Variant("decoy", (16384, 5), block=BLOCK, extra=b.extra)], long=i)


@functools.lru_cache(maxsize=None)
def case_e():
    """chunks of 3 blocks end at stream segment 6: the long record starts in segment 3, so more than a segment of it is carried,
    the chains at segments 4 and 5 with it"""
    rec, g, b, i = _long_record(105, 4, (4, 5))
    return Case("e", rec, g, [Variant("decoy", (3, 16384), block=BLOCK, extra=b.extra), Variant("control", (3, 16384), control_of="decoy", block=BLOCK, extra=b.zeroed())], long=i)


@functools.lru_cache(maxsize=None)
def case_f():
    """blocks of 4 KiB through the long record, one block per chunk: chunks that lie wholly inside one record"""
    rec, g, b, i = _long_record(106, 2, (), n_pairs=200)
    off = b.offsets()
    cuts = uniform_cuts(off[-1], cuts=range(off[i] + 1000, off[i + 1], 4096))
    return Case("f", rec, g, [Variant("plain", (1,), extra=b.extra, cuts=cuts)], long=i)


@functools.lru_cache(maxsize=None)
def case_g():
    """ONE fake header at the start of the last segment of a chunk of two blocks, its block_size leaving the data"""
    rec, g, b, placed = _decoy_case("g", 107, (3, 7), (2, 16384), fake_header(FAR), n_pairs=500)
    return Case("g", rec, g, [Variant("decoy", (2, 16384), block=BLOCK, extra=b.extra), Variant("control", (2, 16384), control_of="decoy", block=BLOCK, extra=b.zeroed())],
                decoys=[at for _, at in placed])


SEAM_K = list(range(37)) + [40, 100]


@functools.lru_cache(maxsize=None)
def case_h():
    """block ends k bytes into a record, k = 0 .. 36, 40, 100 and the record's last byte, every third record, one block per chunk"""
    rec, g = base_records(300, 108, str_frac=0.2)
    off = layout(rec, bamio.sam_header(rec.targets), {})[0]
    seams = [off[2 + 3 * j] + k for j, k in enumerate(SEAM_K)]
    j = 2 + 3 * len(SEAM_K)
    seams.append(off[j + 1] - 1)
    return Case("h", rec, g, [Variant("seams", (1,), cuts=uniform_cuts(off[-1], cuts=seams))], last_byte=off[j + 1] - 1 - off[j])


@functools.lru_cache(maxsize=None)
def case_i():
    """40 KB of header text: the first record lies beyond the second segment of its block; with smaller blocks, in the second block"""
    rec, g = base_records(300, 109)
    text = bamio.sam_header(rec.targets) + "".join(f"@CO\tline {j:04d} " + "x" * 80 + "\n" for j in range(420))
    return Case("i", rec, g, [Variant("one_block", (16384, 3), header_text=text, block=0xFF00), Variant("two_blocks", (16384, 3), header_text=text, block=BLOCK)])


@functools.lru_cache(maxsize=None)
def case_j():
    """chunk 0 ends with a record, on a segment boundary; in chunk 1 a record ends on a segment boundary and another one segment on,
    20 bytes in front of the chunk's end; chunk 2 ends inside its third record"""
    rec, g = base_records(300, 110)
    b = Builder(rec)
    e0, e1, e2 = 3 * SEG, 4 * SEG, 5 * SEG
    ends = [b.end_at(e) for e in (e0, e1, e2)]
    off = b.offsets()
    j = ends[2] + 1
    cuts = [e0, e2 + 20, off[j + 2] + 50]
    return Case("j", rec, g, [Variant("aligned", (1,), extra=b.extra, cuts=uniform_cuts(off[-1], step=0xFF00, cuts=cuts))], ends=(e0, e1, e2), cuts=cuts)


def _seq(rng, n):
    return np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].tobytes().decode()


# name -> predicate over (rec, i): the record shapes rec_parse_kernel must see
SHAPES = {
    "no_cigar_placed": lambda r, i: r.cigar_off[i + 1] == r.cigar_off[i] and r.tid[i] >= 0,
    "no_cigar_unplaced": lambda r, i: r.cigar_off[i + 1] == r.cigar_off[i] and r.tid[i] < 0,
    "no_seq": lambda r, i: r.l_seq[i] == 0 and r.cigar_off[i + 1] > r.cigar_off[i],
    "smallest": lambda r, i: r.l_seq[i] == 0 and r.cigar_off[i + 1] == r.cigar_off[i] and r.qname_off[i + 1] - r.qname_off[i] == 1,
    "name_254": lambda r, i: r.qname_off[i + 1] - r.qname_off[i] == 254,
    "odd_l_seq": lambda r, i: r.l_seq[i] % 2 == 1,
    "cigar_ops": lambda r, i: {int(c) & 15 for c in r.cigar[int(r.cigar_off[i]):int(r.cigar_off[i + 1])]} >= {1, 2, 3, 4, 6, 7, 8},
    "hard_clipped": lambda r, i: r.cigar_off[i + 1] - r.cigar_off[i] >= 3 and int(r.cigar[int(r.cigar_off[i])]) & 15 == 5 and int(r.cigar[int(r.cigar_off[i + 1]) - 1]) & 15 == 5,
    "leading_s": lambda r, i: r.cigar_off[i + 1] > r.cigar_off[i] and int(r.cigar[int(r.cigar_off[i])]) & 15 == 4,
    "trailing_s": lambda r, i: r.cigar_off[i + 1] - r.cigar_off[i] > 1 and int(r.cigar[int(r.cigar_off[i + 1]) - 1]) & 15 == 4,
    "unmapped_with_cigar": lambda r, i: r.flag[i] & 4 and r.cigar_off[i + 1] > r.cigar_off[i],
    "tlen_-1": lambda r, i: r.isize[i] == -1,
    "tlen_0": lambda r, i: r.isize[i] == 0,
    "tlen_4095": lambda r, i: r.isize[i] == 4095,
    "tlen_4096": lambda r, i: r.isize[i] == 4096,
    "pos_-1": lambda r, i: r.pos[i] == -1,
    "secondary": lambda r, i: r.flag[i] & 0x100,
    "supplementary": lambda r, i: r.flag[i] & 0x800,
}


def _shape_rows(targets, rng, copy):
    """one record of every shape (SHAPES says which is which), placed on the contigs at random"""
    def row(q, cigar="", seq="", tid=None, flag=0x1, isize=0, mapq=60, pos=None):
        t = int(rng.integers(0, len(targets))) if tid is None else tid
        p = (int(rng.integers(0, targets[t][1] - 5000)) if t >= 0 else -1) if pos is None else pos
        return dict(tid=t, pos=p, mtid=t, mpos=p, flag=flag, mapq=mapq, cigar=cigar, seq=seq, qname=f"{q}{copy}".encode(), isize=isize)
    ca = "CAG" * 50
    rows = [
        row("ncp", "", ca, flag=0x1 | 0x4), row("ncq", "", _seq(rng, 150)),                         # no cigar, placed: unmapped beside its mate, and a mapped flag
        row("ncu", "", ca, tid=-1, flag=0x1 | 0x4 | 0x8),
        row("nsq", "30M", ""),
        row("n254" + "n" * 249, "150M", ca),
        row("odd", "151M", _seq(rng, 151)), row("od1", "1M", "A"), row("o33", "20S13M", "AC" * 10 + _seq(rng, 13)),
        row("ops", "12S40=3X200N2D20M5I3P30M25S", "AG" * 6 + _seq(rng, 40 + 3 + 20 + 5 + 30) + "CT" * 12 + "C"),
        row("hcl", "5H30S100M20S7H", "AAC" * 10 + _seq(rng, 100) + "GT" * 10),
        row("lds", "60S90M", "AT" * 30 + _seq(rng, 90)), row("trs", "90M60S", _seq(rng, 90) + "CCG" * 20),
        row("umc", "150M", ca, flag=0x1 | 0x4),
        row("tm1", "150M", _seq(rng, 150), flag=0x1 | 0x2, isize=-1), row("t00", "150M", _seq(rng, 150), flag=0x1 | 0x2, isize=0),
        row("t95", "150M", _seq(rng, 150), flag=0x1 | 0x2, isize=4095), row("t96", "150M", _seq(rng, 150), flag=0x1 | 0x2, isize=4096),
        row("pm1", "", _seq(rng, 150), tid=-1, flag=0x4),
        row("sec", "150M", ca, flag=0x1 | 0x100), row("sup", "70S80M", "AG" * 35 + _seq(rng, 80), flag=0x1 | 0x800),
    ]
    return rows


N_SMALLEST = 900


@functools.lru_cache(maxsize=None)
def case_k():
    """every record shape twice among ordinary records, 900 records of the smallest kind (38 bytes: 431 to a segment) at the end;
    `cuts`: one block per chunk, a chunk ending behind one record of every shape"""
    rec0, g = base_records(400, 111)
    rng = np.random.default_rng(111)
    rows = _rows_of(rec0) + _shape_rows(rec0.targets, rng, "a") + _shape_rows(rec0.targets, rng, "b")
    rows += [dict(tid=-1, pos=-1, mtid=-1, mpos=-1, flag=0x4, mapq=0, cigar="", seq="", qname=b"abcdefghijklmnopqrstuvwxyz"[j % 26:j % 26 + 1], isize=0) for j in range(N_SMALLEST)]
    rec = _batch(rows, rec0.targets)
    off = layout(rec, bamio.sam_header(rec.targets), {})[0]
    last = {}
    for name, fn in SHAPES.items():
        i = next(i for i in range(rec.n) if fn(rec, i) and off[i + 1] not in last.values())
        last[name] = off[i + 1]
    return Case("k", rec, g, [Variant("uniform", (16384, 2), block=20011), Variant("cuts", (1,), cuts=uniform_cuts(off[-1], cuts=last.values()))], last=last)


@functools.lru_cache(maxsize=None)
def case_l():
    """one record with a 1.1 MB array, from stream segment 13 on.  Whole in one chunk it is a record like any other; chunks of four
    blocks end at 261120 k, the fifth of them 1.09 MB into the record: a carry of more than FRONT_CARRY_MAX"""
    rec, g = base_records(450, 112)
    b = Builder(rec)
    i = b.put(13 * SEG, b"", tail=1_100_000)
    return Case("l", rec, g, [Variant("huge", (4, 16384), extra=b.extra, block=0xFF00)], long=i)


@functools.lru_cache(maxsize=None)
def case_n():
    """no crafted byte at all: the records of contig 0 at 65536 .. 131071 that base_records() speaks of, 150 of them in a row"""
    rec, g = base_records(500, 113, contig_len=300_000)
    rows = _rows_of(rec)
    rng = np.random.default_rng(113)
    for j in range(150):
        p = 65_600 + 400 * j
        rows.append(dict(tid=0, pos=p, mtid=0, mpos=p + 200, flag=0x1 | 0x2 | 0x40 | 0x20, mapq=60, cigar="150M", seq=_seq(rng, 150), qname=f"nat{j}".encode(), isize=350))
    return Case("n", _batch(rows, rec.targets), g, [Variant("natural", (16384, 2), block=BLOCK)])


CASES = {"a": case_a, "b": case_b, "c": case_c, "d": case_d, "e": case_e, "f": case_f, "g": case_g, "h": case_h, "i": case_i, "j": case_j, "k": case_k, "l": case_l, "n": case_n}


def files():
    """(case name, variant label, chunk_blocks) of everything the scan is run on"""
    return [(n, v.label, cb) for n, fn in CASES.items() for v in fn().variants.values() for cb in v.chunk_blocks]


def cut_inside_last_record(src, dst, keep=50, block=0xFF00):
    """src with its inflated stream ended `keep` bytes into the last record, in valid BGZF blocks + the EOF block
    -> (bytes of the stream kept, offset of the record it ends in)"""
    stream, _ = inflate(src)
    offs = truth(stream, bam_header(stream)[1])
    assert offs[-1] == len(stream) and len(offs) > 2
    n = offs[-2] + keep
    assert n < offs[-1]
    with open(dst, "wb") as f:
        for o in range(0, n, block):
            f.write(bamio._bgzf_block(stream[o:min(n, o + block)]))
        f.write(bamio._EOF)
    return n, offs[-2]
