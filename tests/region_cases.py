"""Inputs that put the three kernels behind the inflate of a region read (strling_amd/csrc/bgzf.hip: crc32_kernel,
region_walk_kernel, region_copy_kernel; strl_regions_fetch and the two other callers of regions_inflate_walk) on their edges,
and a plain-Python model of what they must answer.

Plain builders, no GPU code.  A CALL is what one strl_regions_fetch takes: BGZF blocks (pieces of inflated streams, each
deflated raw by zlib, with its ISIZE and zlib.crc32) and requests (first_block, n_blocks, in_block, tid, beg, end).  A call is
made of SETS -- a stream of BAM records cut into blocks at chosen byte offsets -- laid one behind the other; a set may ask for
its first byte's offset modulo 16 in the call's inflated bytes (a block of zeros in front of it, named by no request, makes
up the difference), because the walk's window and the copy's pieces are aligned on the call's bytes, not on the set's.  A CASE
is one request of a call with a family (w window, k keep rule, s stop rule, e bytes end first, b block layout, m malformed,
c copy), a name and a WITNESS: a predicate over the model's trace of that request which proves that the case reaches the edge
it is named for.  The records come from evidence_cases.rd / batch / raw_of.

The model (walk) restates the rule the header gives for strl_regions_fetch and the comments of region_walk_kernel give for its
window: it returns status, keep and stop, every window (w0, w1) loaded and why, and which of the three ways each CIGAR was
read.  layout() restates where strl_regions_fetch puts each region's bytes.  crc_dealt() restates how crc32_kernel deals a
block's dwords to 64 lanes.  Each takes a `mut` that breaks it the way a wrong kernel would be broken, so that the CPU suite
can show which case tells that break apart.  tests/test_region_cases.py runs all of it on the CPU, and the host's stand-in
(cli/region_feed.cpp: region_walk) against the model; tests/test_regions_edges_device.py runs the calls on the device.
"""
import functools
import struct
import zlib

import numpy as np

from evidence_cases import batch, raw_of, rd

RW_WIN = 4096                 # region_walk_kernel's LDS window
COPY_GRID = 4096              # the blocks region_copy_kernel is launched with at the most
INT32_MAX = 2 ** 31 - 1
FAR = 1_000_000               # an `end` behind every record of a set
ERR_CAPACITY, ERR_FORMAT, ERR_CRC = -4, -6, -8


def deflate(d):
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    return c.compress(d) + c.flush()


# ---- records ---------------------------------------------------------------------------------------------------------------
def R(pos, cigar="30M", name=b"f", tid=0, flag=0, seq=None):
    return rd(pos, cigar, seq, name, flag=flag, tid=tid)


def records(recs):
    """the records' bytes, one bytes object each"""
    raw, out, p = raw_of(batch(recs)), [], 0
    while p < len(raw):
        n = 4 + struct.unpack_from("<I", raw, p)[0]
        out.append(raw[p:p + n])
        p += n
    assert p == len(raw) and len(out) == len(recs)
    return out


def offsets(pieces):
    """where each piece starts in their join, and the join's length"""
    off = [0]
    for x in pieces:
        off.append(off[-1] + len(x))
    return off


S0 = len(records([R(0, name=b"")])[0])        # the filler "30M" with an empty name; a name of n bytes adds n


def fill(total, pos):
    """filler records ("30M" at `pos`) of exactly `total` bytes together"""
    out = []
    assert total >= S0, total
    while total > S0 + 200:
        out.append(R(pos, name=b"x" * (150 - S0)))
        total -= 150
    out.append(R(pos, name=b"x" * (total - S0)))
    return out


def header_only(tid, pos):
    """the 36 bytes of a record with no name, CIGAR or SEQ: block_size 32"""
    return struct.pack("<IiiBBHHHiiii", 32, tid, pos, 0, 0, 4680, 0, 4, 0, -1, -1, 0)


def patch(b, at, fmt, v):
    b = bytearray(b)
    struct.pack_into(fmt, b, at, v)
    return bytes(b)


# ---- the model -------------------------------------------------------------------------------------------------------------
class Trace:
    """what the walk of one request did: status, keep and stop (offsets in the call's bytes; None with status 1), base and lim,
    p0 (where it started) and p (where it ended), wins = [(w0, w1, why, p, w1 before)] with why = "header" or "cigar", paths =
    [(p, way, need, n_cigar)] for every record whose CIGAR was looked at (way = "lds", "global" or "malformed"), recs = the
    records passed, end = why the walk ended ("ref", "pos": a stopping record; "lim-header", "lim-body", "bad-size": status 1),
    max_read = one past the highest byte of the call the rule looked at, outside the window's loads"""
    def __init__(self):
        self.status, self.keep, self.stop, self.wins, self.paths, self.recs, self.end, self.max_read = 1, None, None, [], [], [], None, 0


def walk(call, req, mut=None):
    """strl_regions_fetch's rule for one request.  From base + in_block on, record by record, while a whole 36-byte header lies
    in front of lim (the end of the request's last block): a block_size outside 32 .. 2^28 ends it (status 1); a record on another
    reference or with pos >= end ends it (status 0, stop there); a record that does not end in front of lim ends it (status 1);
    as long as no record is kept, the record is kept if pos + 1 + (the sum of the lengths of ALL its CIGAR operations) > beg --
    a CIGAR that would leave its record is not read and the record is kept; status 0 with nothing kept is an empty range at stop.
    The window: 4096 bytes of the call from p rounded down to 16, cut at u_readable = (total + 64) rounded down to 16; loaded
    when a header is not inside it, and once more from the record's start when a CIGAR of need = 36 + l_name + 4 n_cigar bytes
    crosses its end and need <= 4096 - 16; a CIGAR that is not inside the window then is read from global memory."""
    fb, nb, in_block, tid, beg, end = req
    u, uoff, isize = call.padded, call.uoff, call.isize
    last = fb + nb - 1
    t = Trace()
    t.base, t.lim = uoff[fb], uoff[last] + isize[last]
    readable = (call.tot + 64) & ~15
    p, w0, w1 = t.base + in_block, 0, 0
    t.p0 = p

    def ld32(at):
        t.max_read = max(t.max_read, at + 4)
        return struct.unpack_from("<I", u, at)[0]

    def load(at, why):
        nonlocal w0, w1
        before = w1
        w0 = at & ~15
        w1 = min(w0 + RW_WIN, readable)
        t.wins.append((w0, w1, why, at, before))

    while p + 36 <= t.lim:
        if p < w0 or p + 36 > w1:
            load(p, "header")
            assert p + 36 <= w1
        bs = ld32(p)
        if bs < 32 or bs > 1 << 28:
            t.end = "bad-size"
            break
        ref, pos = struct.unpack("<ii", struct.pack("<II", ld32(p + 4), ld32(p + 8)))
        if ref != tid or (pos > end if mut == "end_gt" else pos >= end):
            t.status, t.end = 0, "ref" if ref != tid else "pos"
            break
        if p + 4 + bs > t.lim:
            t.end = "lim-body"
            break
        if t.keep is None:
            t.max_read = max(t.max_read, p + 18)
            l_name, n_cig = u[p + 12], struct.unpack_from("<H", u, p + 16)[0]
            need = 36 + l_name + 4 * n_cig
            if need <= 4 + bs:
                if p + need > w1 and (need < RW_WIN - 16 if mut == "reload_lt" else need <= RW_WIN - 16) and mut != "no_cigar_reload":
                    load(p, "cigar")
                way = "lds" if p + need <= w1 else "global"
                span = 1 + sum(ld32(p + 36 + l_name + 4 * k) >> 4 for k in range(n_cig))
            else:
                way, span = "malformed", 1 << 40
            t.paths.append((p, way, need, n_cig))
            if (pos + span >= beg) if mut == "beg_ge" else (pos + span > beg):
                t.keep = p
        t.recs.append(p)
        p += 4 + bs
    else:
        t.end = "lim-header"
    t.p = p
    if t.status == 0:
        if t.keep is None and mut != "no_empty_keep":
            t.keep = p
        t.stop = p
    else:
        t.keep = None
    return t


def layout(ranges):
    """where strl_regions_fetch puts the regions' bytes: back to back, every non-empty piece at the next multiple of 16 plus its
    source's offset modulo 16.  ranges = [(keep, stop) or None] -> out_off, out_len, the bytes needed"""
    at, off, ln = 0, [], []
    for r in ranges:
        n = r[1] - r[0] if r else 0
        if n:
            at = ((at + 15) & ~15) + (r[0] & 15)
        off.append(at)
        ln.append(n)
        at += n
    return off, ln, at


class Case:
    def __init__(self, call, family, name, req, witness):
        self.call, self.family, self.name, self.req, self.witness = call, family, name, req, witness

    @property
    def id(self):
        return f"{self.family}-{self.name}"

    def __repr__(self):
        return f"Case({self.id})"


class Call:
    def __init__(self, name):
        self.name, self.blocks, self.cases = name, [], []

    @property
    def tot(self):
        return sum(len(b) for b in self.blocks)

    def add_set(self, pieces, cuts, align=None):
        """the join of `pieces` cut into blocks at the offsets `cuts` (a repeated offset is an empty block) -> (the first block's
        index, the offsets of the pieces in the set)"""
        if align is not None and (align - self.tot) % 16:
            self.blocks.append(bytes((align - self.tot) % 16))
        stream, first = b"".join(pieces), len(self.blocks)
        at = [0] + list(cuts) + [len(stream)]
        assert at == sorted(at) and at[-1] == len(stream), at
        self.blocks += [stream[a:b] for a, b in zip(at, at[1:])]
        self.__dict__.pop("_laid", None)
        return first, offsets(pieces)

    def case(self, family, name, req, witness):
        self.cases.append(Case(self, family, name, tuple(req), witness))

    def block_of(self, first, at):
        """(block, offset inside it) of byte `at` of the set whose first block is `first`"""
        b = first
        while at >= len(self.blocks[b]):
            at -= len(self.blocks[b])
            b += 1
        return b, at

    # what the entry points take, and the model's answers; computed once, when the call is complete
    def _lay(self):
        if "_laid" not in self.__dict__:
            self.isize = [len(b) for b in self.blocks]
            self.uoff = offsets(self.blocks)[:-1]
            self.u = b"".join(self.blocks)
            self.padded = self.u + bytes(64)
            self.streams = [deflate(b) for b in self.blocks]
            self.crcs = [zlib.crc32(b) for b in self.blocks]
            self.requests = [c.req for c in self.cases]
            self.traces = [walk(self, q) for q in self.requests]
            self.ranges = [(t.keep, t.stop) if t.status == 0 else None for t in self.traces]
            self.out_off, self.out_len, self.needed = layout(self.ranges)
            self.expect = [(self.u[t.keep:t.stop] if t.status == 0 else b"", t.status) for t in self.traces]
            self._laid = True
        return self

    def __repr__(self):
        return f"Call({self.name})"


def _stream(recs, tail=()):
    """records (dicts of rd) and ready-made bytes behind them -> pieces"""
    return records(recs) + list(tail)


STOPPER = R(10, tid=1, name=b"stop")          # a record on the next reference


# ---- w. the window -----------------------------------------------------------------------------------------------------------
def family_w():
    C = Call("w")
    big = FAR
    # a record start at every offset mod 16
    recs = [R(1000 + 10 * i, name=b"n" * ((i * 7) % 16)) for i in range(40)] + [STOPPER]
    fb, off = C.add_set(_stream(recs), range(1500, 3000, 1499), align=0)
    base = sum(len(b) for b in C.blocks[:fb])
    for j in range(16):
        i = next(i for i in range(37) if (base + off[i]) % 16 == j)
        b, inb = C.block_of(fb, off[i])
        C.case("w", f"start-mod16-{j}", (b, len(C.blocks) - b, inb, 0, 1000 + 10 * i, 1000 + 10 * (i + 2)),
               lambda t, c, j=j: t.status == 0 and t.keep == t.p0 and t.keep % 16 == j and t.wins[0][:2] == (t.keep - j, t.keep - j + RW_WIN) and len(t.recs) == 2)
    # a header that crosses the window's end by d bytes; by 0: it ends with the window and is read without a reload
    for d in (1, 35, 0):
        recs = fill(RW_WIN - 36 + d, 1000) + [R(2000, name=b"X"), R(2010, name=b"Y"), STOPPER]
        fb, off = C.add_set(_stream(recs), [1501], align=0)
        x = len(recs) - 3
        if d:
            wit = lambda t, c, d=d: t.status == 0 and any(w[2] == "header" and w[3] < w[4] and w[3] + 36 - w[4] == d for w in t.wins[1:]) and t.keep == t.p0
        else:
            wit = lambda t, c: t.status == 0 and any(p + 36 == t.wins[0][1] for p in t.recs) and all(w[3] + 36 != t.wins[0][1] for w in t.wins) and len(t.wins) == 2
        C.case("w", f"header-crosses-by-{d}", (fb, len(C.blocks) - fb, 0, 0, 0, big), wit)
        assert off[x] == RW_WIN - 36 + d
    # a CIGAR that crosses the window's end behind a header inside it: the second load
    recs = fill(RW_WIN - 40, 1000) + [R(2000, name=b"X"), R(2010, name=b"Y"), STOPPER]
    fb, off = C.add_set(_stream(recs), [777], align=0)
    C.case("w", "cigar-crosses-header-inside", (fb, len(C.blocks) - fb, 0, 0, 1500, big),
           lambda t, c: t.status == 0 and [w[2] for w in t.wins[:2]] == ["header", "cigar"] and t.wins[1][3] == t.keep and t.wins[1][3] + 36 <= t.wins[1][4]
           and t.paths[-1][1] == "lds" and t.keep > t.p0)
    # need = 4080: the longest CIGAR the window takes after a reload, from a record start of 15 mod 16; 4081: global memory.  beg =
    # pos + the sum of the operations: the record is kept only if every operation was counted
    for name, way in ((b"abc", "lds"), (b"abcd", "global")):
        need = 36 + len(name) + 1 + 4 * 1010
        recs = fill(1007, 1000) + [R(2000, "1M1I" * 505, name=name), R(2500, name=b"Y"), STOPPER]
        fb, off = C.add_set(_stream(recs), [1000, 4000], align=0)
        C.case("w", f"need-{need}", (fb, len(C.blocks) - fb, 0, 0, 2000 + 1010, big),
               lambda t, c, need=need, way=way: t.status == 0 and t.paths[-1][1:] == (way, need, 1010) and t.keep == t.paths[-1][0] and t.keep % 16 == 15
               and t.keep + need > t.wins[0][1] and ((way == "lds") == any(w[2] == "cigar" for w in t.wins)))
    # a record longer than the window: the next header lies behind the window, not across its end
    recs = fill(500, 1000) + [R(2000, "3000M", name=b"X"), R(2010, name=b"Y"), STOPPER]
    fb, off = C.add_set(_stream(recs), [2222], align=0)
    C.case("w", "record-longer-than-window", (fb, len(C.blocks) - fb, 0, 0, 0, big),
           lambda t, c: t.status == 0 and any(w[2] == "header" and w[3] >= w[4] > 0 for w in t.wins) and len(t.recs) >= 5)
    # a record longer than a BGZF block, over three blocks
    recs = fill(300, 1000) + [R(2000, "100000M", name=b"X"), R(2010, name=b"Y"), STOPPER]
    fb, off = C.add_set(_stream(recs), [65536, 131072], align=0)
    C.case("w", "record-over-three-blocks", (fb, 3, 0, 0, 2000 + 100000, big),
           lambda t, c, fb=fb: t.status == 0 and c.isize[fb:fb + 2] == [65536, 65536] and t.keep < c.uoff[fb + 1] and t.stop > c.uoff[fb + 2] and t.paths[-1][1] == "lds")
    # a CIGAR of 65535 operations (the 360 kB record), kept only if every one of them was counted
    recs = fill(500, 1000) + [R(2000, "1M1I" * 32767 + "1M", name=b"big"), R(3000, name=b"Y"), STOPPER]
    fb, off = C.add_set(_stream(recs), range(65536, 6 * 65536, 65536), align=0)
    C.case("w", "cigar-65535", (fb, len(C.blocks) - fb, 0, 0, 2000 + 65535, big),
           lambda t, c: t.status == 0 and t.paths[-1][1:] == ("global", 36 + 4 + 4 * 65535, 65535) and t.keep == t.paths[-1][0] and t.stop - t.keep > 300_000)
    # the call's last window, cut short by u_readable; the stopping record's header ends with the call's last byte
    pieces = _stream(fill(600, 1000), [header_only(1, 0)])
    fb, off = C.add_set(pieces, [250], align=0)
    C.case("w", "last-window-cut", (fb, len(C.blocks) - fb, 0, 0, 0, big),
           lambda t, c: t.status == 0 and t.stop + 36 == c.tot == t.lim and t.wins[-1][1] == (c.tot + 64) & ~15 and t.wins[-1][1] - t.wins[-1][0] < RW_WIN and t.stop > t.keep)
    return C


# ---- k. the keep rule ------------------------------------------------------------------------------------------------------
def family_k():
    C = Call("k")
    recs = [R(1000, "50M", name=b"r0"),                         # reaches 1050
            R(1010, "3H10S20M5I20M", name=b"r1"),              # 58 with the clips and the insertion, 40 on the reference
            R(1020, "*", name=b"r2", flag=0x1 | 0x4, seq=""),  # no CIGAR: reaches its own pos
            R(1030, "40M", name=b"r3", flag=0x4),              # unmapped, with a CIGAR that counts: 1070
            R(1100, "100M", name=b"r4"),                       # 1200
            R(1110, "5M", name=b"r5"),                         # a short one behind a long one: 1115
            R(1120, "30M", name=b"r6"),
            R(2000, "30M", name=b"r7"),
            STOPPER]
    fb, off = C.add_set(_stream(recs), [333, 700], align=5)
    base = C.tot - off[-1]
    nb = len(C.blocks) - fb

    def one(name, start, beg, end, keep, stop):
        b, inb = C.block_of(fb, off[start])
        C.case("k", name, (b, fb + nb - b, inb, 0, beg, end),
               lambda t, c: t.status == 0 and (t.keep, t.stop) == (base + off[keep], base + off[stop]))

    one("reach-is-beg-minus-1", 0, 1051, 1500, 1, 7)
    one("reach-is-beg", 0, 1050, 1500, 0, 7)
    one("clips-and-insertions-reach", 0, 1068, 1500, 1, 7)
    one("clips-and-insertions-short", 0, 1069, 1500, 3, 7)     # r2 (no CIGAR) is dropped too; r3's flag does not void its CIGAR
    one("unmapped-flag-cigar-short", 0, 1071, 1500, 4, 7)
    one("no-cigar-kept", 2, 1020, 1500, 2, 7)
    one("no-cigar-dropped", 2, 1021, 1500, 3, 7)
    one("short-record-behind-kept", 0, 1150, 1500, 4, 7)       # r5 and r6 end in front of beg and stay in the range
    one("beg-negative", 0, -5, 1015, 0, 2)
    one("nothing-reaches-beg", 0, 1500, 1600, 7, 7)            # an empty range at stop
    return C


# ---- s. the stop rule ------------------------------------------------------------------------------------------------------
def family_s():
    C = Call("s")
    recs = [R(1000, name=b"r0"), R(1099, name=b"r1"), R(1100, name=b"r2"), R(1200, name=b"r3"),
            R(50, tid=1, name=b"r4"), R(60, tid=1, name=b"r5"),
            R(-1, "*", tid=-1, name=b"r6", flag=0x4, seq="ACGT"), R(-1, "*", tid=-1, name=b"r7", flag=0x4, seq="ACGT")]
    fb, off = C.add_set(_stream(recs), [200, 201, 500], align=11)
    base = C.tot - off[-1]
    nb = len(C.blocks) - fb

    def one(name, start, tid, beg, end, keep, stop, why):
        b, inb = C.block_of(fb, off[start])
        C.case("s", name, (b, fb + nb - b, inb, tid, beg, end),
               lambda t, c: t.status == 0 and t.end == why and (t.keep, t.stop) == (base + off[keep], base + off[stop]))

    one("pos-is-end-minus-1", 0, 0, 0, 1100, 0, 2, "pos")       # r1 at end - 1 goes on, r2 at end stops
    one("pos-is-end", 0, 0, 0, 1099, 0, 1, "pos")
    one("next-reference", 0, 0, 0, 5000, 0, 4, "ref")
    one("unplaced-tail", 4, 1, 0, 5000, 4, 6, "ref")
    one("first-record-stops", 0, 0, 0, 1000, 0, 0, "pos")
    one("tid-of-another-reference", 0, 1, 0, 5000, 0, 0, "ref")
    return C


# ---- e. the bytes end first ------------------------------------------------------------------------------------------------
def family_e():
    C = Call("e")
    recs = [R(1000 + 10 * i, name=b"e%d" % i) for i in range(6)]
    pieces = _stream(recs)
    o3 = offsets(pieces)[3]
    fb, off = C.add_set(pieces, [o3, o3 + 1, o3 + 35, o3 + 46], align=3)
    base = C.tot - off[-1]
    for name, nb, end, left in (("ends-behind-a-record", 1, "lim-header", 0), ("ends-1-into-a-header", 2, "lim-header", 1),
                                ("ends-35-into-a-header", 3, "lim-header", 35), ("ends-inside-a-body", 4, "lim-body", 46)):
        C.case("e", name, (fb, nb, 0, 0, 0, FAR),
               lambda t, c, end=end, left=left: t.status == 1 and t.end == end and t.p == base + o3 and t.lim - t.p == left and len(t.recs) == 3)
    C.case("e", "last-blocks-of-the-call", (fb, 5, 0, 0, 0, FAR), lambda t, c: t.status == 1 and t.end == "lim-header" and t.p == t.lim == c.tot and len(t.recs) == 6)
    return C


# ---- b. the block layout ---------------------------------------------------------------------------------------------------
def family_b():
    C = Call("b")
    recs = [R(1000 + 10 * i, name=b"b" * (1 + i % 5)) for i in range(10)] + [STOPPER]
    pieces = _stream(recs)
    o = offsets(pieces)
    odd = o[6] + 3 if (13 + o[6] + 3) % 2 else o[6] + 4
    # blocks: 0 = records 0 and 1, 1 empty, 2, 3 and 4 of one byte each inside record 4's header, 5, 6 from an odd offset, 7 empty
    fb, off = C.add_set(pieces, [o[2], o[2], o[4] + 5, o[4] + 6, o[4] + 7, odd, o[-1]], align=13)
    base = C.tot - off[-1]
    assert len(C.blocks) - fb == 8
    whole = lambda t, c, k=0: t.status == 0 and (t.keep, t.stop) == (base + o[k], base + o[10])
    C.case("b", "in-block-is-isize-two-blocks", (fb, 8, o[2], 0, 0, FAR), lambda t, c: whole(t, c, 2) and c.isize[fb] == o[2] and t.p0 == c.uoff[fb] + c.isize[fb])
    C.case("b", "in-block-is-isize-one-block", (fb, 1, o[2], 0, 0, FAR), lambda t, c: t.status == 1 and t.p0 == t.lim and not t.recs and not t.wins)
    C.case("b", "empty-blocks-inside-and-last", (fb, 8, 0, 0, 0, FAR), lambda t, c: whole(t, c) and c.isize[fb + 1] == 0 and c.isize[fb + 7] == 0)
    C.case("b", "one-byte-blocks", (fb + 2, 5, 0, 0, 0, FAR),
           lambda t, c: whole(t, c, 2) and c.isize[fb + 3:fb + 5] == [1, 1] and c.uoff[fb + 3] - 5 in t.recs)
    C.case("b", "same-blocks-first", (fb, 8, 0, 0, 1035, 1060), lambda t, c: t.status == 0 and (t.keep, t.stop) == (base + o[1], base + o[6]))
    C.case("b", "same-blocks-second", (fb, 8, 0, 0, 1065, 1095), lambda t, c: t.status == 0 and (t.keep, t.stop) == (base + o[4], base + o[10]))
    C.case("b", "later-first-block-odd-uoff", (fb + 6, 2, o[7] - odd, 0, 0, FAR), lambda t, c: whole(t, c, 7) and c.uoff[fb + 6] % 2 == 1 and fb + 6 > 0)
    return C


# ---- m. malformed ------------------------------------------------------------------------------------------------------------
def family_m():
    """inputs the walk is written to take: every case's witness holds the highest byte the rule looks at below lim"""
    C = Call("m")
    inside = lambda t: 0 < t.max_read <= t.lim
    for name, bs in (("block-size-31", 31), ("block-size-2-to-28-plus-1", (1 << 28) + 1)):
        p = _stream([R(1000, name=b"m0"), R(1010, name=b"m1"), R(1020, name=b"bad"), R(1030, name=b"m3"), STOPPER])
        p[2] = patch(p[2], 0, "<I", bs)
        fb, off = C.add_set(p, [150], align=7)
        C.case("m", name, (fb, 2, 0, 0, 0, FAR), lambda t, c, at=C.tot - off[-1] + off[2]: t.status == 1 and t.end == "bad-size" and t.p == at and inside(t))
    # a record whose CIGAR ends with the record (no SEQ): read; one operation more in n_cigar and it leaves the record: kept unread
    for name, n_cig, way in (("cigar-ends-with-record", 2, "lds"), ("cigar-leaves-record-by-4", 3, "malformed"), ("cigar-65535-leaves-record", 65535, "malformed")):
        p = _stream([R(900, name=b"m0"), R(910, name=b"m1"), R(1020, "1M1I", name=b"bad", seq=""), R(1030, name=b"m3"), STOPPER])
        p[2] = patch(p[2], 16, "<H", n_cig)
        bs = struct.unpack_from("<I", p[2], 0)[0]
        assert 36 + 4 + 4 * 2 == 4 + bs
        fb, off = C.add_set(p, [150], align=7)
        beg = 1022 if way == "lds" else INT32_MAX
        C.case("m", name, (fb, 2, 0, 0, beg, INT32_MAX),
               lambda t, c, at=C.tot - off[-1], off=off, way=way, n=n_cig: t.status == 0 and (t.keep, t.stop) == (at + off[2], at + off[4])
               and t.paths[-1] == (at + off[2], way, 40 + 4 * n, n) and inside(t))
    return C


# ---- c. the copy -------------------------------------------------------------------------------------------------------------
def family_c():
    C = Call("c")
    n = 64
    recs = [R(1000 + 10 * i, name=b"c" * ((i * 11 + i // 16) % 17)) for i in range(n)] + [STOPPER]
    pieces = _stream(recs)
    fb, off = C.add_set(pieces, [1000, 3001], align=0)
    base = C.tot - off[-1]
    nb = len(C.blocks) - fb

    def single(i):
        b, inb = C.block_of(fb, off[i])
        return (b, fb + nb - b, inb, 0, 1000 + 10 * i, 1000 + 10 * i + 1)

    for j in range(16):
        i = next(i for i in range(n) if (base + off[i]) % 16 == j)
        C.case("c", f"start-mod16-{j}", single(i), lambda t, c, j=j: t.status == 0 and t.keep % 16 == j and len(t.recs) == 1)
    for j in range(16):
        i = next(i for i in range(n) if len(pieces[i]) % 16 == j)
        C.case("c", f"length-mod16-{j}", single(i), lambda t, c, j=j: t.status == 0 and (t.stop - t.keep) % 16 == j and len(t.recs) == 1)
    C.case("c", "empty-between", (fb, nb, 0, 0, 5000, 5001), lambda t, c: t.status == 0 and t.keep == t.stop)
    C.case("c", "more-than-256-pieces", (fb, nb, 0, 0, 0, FAR), lambda t, c: t.status == 0 and t.stop - t.keep > 256 * 16 + 32)
    return C


def family_c_grid():
    """one call of 4100 requests: the copy's grid of 4096 blocks takes a second turn"""
    C = Call("c-grid")
    n = 12
    recs = [R(1000 + 10 * i, name=b"g%d" % i + b"c" * i) for i in range(n)] + [STOPPER]
    pieces = _stream(recs)
    fb, off = C.add_set(pieces, [400, 801], align=0)
    for r in range(COPY_GRID + 4):
        i = (r * 5 + r // n) % n
        b, inb = C.block_of(fb, off[i])
        C.case("c", f"grid-{r}", (b, 3 - b, inb, 0, 1000 + 10 * i, 1000 + 10 * i + 1),
               lambda t, c, i=i: t.status == 0 and (t.keep, t.stop) == (off[i], off[i + 1]))
    return C


@functools.lru_cache(maxsize=None)
def calls():
    """every call, laid out, with the model's answers"""
    return tuple(c._lay() for c in (family_w(), family_k(), family_s(), family_e(), family_b(), family_m(), family_c(), family_c_grid()))


def call(name):
    return next(c for c in calls() if c.name == name)


WALK_MUTATIONS = ("end_gt", "beg_ge", "no_empty_keep")      # breaks of walk() that change an answer
WINDOW_MUTATIONS = ("no_cigar_reload", "reload_lt")          # ... that change where a CIGAR is read from, and no answer


def copied(call, grid_loop=True):
    """the out buffer of the call as region_copy_kernel fills it (zeros where nothing is written); grid_loop=False: the kernel
    launched with min(n, 4096) blocks and no loop"""
    out = bytearray(call.needed)
    for r, rg in enumerate(call.ranges):
        if rg and (grid_loop or r < COPY_GRID):
            out[call.out_off[r]:call.out_off[r] + call.out_len[r]] = call.u[rg[0]:rg[1]]
    return bytes(out)


# ---- the CRC ---------------------------------------------------------------------------------------------------------------
def _crc_tables():
    tab = []
    for i in range(256):
        c = i
        for _ in range(8):
            c = 0xedb88320 ^ (c >> 1) if c & 1 else c >> 1
        tab.append(c)
    zop = [[tab[(1 << b) & 0xff] ^ ((1 << b) >> 8) for b in range(32)]]          # one zero byte, a column per state bit
    for k in range(1, 17):                                                         # 2^k zero bytes: the operator before, squared
        prev = zop[-1]
        zop.append([functools.reduce(lambda r, j: r ^ (prev[j] if (v >> j) & 1 else 0), range(32), 0) for v in prev])
    return tab, zop


TAB, ZOP = _crc_tables()


def crc_zeros(v, n):
    """the CRC state v run through n zero bytes"""
    k = 0
    while n and v:
        if n & 1:
            v = functools.reduce(lambda r, b: r ^ (ZOP[k][b] if (v >> b) & 1 else 0), range(32), 0)
        n >>= 1
        k += 1
    return v


ADV = [[crc_zeros(v << (8 * t), 256) for v in range(256)] for t in range(4)]       # "advance 256 bytes", a table per byte of the state


def crc_dealt(d, mut=None):
    """CRC-32 of d the way the comment above crc32_kernel deals it: the CRC is linear, so lane j of 64 takes the dwords j, j + 64,
    ... with the Horner step "advance 256 bytes, add the next dword", then advances by the bytes behind its last dword; lane 0 adds
    the last 0..3 bytes and the all-ones start value run through the whole block; the lanes XOR together and the sum is
    complemented.  mut = "drop_lane63" / "drop_tail": the kernel without that lane / without the tail bytes"""
    n = len(d)
    nd = n >> 2
    words = struct.unpack_from(f"<{nd}I", d)
    total = 0
    for lane in range(63 if mut == "drop_lane63" else 64):
        c, last = 0, None
        for i in range(lane, nd, 64):
            c = ADV[0][c & 0xff] ^ ADV[1][(c >> 8) & 0xff] ^ ADV[2][(c >> 16) & 0xff] ^ ADV[3][c >> 24] ^ words[i]
            last = i
        if last is not None:
            c = crc_zeros(c, n - 4 * last)
        if lane == 0:
            t = 0
            for b in d[4 * nd:] if mut != "drop_tail" else b"":
                t = TAB[(t ^ b) & 0xff] ^ (t >> 8)
            c ^= t ^ crc_zeros(0xffffffff, n)
        total ^= c
    return total ^ 0xffffffff


CRC_SIZES = (0, 1, 2, 3, 4, 5, 7, 255, 256, 257, 259, 260, 511, 512, 516, 1027, 65280, 65535, 65536)


class CrcRow:
    """one call: `blocks` (the bytes that are deflated), the CRCs that accept them and the CRCs that must refuse them -- those of
    the twin of block `bad` that differs in one bit (byte `at`, bit `bit`).  An empty block has no bit to flip: its refusing CRC
    is that of one zero byte."""
    def __init__(self, name, blocks, bad, at, bit):
        self.name, self.blocks, self.bad, self.at, self.bit = name, blocks, bad, at, bit
        self.good = [zlib.crc32(b) for b in blocks]
        self.refuse = list(self.good)
        if blocks[bad]:
            twin = bytearray(blocks[bad])
            twin[at] ^= 1 << bit
            self.twin = bytes(twin)
        else:
            self.twin = b"\0"
        self.refuse[bad] = zlib.crc32(self.twin)
        self.sizes = [len(b) for b in blocks]
        self.request = (0, 1, self.sizes[0], 0, 0, 1)          # a walk that ends at once: status 1

    @functools.cached_property
    def streams(self):
        return [deflate(b) for b in self.blocks]

    def __repr__(self):
        return f"CrcRow({self.name})"


def _plain(rng, n):
    """bytes of a sixteen-letter alphabet: they deflate with Huffman codes and matches, not as stored blocks"""
    return bytes(rng.integers(65, 81, n, dtype=np.uint8))


@functools.lru_cache(maxsize=None)
def crc_rows():
    rng = np.random.default_rng(20250117)
    rows = []
    for n in CRC_SIZES:
        d = _plain(rng, n)
        if n == 0:
            rows.append(CrcRow("size0", [d], 0, 0, 0))
            continue
        # first, last, each of the last four, lane 63's first dword, byte 256 (lane 0's second round), one in the middle
        at = [0, n - 1, n - 2, n - 3, n - 4, 252 + n % 4, 256, n // 2]
        for k, a in enumerate(sorted({a for a in at if 0 <= a < n})):
            rows.append(CrcRow(f"size{n}-byte{a}", [d], 0, a, (a + k) % 8))
    d = _plain(rng, 260)
    for lane in range(64):                                       # a bit of every lane's dword; lane 0 also has the second round's 256 .. 259
        rows.append(CrcRow(f"size260-lane{lane}", [d], 0, 4 * lane + lane % 4, (lane * 3) % 8))
    sizes = [37, 1, 258, 0, 515, 3, 1021, 7, 64]                 # odd sizes: uoff takes many alignments; nine blocks: three workgroups, the last with one wave at work
    blocks = [_plain(rng, n) for n in sizes]
    for bad in range(9):
        rows.append(CrcRow(f"nine-blocks-bad{bad}", blocks, bad, sizes[bad] // 2, bad % 8))
    return tuple(rows)


def crc_verdict(row, crcs, mut=None):
    """does crc32_kernel's rule refuse the row's blocks against `crcs`?  mut = "expect_blockidx": the kernel comparing with
    expect[workgroup] instead of expect[block]; or a mut of crc_dealt"""
    bad = False
    for b, d in enumerate(row.blocks):
        want = crcs[b // 4] if mut == "expect_blockidx" else crcs[b]
        bad |= crc_dealt(d, mut if mut != "expect_blockidx" else None) != want
    return bad
