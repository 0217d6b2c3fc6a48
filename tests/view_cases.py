"""Inputs for `strling view` (strling_amd/csrc/view_core.h, view.hip, cli/view_cli.cpp) and the reference its output is held against:
the rule of view_core.h's head written out again in Python with `struct` and `'%g' % value` -- never the code under test, and not
sam_cases.bam_to_sam, which prints floats by repr.  No machine of the project has samtools, so agreement with `samtools view` is
unverified.

Every case is a BAM whose records are packed here byte by byte, tens of records unless noted, the options it runs under and, for a
refusal, the ordinal and the words.  tests/test_view_cases.py runs the cases through the host path and the stand-alone program,
tests/test_view_device.py through the device."""
import math
import os
import struct
import subprocess

import numpy as np

from strling_amd import bamio

TG = [("t0", 1 << 20), ("chrTwo", (1 << 31) - 1), ("empty3", 5000)]
HEADER_TEXT = "@HD\tVN:1.6\tSO:coordinate\n" + "".join(f"@SQ\tSN:{n}\tLN:{l}\n" for n, l in TG)
CODES = "=ACMGRSVTWYHKDBN"
OPS = "MIDNSHP=X"
L_SEQS = (0, 1, 2, 15, 16, 17, 31, 32, 33, 151)
DEFAULTS = dict(f=0, F=0, G=0, q=0)
REFUSALS = dict(size="its name, CIGAR, bases and qualities do not fit its block_size", rname="RNAME: its refID is not one of the header's references",
                rnext="RNEXT: its next refID is not one of the header's references", cigar="CIGAR: an operation code above 8", tag_type="tags: an unknown type",
                tag_z="tags: a Z or H value without its NUL inside the record", tag_b="tags: a B array whose elements leave the record",
                tag_end="tags: they do not end exactly at the record's end")
# the floats the device formats itself, with the spellings checked against Python's %g
DEVICE_FLOATS = [(0.0, "0"), (-0.0, "-0"), (1.0, "1"), (0.5, "0.5"), (0.1, "0.1"), (0.0123, "0.0123"), (0.0001, "0.0001"), (1e-05, "1e-05"), (100000.0, "100000"),
                 (999999.5, "1e+06"), (123456.7, "123457"), (1000005.0, "1e+06"), (1000015.0, "1.00002e+06"), (16777216.0, "1.67772e+07"), (1.234565e-05, "1.23457e-05")]
HARD_FLOATS = [(3.4028235e38, "3.40282e+38"), (1e-45, "1.4013e-45"), (float("inf"), "inf"), (float("nan"), "nan")]


def rec(name=b"r", flag=0, tid=-1, pos=-1, mapq=0, cigar=(), mtid=-1, mpos=-1, tlen=0, seq="", qual=None, aux=b"", pad=0, l_name=None):
    """one record's bytes, its block_size word included.  cigar: [(length, op code)]; seq over CODES; qual: None (0xFF bytes), one
    value or the bytes; pad: the padding nibble of an odd l_seq; l_name: the byte as it is written (default len(name) + 1)."""
    name = name.encode() if isinstance(name, str) else bytes(name)
    l_seq = len(seq)
    q = b"\xff" * l_seq if qual is None else bytes([qual]) * l_seq if isinstance(qual, int) else bytes(qual)
    assert len(q) == l_seq
    codes = [CODES.index(c) for c in seq] + [pad]
    packed = bytes(codes[i] << 4 | codes[i + 1] for i in range(0, l_seq, 2))
    cg = b"".join(struct.pack("<I", l << 4 | op) for l, op in cigar)
    nm = name + b"\0" if l_name is None else name
    body = struct.pack("<iiBBHHHiiii", tid, pos, len(nm) if l_name is None else l_name, mapq, 4680, len(cigar), flag, l_seq, mtid, mpos, tlen) + nm + cg + packed + q + bytes(aux)
    return struct.pack("<I", len(body)) + body


def tag(key, typ, value=None, sub=None):
    k = key.encode()
    if typ in "cCsSiIfd":
        return k + typ.encode() + struct.pack("<" + dict(c="b", C="B", s="h", S="H", i="i", I="I", f="f", d="d")[typ], value)
    if typ == "A":
        return k + b"A" + value
    if typ in "ZH":
        return k + typ.encode() + value + b"\0"
    assert typ == "B"
    return k + b"B" + sub.encode() + struct.pack("<I", len(value)) + b"".join(struct.pack("<" + dict(c="b", C="B", s="h", S="H", i="i", I="I", f="f")[sub], v) for v in value)


def _seq(rng, n):
    return "".join(CODES[int(x)] for x in rng.integers(0, 16, n))


def _quals(rng, n):
    return bytes(rng.integers(0, 94, n, dtype=np.uint8))


def _every_tag():
    ints = [("c", -128), ("c", 127), ("C", 255), ("s", -32768), ("S", 65535), ("i", -(1 << 31)), ("i", (1 << 31) - 1), ("I", (1 << 32) - 1), ("I", 0)]
    out = [tag("X%d" % i, t, v) for i, (t, v) in enumerate(ints)]
    out += [tag("XA", "A", b"!"), tag("XZ", "Z", b"hello world"), tag("XE", "Z", b""), tag("XH", "H", b"1AE301"), tag("XF", "f", 0.5), tag("XD", "d", 0.5), tag("XG", "d", -100000.0)]
    for sub, vals in dict(c=[-128, 127, 0], C=[255, 0, 7], s=[-32768, 32767, 1], S=[65535, 0, 9], i=[-(1 << 31), (1 << 31) - 1, 5], I=[(1 << 32) - 1, 0, 3], f=[0.5, -1.0, 100000.0]).items():
        seventeen = [vals[k % 3] for k in range(17)]
        out += [tag("B" + sub, "B", [], sub), tag("b" + sub, "B", vals[:1], sub), tag("L" + sub, "B", seventeen, sub)]
    return out


def _random(n, seed):
    rng = np.random.default_rng(seed)
    tags = _every_tag()
    floats = [f for f, _ in DEVICE_FLOATS]
    out = []
    for i in range(n):
        l = int(rng.integers(0, 160))
        nc = int(rng.integers(0, 6))
        aux = b"".join(tags[int(k)] for k in rng.integers(0, len(tags), int(rng.integers(0, 5)))) + (tag("fl", "f", floats[i % len(floats)]) if i % 3 == 0 else b"")
        out.append(rec("q%d_%s" % (i, "x" * int(rng.integers(0, 20))), int(rng.integers(0, 1 << 12)), int(rng.integers(-1, 3)), int(rng.integers(-1, 1 << 20)), int(rng.integers(0, 61)),
                       [(int(rng.integers(1, 300)), int(rng.integers(0, 9))) for _ in range(nc)], int(rng.integers(-1, 3)), int(rng.integers(-1, 1 << 20)),
                       int(rng.integers(-1000, 1000)), _seq(rng, l), None if i % 11 == 0 else _quals(rng, l), aux))
    return out


def cases():
    """-> {name: dict(recs=[bytes], opts=, refused=None | (ordinal, key of REFUSALS), block=BGZF block bytes, hard=[ordinals with a hard float])}"""
    rng = np.random.default_rng(5)
    out = {}

    def add(name, recs, refused=None, block=600, hard=(), **opts):
        out[name] = dict(recs=list(recs), opts=dict(DEFAULTS, **opts), refused=refused, block=block, hard=list(hard))

    # SEQ and QUAL at every offset modulo 16 (names of 1 .. 17 bytes) for every length around the 16-byte words
    add("lengths", [rec("n" * k, 0, 0, 100 + k, 30, [(l, 0)] if l else [], seq=_seq(rng, l), qual=_quals(rng, l)) for l in L_SEQS for k in range(1, 18)], block=4000)
    add("padding_nibble", [rec("odd%d" % l, 0, seq=_seq(rng, l), qual=_quals(rng, l), pad=p) for l in (1, 15, 17, 33) for p in (1, 15)] +
        [rec("all", 0, seq=CODES + "A", qual=bytes(range(17)))])
    add("no_name", [rec(b"", 0, seq="ACGT", qual=30), rec(b"", 0, seq="AC", qual=3, l_name=0), rec("x", 4, seq="A", qual=1)])
    add("numbers", [rec("f%d" % f, f, 0, 5, seq="ACGT", qual=20) for f in (0, 9, 10, 99, 100, 65535)] +
        [rec("pos_m1", 0, -1, -1, seq="A", qual=1), rec("pos_max", 0, 1, (1 << 31) - 2, 255, [(1, 0)], 1, (1 << 31) - 2, seq="A", qual=1),
         rec("tlen_min", 0, 0, 0, 9, [(1, 0)], 0, 0, -(1 << 31), seq="A", qual=1), rec("tlen_max", 0, 0, 0, 10, [(1, 0)], 0, 0, (1 << 31) - 1, seq="A", qual=1),
         rec("tagints", 0, aux=b"".join(tag("I%d" % i, t, v) for i, (t, v) in enumerate([("c", -128), ("s", -32768), ("i", -(1 << 31)), ("C", 255), ("S", 65535), ("I", (1 << 32) - 1)])))])
    cig = lambda n: [(1 + k % 7 if k % 5 else (1 << 28) - 1, k % 9) for k in range(n)]
    add("cigars", [rec("c%d" % n, 0, 0, 7, 1, cig(n), seq="ACGTACGT", qual=11) for n in (0, 1, 16, 17)] + [rec("one", 0, 0, 7, 1, [(1, 8)]), rec("big", 0, 0, 7, 1, [((1 << 28) - 1, 0)])])
    add("cigar_65535", [rec("a", 0, 0, 1, seq="AC", qual=2), rec("long", 0, 0, 2, 3, cig(65535), seq="ACG", qual=5), rec("z", 0, 0, 3, seq="T", qual=9)], block=0xFF00)
    add("cigar_op_9", [rec("ok", 0, 0, 1, 1, [(3, 0)]), rec("ok2", 0, 0, 1, 1, [(3, 8)]), rec("bad", 0, 0, 1, 1, [(3, 0), (2, 9), (1, 0)])], refused=(2, "cigar"))
    add("references", [rec("none", 0, -1, -1, mtid=-1), rec("equal", 0, 1, 5, mtid=1, mpos=9), rec("differ", 0, 0, 5, mtid=1, mpos=9), rec("differ2", 0, 2, 5, mtid=0, mpos=0),
                       rec("mate_only", 0, -1, -1, mtid=2, mpos=1), rec("unplaced_mate", 0, 1, 4, mtid=-1)])
    add("tid_n_ref", [rec("ok", 0, 2, 1), rec("bad", 0, 3, 1)], refused=(1, "rname"))
    add("mtid_n_ref", [rec("bad", 0, 0, 1, mtid=3), rec("ok", 0, 2, 1)], refused=(0, "rnext"))
    add("quals", [rec("absent", 0, seq="ACGTA"), rec("later_ff", 0, seq="ACGTA", qual=bytes([10, 0xff, 20, 0xff, 0xff])), rec("q93_94", 0, seq="ACGT", qual=bytes([93, 94, 0, 92])),
                  rec("q254", 0, seq="A" * 40, qual=bytes([254] * 20 + [9] * 20)), rec("first_ff_long", 0, seq="C" * 33, qual=bytes([0xff] + [5] * 32))])
    add("tags", [rec("every", 0, seq="ACGT", qual=9, aux=b"".join(_every_tag())), rec("none", 0, seq="ACGT", qual=9), rec("ends", 0, aux=tag("ZZ", "Z", b"the last byte is the NUL")),
                 rec("ends_b", 0, aux=tag("BB", "B", [1, 2, 3], "S"))] + [rec("t%d" % i, 0, aux=t) for i, t in enumerate(_every_tag())])
    add("tag_unknown", [rec("ok", 0, aux=tag("OK", "i", 1)), rec("bad", 0, aux=b"XXq\1\0\0\0")], refused=(1, "tag_type"))
    add("tag_b_subtype", [rec("bad", 0, aux=b"XXBd\0\0\0\0")], refused=(0, "tag_type"))
    add("tag_z_no_nul", [rec("ok", 0), rec("ok", 0), rec("bad", 0, aux=tag("OK", "C", 1) + b"XXZabc")], refused=(2, "tag_z"))
    add("tag_b_past_end", [rec("bad", 0, aux=b"XXBs" + struct.pack("<I", 3) + b"\1\0\2\0\3")], refused=(0, "tag_b"))
    add("tag_stray_byte", [rec("ok", 0, aux=tag("OK", "C", 1)), rec("bad", 0, aux=tag("OK", "C", 1) + b"\7")], refused=(1, "tag_end"))
    add("tag_value_past_end", [rec("bad", 0, aux=b"XXi\1\0")], refused=(0, "tag_end"))
    add("floats_device", [rec("f%d" % i, 0, seq="AC", qual=4, aux=tag("fl", "f", v) + tag("ng", "f", -v) + tag("ar", "B", [v, -v, v], "f")) for i, (v, _) in enumerate(DEVICE_FLOATS)] +
        [rec("dbl", 0, aux=tag("d0", "d", 0.5) + tag("d1", "d", 1000015.0) + tag("d2", "d", -0.0))])
    filler = [rec("fill%d" % i, 0, 0, i, seq=_seq(rng, 40), qual=_quals(rng, 40), aux=tag("ok", "f", 0.25)) for i in range(60)]
    hard = [rec("h%d" % i, 0, 0, 100 + i, seq="ACGT", qual=4, aux=tag("fl", "f", v) + tag("ok", "f", 1.0)) for i, (v, _) in enumerate(HARD_FLOATS)]
    hard += [rec("dbl", 0, 0, 200, aux=tag("d0", "d", 0.1)), rec("arr", 0, 0, 201, aux=tag("ar", "B", [1.0, 1e-45, 2.0], "f")), rec("tiny", 0, 0, 202, aux=tag("fl", "f", 7.5e-6)),
             rec("huge", 0, 0, 203, aux=tag("fl", "f", float(2 ** 63)))]
    mixed = filler[:20] + hard[:2] + filler[20:45] + hard[2:5] + filler[45:] + hard[5:]
    add("floats_hard", mixed, hard=[i for i, r in enumerate(mixed) if r in hard])
    flt = [rec("r%d" % i, (0x1, 0x10, 0x401, 0x904, 0x63, 0)[i % 6], 0, i, (0, 10, 20, 60)[i % 4], seq=_seq(rng, 30), qual=_quals(rng, 30)) for i in range(48)]
    # each option drops the first record of a chunk, the last record of a chunk and every record of a chunk (one BGZF block a chunk:
    # chunk_members): records of one size, eight or so a block; 8 kept, 24 dropped in a row, 8 kept, then every third one dropped, so that
    # the dropped ones meet the chunks' ends at every phase.  tests/test_view_cases.py asserts the shape.
    for k, v, kept_rec, dropped_rec in (("f", 0x1, dict(flag=0x1, mapq=30), dict(flag=0x10, mapq=30)), ("F", 0x10, dict(flag=0x1, mapq=30), dict(flag=0x11, mapq=30)),
                                        ("G", 0x401, dict(flag=0x1, mapq=30), dict(flag=0x401, mapq=30)), ("q", 20, dict(flag=0x1, mapq=30), dict(flag=0x1, mapq=19))):
        shape = [False] * 8 + [True] * 24 + [False] * 8 + [i % 3 == 0 for i in range(60)]
        add("filter_%s" % k, [rec("r%03d" % i, tid=0, pos=i, seq=_seq(rng, 30), qual=_quals(rng, 30), **(dropped_rec if d else kept_rec)) for i, d in enumerate(shape)], **{k: v})
    add("filter_all_together", flt, f=0x1, F=0x800, G=0x60, q=10)
    add("filter_drops_everything", flt, f=0x8000)
    add("filter_first_and_last", [rec("first", 0x100, seq="A" * 200, qual=7)] + flt[6:18] + [rec("last", 0x100, seq="A" * 200, qual=7)], F=0x100, block=700)
    add("no_record", [])
    add("random_3000", _random(3000, 3000), block=0xFF00)
    return out


# records of the regions cases: coordinate-sorted, on t0 and chrTwo; nothing on empty3
def region_records():
    r = []
    r.append(rec("ends_at_beg", 0, 0, 900, 30, [(100, 0)], seq="A" * 100, qual=5))         # [900, 1000): out of [1000, 2000)
    r.append(rec("reaches_beg_1", 0, 0, 901, 30, [(100, 0)], seq="A" * 100, qual=5))       # [901, 1001): in
    r.append(rec("deletion_reaches", 0, 0, 950, 30, [(10, 0), (45, 2), (10, 4)], seq="A" * 20, qual=5))      # [950, 1005): in
    r.append(rec("no_ref_len", 0, 0, 999, 30, [(4, 4)], seq="ACGT", qual=5))               # [999, 1000): out
    r.append(rec("no_ref_len_in", 0, 0, 1000, 30, [], seq="ACGT", qual=5))                 # [1000, 1001): in
    r.append(rec("flag4_with_pos", 4, 0, 1500, 0, [(50, 0)], seq="A" * 50, qual=5))        # [1500, 1501): in; its CIGAR does not count
    r.append(rec("flag4_before", 4, 0, 990, 0, [(50, 0)], seq="A" * 50, qual=5))
    r.append(rec("last_in", 0, 0, 1999, 30, [(10, 0)], seq="A" * 10, qual=5))              # pos == end - 1: in
    r.append(rec("first_out", 0, 0, 2000, 30, [(10, 0)], seq="A" * 10, qual=5))            # pos == end: out
    r.append(rec("both", 0, 0, 1800, 30, [(300, 0)], seq="A" * 30, qual=5, aux=tag("fl", "f", 0.5)))        # overlaps [1000, 2000) and [1900, 2500)
    r.append(rec("other_contig", 0, 1, 1500, 30, [(10, 0)], seq="A" * 10, qual=5))
    r.append(rec("unplaced", 4, -1, -1, 0, [], seq="AC", qual=5))
    order = sorted(range(len(r)), key=lambda i: ((struct.unpack_from("<i", r[i], 4)[0] & 0xffffffff), struct.unpack_from("<i", r[i], 8)[0]))
    return [r[i] for i in order]


REGIONS = [["t0:1001-2000"], ["t0:1001-2000", "t0:1901-2500"], ["empty3"], ["chrTwo"], ["t0:1-900"], ["t0:2001-2001", "chrTwo:1501-1501", "t0"]]


def raw_bam(recs):
    """the inflated bytes of the BAM of the records"""
    text = HEADER_TEXT.encode()
    refs = struct.pack("<i", len(TG)) + b"".join(struct.pack("<i", len(n) + 1) + n.encode() + b"\0" + struct.pack("<i", l) for n, l in TG)
    return b"BAM\1" + struct.pack("<i", len(text)) + text + refs + b"".join(recs)


def write_case(path, recs, block=600):
    open(path, "wb").write(bamio.bgzf_bytes(raw_bam(recs), block=block))


def case_dir(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("view_cases"))
    paths = {}
    for name, c in cases().items():
        paths[name] = os.path.join(d, name + ".bam")
        write_case(paths[name], c["recs"], c["block"])
    return paths


def regions_bam(d, cli):
    """the regions' records as a BAM with its .csi (chrTwo is longer than a .bai addresses; the host path of `strling sort --write-index --csi` over the sorted records)"""
    src, dst = os.path.join(d, "regions_in.bam"), os.path.join(d, "regions.bam")
    write_case(src, region_records(), 400)
    subprocess.run([cli, "sort", "--write-index", "--csi", "-o", dst, src], check=True, capture_output=True, env=dict(os.environ, STRL_SORT="host"))
    return dst


def chunk_members(recs, block):
    """with one BGZF block a chunk: the ordinals of every chunk's complete records (a record belongs to the chunk its last byte lies in)"""
    at = len(raw_bam([]))
    out = {}
    for i, r in enumerate(recs):
        at += len(r)
        out.setdefault((at - 1) // block, []).append(i)
    return [out[k] for k in sorted(out)]


def filter_shape(recs, block, opts):
    """-> (a chunk whose first record is dropped and another kept, one whose last record is dropped and another kept, one of two or more
    records all dropped), by the reference"""
    dropped = [ref_line(r, opts) is None for r in recs]
    ch = [[dropped[i] for i in m] for m in chunk_members(recs, block)]
    return (any(c[0] and not all(c) for c in ch), any(c[-1] and not all(c) for c in ch), any(len(c) >= 2 and all(c) for c in ch))


def chunks_with(recs, block, ordinals):
    """with one BGZF block a chunk: the number of chunks among whose complete records one of `ordinals` is (a record belongs to the
    chunk its last byte lies in)"""
    at = len(raw_bam([]))
    hit = set()
    for i, r in enumerate(recs):
        at += len(r)
        if i in ordinals:
            hit.add((at - 1) // block)
    return len(hit)


def cli_options(opts):
    return [x for k in "fFGq" if opts[k] for x in ("-" + k, str(opts[k]))]


def abi_options(opts, region=None):
    tid, beg, end = region if region else (-2, 0, 0)
    return dict(require=opts["f"], exclude=opts["F"], exclude_all=opts["G"], min_mapq=opts["q"], tid=tid, beg=beg, end=end)


def names_blob():
    blob = "".join(n for n, _ in TG).encode()
    off = [0]
    for n, _ in TG:
        off.append(off[-1] + len(n))
    return blob, off


# ---- the reference -----------------------------------------------------------------------------------------------------------------
class Refused(Exception):
    def __init__(self, key):
        Exception.__init__(self, REFUSALS[key])
        self.key = key


def _g(v):
    return "%g" % v


def _tags(t):
    out, p, n = [], 0, len(t)
    sizes = dict(c=1, C=1, s=2, S=2, i=4, I=4, f=4)
    fmt = dict(c="b", C="B", s="h", S="H", i="i", I="I", f="f")

    def number(typ, at):
        v = struct.unpack_from("<" + fmt[typ], t, at)[0]
        return _g(v) if typ == "f" else str(v)
    while p < n:
        if n - p < 3:
            raise Refused("tag_end")
        key, typ = t[p:p + 2].decode("latin-1"), chr(t[p + 2])
        p += 3
        if typ == "A":
            if n - p < 1:
                raise Refused("tag_end")
            out.append(key + ":A:" + chr(t[p]))
            p += 1
        elif typ == "d":
            if n - p < 8:
                raise Refused("tag_end")
            out.append(key + ":d:" + _g(struct.unpack_from("<d", t, p)[0]))
            p += 8
        elif typ in "ZH":
            e = t.find(b"\0", p)
            if e < 0:
                raise Refused("tag_z")
            out.append(key + ":" + typ + ":" + t[p:e].decode("latin-1"))
            p = e + 1
        elif typ == "B":
            if n - p < 5:
                raise Refused("tag_b")
            sub, count = chr(t[p]), struct.unpack_from("<I", t, p + 1)[0]
            if sub not in sizes:
                raise Refused("tag_type")
            p += 5
            if count * sizes[sub] > n - p:
                raise Refused("tag_b")
            out.append(key + ":B:" + sub + "".join("," + number(sub, p + k * sizes[sub]) for k in range(count)))
            p += count * sizes[sub]
        elif typ in sizes:
            if n - p < sizes[typ]:
                raise Refused("tag_end")
            out.append(key + (":f:" if typ == "f" else ":i:") + number(typ, p))
            p += sizes[typ]
        else:
            raise Refused("tag_type")
    return out


def ref_line(r, opts, region=None):
    """a record's bytes -> its line (bytes), None when it is not kept; Refused"""
    if len(r) < 36 or struct.unpack_from("<I", r, 0)[0] + 4 != len(r):
        raise Refused("size")
    tid, pos, l_name, mapq, _, n_cig, flag, l_seq, mtid, mpos, tlen = struct.unpack_from("<iiBBHHHiiii", r, 4)
    c0 = 36 + l_name
    s0 = c0 + 4 * n_cig
    q0 = s0 + (l_seq + 1) // 2
    if l_seq < 0 or q0 + l_seq > len(r):
        raise Refused("size")
    cigar = [(w >> 4, w & 15) for w in struct.unpack_from("<%dI" % n_cig, r, c0)]
    if (flag & opts["f"]) != opts["f"] or flag & opts["F"] or (opts["G"] and (flag & opts["G"]) == opts["G"]) or mapq < opts["q"]:
        return None
    if region:
        reflen = sum(l for l, op in cigar if op in (0, 2, 3, 7, 8))
        endpos = pos + (reflen if reflen and not flag & 4 else 1)
        if not (tid == region[0] and pos < region[2] and endpos > region[1]):
            return None
    if tid >= len(TG):
        raise Refused("rname")
    if mtid >= len(TG):
        raise Refused("rnext")
    if any(op > 8 for _, op in cigar):
        raise Refused("cigar")
    name = r[36:36 + l_name - 1] if l_name > 1 else b"*"
    packed = r[s0:q0]
    seq = "".join(CODES[packed[i // 2] >> 4 if i % 2 == 0 else packed[i // 2] & 15] for i in range(l_seq)) or "*"
    q = r[q0:q0 + l_seq]
    qual = "*" if not l_seq or q[0] == 0xff else "".join(chr(min(x, 93) + 33) for x in q)
    f = [str(flag), "*" if tid < 0 else TG[tid][0], str(pos + 1), str(mapq), "".join("%d%s" % (l, OPS[op]) for l, op in cigar) or "*",
         "*" if mtid < 0 else "=" if mtid == tid else TG[mtid][0], str(mpos + 1), str(tlen), seq, qual] + _tags(r[q0 + l_seq:])
    return name + b"\t" + "\t".join(f).encode("latin-1") + b"\n"


def reference(recs, opts, region=None):
    """-> (text, written, dropped), or (None, ordinal, key) for the first record refused"""
    out, written = [], 0
    for i, r in enumerate(recs):
        try:
            line = ref_line(r, opts, region)
        except Refused as e:
            return None, i, e.key
        if line is not None:
            out.append(line)
            written += 1
    return b"".join(out), written, len(recs) - written


def parse_region(s):
    """NAME, NAME:BEG, NAME:BEG-END (1-based, inclusive) -> (tid, beg, end), 0-based and half-open"""
    names = [n for n, _ in TG]
    if s in names:
        return names.index(s), 0, (1 << 31) - 1
    n, _, c = s.rpartition(":")
    b, _, e = c.replace(",", "").partition("-")
    return names.index(n), max(0, int(b) - 1), int(e) if e else (1 << 31) - 1


def regions_reference(recs, opts, regions):
    parts = [reference(recs, opts, parse_region(s)) for s in regions]
    return b"".join(p[0] for p in parts), sum(p[1] for p in parts)


assert all(_g(struct.unpack("<f", struct.pack("<f", v))[0]) == s for v, s in DEVICE_FLOATS + HARD_FLOATS if not math.isnan(v))
