"""Inputs for `strling sort` over SAM text (strling_amd/csrc/sam_core.h, samparse.hip, cli/sam_feed.cpp, cli/sort_cli.cpp) and the
reference its outputs are held against: a SAM-to-BAM encoder written here from the SAM specification with `struct` (sections 1.4,
1.5, 4.2, 4.2.4) -- never the code under test --, Python's stable sorted() over sort_bam_cases.ref_key, and the header rule of
sort_bam_cases.ref_header_text.  Also a BAM-to-SAM printer, for the round trip.

tests/test_sort_sam_cases.py runs the cases through the host path, tests/test_sort_sam_device.py through the device."""
import re
import struct

import numpy as np

import sort_bam_cases as S

SEQ_CODE = {c: i for i, c in enumerate("=ACMGRSVTWYHKDBN")}
CIGAR_OPS = "MIDNSHP=X"
LINES_PER_WORKGROUP = 16          # 256 lanes, 16 a line (the default; 8 and 4 with 32 and 64 lanes divide it)


# ---- the reference encoder -------------------------------------------------------------------------------------------------------------
def reg2bin(beg, end):
    """SAM specification 5.3"""
    end -= 1
    if beg >> 14 == end >> 14:
        return ((1 << 15) - 1) // 7 + (beg >> 14)
    if beg >> 17 == end >> 17:
        return ((1 << 12) - 1) // 7 + (beg >> 17)
    if beg >> 20 == end >> 20:
        return ((1 << 9) - 1) // 7 + (beg >> 20)
    if beg >> 23 == end >> 23:
        return ((1 << 6) - 1) // 7 + (beg >> 23)
    if beg >> 26 == end >> 26:
        return ((1 << 3) - 1) // 7 + (beg >> 26)
    return 0


def _int_tag(v):
    if v < 0:
        return (b"c" + struct.pack("<b", v)) if v >= -128 else (b"s" + struct.pack("<h", v)) if v >= -32768 else (b"i" + struct.pack("<i", v))
    return (b"C" + struct.pack("<B", v)) if v <= 255 else (b"S" + struct.pack("<H", v)) if v <= 65535 else (b"I" + struct.pack("<I", v))


def _f32(text):
    return struct.pack("<f", float(text))


def encode_tag(field):
    tag, ty, val = field[:2], field[3:4], field[5:]
    assert field[2:3] == b":" and field[4:5] == b":"
    if ty == b"A":
        return tag + b"A" + val
    if ty == b"i":
        return tag + _int_tag(int(val))
    if ty == b"f":
        return tag + b"f" + _f32(val.decode())
    if ty in (b"Z", b"H"):
        return tag + ty + val + b"\0"
    assert ty == b"B"
    sub = val[:1].decode()
    items = val[2:].split(b",") if len(val) > 1 else []
    if sub == "f":
        body = b"".join(_f32(x.decode()) for x in items)
    else:
        body = b"".join(struct.pack("<" + {"c": "b", "C": "B", "s": "h", "S": "H", "i": "i", "I": "I"}[sub], int(x)) for x in items)
    return tag + b"B" + sub.encode() + struct.pack("<i", len(items)) + body


def encode_line(line, names):
    """one alignment line (bytes, no newline) -> the BAM record with its block_size word; names: {SN: id}"""
    f = line.split(b"\t")
    qname, flag, rname, pos, mapq, cigar, rnext, pnext, tlen, seq, qual = f[:11]
    flag, pos, mapq, pnext, tlen = int(flag), int(pos) - 1, int(mapq), int(pnext) - 1, int(tlen)
    tid = -1 if rname == b"*" else names[rname]
    mtid = -1 if rnext == b"*" else tid if rnext == b"=" else names[rnext]
    ops = [] if cigar == b"*" else [(int(n), CIGAR_OPS.index(o.decode())) for n, o in re.findall(rb"(\d+)([MIDNSHP=X])", cigar)]
    reflen = sum(n for n, o in ops if o in (0, 2, 3, 7, 8))
    end = pos + (reflen if reflen and not flag & 4 else 1)
    bin_ = reg2bin(pos, min(end, 2**31 - 1)) & 0xffff
    l_seq = 0 if seq == b"*" else len(seq)
    codes = [SEQ_CODE.get(chr(c).upper(), 15) for c in (seq if l_seq else b"")] + [0]
    packed = bytes(codes[i] << 4 | codes[i + 1] for i in range(0, l_seq, 2))
    q = b"\xff" * l_seq if qual == b"*" else bytes(c - 33 for c in qual)
    assert len(q) == l_seq
    body = struct.pack("<iiBBHHHiiii", tid, pos, len(qname) + 1, mapq, bin_, len(ops), flag, l_seq, mtid, pnext, tlen) + qname + b"\0" + \
        b"".join(struct.pack("<I", n << 4 | o) for n, o in ops) + packed + q + b"".join(encode_tag(t) for t in f[11:])
    return struct.pack("<i", len(body)) + body


def split_text(text):
    """SAM text -> (header text, [alignment lines without \\n and \\r])"""
    at = 0
    while at < len(text) and text[at:at + 1] == b"@":
        nl = text.find(b"\n", at)
        at = len(text) if nl < 0 else nl + 1
    body = text[at:]
    lines = body.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    return text[:at], [l[:-1] if l.endswith(b"\r") else l for l in lines]


def header_refs(header):
    """[(SN, LN)] of the @SQ lines in order"""
    out = []
    for h in header.split(b"\n"):
        h = h.rstrip(b"\r")
        if h.startswith(b"@SQ\t"):
            d = dict(x.split(b":", 1) for x in h.split(b"\t")[1:] if b":" in x)
            out.append((d[b"SN"], int(d[b"LN"])))
    return out


def bam_header(header, out_text=None):
    refs = header_refs(header)
    text = header if out_text is None else out_text
    return b"BAM\1" + struct.pack("<i", len(text)) + text + struct.pack("<i", len(refs)) + \
        b"".join(struct.pack("<i", len(n) + 1) + n + b"\0" + struct.pack("<i", l) for n, l in refs)


def reference(text):
    """what `strling sort` must write for the SAM text, inflated -> (stream, records, records without a reference, in order?, the
    encoded records in input order)"""
    header, lines = split_text(text)
    refs = header_refs(header)
    names = {n: i for i, (n, _) in enumerate(refs)}
    recs = [encode_line(l, names) for l in lines]
    keys = [S.ref_key(r, len(refs)) for r in recs]
    perm = sorted(range(len(recs)), key=lambda i: keys[i])
    stream = bam_header(header, S.ref_header_text(header.decode()).encode()) + b"".join(recs[i] for i in perm)
    no_ref = sum(1 for r in recs if struct.unpack_from("<i", r, 4)[0] < 0)
    return stream, len(recs), no_ref, perm == list(range(len(recs))), recs


# ---- BAM -> SAM ------------------------------------------------------------------------------------------------------------------------
def _print_tags(aux):
    out, at = [], 0
    size = {"c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}
    fmt = {"c": "b", "C": "B", "s": "h", "S": "H", "i": "i", "I": "I", "f": "f"}

    def num(t, v):
        return repr(float(v)) if t == "f" else str(v)
    while at < len(aux):
        tag, t = aux[at:at + 2].decode(), chr(aux[at + 2])
        at += 3
        if t == "A":
            out.append(f"{tag}:A:{chr(aux[at])}"); at += 1
        elif t in size:
            v = struct.unpack_from("<" + fmt[t], aux, at)[0]
            out.append(f"{tag}:{'f' if t == 'f' else 'i'}:{num(t, v)}"); at += size[t]
        elif t in "ZH":
            e = aux.index(b"\0", at)
            out.append(f"{tag}:{t}:{aux[at:e].decode()}"); at = e + 1
        else:
            assert t == "B"
            st = chr(aux[at]); n = struct.unpack_from("<i", aux, at + 1)[0]
            vals = struct.unpack_from(f"<{n}{fmt[st]}", aux, at + 5)
            out.append(f"{tag}:B:{st}" + "".join("," + num(st, v) for v in vals)); at += 5 + n * size[st]
    return out


def bam_to_sam(raw):
    """the inflated bytes of a BAM -> SAM text (the header's text, one line a record)"""
    text, refs, n_ref, recs = S.split_stream(raw)
    names, at = [], 4
    for _ in range(n_ref):
        l = struct.unpack_from("<i", refs, at)[0]
        names.append(refs[at + 4:at + 4 + l - 1].decode()); at += 8 + l
    out = [text]
    for r in recs:
        tid, pos, l_name, mapq, _, n_cig, flag, l_seq, mtid, mpos, tlen = struct.unpack_from("<iiBBHHHiiii", r, 4)
        at = 36
        qname = r[at:at + l_name - 1].decode(); at += l_name
        cig = "".join(f"{v >> 4}{CIGAR_OPS[v & 15]}" for v in struct.unpack_from(f"<{n_cig}I", r, at)) or "*"; at += 4 * n_cig
        sq = r[at:at + (l_seq + 1) // 2]; at += (l_seq + 1) // 2
        seq = "".join("=ACMGRSVTWYHKDBN"[(sq[i >> 1] >> (0 if i & 1 else 4)) & 15] for i in range(l_seq)) or "*"
        q = r[at:at + l_seq]; at += l_seq
        qual = "*" if not l_seq or q == b"\xff" * l_seq else "".join(chr(c + 33) for c in q)
        rname = "*" if tid < 0 else names[tid]
        rnext = "*" if mtid < 0 else "=" if mtid == tid else names[mtid]
        out.append("\t".join([qname, str(flag), rname, str(pos + 1), str(mapq), cig, rnext, str(mpos + 1), str(tlen), seq, qual] + _print_tags(r[at:])) + "\n")
    return "".join(out).encode()


# ---- the cases -------------------------------------------------------------------------------------------------------------------------
def sq(refs):
    return "".join(f"@SQ\tSN:{n}\tLN:{l}\n" for n, l in refs)


REFS3 = [("t0", 1 << 20), ("t1", 1 << 20), ("t2", 1 << 20)]
HD3 = "@HD\tVN:1.6\tSO:unsorted\n" + sq(REFS3)


def mk(qname="r", flag=0, rname="t0", pos=1, mapq=30, cigar="*", rnext="*", pnext=0, tlen=0, seq="*", qual="*", tags=()):
    return "\t".join([qname, str(flag), rname, str(pos), str(mapq), cigar, rnext, str(pnext), str(tlen), seq, qual] + list(tags))


def _rand_seq(rng, n):
    return "".join("ACGT"[c] for c in rng.integers(0, 4, n))


def _rand_qual(rng, n):
    return "".join(chr(c) for c in rng.integers(33, 74, n))


def fnv(name):
    h = 2166136261
    for c in name.encode():
        h = ((h ^ c) * 16777619) & 0xffffffff
    return h


def colliding_names(n=3, mask=7):
    """n names whose hash falls on the same first slot of a table of mask + 1 slots (made by search)"""
    got, k = [], 0
    while len(got) < n:
        name = f"c{k}"
        if fnv(name) & mask == 5:
            got.append(name)
        k += 1
    return got


I_TAGS = [-2**31, -32769, -32768, -129, -128, -1, 0, 255, 256, 65535, 65536, 2**31 - 1, 2**31, 2**32 - 1]
B_ENDS = {"c": (-128, 127), "C": (0, 255), "s": (-32768, 32767), "S": (0, 65535), "i": (-2**31, 2**31 - 1), "I": (0, 2**32 - 1)}
F_EDGES = ["123456789012345", "1234567890123456", "1e22", "1e23", "123456789012345e22", "1e-22", "1e-23", ".5", "5.", "-0", "1e-3", "0.000001", "3.14", "-2.5E+3", "+7",
           "0.1", "16777217", "1.17549435e-38", "inf", "nan", "-inf", "0e400", "00000000000000000001.5"]
F_HOST = ["1234567890123456", "1e23", "1e-23", "1.17549435e-38", "inf", "nan", "-inf"]      # spellings of F_EDGES the kernel leaves to the host


def cases():
    """-> [(name, SAM text as bytes)]"""
    out = []
    rng = np.random.default_rng(7)
    # whole cases
    lines = []
    for i in range(3000):
        l = int(rng.integers(20, 160))
        flag = int(rng.choice([0, 16, 4, 99, 147]))
        tags = []
        k = i % 6
        if k >= 1: tags.append(f"NM:i:{int(rng.integers(-40000, 70000))}")
        if k >= 2: tags.append(f"de:f:{rng.random() / 10:.4f}")
        if k >= 3: tags.append("MD:Z:" + _rand_seq(rng, int(rng.integers(0, 12))))
        if k >= 4: tags.append("XB:B:s," + ",".join(str(int(x)) for x in rng.integers(-300, 300, int(rng.integers(1, 9)))))
        if k >= 5: tags.append("XA:A:" + "QZ!~"[i % 4])
        unplaced = i % 11 == 0
        lines.append(mk(f"r{i:06d}", flag | (4 if unplaced else 0), "*" if unplaced else f"t{int(rng.integers(0, 3))}", 0 if unplaced else int(rng.integers(1, 100000)), int(rng.integers(0, 61)),
                        "*" if flag & 4 or unplaced else f"{l}M", "*" if unplaced else "=", 0 if unplaced else int(rng.integers(1, 100000)), int(rng.integers(-500, 500)),
                        _rand_seq(rng, l), _rand_qual(rng, l), tags))
    out.append(("shuffle_3000", HD3 + "\n".join(lines) + "\n"))
    out.append(("one_line", HD3 + mk("only", 16, "t1", 5, cigar="4M", seq="ACGT", qual="IIII") + "\n"))
    out.append(("header_only", HD3))
    out.append(("no_header_star_refs", "".join(mk(f"u{i}", 4, "*", 0, 0, seq=_rand_seq(rng, 30 + i), qual=_rand_qual(rng, 30 + i)) + "\n" for i in range(40))))
    # lengths
    lines = []
    for i in range(300):                       # every length from 60 to 359 bytes: SEQ and QUAL grow, QNAME takes up the rest
        l = 8 + i // 3
        bare = mk("", 0, "t0", 1 + (i * 37) % 5000, cigar=f"{l}M", seq=_rand_seq(rng, l), qual=_rand_qual(rng, l))
        lines.append("q" * (60 + i - len(bare)) + bare)
    out.append(("line_lengths_every_residue", HD3 + "\n".join(lines) + "\n"))
    out.append(("tab_on_16_byte_boundary", sq(REFS3[:1]) + mk("n" * 16, 0, "t0", 7, cigar="32M", seq=_rand_seq(rng, 32), qual=_rand_qual(rng, 32)) + "\n" +
                mk("m" * 15, 0, "t0", 3, cigar="1M", seq="A", qual="#") + "\n"))
    out.append(("l_seq_small", HD3 + "".join(mk(f"s{l}", 0, "t2", 100 - l, cigar=f"{l}M" if l else "*", seq=_rand_seq(rng, l) or "*", qual=_rand_qual(rng, l) or "*") + "\n" for l in (0, 1, 2, 31, 32, 33))))
    out.append(("seq_at_every_alignment", HD3 + "".join(mk("a" * nl, 0, "t1", 50 + nl, cigar=f"{l}M", seq=_rand_seq(rng, l), qual=_rand_qual(rng, l), tags=["X0:i:1"] * (l & 1)) + "\n"
                                                         for nl in range(1, 18) for l in (37, 38, 70, 71))))
    # sequence and quality
    out.append(("seq_alphabet", HD3 + mk("iupac", 0, "t0", 9, cigar="35M", seq="=ACMGRSVTWYHKDBNacmgrsvtwyhkdbnXx.-", qual="!" * 17 + "~" * 18) + "\n" +
                mk("noqual", 0, "t0", 8, cigar="5M", seq="ACGTN", qual="*") + "\n" + mk("noqual_odd_long", 16, "t0", 8, cigar="77M", seq="ACGTNAC" * 11, qual="*") + "\n"))
    # mandatory integers
    big = [("t0", 2**31 - 1)]
    out.append(("integer_ends", "@HD\tVN:1.6\n" + sq(big) + "".join(l + "\n" for l in (
        mk("flag0", 0, "t0", 0), mk("flag65535", 65535, "t0", 1), mk("posmax", 0, "t0", 2147483647, cigar="1M", seq="A", qual="I"), mk("pos1", 16, "t0", 1, pnext=2147483647),
        mk("tlenmin", 0, "t0", 4, tlen=-2**31), mk("tlenmax", 0, "t0", 4, tlen=2**31 - 1), mk("mapq255", 0, "t0", 3, mapq=255), mk("plus", 0, "t0", 2, tlen="+12")))))
    # CIGAR
    out.append(("cigars", HD3 + "".join(l + "\n" for l in (
        mk("each", 0, "t0", 10, cigar="1M1I1D1N1S1H1P1=1X", seq="ACGTA", qual="IIIII"), mk("ops65535", 0, "t1", 10, cigar="1M" * 65535), mk("reflen0", 0, "t0", 20000, cigar="5S3I", seq="A" * 8, qual="I" * 8),
        mk("unmapped_with_cigar", 4, "t0", 16385, cigar="40000M"), mk("mapped_long", 0, "t0", 16385, cigar="40000M"), mk("len_max", 0, "t2", 1, cigar="268435455N")))))
    # lines
    for n in (4 * LINES_PER_WORKGROUP, 4 * LINES_PER_WORKGROUP - 1, 4 * LINES_PER_WORKGROUP + 1):
        out.append((f"lines_{n}", HD3 + "".join(mk(f"w{i}", 16 * (i & 1), f"t{i % 3}", 1000 - i, cigar="10M", seq=_rand_seq(rng, 10), qual=_rand_qual(rng, 10)) + "\n" for i in range(n))))
    crlf = (HD3 + "".join(mk(f"c{i}", 0, "t0", 50 - i, cigar="4M", seq="ACGT", qual="IIII", tags=["XZ:Z:end"] * (i & 1)) + "\n" for i in range(9))).replace("\n", "\r\n")
    out.append(("crlf", crlf))
    out.append(("last_line_without_newline", HD3 + mk("a", 0, "t0", 9) + "\n" + mk("b", 0, "t0", 8, tags=["XZ:Z:tail"])))
    out.append(("line_400kb", HD3 + "".join(mk(f"k{i}", 0, "t1", 700 - i, cigar="20M", seq=_rand_seq(rng, 20), qual=_rand_qual(rng, 20)) + "\n" for i in range(5)) +
                mk("long", 0, "t1", 500, cigar="200000M", seq="ACGTN" * 40000, qual="5I!~#" * 40000, tags=["NM:i:3"]) + "\n" + mk("after", 0, "t0", 1) + "\n"))
    # tags
    out.append(("i_tags", HD3 + "".join(mk(f"i{k}", 0, "t0", 1 + k, tags=[f"XI:i:{v}", "XJ:i:+5"]) + "\n" for k, v in enumerate(I_TAGS))))
    lines = []
    for t, (lo, hi) in B_ENDS.items():
        for vals in ([], [lo], [hi], [lo, hi] * 500):
            lines.append(mk(f"b{t}{len(vals)}", 0, "t0", 1 + len(lines), tags=[f"XB:B:{t}" + "".join(f",{v}" for v in vals), "XT:i:1"]))
    for vals in ([], ["1.5"], ["0.25", "-1e3"] * 500, ["inf", "1e-3"]):
        lines.append(mk(f"bf{len(vals)}", 0, "t0", 1 + len(lines), tags=["XB:B:f" + "".join(f",{v}" for v in vals)]))
    out.append(("b_arrays", HD3 + "\n".join(lines) + "\n"))
    out.append(("other_tags", HD3 + "".join(l + "\n" for l in (mk("a", 0, "t0", 3, tags=["XA:A:!", "XC:A:~"]), mk("z", 0, "t0", 2, tags=["XZ:Z:", "XY:Z:a b:c"]),
                                                                  mk("h", 0, "t0", 1, tags=["XH:H:", "XG:H:1aF0"])))))
    out.append(("f_edges", HD3 + "".join(mk(f"f{k}", 0, "t1", 1 + k, tags=[f"XF:f:{v}", "NM:i:0"]) + "\n" for k, v in enumerate(F_EDGES))))
    out.append(("f_all_host", HD3 + "".join(mk(f"h{i}", 0, f"t{i % 3}", 900 - i, cigar="8M", seq=_rand_seq(rng, 8), qual=_rand_qual(rng, 8),
                                                  tags=[f"xa:f:1234567890123456{i:03d}", "NM:i:1", f"xb:f:{i}e30"]) + "\n" for i in range(200))))
    # headers
    out.append(("sq_extra_fields", "@HD\tVN:1.5\tSO:queryname\tGO:query\n@SQ\tAS:asm\tSN:chrA\tLN:5000\tM5:abcd\n@SQ\tSN:chrB\tUR:file:x\tLN:70\n@PG\tID:aligner\tSN:not_a_reference\n@CO\tfree text\n" +
                mk("x", 0, "chrB", 5, rnext="chrA", pnext=9) + "\n" + mk("y", 0, "chrA", 5, rnext="=", pnext=9) + "\n"))
    refs256 = [(f"ref{t}", 1000 + t) for t in range(256)]
    out.append(("refs_256", sq(refs256) + "".join(mk(f"r{i}", 0, f"ref{(i * 97) % 256}", 1 + i % 7, rnext=f"ref{(i * 31) % 256}", pnext=1) + "\n" for i in range(600))))
    pre = [("chr", 100), ("chr1", 100), ("chr10", 100), ("chr1_alt", 100)]
    out.append(("name_prefixes", sq(pre) + "".join(mk(f"p{i}", 0, pre[i % 4][0], 5, rnext=pre[(i + 1) % 4][0], pnext=1) + "\n" for i in range(16))))
    col = colliding_names()
    out.append(("hash_collisions", sq([(n, 500) for n in col]) + "".join(mk(f"h{i}", 0, col[i % 3], 9 - i % 3, rnext=col[(i + 2) % 3], pnext=1) + "\n" for i in range(12))))
    return [(n, t.encode()) for n, t in out]


def refusals():
    """-> [(name, SAM text, 1-based alignment line or None for the header, words the message holds)]"""
    ok = mk("fine", 0, "t0", 5, cigar="4M", seq="ACGT", qual="IIII")
    bad = [("ten_fields", "\t".join(ok.split("\t")[:10]), "line: fewer than the 11"), ("unknown_rname", mk(rname="chrZ"), "RNAME: not one of the header's @SQ names: chrZ"),
           ("unknown_rnext", mk(rnext="t9"), "RNEXT: not one of the header's @SQ names: t9"), ("flag_65536", mk(flag=65536), "FLAG:"), ("flag_hex", mk(flag="0x10"), "FLAG:"),
           ("pos_2p31", mk(pos=2147483648), "POS:"), ("mapq_256", mk(mapq=256), "MAPQ:"), ("cigar_bad_op", mk(cigar="4M3Q"), "CIGAR: not *"), ("cigar_len_2p28", mk(cigar="268435456M"), "CIGAR: an operation's length"),
           ("cigar_65536_ops", mk(cigar="1M" * 65536), "CIGAR: more than 65535"), ("qual_short", mk(seq="ACGT", qual="III"), "QUAL: not as long"), ("qual_long", mk(seq="ACGT", qual="IIIII"), "QUAL: not as long"),
           ("qual_byte_32", mk(seq="ACGT" * 10, qual="I" * 39 + " "), "QUAL: a byte below 33"), ("qual_without_seq", mk(seq="*", qual="II"), "QUAL: given although"),
           ("i_2p32", mk(tags=["XI:i:4294967296"]), "tag: an i value"), ("i_below_min", mk(tags=["XI:i:-2147483649"]), "tag: an i value"), ("b_c_128", mk(tags=["XB:B:c,1,128"]), "tag: a B array"),
           ("h_odd", mk(tags=["XH:H:abc"]), "tag: an H value"), ("tag_without_type", mk(tags=["XX:5"]), "tag: not TAG:TYPE:VALUE"), ("f_not_a_number", mk(tags=["XF:f:1.5x"]), "tag: an f value"),
           ("empty_line", "", "line: an empty line"), ("qname_255", mk(qname="q" * 255), "QNAME:")]
    out = []
    for k, (name, line, words) in enumerate(bad):
        n_before = 3 + k % 5
        text = HD3 + "".join(ok + "\n" for _ in range(n_before)) + line + "\n" + ok + "\n"
        out.append((name, text.encode(), n_before + 1, words))
    out.append(("duplicate_sn", (sq(REFS3) + "@SQ\tSN:t1\tLN:5\n" + ok + "\n").encode(), None, "SN t1 occurs twice"))
    return out
