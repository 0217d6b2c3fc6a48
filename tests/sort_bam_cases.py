"""Inputs for `strling sort` (strling_amd/csrc/bamsort_core.h, bamsort.hip, cli/sort_cli.cpp) and the reference its outputs are held
against -- Python's stable sorted() over the records parsed from the input's inflated bytes, with the key written out again here.

Every case is a BAM written by bamio.write_bam(index=False): a few thousand short records at most.  tests/test_sort_bam_cases.py
runs them through the host path, tests/test_sort_bam_device.py through the device."""
import gzip
import os
import struct
import zlib

import numpy as np

from strling_amd import bamio
from strling_amd.records import RecordBatch

EOF_BLOCK = bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0])
BLK = 0xFF00


def targets(n_ref, length=1 << 20):
    return [(f"t{t}", length) for t in range(n_ref)]


def batch(tid, pos, flag, tg, l_seq=None, seed=0):
    """records with distinct names (input ordinal), random short reads; an unmapped record has no CIGAR"""
    rng = np.random.default_rng(seed)
    n = len(tid)
    l_seq = [int(x) for x in (l_seq if l_seq is not None else rng.integers(20, 60, n))]
    seqs = ["".join("ACGT"[c] for c in rng.integers(0, 4, l)) if l < 1000 else "ACGT" * (l // 4) for l in l_seq]
    cig = ["*" if (int(f) & 4) else f"{len(s)}M" for f, s in zip(flag, seqs)]
    return RecordBatch.from_fields(tid, pos, [int(t) for t in tid], [max(int(p), 0) for p in pos], flag, [30] * n, cig, seqs,
                                   [f"r{i:06d}" for i in range(n)], isize=[0] * n, targets=tg)


def _shuffled(n, n_ref, seed, span=100_000):
    rng = np.random.default_rng(seed)
    tid = rng.integers(0, max(n_ref, 1), n) if n_ref else np.full(n, -1)
    pos = rng.integers(0, span, n)
    flag = np.where(rng.integers(0, 2, n) == 1, 16, 0)
    return tid, pos, flag


def cases():
    """-> [(name, RecordBatch, header text or None)]"""
    out = []
    tg3 = targets(3)
    tid, pos, flag = _shuffled(3000, 3, 1)
    out.append(("uniform_shuffle", batch(tid, pos, flag, tg3, seed=1), None))
    # sorted and reverse-sorted input
    order = np.lexsort((flag, pos, tid))
    out.append(("already_sorted", batch(tid[order], pos[order], flag[order], tg3, seed=2), None))
    out.append(("reverse_sorted", batch(tid[order][::-1], pos[order][::-1], flag[order][::-1], tg3, seed=3), None))
    # one tile of the radix sort, one less, one more
    for n in (2047, 2048, 2049):
        t, p, f = _shuffled(n, 3, 10 + n)
        out.append((f"n{n}", batch(t, p, f, tg3, l_seq=[20] * n, seed=n), None))
    # hundreds of records on one (tid, pos), both strands, among a few others: forward first, input order kept
    rng = np.random.default_rng(5)
    n = 700
    t = np.full(n, 1); p = np.full(n, 777); f = np.where(rng.integers(0, 2, n) == 1, 16, 0)
    t[::97] = 0; p[::89] = 776; p[::83] = 778
    out.append(("one_position_both_strands", batch(t, p, f, tg3, seed=5), None))
    # placed-unmapped mates (flag 4, the mate's tid / pos) and pos = -1 on a placed record
    t, p, f = _shuffled(600, 3, 6, span=500)
    f = np.where(np.arange(600) % 5 == 0, f | 4, f)
    p = np.where(np.arange(600) % 7 == 0, -1, p)
    out.append(("placed_unmapped_and_pos_minus1", batch(t, p, f, tg3, seed=6), None))
    # records without a reference scattered through the input: all last, in input order
    t, p, f = _shuffled(900, 3, 7)
    nr = np.arange(900) % 4 == 1
    t = np.where(nr, -1, t); p = np.where(nr, -1, p); f = np.where(nr, 4, f)            # (unmapped, no strand: one key)
    out.append(("no_reference_scattered", batch(t, p, f, tg3, seed=7), None))
    # the bit window of the sort follows n_ref
    for n_ref in (0, 1, 3, 4, 255, 256):
        t, p, f = _shuffled(500, n_ref, 20 + n_ref)
        if n_ref:
            t[:n_ref] = np.arange(n_ref)[::-1][:500]          # every reference occurs, the last one too
            t[-7:] = -1
        out.append((f"n_ref_{n_ref}", batch(t, p, f, targets(n_ref), seed=20 + n_ref), None))
    # the largest position a BAM holds
    t, p, f = _shuffled(300, 2, 8)
    p[::3] = 2**31 - 2
    p[1::50] = 2**31 - 3
    out.append(("pos_2p31_minus_2", batch(t, p, f, targets(2, 2**31 - 1), seed=8), None))
    out.append(("one_record", batch([1], [5], [16], tg3, seed=9), None))
    out.append(("no_record", batch([], [], [], tg3, seed=9), None))
    # a 300 KB record among short ones (l_seq 200 000: 100 KB of bases, 200 KB of qualities)
    t, p, f = _shuffled(400, 3, 11)
    ls = [int(x) for x in np.random.default_rng(11).integers(20, 60, 400)]
    ls[137] = 200_000
    out.append(("one_300kb_record", batch(t, p, f, tg3, l_seq=ls, seed=11), None))
    # headers
    t, p, f = _shuffled(200, 3, 12)
    sq = "".join(f"@SQ\tSN:{n}\tLN:{l}\n" for n, l in tg3)
    for name, text in (("hd_unsorted_go", "@HD\tVN:1.5\tSO:unsorted\tGO:query\n" + sq + "@PG\tID:x\tPN:y\n"),
                       ("hd_without_so", "@HD\tVN:1.6\n" + sq),
                       ("hd_ss_and_other_fields", "@HD\tVN:1.6\tSS:coordinate:queryname\tXY:kept\tSO:queryname\n" + sq),
                       ("no_hd", sq + "@RG\tID:a\tSM:b\n"),
                       ("co_lines", "@HD\tVN:1.6\tSO:unknown\n" + sq + "@CO\tSO:unsorted is only a comment here\n@CO\t@HD\tGO:query\n"),
                       ("empty_text", "")):
        out.append((f"header_{name}", batch(t, p, f, tg3, seed=12), text))
    return out


def write_case(path, rec, text):
    bamio.write_bam(path, rec, header_text=text, index=False)


# ---- the reference -----------------------------------------------------------------------------------------------------------------
def ref_header_text(text):
    """the rule of the output's text, written out again"""
    if text.startswith("@HD") and (len(text) == 3 or text[3] in "\t\n"):
        line, sep, rest = text.partition("\n")
        keep, so = [], False
        for f in line.split("\t")[1:]:
            if f.startswith("SO:"):
                if not so:
                    keep.append("SO:coordinate")
                so = True
            elif not f.startswith(("GO:", "SS:")):
                keep.append(f)
        if not so:
            keep.append("SO:coordinate")
        return "\t".join(["@HD"] + keep) + sep + rest
    return "@HD\tVN:1.6\tSO:coordinate\n" + text


def split_stream(raw):
    """inflated bytes of a BAM -> (header text, bytes of the reference list from n_ref on, n_ref, [record bytes with block_size])"""
    assert raw[:4] == b"BAM\1"
    l_text = struct.unpack_from("<i", raw, 4)[0]
    text = raw[8:8 + l_text].decode()
    at = 8 + l_text
    n_ref = struct.unpack_from("<i", raw, at)[0]
    r0 = at
    at += 4
    for _ in range(n_ref):
        at += 8 + struct.unpack_from("<i", raw, at)[0]
    refs = raw[r0:at]
    recs = []
    while at < len(raw):
        bs = struct.unpack_from("<i", raw, at)[0]
        assert bs >= 32 and at + 4 + bs <= len(raw)
        recs.append(raw[at:at + 4 + bs])
        at += 4 + bs
    return text, refs, n_ref, recs


def ref_key(rec, n_ref):
    tid, pos = struct.unpack_from("<ii", rec, 4)
    flag = struct.unpack_from("<H", rec, 4 + 14)[0]
    assert -1 <= tid < n_ref
    return ((n_ref if tid < 0 else tid) << 33) | (((pos + 1) & 0xffffffff) << 1) | ((flag >> 4) & 1)


def reference_stream(path):
    """what `strling sort` must write for the BAM at `path`, inflated -> (stream bytes, number of records, records without a
    reference, whether the input was in order, the permutation)"""
    text, refs, n_ref, recs = split_stream(gzip.decompress(open(path, "rb").read()))
    keys = [ref_key(r, n_ref) for r in recs]
    perm = sorted(range(len(recs)), key=lambda i: keys[i])                 # (stable)
    out_text = ref_header_text(text).encode()
    stream = b"BAM\1" + struct.pack("<i", len(out_text)) + out_text + refs + b"".join(recs[i] for i in perm)
    no_ref = sum(1 for r in recs if struct.unpack_from("<i", r, 4)[0] < 0)
    return stream, len(recs), no_ref, perm == list(range(len(recs))), perm


def members(data):
    """BGZF members of a file -> [(member bytes, inflated bytes)]; every member is checked on its own: header, BSIZE, at most
    64 KiB, a DEFLATE stream that ends where the trailer begins, CRC-32 and ISIZE"""
    out, o = [], 0
    while o < len(data):
        assert data[o:o + 4] == b"\x1f\x8b\x08\x04" and data[o + 10:o + 16] == b"\x06\x00BC\x02\x00", f"member header at {o}"
        bsize = struct.unpack_from("<H", data, o + 16)[0] + 1
        assert bsize <= 65536 and o + bsize <= len(data)
        m = data[o:o + bsize]
        d = zlib.decompressobj(-15)
        raw = d.decompress(m[18:-8])
        assert d.eof and not d.unused_data, "the DEFLATE stream ends where the trailer begins"
        crc, isize = struct.unpack_from("<II", m, bsize - 8)
        assert isize == len(raw) <= 65536 and crc == zlib.crc32(raw)
        out.append((m, raw))
        o += bsize
    return out


def check_file(path, stream):
    """the file at `path` is `stream` in members of 0xFF00 bytes and the EOF block"""
    data = open(path, "rb").read()
    ms = members(data)
    assert ms and ms[-1][0] == EOF_BLOCK, "the EOF block"
    body = ms[:-1]
    assert [len(r) for _, r in body] == [min(BLK, len(stream) - o) for o in range(0, len(stream), BLK)], "members of 0xFF00 input bytes"
    assert b"".join(r for _, r in body) == stream
    return data


def case_dir(tmp_path_factory):
    d = tmp_path_factory.mktemp("sort_bam_cases")
    paths = {}
    for name, rec, text in cases():
        paths[name] = os.path.join(str(d), name + ".bam")
        write_case(paths[name], rec, text)
    return paths
