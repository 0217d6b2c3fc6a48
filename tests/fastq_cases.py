"""Inputs for `strling fastq` (strling_amd/csrc/fastq_core.h, fastq.hip, cli/sort_cli.cpp) and the reference its outputs are held
against: the rule of the issue written out again in Python, with dictionaries keyed by name -- never the code under test.  No
machine of the project has samtools, so agreement with `samtools fastq` is unverified.

Every case is a BAM whose records are packed here byte by byte (so that every 4-bit code, every quality byte, names of 1 and 254
bytes and l_seq 0 can be had), at most a few thousand short records, and the options it runs under.  tests/test_fastq_cases.py runs
the cases through the host path and the stand-alone program, tests/test_fastq_device.py through the device."""
import gzip
import os
import re
import struct

import numpy as np

import sort_bam_cases as S
from strling_amd import bamio

TG = [("t0", 1 << 20), ("t1", 1 << 20)]
HEADER_TEXT = "@HD\tVN:1.6\tSO:unsorted\n" + "".join(f"@SQ\tSN:{n}\tLN:{l}\n" for n, l in TG)
CODES = "=ACMGRSVTWYHKDBN"
COUNT_KEYS = ("kept", "filtered", "empty", "pairs", "singles", "singles_unwritten")
LENGTHS = (1, 2, 15, 16, 17, 31, 32, 33, 255, 256, 257)
DEFAULTS = dict(F=0x900, N=False, v=1, split=False, singles=True)


def rec(name, flag, seq, qual=None, tid=-1, pos=-1, aux=b""):
    """one record.  seq: a string over CODES; qual: None (absent: 0xFF bytes), one value for every base, or the bytes themselves.
    A mapped record (tid >= 0) gets the CIGAR <l_seq>M."""
    name = name.encode() if isinstance(name, str) else bytes(name)
    l_seq = len(seq)
    q = b"\xff" * l_seq if qual is None else bytes([qual]) * l_seq if isinstance(qual, int) else bytes(qual)
    assert len(q) == l_seq and 1 <= len(name) <= 254
    return dict(name=name, flag=flag, seq=seq, qual=q, tid=tid, pos=pos, aux=bytes(aux))


def pack(r):
    """the record's bytes, its block_size word included"""
    l_seq = len(r["seq"])
    cigar = struct.pack("<I", l_seq << 4) if r["tid"] >= 0 and l_seq else b""
    codes = [CODES.index(c) for c in r["seq"]] + [0]
    seq = bytes(codes[i] << 4 | codes[i + 1] for i in range(0, l_seq, 2))
    body = struct.pack("<iiBBHHHiiii", r["tid"], r["pos"], len(r["name"]) + 1, 30, 4680, len(cigar) // 4, r["flag"], l_seq, -1, -1, 0) + r["name"] + b"\0" + cigar + seq + r["qual"] + r["aux"]
    return struct.pack("<I", len(body)) + body


def _seq(rng, n, codes=16):
    return "".join(CODES[int(x)] for x in rng.integers(0, codes, n))


def _quals(rng, n):
    q = bytes(rng.integers(0, 94, n, dtype=np.uint8))
    return b"\x0a" if q == b"\x09" else q                    # (one base of quality 9 is `*` in SAM text, which says absent)


def pair(rng, name, l1, l2=None, rev1=False, rev2=True, extra=0, **kw):
    l2 = l1 if l2 is None else l2
    return [rec(name, 0x1 | 0x40 | (0x10 if rev1 else 0) | extra, _seq(rng, l1), _quals(rng, l1), **kw),
            rec(name, 0x1 | 0x80 | (0x10 if rev2 else 0) | extra, _seq(rng, l2), _quals(rng, l2), **kw)]


def _random_case(n_pairs, n_singles, seed, max_len=30):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n_pairs):
        p = pair(rng, f"p{seed}_{i:05d}", int(rng.integers(1, max_len + 1)), int(rng.integers(1, max_len + 1)), bool(rng.integers(0, 2)), bool(rng.integers(0, 2)),
                 tid=int(rng.integers(-1, 2)), pos=int(rng.integers(0, 5000)))
        out += p if rng.integers(0, 2) else p[::-1]
    for i in range(n_singles):
        l = int(rng.integers(1, max_len + 1))
        out.append(rec(f"s{seed}_{i:05d}", (0, 0x10, 0x40, 0x80 | 0x10, 0xc0)[i % 5], _seq(rng, l), None if i % 7 == 0 else _quals(rng, l), aux=b"NMC\x01" if i % 3 else b""))
    return [out[i] for i in rng.permutation(len(out))]


def one_name(n):
    """n kept records under one name (513: beyond what the device's join resolves)"""
    return [rec("same", 0x1 | (0x40 if i % 2 else 0x80) | (0x10 if i % 3 == 0 else 0), "ACGTN"[: 1 + i % 5], 20 + i % 7) for i in range(n)]


def cases():
    """-> [(name, [records in input order], options, expressible as SAM text)]"""
    rng = np.random.default_rng(11)
    out = []

    def add(name, recs, sam=True, **opts):
        out.append((name, recs, dict(DEFAULTS, **opts), sam))

    # lengths around the 16-byte words and the nibble pairs, forward and reverse; the odd-length reverse reads are the ones that matter
    lengths = []
    for l in LENGTHS:
        lengths += pair(rng, f"len{l}", l, l, False, True) + pair(rng, f"rf{l}", l, l, True, False, tid=0, pos=100 + l)
        lengths += [rec(f"fwd{l}", 0, _seq(rng, l), _quals(rng, l)), rec(f"rev{l}", 0x10, _seq(rng, l), _quals(rng, l), aux=b"NMC\x01")]
    add("lengths", lengths)
    add("lengths_split", lengths, split=True)
    add("lengths_suffix", lengths, N=True)
    add("l_seq_0", [rec("empty", 0, ""), rec("a", 0x41, "ACGT", 30), rec("a", 0x81, ""), rec("b", 0x41, "AC", 30), rec("b", 0x91, "GT", 31), rec("empty_rev", 0x10, "")])
    every = CODES + "A"
    add("all_codes", [rec("c16", 0x41, CODES, 40), rec("c16", 0x91, CODES, 41), rec("c17", 0, every, 40), rec("c17r", 0x10, every, bytes(range(17))), rec("c16r", 0x10, CODES, 30),
                      rec("c15r", 0x10, CODES[1:], 30)])
    add("quals", [rec("absent", 0, "ACGTA"), rec("absent_rev", 0x10, "ACGTA"), rec("q0", 0, "ACG", 0), rec("q93", 0x10, "ACG", 93), rec("p", 0x41, "ACGT"), rec("p", 0x91, "ACGTT", bytes([0, 1, 2, 92, 93]))])
    # what SAM text cannot say: qualities past 93, and 0xFF behind a valid first byte (a value like any other: clamped)
    add("quals_beyond_sam", [rec("q94", 0, "ACG", 94), rec("q254", 0x10, "ACGT", 254), rec("later_ff", 0, "ACGTA", bytes([10, 0xff, 20, 0xff, 0xff])),
                             rec("later_ff_rev", 0x10, "ACGTA", bytes([10, 0xff, 20, 0xff, 0xfe])), rec("p", 0x41, "AC", bytes([93, 94])), rec("p", 0x91, "ACG", bytes([254, 0, 0xff]))], sam=False)
    add("absent_default_40", [rec("absent", 0, "ACGTA"), rec("p", 0x41, "ACGT"), rec("p", 0x91, "ACGTT", 7), rec("absent_rev", 0x10, "AC")], v=40)
    add("absent_default_200", [rec("absent", 0, "ACGTA")], v=200, sam=True)
    long_name = "n" * 100 + "/" + "m" * 153
    add("names", [rec("x", 0x41, "ACGT", 30), rec(long_name, 0x81, "AC", 30), rec("x", 0x81, "TTGA", 31), rec(long_name, 0x41, "ACG", 30), rec("a/1", 0x41, "A", 5), rec("a/2", 0x81, "C", 5),
                  rec("a/1", 0x81, "G", 5), rec("/", 0, "T", 5), rec("y", 0, "ACGTACGTACGTACGTACGT", 9)])
    add("names_suffix", out[-1][1], N=True)
    flags = [rec("r0", 0, "ACGT", 30), rec("r1", 0x40, "ACGT", 30), rec("r2", 0x80, "ACGT", 30), rec("r3", 0xc0, "ACGT", 30),
             rec("lone_r1", 0x41, "ACGTA", 30), rec("two_r1", 0x41, "AC", 30), rec("two_r1", 0x41 | 0x10, "GT", 31),
             rec("sup", 0x41, "ACGTAC", 30), rec("sup", 0x81 | 0x800, "AC", 30), rec("sup", 0x91, "ACGTTT", 33),
             rec("sec", 0x41, "ACG", 30), rec("sec", 0x91, "ACC", 30), rec("sec", 0x81 | 0x100, "AAA", 30),
             rec("unpaired_bits", 0x40, "ACGTAC", 30), rec("unpaired_bits", 0x80 | 0x4 | 0x400 | 0x200, "GGG", 30),      # no other flag bit matters
             rec("r3_pair", 0xc1, "AC", 30), rec("r3_pair", 0x81, "AC", 30), rec("unmapped", 0x4 | 0x41, "ACGT", 30), rec("unmapped", 0x4 | 0x81, "ACGA", 30)]
    add("flags", flags)
    add("flags_suffix", flags, N=True)
    add("flags_filter_0", flags, F=0)                           # the secondary record is kept: three under `sec`, all singles
    add("flags_filter_0x904", flags, F=0x904)
    add("flags_no_singles", flags, singles=False)
    add("flags_split_no_singles", flags, split=True, singles=False)
    far = pair(rng, "far", 20, 30)
    order = [far[1]] + [rec(f"s{i}", 0, _seq(rng, 5 + i), _quals(rng, 5 + i)) for i in range(3)] + pair(rng, "near", 7, 9) + [rec("mid", 0x10, "ACGTN", 30)]
    order += [r for i in range(40) for r in pair(rng, f"fill{i}", 3 + i % 5)] + [far[0], rec("last", 0, "A", 1)]
    add("order", order)
    add("order_split", order, split=True)
    add("no_record", [])
    add("pairs_only", [r for i in range(50) for r in pair(rng, f"q{i}", 1 + i, 51 - i, i % 2 == 0, i % 3 == 0)])
    add("pairs_only_split", out[-1][1], split=True)
    add("singles_only", [rec(f"s{i}", (0, 0x10, 0x40, 0x90)[i % 4], _seq(rng, 1 + i % 37), _quals(rng, 1 + i % 37)) for i in range(90)])
    add("nothing_kept", [rec(f"u{i}", 0x100 if i % 2 else 0x800, "ACGT", 30) for i in range(20)] + [rec("e", 0, "")])
    rnd = _random_case(1200, 600, 3000)
    add("random_3000", rnd)
    add("random_3000_split_no_singles", rnd, split=True, singles=False)
    add("one_name_512", one_name(512))
    return out


def raw_bam(recs):
    """the inflated bytes of the BAM of the records"""
    text = HEADER_TEXT.encode()
    refs = struct.pack("<i", len(TG)) + b"".join(struct.pack("<i", len(n) + 1) + n.encode() + b"\0" + struct.pack("<i", l) for n, l in TG)
    return b"BAM\1" + struct.pack("<i", len(text)) + text + refs + b"".join(pack(r) for r in recs)


def write_case(path, recs):
    open(path, "wb").write(bamio.bgzf_bytes(raw_bam(recs)))


def sam_text(recs):
    """the records as SAM text (qualities up to 93, or absent as a whole)"""
    lines = [HEADER_TEXT]
    for r in recs:
        absent = not r["qual"] or r["qual"] == b"\xff" * len(r["qual"])
        assert absent or max(r["qual"]) <= 93
        mapped = r["tid"] >= 0
        aux = "\tNM:i:1" if r["aux"] else ""
        lines.append("\t".join([r["name"].decode(), str(r["flag"]), TG[r["tid"]][0] if mapped else "*", str(r["pos"] + 1), "30", f"{len(r['seq'])}M" if mapped and r["seq"] else "*", "*", "0", "0",
                                r["seq"] or "*", "*" if absent else "".join(chr(33 + q) for q in r["qual"])]) + aux + "\n")
    return "".join(lines)


def case_dir(tmp_path_factory):
    d = tmp_path_factory.mktemp("fastq_cases")
    paths = {}
    for name, recs, _, sam in cases():
        paths[name] = os.path.join(str(d), name + ".bam")
        write_case(paths[name], recs)
        if sam:
            open(os.path.join(str(d), name + ".sam"), "w").write(sam_text(recs))
    return paths


def oversized(src, dst, ordinal):
    """the BAM at src with record `ordinal`'s l_seq raised so that its bases and qualities no longer fit its block_size"""
    raw = bytearray(gzip.decompress(open(src, "rb").read()))
    _, _, _, recs = S.split_stream(bytes(raw))
    at = len(raw) - sum(len(r) for r in recs) + sum(len(r) for r in recs[:ordinal])
    struct.pack_into("<i", raw, at + 20, struct.unpack_from("<i", raw, at + 20)[0] + 40)
    open(dst, "wb").write(bamio.bgzf_bytes(bytes(raw)))


def cli_options(opts, out_dir, stdout=False):
    """the command line of a case's options -> (arguments, {stream: path})"""
    files = {}
    args = ["-F", hex(opts["F"])] if opts["F"] != 0x900 else []
    args += ["-N"] if opts["N"] else []
    args += ["-v", str(opts["v"])] if opts["v"] != 1 else []
    if opts["split"]:
        files["p1"], files["p2"] = os.path.join(out_dir, "r1.fq"), os.path.join(out_dir, "r2.fq")
        args += ["-1", files["p1"], "-2", files["p2"]]
    elif stdout:
        args += ["-o", "-"]
    else:
        files["p1"] = os.path.join(out_dir, "pairs.fq")
        args += ["-o", files["p1"]]
    if opts["singles"]:
        files["s"] = os.path.join(out_dir, "singles.fq")
        args += ["-s", files["s"]]
    return args, files


def abi_options(opts):
    return dict(filter=opts["F"], suffix=opts["N"], default_qual=opts["v"], interleaved=not opts["split"], singles=opts["singles"])


# ---- the reference -----------------------------------------------------------------------------------------------------------------
_COMPLEMENT = {c: CODES[int(f"{i:04b}"[::-1], 2)] for i, c in enumerate(CODES)}      # the four bits in reverse order


def _entry(r, opts):
    _, _, l_name, _, _, n_cig, flag, l_seq = struct.unpack_from("<iiBBHHHi", r, 4)
    name = bytes(r[36:36 + l_name - 1])
    s0 = 36 + l_name + 4 * n_cig
    packed = r[s0:s0 + (l_seq + 1) // 2]
    seq = "".join(CODES[packed[i // 2] >> 4 if i % 2 == 0 else packed[i // 2] & 15] for i in range(l_seq))
    q = r[s0 + (l_seq + 1) // 2:s0 + (l_seq + 1) // 2 + l_seq]
    qual = [min(opts["v"], 93) + 33] * l_seq if q[0] == 0xff else [min(x, 93) + 33 for x in q]
    if flag & 0x10:
        seq = "".join(_COMPLEMENT[c] for c in reversed(seq))
        qual = qual[::-1]
    rn = (flag >> 6) & 3
    suffix = b"/%d" % rn if opts["N"] and rn in (1, 2) else b""
    return b"@" + name + suffix + b"\n" + seq.encode() + b"\n+\n" + bytes(qual) + b"\n"


def ref_fastq(recs, opts):
    """records (bytes, each with its block_size word) in input order -> (dict(p1=, p2=, s=), counts by COUNT_KEYS)"""
    counts = dict.fromkeys(COUNT_KEYS, 0)
    by_name, kept = {}, []
    for i, r in enumerate(recs):
        _, _, l_name, _, _, _, flag, l_seq = struct.unpack_from("<iiBBHHHi", r, 4)
        if flag & opts["F"]:
            counts["filtered"] += 1
        elif l_seq == 0:
            counts["empty"] += 1
        else:
            counts["kept"] += 1
            kept.append(i)
            by_name.setdefault(bytes(r[36:36 + l_name - 1]), []).append((i, (flag >> 6) & 3))
    first_of, second_of = {}, {}                                # where a pair stands -> (its R1, its R2); the pair's other record
    for members in by_name.values():
        if len(members) == 2 and sorted(rn for _, rn in members) == [1, 2]:
            r1 = [i for i, rn in members if rn == 1][0]
            r2 = [i for i, rn in members if rn == 2][0]
            first_of[min(r1, r2)] = (r1, r2)
            second_of[max(r1, r2)] = True
    streams = dict(p1=[], p2=[], s=[])
    for i in kept:
        if i in first_of:
            r1, r2 = first_of[i]
            counts["pairs"] += 1
            streams["p1"].append(_entry(recs[r1], opts))
            streams["p1" if not opts["split"] else "p2"].append(_entry(recs[r2], opts))
        elif i not in second_of:
            counts["singles"] += 1
            if opts["singles"]:
                streams["s"].append(_entry(recs[i], opts))
            else:
                counts["singles_unwritten"] += 1
    return {k: b"".join(v) for k, v in streams.items()}, counts


def reference(recs, opts):
    """what `strling fastq` must write for the records (as rec() made them) and report"""
    return ref_fastq([pack(r) for r in recs], opts)


COUNT_LINE = re.compile(r"fastq: (\d+) records kept, (\d+) filtered, (\d+) empty, (\d+) pairs, (\d+) singles, (\d+) singles not written")


def counts_of(stderr):
    m = COUNT_LINE.search(stderr)
    assert m, stderr
    return dict(zip(COUNT_KEYS, (int(x) for x in m.groups())))
