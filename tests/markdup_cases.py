"""Inputs for `strling sort --markdup` (strling_amd/csrc/markdup_core.h, markdup.hip, cli/sort_cli.cpp) and the reference its outputs
are held against: the rule of the issue written out again in Python, with dictionaries keyed by name and signatures as tuples --
never the code under test.

Every case is a BAM written by bamio.write_bam(..., quals=, extra=): tens to a few thousand short records, in no order.
tests/test_markdup_cases.py runs them through the host path and the stand-alone program, tests/test_markdup_device.py through the
device."""
import gzip
import os
import re
import struct

import numpy as np

import sort_bam_cases as S
from strling_amd import bamio
from strling_amd.records import RecordBatch

TG = [("t0", 1 << 20), ("t1", 1 << 20), ("t2", 1 << 20)]
QUERY_OPS = "MIS=X"
COUNT_KEYS = ("pairs", "dup_pairs", "fragments", "dup_fragments", "ineligible")


def rec(name, flag, tid, pos, cigar, qual=30, tag=None):
    """one record: qual = one value for every base, or the bytes themselves"""
    l_seq = sum(int(n) for n, op in re.findall(r"(\d+)([MIDNSHP=X])", cigar) if op in QUERY_OPS) if cigar != "*" else 20
    q = bytes([qual]) * l_seq if isinstance(qual, int) else bytes(qual)
    assert len(q) == l_seq
    return dict(name=name, flag=flag, tid=tid, pos=pos, cigar=cigar, qual=q, l_seq=l_seq, tag=tag)


def pair(name, tid1, pos1, cig1, rev1, tid2, pos2, cig2, rev2, q1=30, q2=30, extra_flag=0):
    """the two records of a template: 0x40 then 0x80"""
    f1 = 0x1 | 0x40 | (0x10 if rev1 else 0) | (0x20 if rev2 else 0) | extra_flag
    f2 = 0x1 | 0x80 | (0x10 if rev2 else 0) | (0x20 if rev1 else 0) | extra_flag
    return [rec(name, f1, tid1, pos1, cig1, q1), rec(name, f2, tid2, pos2, cig2, q2)]


def fr(name, pos, q1=30, q2=30, cig1="50M", cig2="50M", pos2=None, tid=0, extra_flag=0):
    """a forward / reverse pair on one reference, the mate 200 bases on"""
    return pair(name, tid, pos, cig1, False, tid, pos + 200 if pos2 is None else pos2, cig2, True, q1, q2, extra_flag)


def _random_case(n_pairs, n_frags, seed, templates=None):
    """pairs drawn from a small pool of templates (so that duplicates are the rule) with random qualities, single-end fragments some
    of which lie on pair ends, shuffled"""
    rng = np.random.default_rng(seed)
    templates = templates or max(4, n_pairs // 3)
    pool = [(int(rng.integers(0, 3)), int(rng.integers(50, 5000)), int(rng.integers(0, 3)), int(rng.integers(50, 5000)), bool(rng.integers(0, 2)), bool(rng.integers(0, 2)))
            for _ in range(templates)]
    clips = [("50M", 0), ("5S45M", 5), ("2H3S45M", 5), ("10S40M", 10)]
    rclips = ["50M", "45M5S", "40M5S5H", "20M5D25M5S", "20M10N20M10S"]
    out = []
    for i in range(n_pairs):
        t1, p1, t2, p2, r1, r2 = pool[int(rng.integers(0, len(pool)))]
        c1, d1 = clips[int(rng.integers(0, len(clips)))] if not r1 else (rclips[int(rng.integers(0, len(rclips)))], 0)
        c2, d2 = clips[int(rng.integers(0, len(clips)))] if not r2 else (rclips[int(rng.integers(0, len(rclips)))], 0)
        l1 = rec("x", 0, 0, 0, c1)["l_seq"]
        l2 = rec("x", 0, 0, 0, c2)["l_seq"]
        out.append(pair(f"p{seed}_{i:05d}", t1, p1 + d1, c1, r1, t2, p2 + d2, c2, r2, bytes(rng.integers(10, 42, l1, dtype=np.uint8)), bytes(rng.integers(10, 42, l2, dtype=np.uint8))))
    for i in range(n_frags):
        if i % 2:
            t, p, _, _, r, _ = pool[int(rng.integers(0, len(pool)))]
        else:
            t, p, r = int(rng.integers(0, 3)), int(rng.integers(50, 300)), bool(rng.integers(0, 2))
        out.append([rec(f"f{seed}_{i:05d}", 0x10 if r else 0, t, p, "50M", bytes(rng.integers(10, 42, 50, dtype=np.uint8)))])
    flat = [r for grp in out for r in grp]
    order = rng.permutation(len(flat))
    return [flat[i] for i in order]


def cases():
    """-> [(name, [records in input order])]"""
    out = []
    # signatures: duplicates only after unclipping; a pair elsewhere is none
    out.append(("unclip_fr", fr("a", 100, 20, 20) + fr("b", 105, 30, 30, cig1="5S45M", pos2=300) + fr("c", 100, 25, 25, pos2=301) + fr("d", 101)))
    # reverse reads whose ends agree only with trailing S and H and with D / N inside counted
    out.append(("reverse_clips", fr("a", 100, cig2="50M", pos2=300) + fr("b", 100, 31, 31, cig2="45M3S2H", pos2=300) + fr("c", 100, 32, 32, cig2="20M3D10M12N5M15S", pos2=285) +
                fr("d", 100, cig2="20M5I25M", pos2=300) + fr("e", 100, cig2="5S45M", pos2=305)))      # d: 45 on the reference, e: a leading clip of a reverse read does not count
    out.append(("hard_and_soft", fr("a", 108, 40, 40, cig1="3H5S42M", pos2=400) + fr("b", 100, pos2=400) + fr("c", 105, 20, 20, cig1="5H45M", pos2=400)))
    out.append(("u_negative", fr("a", 2, cig1="10S40M") + fr("b", 0, 35, 35, cig1="8S42M", pos2=202) + fr("c", 2, 20, 20, cig1="10S40M") + fr("d", 2, cig1="9S41M")))
    out.append(("equal_signatures", pair("a", 1, 500, "50M", False, 1, 500, "50M", False) + pair("b", 1, 500, "50M", False, 1, 500, "50M", False, 35, 35) +
                pair("c", 1, 500, "50M", False, 1, 501, "50M", False)))
    # mates on two references; b has its first read where a has its last: the key orders the two signatures, so they are duplicates
    out.append(("two_references", pair("a", 0, 700, "50M", False, 2, 900, "50M", True) + pair("b", 2, 900, "50M", True, 0, 700, "50M", False, 33, 33) +
                pair("c", 0, 700, "50M", False, 1, 900, "50M", True)))
    # u = 149 forward is not u = 149 reverse
    out.append(("other_strand", pair("a", 0, 149, "50M", False, 0, 400, "50M", True) + pair("b", 0, 100, "50M", True, 0, 400, "50M", True) +
                pair("c", 0, 149, "50M", False, 0, 351, "50M", False)))
    # scores
    out.append(("threshold_14_15", fr("a", 100, 14, 14) + fr("b", 100, 15, 14) + fr("c", 100, 14, 14)))
    out.append(("quals_ff", fr("a", 100, 0xff, 0xff) + fr("b", 100, 16, 0xff) + fr("c", 100, 0xff, 0xff)))
    tie = fr("a", 100) + fr("b", 100) + fr("c", 100)
    out.append(("score_ties", [tie[1], tie[2], tie[4], tie[0], tie[3], tie[5]]))      # 0x40 records in the order b, c, a: b is kept
    # fragments
    out.append(("fragment_at_pair_end", fr("a", 100, 20, 20) + [rec("f1", 0, 0, 100, "50M", 40), rec("f2", 0x10, 0, 300, "50M", 41), rec("f3", 0, 0, 100, "50M", 39),
                                                                rec("f4", 0, 0, 101, "50M", 12)]))
    out.append(("fragments_alone", [rec("f1", 0, 1, 100, "50M", 20), rec("f2", 0, 1, 100, "50M", 30), rec("f3", 0, 1, 105, "5H50M", 30), rec("f4", 0x10, 1, 100, "50M", 30),
                                    rec("f5", 0x10, 1, 51, "99M", 25), rec("f6", 0, 1, 105, "5S45M", 29)]))
    out.append(("mate_unmapped", [rec("a", 0x1 | 0x8 | 0x40, 0, 100, "50M", 30), rec("a", 0x1 | 0x4 | 0x80, 0, 100, "*"), rec("b", 0x1 | 0x8 | 0x40, 0, 100, "50M", 31),
                                  rec("b", 0x1 | 0x4 | 0x80, 0, 100, "*"), rec("c", 0x1 | 0x8 | 0x40, 0, 100, "50M", 29), rec("c", 0x1 | 0x80 | 0x10, 0, 300, "50M", 29)]))
    out.append(("three_under_a_name", fr("a", 100) + [rec("a", 0x1 | 0x80 | 0x10, 0, 300, "50M", 30)] + fr("b", 100, 20, 20) + fr("c", 100, 21, 21)))
    out.append(("two_first_reads", [rec("a", 0x41, 0, 100, "50M", 30), rec("a", 0x41 | 0x10, 0, 300, "50M", 30)] + fr("b", 100, 20, 20) + fr("c", 100, 21, 21)))
    # flags: ineligible records keep their words; an incoming 0x400 on an eligible record is cleared
    keep = []
    for k, f in enumerate((0x100, 0x800, 0x200, 0x4)):
        keep += [rec(f"s{k}", f | 0x400, 0, 100, "50M" if f != 0x4 else "*", 30), rec(f"c{k}", f, 0, 100, "50M" if f != 0x4 else "*", 30)]
    out.append(("ineligible_keep_their_words", fr("a", 100, 30, 30) + keep + fr("b", 100, 20, 20) + [rec("a", 0x1 | 0x40 | 0x800 | 0x400, 0, 600, "20M30H", 30)]))
    out.append(("incoming_dup_cleared", fr("a", 100, 30, 30, extra_flag=0x400) + fr("b", 100, 20, 20) + fr("c", 900, extra_flag=0x400) + [rec("f", 0x400, 2, 5, "50M", 30)]))
    # sizes: one tile of the sorts, one less, one more
    for n in (2047, 2048, 2049):
        out.append((f"pairs_{n}", _random_case(n, 64, n)))
    rng = np.random.default_rng(7)
    copies = []
    for i in range(3000):
        copies += fr(f"k{i:04d}", 1000, bytes(rng.integers(10, 42, 50, dtype=np.uint8)), bytes(rng.integers(10, 42, 50, dtype=np.uint8)))
    out.append(("copies_3000", copies))
    out.append(("one_name_512", one_name(512)))
    out.append(("no_record", []))
    out.append(("no_eligible_record", [rec(f"u{i}", (0x4, 0x100, 0x800 | 0x400, 0x200)[i % 4], 0, 100, "50M" if i % 4 else "*") for i in range(40)]))
    out.append(("random_600", _random_case(300, 40, 600, templates=40)))
    return out


def one_name(n):
    """n eligible records under one name (513: beyond what the device's join resolves)"""
    return [rec("same", 0x1 | (0x40 if i % 2 else 0x80), 0, 100 + i % 3, "50M", 20 + i % 7) for i in range(n)]


def write_case(path, recs):
    n = len(recs)
    seqs = ["ACGT"[i % 4] * r["l_seq"] for i, r in enumerate(recs)]
    batch = RecordBatch.from_fields([r["tid"] for r in recs], [r["pos"] for r in recs], [r["tid"] for r in recs], [r["pos"] for r in recs], [r["flag"] for r in recs], [30] * n,
                                    [r["cigar"] for r in recs], seqs, [r["name"] for r in recs], isize=[0] * n, targets=TG)
    bamio.write_bam(path, batch, header_text="@HD\tVN:1.6\tSO:unsorted\n" + "".join(f"@SQ\tSN:{n}\tLN:{l}\n" for n, l in TG), index=False,
                    quals=[r["qual"] for r in recs], extra={i: b"NMC\x01" for i in range(0, n, 3)})


def case_dir(tmp_path_factory):
    d = tmp_path_factory.mktemp("markdup_cases")
    paths = {}
    for name, recs in cases():
        paths[name] = os.path.join(str(d), name + ".bam")
        write_case(paths[name], recs)
    return paths


def oversized(src, dst, ordinal):
    """the BAM at src with record `ordinal`'s l_seq raised so that its bases and qualities no longer fit its block_size"""
    raw = bytearray(gzip.decompress(open(src, "rb").read()))
    _, _, _, recs = S.split_stream(bytes(raw))
    at = len(raw) - sum(len(r) for r in recs) + sum(len(r) for r in recs[:ordinal])
    struct.pack_into("<i", raw, at + 20, struct.unpack_from("<i", raw, at + 20)[0] + 40)
    open(dst, "wb").write(bamio.bgzf_bytes(bytes(raw)))


# ---- the reference -----------------------------------------------------------------------------------------------------------------
def _fields(r):
    tid, pos, l_name, _, _, n_cig, flag, l_seq = struct.unpack_from("<iiBBHHHi", r, 4)
    name = bytes(r[36:36 + l_name])
    ops = [(w & 15, w >> 4) for w in struct.unpack_from(f"<{n_cig}I", r, 36 + l_name)]
    q0 = 36 + l_name + 4 * n_cig + (l_seq + 1) // 2
    return tid, pos, flag, name, ops, r[q0:q0 + l_seq]


def _signature(tid, pos, flag, ops):
    clip = (4, 5)
    if not flag & 0x10:
        lead = 0
        for op, n in ops:
            if op not in clip:
                break
            lead += n
        return (tid, pos - lead, 0)
    trail = 0
    for op, n in reversed(ops):
        if op not in clip:
            break
        trail += n
    reflen = sum(n for op, n in ops if op in (0, 2, 3, 7, 8))
    return (tid, pos + reflen - 1 + trail, 1)


def ref_markdup(recs):
    """records (bytes, each with its block_size word) in input order -> ([the flag word each leaves with], counts by COUNT_KEYS)"""
    flags, sig, score, by_name = [], {}, {}, {}
    counts = dict.fromkeys(COUNT_KEYS, 0)
    for i, r in enumerate(recs):
        tid, pos, flag, name, ops, quals = _fields(r)
        if flag & (0x4 | 0x100 | 0x200 | 0x800):
            flags.append(flag)
            counts["ineligible"] += 1
            continue
        flags.append(flag & ~0x400)
        sig[i] = _signature(tid, pos, flag, ops)
        score[i] = sum(q for q in quals if q >= 15 and q != 0xff)
        by_name.setdefault(name, []).append((i, flag))
    pairs, in_pair = [], set()
    for name, members in by_name.items():
        if len(members) != 2 or any(not f & 0x1 or f & 0x8 for _, f in members):
            continue
        first = [i for i, f in members if f & 0x40 and not f & 0x80]
        last = [i for i, f in members if f & 0x80 and not f & 0x40]
        if len(first) == 1 and len(last) == 1:
            pairs.append((first[0], last[0]))
            in_pair.update((first[0], last[0]))
    counts["pairs"] = len(pairs)
    by_key = {}
    for a, b in pairs:
        by_key.setdefault(tuple(sorted((sig[a], sig[b]))), []).append((-(score[a] + score[b]), a, b))
    pair_ends = set()
    for group in by_key.values():
        group.sort()
        for _, a, b in group[1:]:
            flags[a] |= 0x400
            flags[b] |= 0x400
            counts["dup_pairs"] += 1
    for a, b in pairs:
        pair_ends.update((sig[a], sig[b]))
    frags = {}
    for i in sig:
        if i not in in_pair:
            frags.setdefault(sig[i], []).append((-score[i], i))
    for e, group in frags.items():
        counts["fragments"] += len(group)
        group.sort()
        for _, i in (group if e in pair_ends else group[1:]):
            flags[i] |= 0x400
            counts["dup_fragments"] += 1
    return flags, counts


def reference(path):
    """what `strling sort --markdup` must write for the BAM at `path`, inflated, and report -> (stream bytes, counts, flags by
    input ordinal): plain sort's stream (sort_bam_cases.reference_stream's rule) over the records with the decided flag words"""
    text, refs, n_ref, recs = S.split_stream(gzip.decompress(open(path, "rb").read()))
    flags, counts = ref_markdup(recs)
    marked = [r[:18] + struct.pack("<H", f) + r[20:] for r, f in zip(recs, flags)]
    perm = sorted(range(len(recs)), key=lambda i: S.ref_key(recs[i], n_ref))
    out_text = S.ref_header_text(text).encode()
    return b"BAM\1" + struct.pack("<i", len(out_text)) + out_text + refs + b"".join(marked[i] for i in perm), counts, flags


COUNT_LINE = re.compile(r"markdup: (\d+) pairs, (\d+) duplicate pairs, (\d+) fragments, (\d+) duplicate fragments, (\d+) ineligible records")


def counts_of(stderr):
    m = COUNT_LINE.search(stderr)
    assert m, stderr
    return dict(zip(COUNT_KEYS, (int(x) for x in m.groups())))
