"""Shared helpers for the parity tests (test infrastructure)."""
import numpy as np

CODE = {"C": 0, "A": 1, "T": 2, "G": 3}


def pack_word(unit, count, skipped=False):
    """(unit str, count) -> packed scorer word of include/strling_amd.h"""
    if isinstance(unit, bytes):
        unit = unit.decode()
    k = len(unit)
    code = 0
    for ch in unit:
        code = (code << 2) | CODE[ch]
    return (code | (k << 12) | (int(count) << 16) | (0x8000 if skipped else 0)) & 0xFFFFFFFF


def oracle_words(O, rec, g, opts):
    """Oracle scorer outputs in the packed layout the device produces: (whole u32[n], dict (read,side)->(first,after))."""
    sk, wu, wc, su, sc = O.score_records_packed(rec, g, opts)
    whole = np.array([pack_word(wu[i], wc[i], sk[i]) for i in range(rec.n)], dtype=np.uint32)
    soft = {}
    for i in range(rec.n):
        for side in (0, 1):
            soft[(i, side)] = (pack_word(su[i, 2 * side], sc[i, 2 * side]), pack_word(su[i, 2 * side + 1], sc[i, 2 * side + 1]))
    return whole, soft


def soft_items_expected(rec, whole, min_mapq):
    """Which (read, side) items add_soft would look at (extract.nim:97-106), given the whole-read words."""
    items = []
    for i in range(rec.n):
        a, b = int(rec.cigar_off[i]), int(rec.cigar_off[i + 1])
        L = b - a
        if L == 0 or rec.mapq[i] < min_mapq or (whole[i] & 0x8000):
            continue
        first_s = (int(rec.cigar[a]) & 0xF) == 4
        last_s = (int(rec.cigar[b - 1]) & 0xF) == 4
        has_unit = ((int(whole[i]) >> 12) & 7) != 0
        if first_s and (has_unit or (int(rec.cigar[a]) >> 4) > 16):
            items.append((i, 0))
        if last_s and L > 1 and (has_unit or (int(rec.cigar[b - 1]) >> 4) > 16):
            items.append((i, 1))
    return items


def treads_equal(a, b, fields=("tid", "position", "repeat", "flag", "split", "mapping_quality", "repeat_count", "align_length",
                               "qname_id")):
    if len(a) != len(b):
        return False, f"length {len(a)} != {len(b)}"
    for f in fields:
        if not np.array_equal(np.asarray(a[f]), np.asarray(b[f])):
            bad = np.nonzero(np.asarray(a[f]) != np.asarray(b[f]))[0][:5]
            return False, f"field {f} differs at {bad.tolist()}: {a[f][bad].tolist()} vs {b[f][bad].tolist()}"
    return True, ""


def bounds_rows(bounds, targets, row_fn):
    return [row_fn(b, targets[int(b["tid"])][0]) for b in bounds]


def device_batch(torch, dev, soa, rows, qh, with_meta=True, offset=0):
    """the arrays of a host batch uploaded to the device -> (CReadSoa, CPairSoa, keep-alive list): device-resident input
    is what makes strl_extract_device overlap a batch's pair logic with the next batch's scorer.
    offset: every per-read column starts `offset` elements into its allocation (offset=1: no column is 16-byte aligned, so the
    skip-predicate pass takes its scalar variant); SEQ, the packed rows and the pairing arrays, which are read 16 bytes at a time,
    stay where the allocator put them"""
    from strling_amd import api

    def up(a, off=0):
        a = np.ascontiguousarray(a)
        if not off:
            return torch.from_numpy(a).to(dev)
        padded = np.zeros(a.size + off, a.dtype)
        padded[off:] = a
        return torch.from_numpy(padded).to(dev)[off:]
    d = {k: up(getattr(soa, k), offset) for k in ("tid", "pos", "end", "seq_off", "l_seq", "clip_l", "clip_r", "mapq", "cig")}
    d["seq4"] = up(soa.seq4)
    drows, dqh = up(rows.view(np.uint8)), up(qh)
    d["meta"] = up(soa.meta_rows().view(np.int32)) if with_meta else None
    cs = api.CReadSoa(soa.n, d["tid"].data_ptr(), d["pos"].data_ptr(), d["end"].data_ptr(), d["seq_off"].data_ptr(), d["l_seq"].data_ptr(),
                      d["clip_l"].data_ptr(), d["clip_r"].data_ptr(), d["mapq"].data_ptr(), d["cig"].data_ptr(), d["seq4"].data_ptr(),
                      d["seq4"].numel(), soa.max_l_seq, api.MEM_DEVICE, d["meta"].data_ptr() if with_meta else None)
    cp = api.CPairSoa(drows.data_ptr(), dqh.data_ptr())
    torch.cuda.synchronize()
    return cs, cp, [d, drows, dqh]


FRONT_FIELDS = ("tid", "position", "repeat", "flag", "split", "mapping_quality", "repeat_count", "align_length", "qname_id")


def check_front_extract(ctx, rec, g, path, chunk_blocks, exp):
    """`ctx.extract_bam_device(path)` (inflate, record scan, parse, scorer, pair logic on the device) against the treads `exp` of
    the records the file was written from: every field in .bin order, the qnames, the fragment-length words of every record, the
    chunk summaries' counts, the contigs seen -> what the device returned"""
    from oracle import oracle as O
    from strling_amd import synth
    med = O.median(synth.frag_hist(rec))
    ctx.set_opts(0.8, 40, med)
    ctx.set_genome(g)
    got = ctx.extract_bam_device(path, chunk_blocks=chunk_blocks)
    assert got["n_records"] == rec.n
    assert [t[0] for t in got["targets"]] == [t[0] for t in rec.targets]
    for f in FRONT_FIELDS:
        assert np.array_equal(got["treads"][f], exp[f]), (f, chunk_blocks)
    assert got["qnames"] == [rec.qname(int(i)) for i in exp["qname_id"]]
    isz = rec.isize if rec.isize is not None else np.zeros(rec.n, np.int32)
    fw = rec.flag.astype(np.uint32) | (np.where((isz >= 0) & (isz <= 4095), isz, 0xffff).astype(np.uint32) << 16)
    assert np.array_equal(got["fragwords"], fw)
    prim = (rec.flag & 0x900) == 0
    assert sum(c["n_primary"] for c in got["chunks"]) == int(prim.sum())
    n_tail = 0
    while n_tail < rec.n and rec.tid[rec.n - 1 - n_tail] < 0:
        n_tail += 1
    assert got["n_tail"] == n_tail
    if n_tail < rec.n:      # the last chunk with a placed record counts the primary records behind it
        last = [c for c in got["chunks"] if c["last_placed"] >= 0][-1]
        assert last["tail_primary"] <= int(prim[rec.n - n_tail:].sum())
    seen = np.zeros(len(rec.targets), np.uint8)
    seen[np.unique(rec.tid[prim & (rec.tid >= 0)])] = 1
    assert np.array_equal(got["tids_seen"], seen)
    return got
