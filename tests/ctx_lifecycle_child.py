"""Child process of test_ctx_lifecycle.py (STRL_DEVICE_MEM_LIMIT_MB is read once, at a process' first allocation): contexts made,
used and closed one after the other under that limit.  Prints one JSON line: per cycle what it produced or the error that
ended it, the status of the refused strl_extract_begin, and the cycle after it."""
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from strling_amd import api, synth  # noqa: E402
from strling_amd.records import CIGAR_OPS, RecordBatch  # noqa: E402

CYCLES = 8


def make_batch():
    """4096 reads of synth_wgs (soft-clipped ones among them), two of them replaced by reads the kernels pass to the host twin:
    700 plain bases, and 720 bases with a CAG tract clipped on either side"""
    rec, g = synth.synth_wgs(2048, seed=29, contig_len=400_000)
    assert rec.n == 4096
    rng = np.random.default_rng(3)
    rnd = lambda n: np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].tobytes().decode()
    S, M = CIGAR_OPS.index("S"), CIGAR_OPS.index("M")
    seqs = [rec.sequence(i) for i in range(rec.n)]
    cigs = [[int(c) for c in rec.cigar[int(rec.cigar_off[i]):int(rec.cigar_off[i + 1])]] for i in range(rec.n)]
    mapq = rec.mapq.copy()
    a, b = [int(i) for i in np.nonzero((rec.tid >= 0) & (np.diff(rec.cigar_off) == 1))[0][[5, 900]]]
    seqs[a], cigs[a] = rnd(700), [(700 << 4) | M]
    seqs[b], cigs[b], mapq[b] = "CAG" * 20 + rnd(600) + "CAG" * 20, [(60 << 4) | S, (600 << 4) | M, (60 << 4) | S], 60
    out = RecordBatch.from_fields(rec.tid, rec.pos, rec.mtid, rec.mpos, rec.flag, mapq, cigs, seqs, [rec.qname(i) for i in range(rec.n)],
                                  isize=rec.isize, targets=rec.targets)
    return out, g


def cycle(rec, g, soa, rows, qh):
    """strl_score_reads on the host batch (staging buffers, the long reads' list), strl_extract_device twice on a device-resident
    copy (the overlapped mode: both buffer sets, the side streams), the treads, a clustering pass"""
    ctx = api.Context(0)
    L = ctx.L
    held = []
    try:
        ctx.set_opts(0.8, 40, 350)
        ctx.set_genome(g)
        whole, soft, st = ctx.score_reads(soa)
        assert st.n_soft_items > 0 and int(soa.l_seq.max()) > 510

        def up(a):
            a = np.ascontiguousarray(a)
            p = C.c_void_p()
            api._check(L.strl_dev_alloc(ctx.h, C.c_uint64(a.nbytes), C.byref(p)))
            held.append(p)
            api._check(L.strl_copy(ctx.h, p, C.c_void_p(a.ctypes.data), C.c_uint64(a.nbytes), 1))
            return p.value
        cs = api.CReadSoa(soa.n, up(soa.tid), up(soa.pos), up(soa.end), up(soa.seq_off), up(soa.l_seq), up(soa.clip_l), up(soa.clip_r), up(soa.mapq),
                          up(soa.cig), up(soa.seq4), soa.seq4.size, soa.max_l_seq, api.MEM_DEVICE)
        cp = api.CPairSoa(up(rows.view(np.uint8)), up(qh))
        n_tail = int((rec.tid < 0).sum())
        ctx.extract_device(cs, cp, n_tail)
        ctx.extract_device(cs, cp, n_tail)
        assert ctx.tail_stream() != ctx.stream
        treads, st2 = ctx.treads_fetch()
        assert st2.n_reads == rec.n and st2.n_soft_items == st.n_soft_items
        bounds, unplaced, _ = ctx.cluster(treads, api.MODE_CALL, 560, min_support=2, max_clip_dist=175)
        return dict(ok=True, treads=len(treads), bounds=len(bounds), words=int(whole.astype(np.uint64).sum()))
    except api.StrlingError as e:
        return dict(ok=False, error=str(e))
    finally:
        for p in held:
            L.strl_dev_free(ctx.h, p)
        ctx.close()


def main():
    rec, g = make_batch()
    soa = api.Soa(rec)
    rows, qh = soa.pair_rows()
    out = dict(cycles=[])
    for _ in range(CYCLES):
        out["cycles"].append(cycle(rec, g, soa, rows, qh))
        if not out["cycles"][-1]["ok"]:
            break
    else:
        ctx = api.Context(0)
        ctx.set_opts(0.8, 40, 350)
        out["refused"] = int(ctx.L.strl_extract_begin(ctx.h, 1 << 31))
        out["refused_error"] = ctx.L.strl_last_error().decode()
        ctx.close()
        out["after"] = cycle(rec, g, soa, rows, qh)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
