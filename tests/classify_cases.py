"""Batches for the two kinds of turn of classify_kernel (strling_amd/csrc/score.hip, classify_turn.h): FULL turns, which load,
test and store without a bounds test while the next turn's vectors are in flight, and GENERAL turns (the last two of a wave's
range, ragged ends, the scalar variant).  A case is a shape (the number of reads: it decides which turns of which waves are
full) and a kind of records (what the skip predicate meets in those turns), built with the builders of tests/loop_cases.py.
tests/test_classify_cases.py shows on the CPU which turn every edge falls into; tests/test_classify_turns_device.py runs the
cases through the kernel.  Run as a script (`python classify_cases.py OUT.npz`) this file is the child process of that test:
STRL_GRID_C is read once per process.

The queued ids are read back from the device (Context.score_queue_ids) and compared, sorted, with the kept reads.  Every read is
also a repeat tract, so the packed word of a kept read is never zero: the pass writes zero for a kept read and the scorer the real
word, and only for the ids classify queued -- the `whole` words say the same a second way, through the scorer.
"""
import collections
import functools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import loop_cases as LC  # noqa: E402
from strling_amd.records import GenomeStr  # noqa: E402

# Under STRL_GRID_C=1 (four waves, a share of ceil(n / 4) rounded up to 256):
SHAPES_TURNS = {
    4096: "every wave: one full turn, then one general turn; the full turn's prefetch ends exactly at r1",
    4095: "the last wave has no full turn, its last group is ragged",
    4097: "shares of 1280: full, general, half a general turn; the last wave owns 257 reads",
    6144: "two full turns in a row: the hand-over between two full turns, both register sets",
    7168: "shares of 1792: two full turns, a whole general turn, half a general turn",
    8192: "an odd number of full turns (three), then one general turn",
}
SHAPES_SMALL = {1: "three waves own nothing", 3: "one ragged group", 255: "one wave, no whole group row", 256: "one wave of exactly its share",
                257: "a second wave with one read", 1021: "four waves of one general turn, the last one ragged"}
KINDS = ("reload", "contig", "dense", "backwards", "keep_all", "keep_none")
SMALL_KINDS = ("reload", "keep_all", "keep_none")
CONFIGS = {"one": dict(STRL_GRID_C=1), "two": dict(STRL_GRID_C=2)}      # and "default": the parent process itself
OPTS = LC.OPTS
L = 100
STEP = 30                 # bases between consecutive reads: a turn of 512 reads spans 15 kb, a window of JOIN_WIN sparse starts ~24 kb
SEQS = [(u * (L // len(u) + 1))[:L] for u in ("CAG", "AC", "AAAG", "AAT")]
Case = collections.namedtuple("Case", "name kind n rec genome opts")


def _records(tid, pos, length=L):
    n = len(pos)
    return LC._batch([int(t) for t in tid], [int(p) for p in pos], ["%dM" % length] * n, [SEQS[i % 4][:length] for i in range(n)], n_targets=4)


def _regular(lo, hi, every=3000, width=137):
    """one interval every 3 kb: a turn's span of 15.4 kb holds six starts at the most (the window of eight, loaded at the bin of
    the smallest stop, reaches at least 21 kb: it holds the turn) and the next turn's ends 30.8 kb on (it never holds that)"""
    return [(s, s + width) for s in range(lo, hi, every)]


def _turn_of(n):
    """turn number, inside its wave under STRL_GRID_C=1, of every read"""
    t = np.zeros(n, np.int64)
    for its in LC.Model().iterations(n, "C", CONFIGS["one"]):
        for k, (a, b) in enumerate(its):
            t[a:b] = k
    return t


@functools.lru_cache(maxsize=None)
def case(kind, n):
    pos = 100_000 + STEP * np.arange(n)
    hi = int(pos[-1]) + 10_000
    tid = np.zeros(n, np.int64)
    length = L
    if kind == "reload":            # a turn leaves the window the turn before loaded: every turn loads its own
        g = GenomeStr.from_lists(1, {0: _regular(90_500, hi)})
    elif kind == "contig":          # the contig changes with every turn of the four-wave partition, the coordinates go on
        tid = _turn_of(n) % 2
        g = GenomeStr.from_lists(2, {0: _regular(90_500, hi), 1: _regular(91_700, hi)})
    elif kind == "dense":           # 40 starts in one 4 KiB bin, every read behind the eighth of them: the window never holds the span
        bin0 = 30 << 12
        cluster = [(bin0 + 100 * j, bin0 + 100 * j + 12) for j in range(40)]
        pos = bin0 + 800 + (np.arange(n) * 3000) // max(n, 1)
        length = 40
        g = GenomeStr.from_lists(1, {0: [(110_000, 110_200)] + cluster + [(135_000, 135_040)]})
    elif kind == "backwards":       # blocks of 256 reads in descending order: every turn lies below the window it inherits
        order = np.concatenate([np.arange(b, min(b + 256, n)) for b in range((n - 1) // 256 * 256, -1, -256)])
        pos = pos[order]
        g = GenomeStr.from_lists(1, {0: _regular(90_500, hi)})
    elif kind == "keep_all":        # no table: every read is queued, the stage is flushed in every turn, the prefetch in flight
        g = None
    elif kind == "keep_none":       # one interval far below every read: all skipped, nothing is ever staged
        g = GenomeStr.from_lists(1, {0: [(1000, 1100)]})
    else:
        raise KeyError(kind)
    return Case("%s_%d" % (kind, n), kind, n, _records(tid, pos, length), g, OPTS)


def all_cases():
    return [(k, n) for n in SHAPES_TURNS for k in KINDS] + [(k, n) for n in SHAPES_SMALL for k in SMALL_KINDS]


ALL = ["%s_%d" % kn for kn in all_cases()]


def by_name(name):
    kind, n = name.rsplit("_", 1)
    return case(kind, int(n))


@functools.lru_cache(maxsize=None)
def expected(name):
    """the oracle's packed words of a case, once per process"""
    from oracle import oracle as O
    from helpers import oracle_words
    c = by_name(name)
    whole, _ = oracle_words(O, c.rec, c.genome, O.make_opts(c.opts[2], c.opts[0], c.opts[1]))
    return dict(whole=whole, skipped=(whole & 0x8000) != 0)


def turn_kinds(n, cfg):
    """[(wave, turn, base, end, kind)] under a configuration; kind: "full", "seam" (the first general turn behind a full one),
    "behind" (every later general turn of a wave that had a full turn) or "general" (a wave without a full turn)"""
    m = LC.Model()
    step = 64 * m.CL_ILP
    out = []
    for w, its in enumerate(m.iterations(n, "C", cfg)):
        whole = [b - a == step for a, b in its]
        n_full = 0
        for k, (a, b) in enumerate(its):
            full = whole[k] and k + 1 < len(its) and whole[k + 1]
            n_full += full
            out.append((w, k, a, b, "full" if full else "general" if not n_full else "seam" if k == n_full else "behind"))
    return out


STAT_FIELDS = ("n_reads", "n_skipped", "n_scored")


def run_cases(ctx, out_path):
    """every case through the skip-predicate pass and the scorer, device-resident: 16-byte aligned (classify_kernel<true>) and one
    element into the allocations (<false>).  Nothing is compared here -> seconds"""
    import time
    import torch
    from helpers import device_batch
    from strling_amd import api
    dev = torch.device("cuda", 0)
    out = {}
    t0 = time.perf_counter()
    for name in ALL:
        c = by_name(name)
        ctx.set_opts(c.opts[0], c.opts[1], c.opts[2])
        ctx.set_genome(c.genome)
        soa = api.Soa(c.rec)
        rows, qh = soa.pair_rows()
        n = soa.n
        try:
            for off in (0, 1):
                cs, cp, keep = device_batch(torch, dev, soa, rows, qh, with_meta=off == 0, offset=off)
                w = torch.zeros(n, dtype=torch.int32, device=dev)
                s = torch.zeros((2 * n + 2) * 4, dtype=torch.int32, device=dev)
                _, st = ctx.score_device(cs, w.data_ptr(), s.data_ptr(), 2 * n + 2, sync=True)
                torch.cuda.synchronize()
                out["%s.dev%d.whole" % (name, off)] = w.cpu().numpy().view(np.uint32)
                out["%s.dev%d.stats" % (name, off)] = np.array([int(getattr(st, f)) for f in STAT_FIELDS], np.int64)
                ids, n_ids = ctx.score_queue_ids(n)               # what classify_kernel itself queued, read back
                out["%s.dev%d.queue" % (name, off)] = ids
                out["%s.dev%d.n_queue" % (name, off)] = np.array(n_ids)
                del cs, cp, keep, w, s
        except api.StrlingError as e:
            if "error -2" in str(e) or "illegal memory access" in str(e):       # a HIP error: nothing more is started on the device
                raise
            out[name + ".error"] = np.array(str(e))
    ctx.sync()
    secs = time.perf_counter() - t0
    out["seconds"] = np.array(secs)
    np.savez(out_path, **out)
    return secs


if __name__ == "__main__":
    import torch
    from strling_amd import api
    # torch first, as in the parent: its HIP runtime, loaded behind the library's, finds no device
    assert torch.cuda.is_available()
    torch.cuda.init()
    ctx = api.Context(0)
    secs = run_cases(ctx, sys.argv[1])
    ctx.close()
    print("classify child: %d cases in %.2f s" % (len(ALL), secs), flush=True)
