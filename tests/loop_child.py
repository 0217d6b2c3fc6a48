"""Runs every case of tests/loop_cases.py through the device and writes what came back to an .npz (test infrastructure).

The grid variables (STRL_GRID_A / _B / _C / _P / _K, STRL_SPLIT_SEGMENTS) are read once per process, so tests/test_loop_device.py
starts this file as a child process per grid configuration (`python loop_child.py OUT.npz`) and calls run_cases() itself for the
default grids.  Nothing is compared here: the parent holds the results against the oracle.
"""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

STAT_FIELDS = ("n_reads", "n_skipped", "n_scored", "n_soft_items", "n_stage_b_whole", "n_stage_b_soft")


def _stats(st):
    return np.array([int(getattr(st, f)) for f in STAT_FIELDS], np.int64)


def _sorted_soft(soft):
    return soft[np.argsort(soft["read_side"], kind="stable")]


def run_cases(ctx, out_path, names=None):
    """-> seconds per case (and "total"); the arrays go to out_path: "<case>.<what>" """
    import torch
    import loop_cases as LC
    from helpers import device_batch
    from strling_amd import api
    dev = torch.device("cuda", 0)
    out, secs = {}, {}
    t_all = time.perf_counter()
    for name in names or LC.ALL_CASES:
        t0 = time.perf_counter()
        c = LC.case(name)
        ctx.set_opts(c.opts[0], c.opts[1], c.opts[2])
        ctx.set_genome(c.genome)
        soa = api.Soa(c.rec)
        try:
            _run_case(ctx, LC, api, torch, dev, device_batch, name, c, soa, out)
        except api.StrlingError as e:
            # an error of the library's own (a capacity, an assertion of the reference) is a result the parent reports for this case;
            # a HIP error is not: nothing more is started on the device
            if "error -2" in str(e) or "illegal memory access" in str(e):
                raise
            out[name + ".error"] = np.array(str(e))
        secs[name] = time.perf_counter() - t0
    ctx.sync()
    secs["total"] = time.perf_counter() - t_all
    out["seconds"] = np.array([secs[k] for k in sorted(secs)])
    out["seconds_of"] = np.array(sorted(secs))
    np.savez(out_path, **out)
    return secs


def _run_case(ctx, LC, api, torch, dev, device_batch, name, c, soa, out):
    n = soa.n
    whole, soft, st = ctx.score_reads(soa)
    out[name + ".whole"], out[name + ".soft"], out[name + ".stats"] = whole, soft, _stats(st)
    if name in LC.SKIP_CASES:
        # device-resident columns, 16-byte aligned (the vector variant of the skip-predicate pass, the packed rows given) and one
        # element into their allocations (the scalar variant; the rows built from the shifted columns)
        rows, qh = soa.pair_rows()
        for off in (0, 1):
            cs, cp, keep = device_batch(torch, dev, soa, rows, qh, with_meta=off == 0, offset=off)
            w = torch.zeros(n, dtype=torch.int32, device=dev)
            s = torch.zeros((2 * n + 2) * 4, dtype=torch.int32, device=dev)
            ns, st = ctx.score_device(cs, w.data_ptr(), s.data_ptr(), 2 * n + 2, sync=True)
            torch.cuda.synchronize()
            out["%s.dev%d.whole" % (name, off)] = w.cpu().numpy().view(np.uint32)
            out["%s.dev%d.soft" % (name, off)] = _sorted_soft(s.cpu().numpy().view(api.SOFT_DTYPE)[:ns])
            out["%s.dev%d.stats" % (name, off)] = _stats(st)
            del cs, cp, keep, w, s
    if name in LC.EXTRACT_CASES:
        treads, st = ctx.extract(c.rec, 0)
        out[name + ".treads"], out[name + ".extract_stats"] = treads, _stats(st)
    if name in LC.PAIR_CASES:
        # the join items are the reads of the hot qname groups (and what the Bloom bitmap lets through beside them): one slot
        # less than that must end in STRL_ERR_CAPACITY, not in treads
        cap = int(LC.expected(name)["probe_hit"].sum()) - 1
        rows, qh = soa.pair_rows()
        cp = api.CPairSoa(rows.ctypes.data, qh.ctypes.data)
        msg = ""
        try:
            ctx.extract_device(soa.c_struct(), cp, 0, item_cap=cap, tread_cap=8 * n + 16)
            got, _ = ctx.treads_fetch()
            msg = "no error: %d treads" % len(got)
        except api.StrlingError as e:
            msg = str(e)
        out[name + ".capacity_error"] = np.array(msg)
        out[name + ".capacity"] = np.array(cap)


if __name__ == "__main__":
    import torch
    from strling_amd import api
    t0 = time.perf_counter()
    # torch first, as in the parent (conftest asks it for the device before any context exists): its HIP runtime, loaded behind the
    # library's, finds no device
    assert torch.cuda.is_available()
    torch.cuda.init()
    ctx = api.Context(0)
    secs = run_cases(ctx, sys.argv[1])
    ctx.close()
    print("loop_child: %s" % " ".join("%s=%.2fs" % kv for kv in secs.items()), flush=True)
    print("loop_child: process %.2fs" % (time.perf_counter() - t0), flush=True)
