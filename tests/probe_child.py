"""Runs every case of tests/probe_cases.py through Context.extract_device and writes the treads and the join-item count to an .npz
(test infrastructure).  STRL_GRID_P is read once per process, so tests/test_pair_probe_device.py starts this file as a child
process for the one-block grid (`python probe_child.py OUT.npz`) and calls run_cases() itself for the default grid.  Nothing is
compared here."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)


def run_cases(ctx, out_path):
    import loop_cases as LC
    import probe_cases as PC
    from strling_amd import api
    out = {}
    ctx.set_opts(*LC.OPTS)
    ctx.set_genome(None)
    for name in PC.ALL:
        c = PC.case(name)
        soa = api.Soa(c.rec)
        rows, _ = soa.pair_rows()
        qh = np.ascontiguousarray(c.qhash, np.uint64)
        cp = api.CPairSoa(rows.ctypes.data, qh.ctypes.data)
        n = soa.n
        try:
            ctx.extract_device(soa.c_struct(), cp, 0, item_cap=4 * n + 16, tread_cap=8 * n + 16)
            treads, _ = ctx.treads_fetch()
            out[name + ".treads"], out[name + ".items"] = treads, np.array(ctx.pair_items())
        except api.StrlingError as e:
            if "error -2" in str(e) or "illegal memory access" in str(e):      # a HIP error: nothing more is started on the device
                raise
            out[name + ".error"] = np.array(str(e))
    ctx.sync()
    np.savez(out_path, **out)


if __name__ == "__main__":
    import torch
    from strling_amd import api
    assert torch.cuda.is_available()
    torch.cuda.init()
    ctx = api.Context(0)
    run_cases(ctx, sys.argv[1])
    ctx.close()
    print("probe_child: done", flush=True)
