"""A context gives back all the device memory it took when it is destroyed, on the normal path and after a refused call.

Every device buffer of the library is a DevBuf, which owns its allocation; the library counts what it holds and
STRL_DEVICE_MEM_LIMIT_MB makes it refuse (STRL_ERR_NOMEM) to go past a limit.  A process that makes, uses and closes contexts one
after the other under a limit of about twice one context's footprint therefore runs out exactly when a destroyed context
kept something.

One cycle's footprint follows from the allocation sizes (the library counts what it asks for, so the figure does not depend on
the device): the scorer's `inv_spill` for the 510-base class is 72 MB, everything else a 4096-read batch takes stays under
10 MB, so one cycle passes under 128 MB (ONE_CYCLE_MB, the smallest multiple of 64 MB) and the test's limit is twice that.
Before DevBuf owned its memory, strl_ctx_destroy released the buffers from a hand-kept list that had no `inv_spill`: 72 MB
stayed behind per context that scored anything, and under the same limit the fourth cycle (FAILED_BEFORE) has no room."""
import json
import os
import subprocess
import sys

import pytest

ONE_CYCLE_MB = 128        # smallest limit, rounded up to a multiple of 64 MB, under which one cycle passes
LIMIT_MB = 2 * ONE_CYCLE_MB
FAILED_BEFORE = 4
STRL_ERR_NOMEM = -10


@pytest.mark.gpu
def test_contexts_made_and_closed_in_a_row_stay_under_a_memory_limit():
    """eight cycles of create / set options / score 4096 reads (long and soft-clipped ones among them) / extract on the device /
    cluster / close, then an strl_extract_begin for 2^31 reads that the limit refuses, close, and one more cycle: no cycle
    runs out of memory, every cycle produces the same treads and bounds"""
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ctx_lifecycle_child.py")
    env = dict(os.environ, STRL_DEVICE_MEM_LIMIT_MB=str(LIMIT_MB))
    r = subprocess.run([sys.executable, child], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr
    out = json.loads(r.stdout.strip().splitlines()[-1])
    print(out)
    cycles = out["cycles"]
    assert all(c["ok"] for c in cycles), (len(cycles), cycles[-1])
    assert len(cycles) == 8
    assert cycles[0]["treads"] > 20 and cycles[0]["bounds"] > 0
    assert all(c == cycles[0] for c in cycles)
    assert out["refused"] == STRL_ERR_NOMEM and "out of device memory" in out["refused_error"], out
    assert out["after"] == cycles[0], out["after"]
