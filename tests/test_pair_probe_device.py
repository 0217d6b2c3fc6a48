"""pair_probe_kernel and the Bloom bitmap's layout on the device (-m gpu): the cases of tests/probe_cases.py -- hot keys at the
edges of the layout (no false negative), cold keys one bit short of a hot key's pattern or in another word (no item), batch sizes
around a wave's range and a turn with the last read hot (the clamped loads make no item twice), a wave that flushes inside its
loop -- through Context.extract_device on host-staged batches.  Treads against the oracle's, exactly; the join-item count against
the reads of the hot groups plus their hot soft-clip records, exactly.

STRL_GRID_P is read once per process: the default grid runs in this process, the one-block grid in one child (tests/probe_child.py).
A child that ends by a signal, at its time limit or with a HIP fault in its output fails every test of its configuration.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import probe_cases as PC
import probe_child
from helpers import treads_equal

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
CHILD_TIMEOUT = 30
FAULT_WORDS = ("illegal memory access", "Memory access fault", "HSA_STATUS_ERROR", "Aborted", "Segmentation fault")


def _load(path):
    with np.load(path, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def runs(ctx, tmp_path_factory):
    assert "STRL_GRID_P" not in os.environ, "the parent runs the default grid: unset STRL_GRID_P"
    tmp = tmp_path_factory.mktemp("probe")
    out = {}
    probe_child.run_cases(ctx, str(tmp / "default.npz"))
    out["default"] = _load(tmp / "default.npz")
    for cfg, env_add in PC.CONFIGS.items():
        env = dict(os.environ)
        env.update({k: str(v) for k, v in env_add.items()})
        path = tmp / (cfg + ".npz")
        try:
            p = subprocess.run([sys.executable, os.path.join(HERE, "probe_child.py"), str(path)], env=env, timeout=CHILD_TIMEOUT,
                               stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            text, rc = p.stdout, p.returncode
        except subprocess.TimeoutExpired as e:
            text, rc = (e.stdout.decode(errors="replace") if isinstance(e.stdout, bytes) else (e.stdout or "")), "time limit of %d s" % CHILD_TIMEOUT
        fault = [w for w in FAULT_WORDS if w in text]
        if rc != 0 or fault:
            out[cfg] = ("dead", "%s: exit %s%s\n%s" % (cfg, rc, ", " + fault[0] if fault else "", "\n".join(text.splitlines()[-15:])))
            break
        out[cfg] = _load(path)
    return out


@pytest.mark.parametrize("name", PC.ALL)
@pytest.mark.parametrize("cfg", ("default",) + tuple(PC.CONFIGS))
def test_probe_case(runs, cfg, name):
    r = runs.get(cfg, ("not run", "an earlier child died"))
    if isinstance(r, tuple):
        pytest.fail("child %s: %s" % r)
    if name + ".error" in r:
        pytest.fail("%s/%s: the library refused the case: %s" % (cfg, name, r[name + ".error"]))
    e = PC.expected(name)
    items = int(r[name + ".items"])
    print("%s/%s: %d reads, %d join items, expected %d (%d reads of hot groups + %d hot soft-clip records)"
          % (cfg, name, PC.case(name).rec.n, items, e["items"], int(e["probe_hit"].sum()), e["n_hot_soft"]))
    ok, why = treads_equal(r[name + ".treads"], e["treads"])
    assert ok, "%s/%s: treads in .bin order: %s" % (cfg, name, why)
    assert len(e["treads"]) > 0
    # fewer: a hot read was missed (a false negative) -- the treads above would differ too; more: a cold key passed, or a lane
    # past the end of its wave's range made an item of the read it was clamped to
    assert items == e["items"], (cfg, name)
