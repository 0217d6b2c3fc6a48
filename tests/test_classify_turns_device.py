"""The full and the general turns of classify_kernel on the device (-m gpu): the cases of tests/classify_cases.py -- shapes that put
one, two and three full turns, the full / general seam, the turn behind it, ragged ends and waves without a read into a launch of
four waves; records that bring a window reload, a contig change, the skip_one fallback, descending blocks, a flush in every turn
and no kept read at all into those turns -- against the oracle, exactly: the `whole` words, the queued ids as a set (read back
from the device), n_skipped and n_scored.  tests/test_classify_cases.py shows on the CPU that the cases reach these turns.

STRL_GRID_C is read once per process: the default grid runs in this process, STRL_GRID_C=1 and =2 in one child each
(`python classify_cases.py OUT.npz`), each case device-resident 16-byte aligned (classify_kernel<true>) and one element into the
allocations (<false>).  The children run in order; one that ends by a signal, at its time limit or with a HIP fault in its output
is the last one started, and the tests of the configuration behind it fail with "not run".
"""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import classify_cases as CC

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
CHILDREN = tuple(CC.CONFIGS)
# The default-grid pass over all cases, measured once on an MI355X in the parent process (warm context): 0.73 s.  A child gets ten
# times that, for its whole life (interpreter start, library load and building the cases included; measured: 2.6 - 2.7 s).
DEFAULT_PASS_SECONDS = 0.73
CHILD_TIMEOUT = 10 * DEFAULT_PASS_SECONDS
FAULT_WORDS = ("illegal memory access", "Memory access fault", "HSA_STATUS_ERROR", "Aborted", "Segmentation fault")


def _load(path):
    with np.load(path, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def runs(ctx, tmp_path_factory):
    """{configuration: results dict | ("dead", why) | ("not run", why)}; "default" first, in this process"""
    assert "STRL_GRID_C" not in os.environ, "the parent runs the default grid: unset STRL_GRID_C"
    tmp = tmp_path_factory.mktemp("classify")
    out = {}
    secs = CC.run_cases(ctx, str(tmp / "default.npz"))
    out["default"] = _load(tmp / "default.npz")
    print("\nclassify cases, default grid (parent): %.2f s" % secs)
    dead = None
    for cfg in CHILDREN:
        if dead:
            out[cfg] = ("not run", "an earlier child died (%s)" % dead)
            continue
        env = dict(os.environ)
        env.update({k: str(v) for k, v in CC.CONFIGS[cfg].items()})
        path = tmp / (cfg + ".npz")
        t0 = time.perf_counter()
        try:
            p = subprocess.run([sys.executable, os.path.join(HERE, "classify_cases.py"), str(path)], env=env, timeout=CHILD_TIMEOUT,
                               stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            text, rc = p.stdout, p.returncode
        except subprocess.TimeoutExpired as e:
            text, rc = (e.stdout.decode(errors="replace") if isinstance(e.stdout, bytes) else (e.stdout or "")), "time limit of %.0f s" % CHILD_TIMEOUT
        child_secs = time.perf_counter() - t0
        print("classify cases, child %s: %.2f s, exit %s\n%s" % (cfg, child_secs, rc, "\n".join(text.splitlines()[-3:])))
        fault = [w for w in FAULT_WORDS if w in text]
        if rc != 0 or fault:
            dead = "%s: exit %s%s" % (cfg, rc, ", " + fault[0] if fault else "")
            out[cfg] = ("dead", dead + "\n" + "\n".join(text.splitlines()[-15:]))
            continue
        out[cfg] = _load(path)
        out[cfg]["child_seconds"] = child_secs
    return out


def _where(cfg, n, i):
    for w, k, a, b, kind in CC.turn_kinds(n, CC.CONFIGS.get(cfg)):
        if a <= i < b:
            return "wave %d, turn %d (%s)" % (w, k, kind)
    return "?"


@pytest.mark.parametrize("name", CC.ALL)
@pytest.mark.parametrize("cfg", ("default",) + CHILDREN)
def test_classify_case(runs, cfg, name):
    r = runs[cfg]
    if isinstance(r, tuple):
        pytest.fail("%s: %s" % r if r[0] == "not run" else "child %s" % r[1])
    if name + ".error" in r:
        pytest.fail("%s/%s: the library refused the case: %s" % (cfg, name, r[name + ".error"]))
    c, e = CC.by_name(name), CC.expected(name)
    n_skipped = int(e["skipped"].sum())
    for off, variant in ((0, "aligned: vector variant"), (1, "one element in: scalar variant")):
        what = "%s/%s (%s)" % (cfg, name, variant)
        got = r["%s.dev%d.whole" % (name, off)]
        assert got.shape == e["whole"].shape, what
        if not np.array_equal(got, e["whole"]):
            bad = np.flatnonzero(got != e["whole"])
            j = int(bad[0])
            flips = int((((got ^ e["whole"]) & 0x8000) != 0).sum())
            zero = int(((got == 0) & (e["whole"] != 0)).sum())
            raise AssertionError("%s: %d of %d words differ (%d in the skipped bit, %d kept reads never scored), first at read %d (%s): got %#x, "
                                 "expected %#x; reads %s" % (what, bad.size, c.n, flips, zero, j, _where(cfg, c.n, j), int(got[j]), int(e["whole"][j]),
                                                             bad[:8].tolist()))
        # the ids classify_kernel queued, as a set: read back from the device
        kept = np.flatnonzero(~e["skipped"]).astype(np.uint32)
        queue = np.sort(r["%s.dev%d.queue" % (name, off)])
        assert int(r["%s.dev%d.n_queue" % (name, off)]) == kept.size, what
        if not np.array_equal(queue, kept):
            miss, extra = np.setdiff1d(kept, queue), np.setdiff1d(queue, kept)
            raise AssertionError("%s: queued ids: %d missing (first %s: %s), %d unexpected (%s), %d duplicates"
                                 % (what, miss.size, miss[:4].tolist(), _where(cfg, c.n, int(miss[0])) if miss.size else "-", extra.size,
                                    extra[:4].tolist(), queue.size - np.unique(queue).size))
        st = dict(zip(CC.STAT_FIELDS, r["%s.dev%d.stats" % (name, off)].tolist()))
        assert st == dict(n_reads=c.n, n_skipped=n_skipped, n_scored=c.n - n_skipped), what


def test_every_child_ran_within_its_limit(runs):
    for cfg in CHILDREN:
        r = runs[cfg]
        assert not isinstance(r, tuple), r
        assert r["child_seconds"] < CHILD_TIMEOUT
    print("default-grid pass: %.2f s; children: %s" % (float(runs["default"]["seconds"]), ", ".join("%s %.2f s" % (c, runs[c]["child_seconds"]) for c in CHILDREN)))
