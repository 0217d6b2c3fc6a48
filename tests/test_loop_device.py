"""The loop-carried state of the streaming kernels, on the device (-m gpu): every case of tests/loop_cases.py under grids so small
that every wave, lane and block takes several turns of its loop, against the oracle.  Equality is exact everywhere.

The grid variables are read once per process, so a configuration is a child process (tests/loop_child.py): `one` (every grid one
block), `odd` (A=3, B=2, C=2, P=3, K=2: other wave ranges, strides and rounds) and `split` (`one` with the three-launch segment
scorer).  The parent runs the same cases under the default grids, which tells a wrong case from a wrong loop, and compares
everything.  tests/test_loop_cases.py shows on the CPU that the cases reach their edges under these configurations.

The children run in order from one module-scoped fixture.  A child that ends by a signal, at its time limit, or with a HIP fault
in its output is the last one started: the card is handed nothing more, and the tests of the configurations behind it fail
with "not run: an earlier child died".
"""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import loop_cases as LC
import loop_child
from helpers import treads_equal
from strling_amd.records import unpack_result

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
CHILDREN = ("one", "odd", "split")
# The default-grid pass over all cases, measured once on an MI355X in the parent process (warm context): DEFAULT_PASS_SECONDS.  A
# child gets ten times that, for its whole life (interpreter start, library load, oracle included).
DEFAULT_PASS_SECONDS = 2.0
CHILD_TIMEOUT = 10 * DEFAULT_PASS_SECONDS
FAULT_WORDS = ("illegal memory access", "Memory access fault", "HSA_STATUS_ERROR", "Aborted", "Segmentation fault")


def _load(path):
    with np.load(path, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def runs(ctx, tmp_path_factory):
    """{configuration: results dict | ("dead", why) | ("not run", why)}; "default" first, in this process"""
    assert not [v for v in LC.GRID_VARS if v in os.environ], "the parent compares against the default grids: unset " + ", ".join(LC.GRID_VARS)
    tmp = tmp_path_factory.mktemp("loop")
    out = {}
    t0 = time.perf_counter()
    loop_child.run_cases(ctx, str(tmp / "default.npz"))
    out["default"] = _load(tmp / "default.npz")
    print("\nloop cases, default grids (parent): %.2f s" % (time.perf_counter() - t0))
    dead = None
    for cfg in CHILDREN:
        if dead:
            out[cfg] = ("not run", "an earlier child died (%s)" % dead)
            continue
        env = {k: v for k, v in os.environ.items() if k not in LC.GRID_VARS}
        env.update({k: str(v) for k, v in LC.CONFIGS[cfg].items()})
        path = tmp / (cfg + ".npz")
        t0 = time.perf_counter()
        try:
            p = subprocess.run([sys.executable, os.path.join(HERE, "loop_child.py"), str(path)], env=env, timeout=CHILD_TIMEOUT,
                               stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            text, rc = p.stdout, p.returncode
        except subprocess.TimeoutExpired as e:
            text, rc = (e.stdout.decode(errors="replace") if isinstance(e.stdout, bytes) else (e.stdout or "")), "time limit of %.0f s" % CHILD_TIMEOUT
        secs = time.perf_counter() - t0
        print("loop cases, child %s: %.2f s, exit %s\n%s" % (cfg, secs, rc, "\n".join(text.splitlines()[-3:])))
        fault = [w for w in FAULT_WORDS if w in text]
        if rc != 0 or fault:
            dead = "%s: exit %s%s" % (cfg, rc, ", " + fault[0] if fault else "")
            out[cfg] = ("dead", dead + "\n" + "\n".join(text.splitlines()[-15:]))
            continue
        out[cfg] = _load(path)
        out[cfg]["child_seconds"] = secs
    return out


def _word(w):
    unit, count, skipped = unpack_result(w)
    return "%s x %d%s" % (unit or "-", count, " (skipped)" if skipped else "")


def _where(cfg, n, i):
    """wave and turn of classify_kernel that handle read i under the configuration"""
    its = LC.Model().iterations(n, "C", LC.CONFIGS.get(cfg))
    for w, turns in enumerate(its):
        for k, (a, b) in enumerate(turns):
            if a <= i < b:
                return "classify wave %d, turn %d of %d" % (w, k, len(turns))
    return "?"


def _same_words(got, exp, what, cfg, n):
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    if not np.array_equal(got, exp):
        bad = np.flatnonzero(got != exp)
        j = int(bad[0])
        flips = int((((got ^ exp) & 0x8000) != 0).sum())
        raise AssertionError("%s: %d of %d words differ (%d in the skipped bit), first at read %d (%s): got %s, expected %s; reads %s"
                             % (what, bad.size, n, flips, j, _where(cfg, n, j), _word(got[j]), _word(exp[j]), bad[:8].tolist()))


def _same_soft(got, e, what):
    if not np.array_equal(got["read_side"], e["soft_side"]):
        g, x = set(got["read_side"].tolist()), set(e["soft_side"].tolist())
        raise AssertionError("%s: soft records of %d read sides, expected %d; missing %s, unexpected %s, %d duplicates"
                             % (what, len(got), len(x), sorted(x - g)[:6], sorted(g - x)[:6], len(got) - len(g)))
    for f, k in (("res_first", "soft_first"), ("res_after", "soft_after")):
        if not np.array_equal(got[f], e[k]):
            bad = np.flatnonzero(got[f] != e[k])
            j = int(bad[0])
            raise AssertionError("%s: %s differs in %d of %d soft records, first at read %d side %d (segment of %d bases): got %s, expected %s"
                                 % (what, f, bad.size, len(got), int(got["read_side"][j]) >> 1, int(got["read_side"][j]) & 1, int(got["seg_len"][j]),
                                    _word(got[f][j]), _word(e[k][j])))


def _same_stats(st, e, n, what):
    got = dict(zip(loop_child.STAT_FIELDS, st.tolist()))
    want = dict(n_reads=n, n_skipped=int(e["skipped"].sum()), n_scored=n - int(e["skipped"].sum()), n_soft_items=len(e["items"]))
    assert {k: got[k] for k in want} == want, what
    return got


@pytest.mark.parametrize("name", LC.ALL_CASES)
@pytest.mark.parametrize("cfg", ("default",) + CHILDREN)
def test_loop_case(runs, cfg, name):
    r = runs[cfg]
    if isinstance(r, tuple):
        pytest.fail("%s: %s" % r if r[0] == "not run" else "child %s" % r[1])
    if name + ".error" in r:
        pytest.fail("%s/%s: the library refused the case: %s" % (cfg, name, r[name + ".error"]))
    c, e = LC.case(name), LC.expected(name)
    n = c.rec.n
    what = "%s/%s" % (cfg, name)
    _same_words(r[name + ".whole"], e["whole"], what, cfg, n)
    _same_soft(r[name + ".soft"], e, what)
    st = _same_stats(r[name + ".stats"], e, n, what)
    if name in LC.SKIP_CASES:
        for off, variant in ((0, "resident, aligned: vector variant"), (1, "resident, one element in: scalar variant")):
            w = "%s (%s)" % (what, variant)
            _same_words(r["%s.dev%d.whole" % (name, off)], e["whole"], w, cfg, n)
            _same_soft(r["%s.dev%d.soft" % (name, off)], e, w)
            _same_stats(r["%s.dev%d.stats" % (name, off)], e, n, w)
    if name in LC.EXTRACT_CASES:
        ok, why = treads_equal(r[name + ".treads"], e["treads"])
        assert ok, "%s: treads in .bin order: %s" % (what, why)
        _same_stats(r[name + ".extract_stats"], e, n, what + " (extract)")
    if name in LC.PAIR_CASES:
        msg = str(r[name + ".capacity_error"])
        assert "error -4" in msg and "join items" in msg, "%s: item_cap %d, one below the hot reads: %s" % (what, int(r[name + ".capacity"]), msg)
    if cfg != "default" and name in LC.SCORER_CASES:
        # stage B took more than one turn per lane as well (the device's own count of stage A's survivors)
        m = LC.Model()
        gb, block = m.score_grid(n, c.meta["max_l"], "B", LC.CONFIGS[cfg])
        assert st["n_stage_b_whole"] >= 2 * gb * block, (what, st)
        if c.meta["max_l"] > 160 or cfg == "split":
            assert st["n_stage_b_soft"] >= 2 * gb * block, (what, st)


def test_every_child_ran_within_its_limit(runs):
    for cfg in CHILDREN:
        r = runs[cfg]
        assert not isinstance(r, tuple), r
        assert r["child_seconds"] < CHILD_TIMEOUT
    d = dict(zip(runs["default"]["seconds_of"].tolist(), runs["default"]["seconds"].tolist()))
    print("default-grid pass: %.2f s; children: %s" % (d["total"], ", ".join("%s %.2f s" % (c, runs[c]["child_seconds"]) for c in CHILDREN)))
