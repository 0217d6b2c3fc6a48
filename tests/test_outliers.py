"""`strling outliers`: the fifth stage (the reference's scripts/strling-outliers.py) -- kernels, C ABI and CLI.

CPU part: the restatement (tests/outliers_ref.py) reproduces the script's recorded outputs (tests/golden/outliers/) and its
Huber vectors; the CLI's help and argument / input errors, which are decided before the device is opened.
GPU part: the CLI on every recorded case, each ABI stage against the restatement on large random matrices, determinism.

Comparison rules: text and integer columns, sum_str_log, depth, method and depths.tsv equal; mu / sd within 1e-6 relative;
the '.2g' columns equal unless the exact value is within 1e-6 of a rounding boundary.  Rows whose sort keys tie are
compared as multisets (the script's tie order follows Python set / glob order; this build's is sample name, then locus).
"""
import json
import math
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import outliers_ref as R
from strling_amd import build

CLI = build.CLI
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "outliers")
RUNS = json.load(open(os.path.join(GOLD, "runs.json")))
RTOL = 1e-6
G2_COLS = ("outlier", "p", "p_adj")


def _args(run, out_dir):
    """the run's command line: input patterns, --out prefix into out_dir, extra args with @ -> golden root"""
    spec = RUNS[run]
    cdir = os.path.join(GOLD, "inputs", spec["cohort"])
    a = ["--genotypes", os.path.join(cdir, "*-genotype.txt"), "--unplaced", os.path.join(cdir, "*-unplaced.txt"),
         "--out", os.path.join(out_dir, "out_")]
    for x in spec["args"]:
        if x.startswith("@"):
            x = os.path.join(GOLD, x[1:])
        elif x == "emit.tsv":
            x = os.path.join(out_dir, "emit.tsv")
        a.append(x)
    return a


def _ref_kwargs(argv):
    kw = dict(genotypes=[], unplaced=[])
    i = 0
    while i < len(argv):
        k = argv[i]
        if k in ("--genotypes", "--unplaced"):
            kw[k[2:]].append(argv[i + 1]); i += 2
        elif k == "--debug":
            kw["debug"] = True; i += 1
        elif k in ("--min_size", "--min_clips"):
            kw[k[2:]] = int(argv[i + 1]); i += 2
        else:
            kw[k[2:]] = argv[i + 1]; i += 2
    return kw


def _expected_files(run):
    d = os.path.join(GOLD, "expected", run)
    return {f: open(os.path.join(d, f)).read() for f in sorted(os.listdir(d)) if f.endswith(".tsv") and f != "emit_old_header.tsv"}


def _g2_close(a, b, exact):
    """two '.2g' texts agree, or the exact value is within RTOL of the boundary between them"""
    if a == b:
        return True
    if exact is None or exact != exact:
        return False
    lo, hi = exact * (1 - RTOL), exact * (1 + RTOL)
    return {format(lo, ".2g"), format(hi, ".2g")} >= {a, b} or {a, b} <= {format(lo, ".2g"), format(exact, ".2g"), format(hi, ".2g")}


def _float_close(a, b):
    fa, fb = float(a or "nan"), float(b or "nan")
    if fa != fa or fb != fb:
        return fa != fa and fb != fb
    return abs(fa - fb) <= RTOL * max(abs(fa), abs(fb), 1e-300)


def compare_strs(got, exp, exact=None):
    """STRs.tsv texts: header equal, runs of equal (outlier, allele2_est) text compared as multisets, rows field by field.
    exact: {(locus, sample): {col: value}} for the '.2g' boundary rule."""
    gl, el = got.rstrip("\n").split("\n"), exp.rstrip("\n").split("\n")
    assert gl[0] == el[0], (gl[0], el[0])
    cols = el[0].split("\t")
    assert len(gl) == len(el), (len(gl), len(el))
    io, ia, il, isa = cols.index("outlier"), cols.index("allele2_est"), cols.index("locus"), cols.index("sample")

    def runs(lines):
        out, cur, key = [], [], None
        for l in lines:
            f = l.split("\t")
            k = (f[io], f[ia])
            if k != key and cur:
                out.append(cur); cur = []
            key = k
            cur.append(f)
        if cur:
            out.append(cur)
        return out

    gr, er = runs(gl[1:]), runs(el[1:])
    # run boundaries may differ only where '.2g' texts differ at a boundary: compare on the flattened, run-sorted rows
    flat = lambda rs: [r for run in rs for r in sorted(run, key=lambda f: (f[isa], f[il]))]
    gf, ef = flat(gr), flat(er)
    for g, e in zip(gf, ef):
        assert (g[isa], g[il]) == (e[isa], e[il]), (g, e)
        for c, x, y in zip(cols, g, e):
            if c in G2_COLS:
                v = None if exact is None else exact.get((e[il], e[isa]), {}).get(c)
                assert _g2_close(x, y, v), (c, x, y, v, e[il], e[isa])
            else:
                assert x == y, (c, x, y, e[il], e[isa])


def compare_emit(got, exp):
    gl, el = got.rstrip("\n").split("\n"), exp.rstrip("\n").split("\n")
    assert gl[0] == el[0] and len(gl) == len(el)
    for g, e in zip(gl[1:], el[1:]):
        g, e = g.split("\t"), e.split("\t")
        assert g[0] == e[0] and g[3] == e[3], (g, e)
        assert _float_close(g[1], e[1]) and _float_close(g[2], e[2]), (g, e)


def compare_run(got_files, exp_files, exact=None):
    assert sorted(got_files) == sorted(exp_files), (sorted(got_files), sorted(exp_files))
    for f in exp_files:
        if f.endswith("STRs.tsv"):
            compare_strs(got_files[f], exp_files[f], exact)
        elif f.startswith("emit"):
            compare_emit(got_files[f], exp_files[f])
        elif f.endswith("unplaced.tsv"):
            # the script's sample order here is Python set order; this build's is sorted: compare as multisets
            g, e = got_files[f].split("\n"), exp_files[f].split("\n")
            assert g[0] == e[0] and sorted(g[1:]) == sorted(e[1:]), f
        else:
            assert got_files[f] == exp_files[f], f


def _ref_run(run, out_dir="."):
    kw = _ref_kwargs(_args(run, "@@"))
    files = R.run(**kw)
    return {os.path.basename(k): v for k, v in files.items()}


# ---------------------------------------------------------------- CPU: the restatement against the recordings

@pytest.mark.parametrize("run", [r for r in RUNS if r != "one_locus"])
def test_restatement_reproduces_recorded_run(run):
    compare_run(_ref_run(run), _expected_files(run))


def test_restatement_one_locus():
    """the script writes unplaced.tsv and depths.tsv and then fails (KeyError: 'p', :377-386 make no 'p' column); this
    build finishes the file with p = p_adj = norm.sf(z), unadjusted, as the single-locus branch intends"""
    got = _ref_run("one_locus")
    exp = _expected_files("one_locus")
    assert open(os.path.join(GOLD, "expected", "one_locus", "rc.txt")).read().strip() == "1"
    for f in exp:
        compare_run({f: got[f]}, {f: exp[f]})
    rows = [l.split("\t") for l in got["out_STRs.tsv"].rstrip("\n").split("\n")]
    c = rows[0]
    for r in rows[1:]:
        assert r[c.index("p")] == r[c.index("p_adj")] != "nan"


def test_restatement_huber_vectors():
    vec = json.load(open(os.path.join(GOLD, "huber_vectors.json")))
    assert len(vec) >= 10
    kinds = set()
    for v in vec:
        x = np.array([float(t) for t in v["x"]])
        mu, sd, method = R.huber(x)
        kinds.add(v["kind"])
        assert method == v["method"], v
        emu, esd = float(v["mu"]), float(v["sd"])
        assert _float_close(repr(mu), repr(emu)) and _float_close(repr(sd), repr(esd)), (v, mu, sd)
    assert {"huber", "two_values", "mad_zero", "den_le_zero", "one_value", "overflow"} <= kinds, kinds


def test_bh_restatement_small():
    """fdrcorrection by hand: ties share the adjusted value, NaN passes through, the clip at 1"""
    p = np.array([0.01, np.nan, 0.04, 0.04, 1.0, 0.0])
    got = R.bh(p)
    assert np.isnan(got[1])
    assert got[2] == got[3] == pytest.approx(0.05)
    assert got[5] == 0.0 and got[4] == 1.0
    assert got[0] == pytest.approx(0.01 * 5 / 2)


# ---------------------------------------------------------------- CPU: the CLI before the device

def _cli(args, **kw):
    return subprocess.run([CLI, "outliers"] + args, capture_output=True, text=True, **kw)


def test_outliers_help():
    assert os.path.exists(CLI), "strling CLI not built (python -m strling_amd.build)"
    r = _cli(["-h"])
    assert r.returncode == 0, r.stderr
    assert r.stdout.startswith("usage: strling outliers")
    for opt in ("--genotypes", "--unplaced", "--out", "--control", "--emit", "--slop", "--min_clips", "--min_size", "--debug", "-v"):
        assert opt in r.stdout, opt
    top = subprocess.run([CLI], capture_output=True, text=True)
    assert "outliers" in top.stdout


def test_outliers_missing_unplaced_file(tmp_path):
    src = os.path.join(GOLD, "inputs", "basic")
    for f in os.listdir(src):
        if f != "S4-unplaced.txt":
            shutil.copy(os.path.join(src, f), tmp_path / f)
    r = _cli(["--genotypes", str(tmp_path / "*-genotype.txt"), "--unplaced", str(tmp_path / "*-unplaced.txt"),
              "--out", str(tmp_path / "o_")])
    assert r.returncode == 1
    assert "ERROR: One or more files are missing for sample(s): S4" in r.stderr
    assert not os.path.exists(tmp_path / "o_STRs.tsv")


def test_outliers_argument_errors(tmp_path):
    r = _cli(["--unplaced", "x"])
    assert r.returncode == 2 and "--genotypes" in r.stderr            # argparse: required arguments
    r = _cli(["--genotypes", "a", "--unplaced", "b", "--min_size", "x"])
    assert r.returncode == 2 and "invalid int value" in r.stderr
    empty = tmp_path / "E-genotype.txt"
    empty.write_text("")
    (tmp_path / "E-unplaced.txt").write_text("AT\t3\n")
    r = _cli(["--genotypes", str(empty), "--unplaced", str(tmp_path / "E-unplaced.txt"), "--out", str(tmp_path / "o_")])
    assert r.returncode == 1 and f"ERROR: file {empty} was empty." in r.stderr
    r = _cli(["--genotypes", str(tmp_path / "none*"), "--unplaced", str(tmp_path / "none*")])
    assert r.returncode == 1 and "No objects to concatenate" in r.stderr


# ---------------------------------------------------------------- GPU: the CLI on every recorded case

def _cli_files(tmp_path, run, extra=()):
    out = tmp_path / run
    out.mkdir()
    r = _cli(_args(run, str(out)) + list(extra))
    assert r.returncode == 0, r.stderr
    return {f: open(out / f).read() for f in sorted(os.listdir(out)) if f.endswith(".tsv")}, r


@pytest.mark.gpu
@pytest.mark.parametrize("run", list(RUNS))
def test_cli_recorded_run(tmp_path, run):
    got, _ = _cli_files(tmp_path, run)
    exact = {}
    ref = R.run(**_ref_kwargs(_args(run, "@@")), values=exact)
    ref = {os.path.basename(k): v for k, v in ref.items()}
    exp = _expected_files(run)
    if run == "one_locus":     # the script stops before STRs.tsv (see test_restatement_one_locus): the restatement stands in
        exp = dict(ref, **exp)
    compare_run(got, exp, exact)
    # and against the restatement itself, which fixes this build's tie order: equal texts outside the '.2g' boundary rule
    compare_run(got, ref, exact)


@pytest.mark.gpu
def test_cli_verbose_changes_no_file(tmp_path):
    a, r = _cli_files(tmp_path, "basic", ["-v"])
    assert '"huber"' in r.stderr and '"parse"' in r.stderr and '"format / write"' in r.stderr
    (tmp_path / "again").mkdir()
    b, _ = _cli_files(tmp_path / "again", "basic")
    assert a == b      # and two runs give the same bytes


# ---------------------------------------------------------------- GPU: the ABI stages on large random matrices

def _matrix(rows, cols, seed):
    """NaN holes, ties, constant rows, single-value rows, heavy outliers, rows that fall back (MAD = 0, den <= 0)"""
    rng = np.random.default_rng(seed)
    x = rng.normal(-2.0, 0.5, (rows, cols))
    x[rng.random((rows, cols)) < 0.05] = np.nan
    x[:, : cols // 3] = np.round(x[:, : cols // 3], 1)                        # many ties
    out = rng.random((rows, cols)) < 0.002
    x[out] = rng.normal(0, 1, out.sum()) * 1e3                                 # heavy outliers
    k = rows // 50
    x[0:k] = 1.25                                                              # constant rows
    x[k:2 * k, 1:] = np.nan                                                    # single finite value
    x[2 * k:3 * k, : cols // 2 + 1] = -3.0                                     # more than half equal: MAD = 0
    x[3 * k:4 * k, 3:] = np.nan                                                # three values ...
    x[3 * k:4 * k, 2] = 40.0                                                   # ... one far: den <= 0
    x[4 * k] = np.nan                                                          # an empty row
    return x


@pytest.fixture(scope="module")
def ctx():
    from strling_amd import api
    c = api.Context(0)
    yield c
    c.close()


def _close(a, b, rtol=RTOL):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    both = np.isnan(a) & np.isnan(b)
    ok = both | (np.abs(a - b) <= rtol * np.maximum(np.abs(a), np.abs(b)))
    return bool(ok.all()), np.flatnonzero(~ok)[:5]


@pytest.mark.gpu
def test_abi_row_medians(ctx):
    x = _matrix(1500, 20000, 1)[:, :]
    x[5] = np.nan
    keep = (np.arange(x.shape[1]) % 7 != 0).astype(np.uint8)
    xz = x.copy()
    xz[:, ::11] = 0.0
    a, b, c = ctx.outliers_row_medians(xz, keep)
    with np.errstate(all="ignore"):
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            ea = np.nanmedian(xz, axis=1)
            k = xz[:, keep.astype(bool)].copy()
            k[k == 0] = np.nan
            eb = np.nanmedian(k, axis=1)
            kf = np.where(np.isnan(k), eb[:, None], k)
            ec = np.nanmedian(kf, axis=1)
    for g, e in ((a, ea), (b, eb), (c, ec)):
        assert np.array_equal(g, e, equal_nan=True), np.flatnonzero(~((g == e) | (np.isnan(g) & np.isnan(e))))[:5]


def _huber_check(ctx, x, rows):
    mu, sd, m = ctx.outliers_huber(x)
    for r in rows:
        emu, esd, em = R.huber(x[r])
        assert m[r] == em, (r, m[r], em)
        ok, _ = _close([mu[r], sd[r]], [emu, esd])
        assert ok, (r, mu[r], sd[r], emu, esd)
    return mu, sd, m


@pytest.mark.gpu
def test_abi_huber_lds_and_wide_paths(ctx):
    x = _matrix(20000, 1500, 2)
    k = 20000 // 50
    rng = np.random.default_rng(3)
    rows = sorted(set(range(0, 5 * k, 37)) | set(rng.integers(0, 20000, 400).tolist()) | {4 * k})
    mu, sd, m = _huber_check(ctx, x, rows)
    assert set(m[:k]) == {"MAD"} and np.isnan(sd[:k]).all()                   # constant rows: MAD = 0 -> NaN
    assert list(m[2 * k:4 * k]) == [R.huber(x[r])[2] for r in range(2 * k, 4 * k)]      # every edge row's method
    assert (m[2 * k:3 * k] == "MAD").all()                                   # MAD = 0
    assert (m == "Huber").sum() > 15000
    # the same rows through the global-memory path (forced), then rows wider than LDS
    env = dict(os.environ, STRL_OUTLIERS_WIDE="1")
    code = ("import numpy as np, sys; from strling_amd import api; x = np.load(sys.argv[1]); c = api.Context(0); "
            "mu, sd, m = c.outliers_huber(x); np.save(sys.argv[2], np.stack([mu, sd, (m == 'MAD').astype(float)]))")
    d = os.path.join(os.environ.get("TMPDIR", "/tmp"), f"huber_wide_{os.getpid()}")
    os.makedirs(d, exist_ok=True)
    sub = x[:4000]
    np.save(os.path.join(d, "x.npy"), sub)
    root = os.path.dirname(os.path.dirname(os.path.dirname(GOLD)))
    r = subprocess.run([sys.executable, "-c", code, os.path.join(d, "x.npy"), os.path.join(d, "y.npy")], env=env, capture_output=True,
                       text=True, cwd=root, timeout=600)
    assert r.returncode == 0, r.stderr
    y = np.load(os.path.join(d, "y.npy"))
    shutil.rmtree(d)
    assert np.array_equal(y[2] == 1, m[:4000] == "MAD")
    ok, bad = _close(y[0], mu[:4000])
    assert ok, bad
    ok, bad = _close(y[1], sd[:4000])
    assert ok, bad
    w = _matrix(200, 10000, 4)
    _huber_check(ctx, w, list(range(0, 200, 3)))


@pytest.mark.gpu
def test_abi_scores_bh(ctx):
    rng = np.random.default_rng(5)
    L, S = 20000, 1500
    x = _matrix(L, S, 6)
    mu = rng.normal(-2, 0.2, L)
    sd = np.abs(rng.normal(0.5, 0.1, L))
    sd[::97] = np.nan
    z, p, q = ctx.outliers_scores(x, mu, sd)
    with np.errstate(all="ignore"):
        ez = (x - mu[:, None]) / sd[:, None]
    assert np.array_equal(z, ez, equal_nan=True)
    ok, bad = _close(p, R.norm_sf(ez))
    assert ok, bad
    cols = list(range(0, S, 7))
    for c in cols:
        ok, bad = _close(q[:, c], R.bh(p[:, c]))
        assert ok, (c, bad)


@pytest.mark.gpu
def test_abi_bh_ties_edges_and_null_rows(ctx):
    """p = 0 (z huge), p = 1 (z = -inf), ties, NaN, and control-only rows that count in each column's BH"""
    x = np.array([[50.0, 1.0, np.nan], [1.0, 1.0, 0.5], [-np.inf, 1.0, 0.5], [2.0, 3.0, 0.5], [0.3, -1.0, 0.5]])
    mu, sd = np.zeros(5), np.ones(5)
    null_x = np.array([0.7, 2.5, 0.1])
    null_mu, null_sd = np.array([0.0, 0.1, 0.2]), np.array([1.0, 1.0, 2.0])
    z, p, q = ctx.outliers_scores(x, mu, sd, null_x, null_mu, null_sd)
    zn = (null_x[None, :] - null_mu[:, None]) / null_sd[:, None]
    full = np.vstack([R.norm_sf(x), R.norm_sf(zn)])
    for c in range(3):
        ok, bad = _close(q[:, c], R.bh(full[:, c])[:5])
        assert ok, (c, q[:, c], R.bh(full[:, c]))
    assert p[0, 0] == 0.0 and q[0, 0] == 0.0 and p[2, 0] == 1.0
    assert q[1, 1] == q[2, 1]                       # tied p share their adjusted value
    # without null_x the control-only rows are NaN and change nothing (what the CLI passes, as the script does)
    z2, p2, q2 = ctx.outliers_scores(x, mu, sd, None, null_mu, null_sd)
    z3, p3, q3 = ctx.outliers_scores(x, mu, sd)
    assert np.array_equal(q2, q3, equal_nan=True)


@pytest.mark.gpu
def test_abi_order_large(ctx):
    rng = np.random.default_rng(8)
    L, S = 20000, 1000
    z = np.round(rng.normal(0, 1, (L, S)), 1)               # many ties in the primary key
    z[rng.random((L, S)) < 0.05] = np.nan
    a2 = np.round(rng.normal(30, 5, (L, S)), 0)
    a2[rng.random((L, S)) < 0.05] = np.nan
    z[0, 0] = -0.0
    o = ctx.outliers_order(z, a2)
    # the rule: outlier desc, allele2_est desc, NaN last; ties by sample (column), then locus (row)
    r, c = np.divmod(np.arange(L * S), S)
    zf, af = z.ravel(), a2.ravel()
    zk = np.where(np.isnan(zf), np.inf, -zf)
    ak = np.where(np.isnan(af), np.inf, -af)
    zk[zk == 0] = 0.0
    e = np.lexsort((r, c, ak, zk))
    assert np.array_equal(o, e.astype(np.uint32))
    assert np.array_equal(ctx.outliers_order(z, a2), o)


@pytest.mark.gpu
def test_abi_two_runs_same_bits(ctx):
    x = _matrix(3000, 1500, 9)
    a = ctx.outliers_huber(x)
    b = ctx.outliers_huber(x)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and np.array_equal(a[2], b[2])
    mu, sd = np.nan_to_num(a[0]), np.where(np.isnan(a[1]), 1.0, a[1])
    s1 = ctx.outliers_scores(x, mu, sd)
    s2 = ctx.outliers_scores(x, mu, sd)
    assert all(u.tobytes() == v.tobytes() for u, v in zip(s1, s2))
