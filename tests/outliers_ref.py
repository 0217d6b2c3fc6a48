"""A numpy + scipy restatement of the reference's outliers script (scripts/strling-outliers.py, "the script" below).

Test infrastructure only: the tests pin it to the recorded outputs of the script under tests/golden/outliers/, and then hold
`strling outliers` and the C ABI stages (csrc/outliers.hip) against it.  Nothing under strling_amd/ imports it.  Line numbers
cite the script.

The script's data flow, restated on dense matrices: loci (rows, in the pivot's sorted order) x samples (columns, sorted).
"""
import glob as _glob
import math
import os

import numpy as np

try:
    from scipy.special import ndtr as _ndtr
except ImportError:          # norm.sf(z) = ndtr(-z) = erfc(z / sqrt 2) / 2
    _ndtr = None

HUBER_C = 1.5                                   # statsmodels Huber(c=1.5, tol=1e-8), hubers_est :118 (maxiter=1000)
HUBER_TOL = 1.0e-08
HUBER_MAXITER = 1000
HUBER_GAMMA = float.fromhex("0x1.8e92fe2915f98p-1")   # Huber.gamma: tmp + c^2 (1 - tmp) - 2 c pdf(c), tmp = 2 cdf(c) - 1
MAD_C = 0.6744897501960817                      # robust.mad's c = norm.ppf(3/4)

OUT_COLS = ["chrom", "left", "right", "locus", "sample", "repeatunit", "allele1_est", "allele2_est", "spanning_reads",
            "spanning_pairs", "left_clips", "right_clips", "unplaced_pairs", "sum_str_counts", "sum_str_log", "depth",
            "outlier", "p", "p_adj"]                                                            # :438-445
INT_COLS = ["left", "right", "sum_str_counts", "spanning_reads", "spanning_pairs", "left_clips", "right_clips",
            "unplaced_pairs"]                                                                   # :457-458
NA_TOKENS = {"", "nan", "NaN", "NA", "N/A", "NULL", "null", "n/a", "-nan", "-NaN", "#N/A", "<NA>", "None", "1.#QNAN", "#NA",
             "#N/A N/A", "-1.#QNAN", "-1.#IND", "1.#IND"}     # pandas read_csv's default NA strings


class ScriptExit(Exception):
    """what the script ends with instead of its outputs (sys.exit(message) or an exception)"""


# ---------------------------------------------------------------- statistics

def median(x):
    """np.median of a NaN-free 1-D array: the middle value, or the mean of the two middle values"""
    x = np.sort(np.asarray(x, dtype=np.float64))
    n = x.size
    if n == 0:
        return math.nan
    h = n // 2
    return float(x[h]) if n % 2 else float((x[h - 1] + x[h]) / 2.0)   # np.mean of the two: (a + b) / 2


def mad(x):
    """robust.mad(x): median(|x - median(x)| / c), the division first (scale.py mad)"""
    return median(np.abs(x - median(x)) / MAD_C)


def huber(x):
    """hubers_est :115-136 -- (mu, sd, method).  NaNs dropped; statsmodels Huber(maxiter=1000) under warnings-as-errors:
    a numpy divide / invalid / overflow event anywhere, or no convergence, falls back to (median, mad, 'MAD');
    sd == 0 becomes NaN."""
    x = np.asarray(x, dtype=np.float64)
    x = x[~np.isnan(x)]                                                                         # :120
    if x.size == 0:
        return math.nan, math.nan, "MAD"      # the script dies here (np.median of an empty array warns inside the handler)
    try:
        with np.errstate(divide="raise", invalid="raise", over="raise", under="ignore"):
            mu, s = _huber_loop(x)
        method = "Huber"
    except (FloatingPointError, ValueError):                                                    # :128-132
        mu, s, method = median(x), mad(x), "MAD"
    if s == 0:                                                                                  # :133-134
        s = math.nan
    return float(mu), float(s), method


def _huber_loop(a):
    """statsmodels Huber._estimate_both with est_mu, norm=None (scale.py), elementwise as numpy evaluates it"""
    c = HUBER_C
    n = a.size - 1
    mu = np.float64(median(a))
    scale = np.float64(mad(a))
    for _ in range(HUBER_MAXITER):
        nmu = np.clip(a, mu - c * scale, mu + c * scale).sum() / a.size
        subset = np.less_equal(np.abs((a - mu) / scale), c)
        card = subset.sum()
        num = np.sum(subset * (a - nmu) ** 2)
        den = n * HUBER_GAMMA - (a.size - card) * c ** 2
        nscale = np.sqrt(num / den)
        if np.abs(scale - nscale) <= nscale * HUBER_TOL and np.abs(mu - nmu) <= nscale * HUBER_TOL:
            return nmu, nscale
        mu, scale = nmu, nscale
    raise ValueError("no convergence")


def norm_sf(z):
    """scipy.stats.norm.sf"""
    z = np.asarray(z, dtype=np.float64)
    if _ndtr is not None:
        return _ndtr(-z)
    return np.vectorize(lambda v: 0.5 * math.erfc(v / math.sqrt(2.0)) if v == v else math.nan)(z)


def bh(p):
    """p_adj_bh :143-168: statsmodels fdr_bh over the finite values of one column; the rest passes through"""
    p = np.asarray(p, dtype=np.float64)
    out = p.copy()
    m = np.isfinite(p)
    if not m.any():
        return out
    v = p[m]
    o = np.argsort(v, kind="stable")
    vs = v[o]
    k = vs.size
    raw = vs / (np.arange(1, k + 1) / float(k))                    # multitest fdrcorrection: p_sorted / ecdf
    adj = np.minimum.accumulate(raw[::-1])[::-1]
    adj[adj > 1] = 1
    r = np.empty_like(adj)
    r[o] = adj
    out[m] = r
    return out


# ---------------------------------------------------------------- formatting

def fmt_float(x):
    """pandas to_csv of a float64 cell: repr, NaN as 'NaN' (na_rep)"""
    return "NaN" if x != x else repr(float(x))


def fmt_g2(x):
    """format(x, '.2g') :453-455"""
    return format(float(x), ".2g")


def round1(x):
    """DataFrame.round({'sum_str_log': 1}) :456 -- numpy's round: rint(x * 10) / 10"""
    return np.rint(np.asarray(x, dtype=np.float64) * 10.0) / 10.0


# ---------------------------------------------------------------- input

def get_sample(path):
    """:64-67"""
    return os.path.basename(path).rsplit("-", 1)[0]


def glob_list(patterns):
    """:170-175 (this build expands each pattern with glob(3): sorted)"""
    out = []
    for p in patterns:
        out.extend(sorted(_glob.glob(p)))
    return out


def _num(tok):
    return math.nan if tok in NA_TOKENS else float(tok)


def _is_int_token(tok):
    t = tok[1:] if tok[:1] in "+-" else tok
    return t.isdigit()


def read_table(path):
    """whitespace-separated table -> (header tokens, rows of tokens); raises ScriptExit like :75-76 / :87-90 on empty input"""
    with open(path) as f:
        lines = [l.split() for l in f.read().split("\n")]
    lines = [l for l in lines if l]
    return lines


def parse_genotypes(path):
    rows = read_table(path)
    if not rows:
        raise ScriptExit("ERROR: file {0} was empty.\n".format(path))                       # :87-88
    head = ["chrom" if h == "#chrom" else h for h in rows[0]]
    if len(rows) == 1:
        raise ScriptExit("ERROR: file {0} contained 0 loci.\n".format(path))                # :89-90
    return head, rows[1:]


# ---------------------------------------------------------------- the script

def run(genotypes, unplaced, out="", control="", emit="", min_clips=0, min_size=0, debug=False, values=None):
    """the script's main() :177-475 over the given patterns; returns {file name: text} of everything it writes (the tie
    order of this build: sample name, then locus).  Raises ScriptExit where the script stops.  values (a dict): receives
    {(locus, sample): {'outlier': z, 'p': p, 'p_adj': p_adj}} unrounded."""
    files = {}
    gfiles, ufiles = glob_list(genotypes), glob_list(unplaced)
    gids, uids = {get_sample(f) for f in gfiles}, {get_sample(f) for f in ufiles}
    if gids != uids:                                                                            # :197-202
        alls = gids | uids
        missing = (alls - gids) | (alls - uids)
        raise ScriptExit("ERROR: One or more files are missing for sample(s): " + " ".join(sorted(missing)))
    if not ufiles:
        raise ScriptExit("No objects to concatenate")                                          # pd.concat of nothing :211
    samples = sorted(gids)
    S = len(samples)
    sidx = {s: i for i, s in enumerate(samples)}

    # ---- unplaced :211-230: pivot (repeatunit x sample), fillna(0), melt; float when the pivot made holes
    ucnt = {}
    ufloat = False
    for f in ufiles:
        rows = read_table(f)
        if not rows:
            raise ScriptExit("ERROR: file {0} was empty.\n".format(f))
        s = get_sample(f)
        for r in rows:
            tok = r[1] if len(r) > 1 else ""
            ufloat |= not _is_int_token(tok)
            ucnt[(r[0], s)] = _num(tok)
    units = sorted({u for u, _ in ucnt})
    ufloat |= len(ucnt) < len(units) * S
    lines = ["repeatunit\tsample\tunplaced_count"]
    for s in samples:
        for u in units:
            v = ucnt.get((u, s), 0.0)
            lines.append(f"{u}\t{s}\t{fmt_float(v) if ufloat else str(int(v))}")
    files[out + "unplaced.tsv"] = "\n".join(lines) + "\n"

    # ---- genotypes :235-242
    cells = {}          # (locus, sample) -> dict of column -> token
    depth_all = [[] for _ in range(S)]
    for f in gfiles:
        head, rows = parse_genotypes(f)
        s = get_sample(f)
        for r in rows:
            d = dict(zip(head, r))
            loc = f"{d['chrom']}-{d['left']}-{d['right']}-{d['repeatunit']}"               # :242
            cells[(loc, s)] = d
            depth_all[sidx[s]].append(_num(d["depth"]))
    # :247-249 median depth per sample over every row of its file
    m0 = [median([v for v in depth_all[i] if v == v]) for i in range(S)]
    files[out + "depths.tsv"] = "depth\tsample\n" + "".join(f"{fmt_float(m0[i])}\t{samples[i]}\n" for i in range(S))

    loci_all = sorted({l for l, _ in cells})
    ssc = np.full((len(loci_all), S), np.nan)
    lidx_all = {l: i for i, l in enumerate(loci_all)}
    for (l, s), d in cells.items():
        ssc[lidx_all[l], sidx[s]] = _num(d["sum_str_counts"])
    keep = ~np.all(np.isnan(ssc) | (ssc == 0), axis=1)                                          # :260-262
    loci = [l for l, k in zip(loci_all, keep) if k]
    L = len(loci)
    X = ssc[keep]
    dep = np.full((L, S), np.nan)
    for j, l in enumerate(loci):
        for i, s in enumerate(samples):
            d = cells.get((l, s))
            if d is not None:
                dep[j, i] = _num(d["depth"])
    dep[dep == 0] = np.nan                                                                      # :280
    m1 = np.array([median(c[~np.isnan(c)]) for c in dep.T])                                     # :281-282
    depf = np.where(np.isnan(dep), m1[None, :], dep)
    with np.errstate(all="ignore"):
        ssl = np.log2((X + 1) / depf)                                                           # :290
    m2 = np.array([median(c[~np.isnan(c)]) for c in depf.T])                                    # :296
    with np.errstate(all="ignore"):
        null_vals = np.log2(1 / m2)                                                             # :298
    null_mu, null_sd, _ = huber(null_vals)                                                      # :300

    est = [huber(ssl[j]) for j in range(L)]                                                     # :312
    mu = np.array([e[0] for e in est])
    sd = np.array([e[1] for e in est])
    method = [e[2] for e in est]
    if emit:                                                                                    # :329-336
        lines = ["locus\tmu\tsd\tn"]
        ef = lambda v: "" if v != v else repr(float(v))
        for j in range(L):
            lines.append(f"{loci[j]}\t{ef(mu[j])}\t{ef(sd[j])}\t{S}")
        lines.append(f"null_locus_counts\t{ef(null_mu)}\t{ef(null_sd)}\t{S}")
        files[emit] = "\n".join(lines) + "\n"

    n_null = 0
    if control:                                                                                 # :340-351
        rows = read_table(control)
        cols = rows[0][1:]                  # index_col=0
        if not (len(cols) >= 2 and cols[0] in ("mu", "median") and cols[1] in ("sd", "SD")):
            raise ScriptExit("The column names in the control file don't look right, expecting columns named median, SD "
                             "or mu, sd. Column names are " + str(cols) + ". Check the file: " + control)
        ctl = {}
        for r in rows[1:]:
            ctl[r[0]] = (_num(r[1]) if len(r) > 1 else math.nan, _num(r[2]) if len(r) > 2 else math.nan)
        if "null_locus_counts" not in ctl:
            raise ScriptExit("KeyError: 'null_locus_counts'")
        cnull = ctl["null_locus_counts"]
        kept = set(loci)
        n_null = sum(1 for l in ctl if l != "null_locus_counts" and l not in kept)              # :344-345
        use_mu = np.array([ctl.get(l, cnull)[0] for l in loci])
        use_sd = np.array([ctl.get(l, cnull)[1] for l in loci])
        use_mu = np.where(np.isnan(use_mu), cnull[0], use_mu)                                   # fillna :350-351
        use_sd = np.where(np.isnan(use_sd), cnull[1], use_sd)
    else:
        use_mu, use_sd = mu, sd
    with np.errstate(all="ignore"):
        z = (ssl - use_mu[:, None]) / use_sd[:, None]                                           # :359, z_score :141
    # :364-373: the control-only loci join z as rows of NaN (the fillna at :368 aligns a sample-indexed frame on the
    # loci axis and fills nothing), so they are counted in no sample's BH
    if L + n_null == 0:
        raise ScriptExit("ValueError: z score table is empty")                                  # :432-433
    p = norm_sf(z)                                                                              # :381 / :395
    if L + n_null == 1:
        padj = p.copy()                     # :377-386 one locus: no adjustment (the script then fails to find a 'p' column)
    elif np.all(np.isnan(p)):
        padj = p.copy()                                                                         # :398-399
    else:
        padj = np.column_stack([bh(p[:, i]) for i in range(S)]) if L else p.copy()              # :402
    if values is not None:
        for j, l in enumerate(loci):
            for i, sn in enumerate(samples):
                values[(l, sn)] = {"outlier": float(z[j, i]), "p": float(p[j, i]), "p_adj": float(padj[j, i])}
    return _write(files, out, loci, samples, cells, X, ssl, depf, z, p, padj, method, min_clips, min_size, debug)


def order_key(outlier, allele2):
    """sort_values(['outlier', 'allele2_est'], ascending=False) :451, NaN last"""
    return (1 if outlier != outlier else 0, -outlier if outlier == outlier else 0.0,
            1 if allele2 != allele2 else 0, -allele2 if allele2 == allele2 else 0.0)


def _write(files, out, loci, samples, cells, X, ssl, depf, z, p, padj, method, min_clips, min_size, debug):
    L, S = len(loci), len(samples)
    cols = OUT_COLS + (["method"] if debug else [])
    recs = []
    for i, s in enumerate(samples):          # tie order: sample name, then locus
        for j, l in enumerate(loci):
            d = cells.get((l, s))
            a2 = _num(d["allele2_est"]) if d else math.nan
            recs.append((order_key(float(z[j, i]), a2), j, i, d, a2))
    recs.sort(key=lambda r: r[0])
    rows = []
    for _, j, i, d, a2 in recs:
        l, s = loci[j], samples[i]
        get = lambda c: d[c] if d else None
        intc = lambda c: "NaN" if d is None or d[c] in NA_TOKENS else str(int(float(d[c])))
        fl = lambda c: "NaN" if d is None else fmt_float(_num(d[c]))
        v = {
            "chrom": d["chrom"] if d else "NaN",
            "left": intc("left") if d else "0", "right": intc("right") if d else "0",            # fillna(0) :274-275
            "locus": l, "sample": s, "repeatunit": get("repeatunit") or "NaN",
            "allele1_est": fl("allele1_est"), "allele2_est": fl("allele2_est"),
            "spanning_reads": intc("spanning_reads"), "spanning_pairs": intc("spanning_pairs"),
            "left_clips": intc("left_clips"), "right_clips": intc("right_clips"), "unplaced_pairs": intc("unplaced_pairs"),
            "sum_str_counts": "NaN" if X[j, i] != X[j, i] else str(int(X[j, i])),
            "sum_str_log": fmt_float(float(round1(ssl[j, i]))), "depth": fmt_float(float(depf[j, i])),
            "outlier": fmt_g2(z[j, i]), "p": fmt_g2(p[j, i]), "p_adj": fmt_g2(padj[j, i]), "method": method[j],
        }
        keep_s = a2 == a2 and a2 >= min_size                                                    # :467
        if keep_s and d is not None:
            keep_s = int(float(d["left_clips"])) + int(float(d["right_clips"])) >= min_clips    # :468
        rows.append((s, "\t".join(v[c] for c in cols), keep_s))
    head = "\t".join(cols) + "\n"
    files[out + "STRs.tsv"] = head + "".join(r + "\n" for _, r, _ in rows)                      # :472-473
    for s in samples:                                                                           # :462-469
        files[out + s + ".STRs.tsv"] = head + "".join(r + "\n" for ss, r, k in rows if ss == s and k)
    return files
