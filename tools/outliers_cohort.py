"""Synthetic `strling call` outputs for a cohort: <sample>-genotype.txt and <sample>-unplaced.txt per sample.

The rows have the columns and number formats `strling call` writes (call_logic.cpp strl_call_row), so `strling outliers`
reads them as it reads real call output.  Used by tools/outliers_bench.py (a large cohort) and to make the small cohorts
under tests/golden/outliers/ (their README gives the calls).

    python tools/outliers_cohort.py OUTDIR --samples 1000 --loci 20000 [--seed 1]
"""
import argparse
import os

import numpy as np

HEADER = ("#chrom\tleft\tright\trepeatunit\tallele1_est\tallele2_est\tanchored_reads\tspanning_reads\tspanning_pairs\t"
          "expected_spanning_pairs\tspanning_pairs_pctl\tleft_clips\tright_clips\tunplaced_pairs\tdepth\tsum_str_counts\n")
UNITS = ["AAG", "AT", "CAG", "GGCCCC", "AAAAT", "AC", "CCG", "AGC", "ATTCT", "A"]


def nim_float(x):
    """depth as the call writer prints it: Nim's $ of a float ("30.0", "nan")"""
    return "nan" if x != x else repr(float(x))


def loci(n, rng):
    """n distinct (chrom, left, right, unit) keys"""
    out, seen = [], set()
    while len(out) < n:
        c = "chr%d" % int(rng.integers(1, 4))
        left = int(rng.integers(10_000, 50_000_000))
        u = UNITS[int(rng.integers(0, len(UNITS)))]
        k = (c, left, u)
        if k in seen:
            continue
        seen.add(k)
        out.append((c, left, left + int(rng.integers(1, 60)), u))
    return out


def genotype_row(key, a1, a2, anchored, spanning_reads, spanning_pairs, left_clips, right_clips, unplaced_pairs, depth, ssc):
    c, left, right, u = key
    return (f"{c}\t{left}\t{right}\t{u}\t{a1:.2f}\t{a2:.2f}\t{anchored}\t{spanning_reads}\t{spanning_pairs}\t{0.0:.2f}\t{0.0:.2f}\t"
            f"{left_clips}\t{right_clips}\t{unplaced_pairs}\t{nim_float(depth)}\t{ssc}\n")


def write_sample(d, name, rows, unplaced):
    """rows: genotype_row strings; unplaced: [(unit, count)]"""
    with open(os.path.join(d, name + "-genotype.txt"), "w") as f:
        f.write(HEADER)
        f.writelines(rows)
    with open(os.path.join(d, name + "-unplaced.txt"), "w") as f:
        f.writelines(f"{u}\t{c}\n" for u, c in unplaced)


def cohort(d, n_samples, n_loci, seed=1, names=None, p_missing=0.05, p_zero_depth=0.02, outliers=((0, 0, 25.0),),
           all_zero_loci=1, drop=()):
    """A cohort with missing cells, zero depths, all-zero loci (dropped by the scorer) and planted expansions
    (outliers: (sample, locus, factor) on the STR count).  Loci in `drop` are drawn but written for no sample."""
    rng = np.random.default_rng(seed)
    os.makedirs(d, exist_ok=True)
    keys = loci(n_loci, rng)
    names = names or [f"S{k:04d}" for k in range(n_samples)]
    cov = rng.uniform(20, 45, n_samples)
    rate = rng.uniform(0.5, 12.0, n_loci)
    rate[:all_zero_loci] = 0.0
    planted = {(s, l): f for s, l, f in outliers}
    for s, name in enumerate(names):
        depth = rng.poisson(cov[s], n_loci).astype(float)
        depth[rng.random(n_loci) < p_zero_depth] = 0.0
        ssc = rng.poisson(rate * cov[s] / 30.0)
        present = rng.random(n_loci) >= p_missing
        rows = []
        for l in range(n_loci):
            if not present[l] or l in drop:
                continue
            cnt = int(ssc[l])
            if (s, l) in planted:
                cnt = int(round((cnt + 1) * planted[(s, l)]))
            a2 = 10.0 + 3.0 * cnt + rng.normal(0, 2)
            a1 = min(a2, 10.0 + rng.normal(0, 2))
            lc, rc = int(rng.integers(0, 6)), int(rng.integers(0, 6))
            rows.append(genotype_row(keys[l], a1, a2, int(rng.integers(0, 20)), int(rng.integers(0, 30)), int(rng.integers(0, 30)),
                                     lc, rc, int(rng.integers(0, 4)), depth[l], cnt))
        units = [u for u in UNITS if rng.random() < 0.7] or UNITS[:1]
        write_sample(d, name, rows, [(u, int(rng.integers(0, 50))) for u in units])
    return names, keys


def _edge(d, n_samples, cells, unplaced=(("AT", 3),)):
    """a cohort written cell by cell: cells[locus key] = {sample index: (sum_str_counts, depth)}"""
    os.makedirs(d, exist_ok=True)
    names = [f"E{k}" for k in range(n_samples)]
    for s, name in enumerate(names):
        rows = [genotype_row(key, 10.0 + ssc, 10.0 + 2.0 * ssc, 3, 4, 5, 1, 2, 0, dep, ssc)
                for key, per in cells.items() if s in per for ssc, dep in [per[s]]]
        write_sample(d, name, rows, unplaced)
    return names


def fixtures(root):
    """the input cohorts of tests/golden/outliers/ (the README there gives the reference runs over them)"""
    # 1: basic -- missing cells, zero depths, an all-zero locus, one planted expansion, a sample name holding '-'
    cohort(os.path.join(root, "basic"), 8, 30, seed=3, names=["S0", "S1", "S2", "NA-12878", "S4", "S5", "S6", "S7"],
           p_missing=0.08, p_zero_depth=0.05, outliers=((3, 7, 20.0),))
    # 2: Huber edge rows on 5 samples, and a two-sample cohort
    k = lambda i, u="AT": ("chr1", 1000 + 100 * i, 1020 + 100 * i, u)
    cells = {
        k(0): {0: (4, 30.0), 1: (4, 30.0), 2: (4, 30.0), 3: (9, 25.0), 4: (1, 33.0)},      # MAD = 0: 3 of 5 equal
        k(1): {0: (2, 30.0), 1: (3, 30.0), 4: (60, 30.0)},                                   # 3 values, one far: den <= 0
        k(2): {2: (7, 28.0)},                                                                 # one finite value
        k(3): {0: (3, 31.0), 1: (5, 29.0), 2: (8, 35.0), 3: (6, 0.0), 4: (4, 27.0)},         # ordinary (a zero depth)
        k(4): {0: (0, 30.0), 1: (0, 31.0), 2: (0, 0.0), 3: (0, 28.0), 4: (0, 27.0)},         # all zero: dropped
        k(5, "CAG"): {0: (10, 30.0), 1: (12, 30.0), 2: (11, 29.0), 3: (40, 31.0), 4: (9, 30.0)},
        k(6, "CAG"): {0: (1, 30.0), 1: (1, 30.0), 3: (1, 30.0), 4: (1, 30.0)},              # constant row
    }
    _edge(os.path.join(root, "huber_edges"), 5, cells)
    _edge(os.path.join(root, "two_samples"), 2, {k(0): {0: (3, 30.0), 1: (9, 28.0)}, k(1): {0: (5, 30.0), 1: (5, 30.0)},
                                                  k(2): {0: (2, 25.0), 1: (14, 31.0)}})
    # 3: one locus
    _edge(os.path.join(root, "one_locus"), 4, {k(0): {0: (3, 30.0), 1: (9, 28.0), 2: (4, 26.0), 3: (5, 33.0)}})
    # 4: one sample, no control file
    cohort(os.path.join(root, "one_sample"), 1, 12, seed=5, names=["solo"])
    # 5: a cohort scored against the --emit of cohort 1: the same seed draws the same first 30 loci; 20..24 are left out
    # (control only) and 30..39 are new (not in the control)
    cohort(os.path.join(root, "controlled"), 5, 40, seed=3, names=[f"C{k}" for k in range(5)], outliers=((1, 12, 15.0),),
           drop=range(20, 25))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("out")
    ap.add_argument("--samples", type=int, default=1000)
    ap.add_argument("--loci", type=int, default=20000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--fixtures", action="store_true", help="write the small test cohorts into OUT instead")
    a = ap.parse_args()
    if a.fixtures:
        fixtures(a.out)
    else:
        cohort(a.out, a.samples, a.loci, a.seed)


if __name__ == "__main__":
    main()
