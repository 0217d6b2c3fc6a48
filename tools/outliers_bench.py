"""`strling outliers` on a synthetic cohort: wall clock and the phase split of `-v`, one JSON line.

    python tools/outliers_bench.py [--samples 1000] [--loci 20000] [--dir DIR] [--keep]

The cohort has the shape `strling call` writes (tools/outliers_cohort.py's columns; 5 % missing cells, 2 % zero depths, a
few planted expansions) and is written by up to 16 processes.  The phases are the CLI's own laps: parse (files, interning,
matrices), device context, depth medians, sum_str_log, upload, huber, z / p / BH, order (device sort + the copies back),
format / write.
"""
import argparse
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time
from multiprocessing import Pool

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import outliers_cohort as oc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _write_one(job):
    d, s, keys, rate, seed = job
    rng = np.random.default_rng([seed, s])
    L = len(keys)
    cov = rng.uniform(20, 45)
    depth = rng.poisson(cov, L).astype(float)
    depth[rng.random(L) < 0.02] = 0.0
    ssc = rng.poisson(rate * cov / 30.0)
    if s % 97 == 0:
        ssc[rng.integers(0, L, 3)] *= 20
    present = rng.random(L) >= 0.05
    a2 = 10.0 + 3.0 * ssc + rng.normal(0, 2, L)
    a1 = np.minimum(a2, 10.0 + rng.normal(0, 2, L))
    ints = rng.integers(0, 30, (L, 6))
    rows = [oc.genotype_row(keys[l], a1[l], a2[l], ints[l, 0], ints[l, 1], ints[l, 2], ints[l, 3] % 6, ints[l, 4] % 6, ints[l, 5] % 4,
                            depth[l], int(ssc[l])) for l in np.flatnonzero(present)]
    oc.write_sample(d, f"S{s:05d}", rows, [(u, int(rng.integers(0, 50))) for u in oc.UNITS if rng.random() < 0.7])


def write_cohort(d, samples, loci, seed=1):
    rng = np.random.default_rng(seed)
    keys = oc.loci(loci, rng)
    rate = rng.uniform(0.5, 12.0, loci)
    os.makedirs(d, exist_ok=True)
    with Pool(min(16, os.cpu_count() or 1)) as pool:
        pool.map(_write_one, [(d, s, keys, rate, seed) for s in range(samples)], chunksize=4)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--samples", type=int, default=1000)
    ap.add_argument("--loci", type=int, default=20000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--dir", default=None, help="where the cohort and the outputs go (default: a temporary directory)")
    ap.add_argument("--keep", action="store_true", help="leave the cohort and the outputs behind")
    ap.add_argument("--prefix", default="", help="run the CLI under this command (e.g. a profiler's, ending in --)")
    a = ap.parse_args()
    d = a.dir or tempfile.mkdtemp(prefix="outliers_bench_")
    t0 = time.time()
    cdir = os.path.join(d, "cohort")
    if not os.path.exists(os.path.join(cdir, f"S{a.samples - 1:05d}-unplaced.txt")):
        write_cohort(cdir, a.samples, a.loci, a.seed)
    t_gen = time.time() - t0
    odir = os.path.join(d, "out")
    os.makedirs(odir, exist_ok=True)
    cli = os.path.join(ROOT, "strling_amd", "lib", "strling")
    cmd = a.prefix.split() + [cli, "outliers", "-v", "--genotypes", os.path.join(cdir, "*-genotype.txt"), "--unplaced",
                              os.path.join(cdir, "*-unplaced.txt"), "--out", os.path.join(odir, "b_")]
    t1 = time.time()
    r = subprocess.run(cmd, capture_output=True, text=True)
    wall = time.time() - t1
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-4000:])
        sys.exit(r.returncode)
    m = re.search(r"\[strling outliers\] samples (\d+) loci (\d+) \(kept (\d+)\) cells (\d+) seconds (\{.*\})", r.stderr)
    phases = json.loads(m.group(5)) if m else {}
    in_bytes = sum(os.path.getsize(os.path.join(cdir, f)) for f in os.listdir(cdir))
    out_bytes = sum(os.path.getsize(os.path.join(odir, f)) for f in os.listdir(odir))
    print(json.dumps({"tool": "outliers_bench", "samples": a.samples, "loci": a.loci, "cells": int(m.group(4)) if m else None,
                      "kept_loci": int(m.group(3)) if m else None, "input_mb": round(in_bytes / 1e6, 1),
                      "output_mb": round(out_bytes / 1e6, 1), "cohort_write_s": round(t_gen, 2), "wall_s": round(wall, 3),
                      "phases_s": phases}))
    if not a.keep and not a.dir:
        shutil.rmtree(d)


if __name__ == "__main__":
    main()
