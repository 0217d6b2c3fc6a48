"""`strling call --sweep` against `strling call` without the flag, and against the build of the parent commit (whose default path
is the same code), over growing numbers of bounds: where does one pass over the file overtake one indexed read per bound?
Writes one 30x synthetic BAM (bamio.write_bam_slabs, the size tools/evidence_bench.py uses by default), extracts it once, draws
`-l` BED files of --loci loci (each at most 1000 bases wide, fixed seed), then alternates the three commands --runs times each
and prints medians, spreads, whether the three output files agree, and the `-v` line of the sweep (answered / seam / passed-on
bounds, chunks, seconds).  --trace: one more run of the sweep under `rocprofv3 --kernel-trace --stats`, in a process of its own,
with no counters, and the kernel table of that run.

usage: python tools/sweep_bench.py [--parent DIR] [--slabs 16] [--pairs 262144] [--loci 4000,32000,256000] [--runs 5] [--out DIR] [--trace]
  DIR = a checkout of the parent commit with its library and CLI built (python -m strling_amd.build inside it); without it the
  baseline is left out."""
import argparse
import csv
import glob
import json
import os
import re
import statistics
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from strling_amd import bamio, build  # noqa: E402

FILES = ("-bounds.txt", "-genotype.txt", "-unplaced.txt")
UNITS = ("A", "AC", "CAG", "AAAG", "AAGGG", "AAGGGC")


def write_loci(path, targets, n, seed):
    """n loci of 1 .. 1000 bases, spread over the references in proportion to their lengths, sorted"""
    rng = np.random.default_rng(seed)
    lens = np.array([t[1] for t in targets], np.float64)
    tid = np.sort(rng.choice(len(targets), size=n, p=lens / lens.sum()))
    rows = []
    for t in tid:
        w = int(rng.integers(1, 1001))
        left = int(rng.integers(0, max(1, targets[t][1] - w)))
        rows.append((int(t), left, left + w, UNITS[int(rng.integers(0, len(UNITS)))]))
    rows.sort()
    with open(path, "w") as f:
        for k, (t, a, b, u) in enumerate(rows):
            f.write(f"{targets[t][0]}\t{a}\t{b}\t{u}\tL{k}\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None)
    ap.add_argument("--slabs", type=int, default=16)
    ap.add_argument("--pairs", type=int, default=1 << 18)
    ap.add_argument("--loci", default="4000,32000,256000")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--min-support", type=int, default=5)
    ap.add_argument("--out", default=os.environ.get("TMPDIR", "/tmp"))
    ap.add_argument("--trace", action="store_true")
    a = ap.parse_args()
    clis = {"default": build.CLI, "sweep": build.CLI}
    if a.parent:
        clis["parent"] = os.path.join(a.parent, "strling_amd", "lib", "strling")
    for k, p in clis.items():
        assert os.path.exists(p), f"{k} CLI not built: {p}"
    os.makedirs(a.out, exist_ok=True)
    bam, bed, binp = (os.path.join(a.out, x) for x in ("sb.bam", "sb.str", "sb.bin"))
    info = bamio.write_bam_slabs(bam, a.slabs, a.pairs, seed=4242, bed=bed)
    print(json.dumps({"input": "write_bam_slabs", "slabs": a.slabs, "pairs_per_slab": a.pairs, "reads": info["reads"], "bam_MB": round(info["bytes"] / 1e6, 1),
                      "written_s": round(info["seconds"], 1), "cpus": len(os.sched_getaffinity(0))}), flush=True)
    r = subprocess.run([build.CLI, "extract", "-g", bed, bam, binp], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-500:]

    def call(which, loci, tag, wrap=()):
        pre = os.path.join(a.out, f"sb_{which}_{tag}")
        cmd = list(wrap) + [clis[which], "call", "-v", "-m", str(a.min_support), "-o", pre, "-l", loci] + (["--sweep"] if which == "sweep" else []) + [bam, binp]
        t0 = time.perf_counter()
        r = subprocess.run(cmd, capture_output=True, text=True)
        dt = time.perf_counter() - t0
        assert r.returncode == 0, r.stderr[-800:]
        return dt, [open(pre + s).read() for s in FILES], r.stderr

    for n in [int(x) for x in a.loci.split(",")]:
        loci = os.path.join(a.out, f"sb_{n}.bed")
        write_loci(loci, info["targets"], n, seed=n)
        for which in clis:
            call(which, loci, "warm")
        times, outs, err = {k: [] for k in clis}, {}, {}
        for _ in range(a.runs):
            for which in clis:
                dt, outs[which], err[which] = call(which, loci, str(n))
                times[which].append(dt)
        res = {"loci": n, "runs": a.runs, "outputs_identical": all(outs[k] == outs["default"] for k in clis), "bounds_rows": outs["default"][0].count("\n") - 1}
        for which, t in times.items():
            res[which] = {"median_s": round(statistics.median(t), 4), "min_s": round(min(t), 4), "max_s": round(max(t), 4), "all_s": [round(x, 4) for x in t]}
            w = re.search(r"evidence \+ genotypes of (\d+) bounds on (\d+) threads ([0-9.]+) ", err[which])
            if w:
                res[which]["evidence_stage_s"] = float(w.group(3))
        res["sweep_over_default"] = round(res["sweep"]["median_s"] / res["default"]["median_s"], 4)
        m = re.search(r"sweep: bounds answered by the sweep (\d+), seam bounds (\d+), passed on .*? (\d+), chunks (\d+), records (\d+), seconds: the pass ([0-9.]+), sweep kernels ([0-9.]+), "
                      r"evidence kernels ([0-9.]+)", err["sweep"])
        if m:
            g = [float(x) for x in m.groups()]
            tot = max(1.0, g[0] + g[1] + g[2])
            res["sweep_line"] = {"answered": int(g[0]), "seam": int(g[1]), "passed_on": int(g[2]), "seam_share": round(g[1] / tot, 6), "passed_on_share": round(g[2] / tot, 6),
                                 "chunks": int(g[3]), "records": int(g[4]), "pass_s": g[5], "sweep_kernels_s": g[6], "evidence_kernels_s": g[7]}
        print(json.dumps(res), flush=True)
        assert res["outputs_identical"], "the outputs differ"
        if a.trace and n == max(int(x) for x in a.loci.split(",")):
            tdir = os.path.join(a.out, "sb_trace")
            call("sweep", loci, "trace", wrap=("rocprofv3", "--kernel-trace", "--stats", "-d", tdir, "--output-format", "csv", "--"))
            for p in glob.glob(os.path.join(tdir, "**", "*kernel_stats.csv"), recursive=True):
                rows = list(csv.DictReader(open(p)))
                print(json.dumps({"kernel_stats": [{k: r_[k] for k in ("Name", "Calls", "TotalDurationNs", "AverageNs", "Percentage") if k in r_} for r_ in rows[:16]]}), flush=True)


if __name__ == "__main__":
    main()
