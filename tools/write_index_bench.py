"""`strling extract --write-index` beside `extract` without the flag and `bamindex` of the parent commit, one JSON line.

    python tools/write_index_bench.py --parent DIR [--pairs N] [--repeats K] [--trace OUTDIR] [--dir D]

The input is the whole-genome BAM `bench.py --full` caches (tools/e2e_bench.py) when its side-car is in the work directory; else a
file of --pairs pairs from the same writer (bamio.write_bam_slabs), whose size the line states.  Four commands on that file, K
rounds, one process at a time, in turn inside a round:
  (a) the parent commit's `strling extract` (--parent: a checkout of the parent with `python -m strling_amd.build` run in it);
  (b) this build's `strling extract`;
  (c) this build's `strling extract --write-index --index-out <scratch>`;
  (d) the parent's `strling bamindex -o <scratch>`.
Reported: every wall time; (b) against (a) with the run-to-run spread of (a) -- the claim is "unchanged"; (c) - (b) against (d)
-- the claim is that the index inside the pass costs less than a pass of its own -- as medians and best-of, whatever the ratio
is; whether (c)'s index equals (d)'s and (c)'s .bin equals (b)'s, byte for byte.  No margin is asserted.
--trace: runs of their own under `rocprofv3 --kernel-trace --stats` with STRL_FRONT_SERIAL=1 (every launch on one stream, no
kernel beside another): (c), (c) with STRL_BAI_RECORDS=1 (the record-reading per-record kernel launched in the pass as it is)
and this build's `bamindex`; the tables go to OUTDIR, the bai_* kernels' times into the line.
"""
import argparse
import csv
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import e2e_bench  # noqa: E402


def _timed(cmd, env=None):
    t = time.time()
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=900)
    w = time.time() - t
    if r.returncode != 0:
        sys.stderr.write(" ".join(cmd) + "\n" + r.stderr[-4000:])
        sys.exit(r.returncode or 1)
    return r, round(w, 3)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--pairs", type=int, default=2 ** 22, help="read pairs of the file written when the whole-genome one is not cached (default 2^22: 8.4e6 reads)")
    ap.add_argument("--parent", required=True, help="checkout of the parent commit, built")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--trace", default="", help="directory for the kernel tables of the runs under rocprofv3 --kernel-trace --stats")
    ap.add_argument("--dir", default=None, help="where the input lives (default: e2e_bench's work directory)")
    a = ap.parse_args()
    full = 2 ** 28
    d = a.dir or e2e_bench.work_dir(full * 2 * 115)
    n_pairs = full if os.path.exists(f"{d}/e2e_{full}_6.input.json") else a.pairs
    inp = e2e_bench.make_input(n_pairs, d=d if n_pairs == full else a.dir)
    bam, bed = inp["bam"], inp["bed"]
    cli = os.path.join(ROOT, "strling_amd", "lib", "strling")
    parent_cli = os.path.join(a.parent, "strling_amd", "lib", "strling")
    scratch = tempfile.mkdtemp(prefix="write_index_bench_", dir=os.path.dirname(bam))
    p = lambda f: os.path.join(scratch, f)
    cmds = {"a_parent_extract": [parent_cli, "extract", "-g", bed, bam, p("a.bin")],
            "b_extract": [cli, "extract", "-g", bed, bam, p("b.bin")],
            "c_extract_write_index": [cli, "extract", "-g", bed, "-v", "--write-index", "--index-out", p("c.bai"), bam, p("c.bin")],
            "d_parent_bamindex": [parent_cli, "bamindex", "-o", p("d.bai"), bam]}
    res = {"tool": "write_index_bench", "input": inp.get("input"), "reads": inp["reads"], "bam_MB": inp["bam_MB"], "whole_genome_cache": n_pairs == full, "rounds": a.repeats}
    wall = {k: [] for k in cmds}
    for _ in range(a.repeats):
        for k, cmd in cmds.items():
            r, w = _timed(cmd)
            wall[k].append(w)
            if k == "c_extract_write_index":
                res["index_says"] = next((l for l in r.stderr.splitlines() if l.startswith("[strling] index")), None)
    res["wall_s"] = wall
    med = {k: statistics.median(v) for k, v in wall.items()}
    best = {k: min(v) for k, v in wall.items()}
    res["median_s"], res["best_s"] = med, best
    res["a_spread_s"] = round(max(wall["a_parent_extract"]) - min(wall["a_parent_extract"]), 3)
    res["b_minus_a_median_s"] = round(med["b_extract"] - med["a_parent_extract"], 3)
    res["b_minus_a_best_s"] = round(best["b_extract"] - best["a_parent_extract"], 3)
    for tag, m in (("median", med), ("best", best)):
        extra = m["c_extract_write_index"] - m["b_extract"]
        res[f"c_minus_b_{tag}_s"] = round(extra, 3)
        res[f"c_minus_b_over_d_{tag}"] = round(extra / m["d_parent_bamindex"], 3)
    res["index_equals_bamindex"] = open(p("c.bai"), "rb").read() == open(p("d.bai"), "rb").read()
    res["bin_equals_plain"] = open(p("c.bin"), "rb").read() == open(p("b.bin"), "rb").read() == open(p("a.bin"), "rb").read()
    res["bai_bytes"] = os.path.getsize(p("c.bai"))
    if a.trace:
        os.makedirs(a.trace, exist_ok=True)
        serial = dict(os.environ, STRL_FRONT_SERIAL="1")
        runs = (("extract_write_index_serial", cmds["c_extract_write_index"], serial),
                ("extract_write_index_records_serial", cmds["c_extract_write_index"], dict(serial, STRL_BAI_RECORDS="1")),
                ("bamindex_serial", [cli, "bamindex", "-o", p("e.bai"), bam], serial))
        for tag, cmd, env in runs:
            kt = p("kt_" + tag)
            r = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", kt, "-o", "run", "--"] + cmd, capture_output=True, text=True, env=env, timeout=900)
            f = glob.glob(os.path.join(kt, "**", "run_kernel_stats.csv"), recursive=True)
            if r.returncode != 0 or not f:
                res["trace_" + tag] = {"error": (r.stderr or "no kernel table")[-500:]}
                continue
            shutil.copy(f[0], os.path.join(a.trace, "kernel_stats_" + tag + ".csv"))
            rows = list(csv.DictReader(open(f[0])))
            ns = lambda pat: sum(int(x["TotalDurationNs"]) for x in rows if pat in x["Name"])
            res["trace_" + tag] = {"all_kernels_ms": round(sum(int(x["TotalDurationNs"]) for x in rows) / 1e6, 3), "inflate_ms": round(ns("inflate") / 1e6, 3),
                                   "rec_parse_ms": round(ns("rec_parse") / 1e6, 3),
                                   "bai_kernels_ms": {x["Name"].split("(")[0].split("::")[-1]: round(int(x["TotalDurationNs"]) / 1e6, 3) for x in rows if "bai_" in x["Name"]}}
    shutil.rmtree(scratch, ignore_errors=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
