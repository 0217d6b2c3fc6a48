"""`strling call` with the per-bound evidence on the device against the build of the parent commit, which computes it on host
threads (strl_spanners).  Writes one 30x synthetic BAM (bamio.write_bam_slabs), extracts it once, then alternates `call` of the
two builds -- with every CPU the process may use, and pinned to two (`taskset -c 0-1`: one process per sample per device on a
node leaves a `call` about two cores) -- and prints medians, the spread of each, and whether the three output files agree.

usage: python tools/evidence_bench.py --parent DIR [--slabs 16] [--pairs 262144] [--runs 5] [--out DIR]
  DIR = a checkout of the parent commit with its library and CLI built (python -m strling_amd.build inside it)."""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from strling_amd import bamio, build  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True)
    ap.add_argument("--slabs", type=int, default=16)
    ap.add_argument("--pairs", type=int, default=1 << 18)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--min-support", type=int, default=5)
    ap.add_argument("--out", default=os.environ.get("TMPDIR", "/tmp"))
    a = ap.parse_args()
    clis = {"parent": os.path.join(a.parent, "strling_amd", "lib", "strling"), "new": build.CLI}
    for k, p in clis.items():
        assert os.path.exists(p), f"{k} CLI not built: {p}"
    os.makedirs(a.out, exist_ok=True)
    bam, bed, binp = (os.path.join(a.out, x) for x in ("eb.bam", "eb.str", "eb.bin"))
    info = bamio.write_bam_slabs(bam, a.slabs, a.pairs, seed=4242, bed=bed)
    print(json.dumps({"input": "write_bam_slabs", "slabs": a.slabs, "pairs_per_slab": a.pairs, "reads": info["reads"], "bam_MB": round(info["bytes"] / 1e6, 1),
                      "written_s": round(info["seconds"], 1)}), flush=True)
    r = subprocess.run([clis["new"], "extract", "-g", bed, bam, binp], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-500:]

    def call(which, pin, tag):
        pre = os.path.join(a.out, f"eb_{which}_{tag}")
        cmd = (["taskset", "-c", pin] if pin else []) + [clis[which], "call", "-v", "-m", str(a.min_support), "-o", pre, bam, binp]
        t0 = time.perf_counter()
        r = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, STRL_CALL_EVIDENCE="device"))   # (the parent build does not read it)
        dt = time.perf_counter() - t0
        assert r.returncode == 0, r.stderr[-500:]
        return dt, [open(pre + s).read() for s in ("-bounds.txt", "-genotype.txt", "-unplaced.txt")], r.stderr

    call("parent", None, "warm")
    call("new", None, "warm")
    for pin, label in ((None, "all CPUs"), ("0-1", "taskset -c 0-1")):
        times = {"parent": [], "new": []}
        outs, last_err = {}, {}
        for _ in range(a.runs):
            for which in ("parent", "new"):
                dt, files, err = call(which, pin, "pin" if pin else "all")
                times[which].append(dt)
                outs[which], last_err[which] = files, err
        same = outs["parent"] == outs["new"]
        res = {"cpus": label, "runs": a.runs, "outputs_identical": same, "bounds_rows": outs["new"][0].count("\n") - 1}
        for which in ("parent", "new"):
            t = times[which]
            res[which] = {"median_s": round(statistics.median(t), 4), "min_s": round(min(t), 4), "max_s": round(max(t), 4), "spread_s": round(max(t) - min(t), 4),
                          "all_s": [round(x, 4) for x in t]}
        res["new_over_parent"] = round(res["new"]["median_s"] / res["parent"]["median_s"], 4)
        m = re.search(r"regions through the device (\d+), on the host (\d+)", last_err["new"])
        e = re.search(r"computed on the device (\d+), passed on to the host \(.*?\) (\d+), evidence kernels ([0-9.]+) s", last_err["new"])
        if m and e:
            n_dev = int(m.group(1)) + int(e.group(2))
            res["regions"] = {"through_the_device": int(m.group(1)), "on_the_host": int(m.group(2)), "evidence_on_the_device": int(e.group(1)),
                              "passed_on_status_2": int(e.group(2)), "passed_on_share": round(int(e.group(2)) / max(1, n_dev), 6), "evidence_kernels_s": float(e.group(3))}
        for which in ("parent", "new"):
            w = re.search(r"evidence \+ genotypes of (\d+) bounds on (\d+) threads ([0-9.]+) \(summed over the threads: region records ([0-9.]+), spanners \+ genotype ([0-9.]+)", last_err[which])
            if w:
                res[which]["evidence_stage_s"] = float(w.group(3))
                res[which]["worker_cpu_s"] = round(float(w.group(4)) + float(w.group(5)), 3)
        print(json.dumps(res), flush=True)
        assert same, "the outputs of the two builds differ"


if __name__ == "__main__":
    main()
