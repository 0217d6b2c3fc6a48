"""Given loci take their reads: strl_assign_reads_loci (host, one thread: the yardstick) against strl_assign_reads_loci_device,
and `strling call -b` with and without STRL_ASSIGN=device against the build of the parent commit.

Input, fixed seeds: --treads treads (default 8.25e6, the headline file's count) on 25 references, 500 units drawn Zipf, uniform
positions; lists of --loci loci (default 4000, 32000, 256000) drawn from the treads' own positions.
  library leg  one child process per list: both entry points on the same arrays, every output asserted equal (the split column,
               the loci, the offsets, the assigned lists); seconds of the host function (--host-runs) and of the device entry
               point (--runs after a warm-up), with the figures of strl_assign_info_last
  CLI leg      a small BAM (bamio.write_bam_slabs) is extracted, its .bin is rewritten with the drawn treads under the same
               header, the loci are written as a -b file; `call -b` without the variable, with it, and the parent's CLI
               (--parent DIR: a checkout of the parent commit with its library and CLI built) alternate --runs times after a
               warm-up; the three output files are asserted identical.  The evidence of every given bound is read from the BAM
               in all three, so this leg takes lists of --cli-loci (default: the first of --loci)
  --trace      one more run of the device entry point under `rocprofv3 --kernel-trace --stats`, in a process of its own,
               without counters, and its kernel table
Every step that uses the GPU is a process of its own under its own time limit (--step-timeout).  One JSON line per result.

usage: python tools/assign_bench.py [--parent DIR] [--treads N] [--loci 4000,32000,256000] [--cli-loci 4000] [--runs 5]
                                    [--host-runs 1] [--out DIR] [--trace] [--skip-cli] [--skip-library]"""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from strling_amd import api, bamio, build  # noqa: E402

FILES = ("-bounds.txt", "-genotype.txt", "-unplaced.txt")
LINE = "loci take their reads on the device"


def draw_units(rng, k=500):
    units = set()
    while len(units) < k:
        units.add(bytes(b"ACGT"[int(b)] for b in rng.integers(0, 4, int(rng.integers(1, 7)))))
    return np.array(sorted(units), "S6")


def draw_treads(n, targets, seed=8250):
    rng = np.random.default_rng(seed)
    units = draw_units(rng)
    t = np.zeros(n, api.TREAD_DTYPE)
    lens = np.array([l for _, l in targets], np.int64)
    t["tid"] = rng.integers(0, len(targets), n)
    t["position"] = (rng.random(n) * lens[t["tid"]]).astype(np.uint32)
    t["repeat"] = units[np.minimum(rng.zipf(1.3, n) - 1, len(units) - 1)]
    t["split"] = rng.choice([0, 1, 3], n)
    t["mapping_quality"], t["repeat_count"], t["align_length"] = 60, 10, 100
    t["qname_id"] = np.arange(n) % 1024
    return t


def draw_loci(t, n, seed):
    """n loci at treads' own positions and units, each 1 .. 1000 bases wide, in drawn (not sorted) order"""
    rng = np.random.default_rng(seed)
    src = t[rng.integers(0, len(t), n)]
    lo = np.zeros(n, api.LOCUS_DTYPE)
    w = rng.integers(1, 1001, n)
    left = np.maximum(src["position"].astype(np.int64) - w // 2, 0)
    b = lo["b"]
    b["tid"], b["repeat"] = src["tid"], src["repeat"]
    b["left"], b["right"] = left + 1, left + w
    b["left_most"], b["right_most"], b["center_mass"] = b["left"], b["right"], b["left"]
    lo["name"] = [b"L%d" % k for k in range(n)]
    return lo


def library_child(a):
    """both entry points on one list (this process owns the GPU)"""
    targets = [(f"chr{k + 1}", 100_000_000) for k in range(25)]
    t = draw_treads(a.treads, targets)
    lo = draw_loci(t, a.child_library, seed=a.child_library)
    L = api.load()
    ctx = api.Context(0)

    def run(device):
        tt, ll = t.copy(), lo.copy()
        off = np.zeros(lo.size + 1, np.uint64)
        idx = np.zeros(t.size, np.uint32)
        t0 = time.perf_counter()
        if device:
            rc = L.strl_assign_reads_loci_device(ctx.h, tt.ctypes.data, tt.size, api.MODE_CALL, ll.ctypes.data, ll.size, off.ctypes.data, idx.ctypes.data, idx.size)
        else:
            rc = L.strl_assign_reads_loci(tt.ctypes.data, tt.size, api.MODE_CALL, ll.ctypes.data, ll.size, off.ctypes.data, idx.ctypes.data, idx.size)
        dt = time.perf_counter() - t0
        assert rc == 0, L.strl_last_error()
        return dt, (tt["split"], ll["b"]["n_total"], ll["b"]["n_left"], ll["b"]["n_right"], off, idx[:int(off[-1])])

    if a.trace_child:
        run(True)
        return
    run(True)                                                  # warm-up: the context's buffers, the code objects
    dev = [run(True) for _ in range(a.runs)]
    info = api.assign_info_last(ctx)
    host = [run(False) for _ in range(a.host_runs)]
    same = all(np.array_equal(x, y) for x, y in zip(dev[-1][1], host[-1][1])) and all(
        all(np.array_equal(x, y) for x, y in zip(d[1], dev[0][1])) for d in dev)
    ds, hs = [d[0] for d in dev], [h[0] for h in host]
    print(json.dumps({"leg": "library", "treads": int(t.size), "loci": int(lo.size), "outputs_equal": bool(same),
                      "host_s": {"median": round(statistics.median(hs), 4), "all": [round(x, 4) for x in hs]},
                      "device_s": {"median": round(statistics.median(ds), 4), "min": round(min(ds), 4), "max": round(max(ds), 4), "all": [round(x, 4) for x in ds]},
                      "host_over_device": round(statistics.median(hs) / statistics.median(ds), 2),
                      "groups_with_loci": int(info.n_groups), "assigned": int(info.n_assigned), "lost": int(info.n_lost)}), flush=True)
    assert same, "the outputs differ"


def step(cmd, timeout, env=None):
    """a process of its own under its own time limit; its standard output goes through line by line"""
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, env=env)
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-2000:])
        raise SystemExit(f"step failed ({r.returncode}): {' '.join(cmd[:6])} ...")
    return r


def cli_leg(a, sizes):
    clis = {"host": build.CLI, "device": build.CLI}
    if a.parent:
        clis["parent"] = os.path.join(a.parent, "strling_amd", "lib", "strling")
    for k, p in clis.items():
        assert os.path.exists(p), f"{k} CLI not built: {p}"
    bam, bed, binp, big = (os.path.join(a.out, x) for x in ("ab.bam", "ab.str", "ab.bin", "ab_big.bin"))
    info = bamio.write_bam_slabs(bam, a.slabs, a.pairs, seed=4242, bed=bed)
    step([build.CLI, "extract", "-g", bed, bam, binp], a.step_timeout)
    real = api.bin_read(binp)
    t = draw_treads(a.treads, info["targets"])
    names = [b"q%04d" % k for k in range(1024)]
    qoff = np.concatenate([[0], np.cumsum([len(x) for x in names])]).astype(np.uint64)
    api.bin_write(big, 0.8, real["min_mapq"], real["frag"], real["header"], t, qoff, b"".join(names))
    print(json.dumps({"leg": "cli", "input": "write_bam_slabs", "slabs": a.slabs, "pairs_per_slab": a.pairs, "reads": info["reads"], "treads": int(t.size),
                      "cpus": len(os.sched_getaffinity(0))}), flush=True)

    def call(which, bounds, tag):
        pre = os.path.join(a.out, f"ab_{which}_{tag}")
        env = {k: v for k, v in os.environ.items() if k != "STRL_ASSIGN"}
        if which == "device":
            env["STRL_ASSIGN"] = "device"
        t0 = time.perf_counter()
        r = step([clis[which], "call", "-v", "-o", pre, "-b", bounds, bam, big], a.step_timeout, env)
        dt = time.perf_counter() - t0
        assert (LINE in r.stderr) == (which == "device"), r.stderr[-800:]
        line = [x for x in r.stderr.splitlines() if LINE in x]
        return dt, [open(pre + s).read() for s in FILES], line[0] if line else ""

    for n in sizes:
        lo = draw_loci(t, n, seed=n)
        bounds = os.path.join(a.out, f"ab_{n}-bounds.txt")
        with open(bounds, "w") as f:
            f.write("#chrom\tleft\tright\trepeat\tname\tleft_most\tright_most\tcenter_mass\tn_left\tn_right\tn_total\n")
            for j in range(n):
                b = lo["b"][j]
                f.write(api.bounds_row(b, info["targets"][int(b["tid"])][0]) + "\n")
        for which in clis:
            call(which, bounds, "warm")
        times, outs, line = {k: [] for k in clis}, {}, {}
        for _ in range(a.runs):
            for which in clis:
                dt, outs[which], line[which] = call(which, bounds, str(n))
                times[which].append(dt)
        res = {"leg": "cli", "loci": n, "runs": a.runs, "outputs_identical": all(outs[k] == outs["host"] for k in clis), "device_line": line["device"]}
        for which, ts in times.items():
            res[which] = {"median_s": round(statistics.median(ts), 4), "min_s": round(min(ts), 4), "max_s": round(max(ts), 4), "all_s": [round(x, 4) for x in ts]}
        print(json.dumps(res), flush=True)
        assert res["outputs_identical"], "the outputs differ"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None)
    ap.add_argument("--treads", type=int, default=8_250_000)
    ap.add_argument("--loci", default="4000,32000,256000")
    ap.add_argument("--cli-loci", default=None)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--host-runs", type=int, default=1)
    ap.add_argument("--slabs", type=int, default=2)
    ap.add_argument("--pairs", type=int, default=1 << 16)
    ap.add_argument("--step-timeout", type=int, default=600)
    ap.add_argument("--out", default=os.environ.get("TMPDIR", "/tmp"))
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--skip-cli", action="store_true")
    ap.add_argument("--skip-library", action="store_true")
    ap.add_argument("--child-library", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--trace-child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child_library:
        return library_child(a)
    os.makedirs(a.out, exist_ok=True)
    sizes = [int(x) for x in a.loci.split(",")]
    me = [sys.executable, os.path.abspath(__file__), "--treads", str(a.treads), "--runs", str(a.runs), "--host-runs", str(a.host_runs)]
    if not a.skip_library:
        for n in sizes:
            sys.stdout.write(step(me + ["--child-library", str(n)], a.step_timeout).stdout)
            sys.stdout.flush()
    if a.trace:
        tdir = os.path.join(a.out, "ab_trace")
        step(["rocprofv3", "--kernel-trace", "--stats", "-d", tdir, "--output-format", "csv", "--"] + me + ["--child-library", str(max(sizes)), "--trace-child"], a.step_timeout)
        for p in glob.glob(os.path.join(tdir, "**", "*kernel_stats.csv"), recursive=True):
            rows = list(csv.DictReader(open(p)))
            print(json.dumps({"kernel_stats": [{k: r_[k] for k in ("Name", "Calls", "TotalDurationNs", "AverageNs", "Percentage") if k in r_} for r_ in rows[:24]]}), flush=True)
    if not a.skip_cli:
        cli_leg(a, [int(x) for x in a.cli_loci.split(",")] if a.cli_loci else sizes[:1])


if __name__ == "__main__":
    main()
