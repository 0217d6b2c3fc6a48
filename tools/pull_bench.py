"""`strling pull` on a slab BAM: one 1 Mbp region and one -L file of some hundred loci, on the device path and with STRL_PULL=host,
one JSON line.

    python tools/pull_bench.py [--slabs N] [--pairs P] [--loci K] [--repeats R] [--trace OUTDIR] [--dir D]

The input comes from bamio.write_bam_slabs (30x geometry, zlib level 6, binned qualities, aux tags): --slabs slabs of two contigs
of 5 * --pairs bases each, kept in --dir between runs.  One after the other on one box, R runs each (the first pays for the page
cache and, on the device path, for the driver):
  * `strling pull -v -o <scratch> BAM s0chr1:100001-1100000`, device path and STRL_PULL=host;
  * `strling pull -v -o <scratch> -L loci.bed BAM` with K loci of 2 kb spread over all contigs, both paths;
  * the two paths' outputs compared byte for byte;
  * --trace: one more device run of each under `rocprofv3 --kernel-trace --stats` (runs of their own), the region run's table
    copied to OUTDIR/kernel_stats.csv and the loci run's to OUTDIR/kernel_stats_loci.csv.
The line holds the wall times and what `pull -v` says itself: tiles and windows on the device and on the host, the HIP-event
time of the select and of the mate kernels.  The reference's `pull_region` is not on these machines: no time of it is given.
"""
import argparse
import csv
import glob
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from strling_amd import bamio  # noqa: E402


def _timed(cmd, env=None):
    t = time.time()
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=900)
    return r, time.time() - t


def _says(stderr):
    m = re.search(r"\[strling\] pull: (\{.*\})", stderr)
    return json.loads(m.group(1)) if m else None


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--slabs", type=int, default=4)
    ap.add_argument("--pairs", type=int, default=2 ** 18, help="read pairs per slab (default 2^18: two contigs of 1.31 Mbp at 30x)")
    ap.add_argument("--loci", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--trace", default="", help="directory for the kernel tables of one more run each under rocprofv3 --kernel-trace --stats")
    ap.add_argument("--dir", default=os.path.join(tempfile.gettempdir(), "strling_pull_bench"))
    a = ap.parse_args()
    os.makedirs(a.dir, exist_ok=True)
    bam = os.path.join(a.dir, f"slabs_{a.slabs}_{a.pairs}.bam")
    side = bam + ".json"
    if not (os.path.exists(bam) and os.path.exists(bam + ".bai") and os.path.exists(side)):
        info = bamio.write_bam_slabs(bam, a.slabs, a.pairs)
        json.dump({"reads": info["reads"], "bytes": info["bytes"], "targets": info["targets"]}, open(side, "w"))
    info = json.load(open(side))
    targets = info["targets"]
    contig_len = targets[0][1]
    if contig_len < 1_100_000:
        sys.exit(f"contigs of {contig_len} bases: --pairs too small for a 1 Mbp region")
    cli = os.path.join(ROOT, "strling_amd", "lib", "strling")
    scratch = tempfile.mkdtemp(prefix="pull_bench_", dir=a.dir)
    bed = os.path.join(scratch, "loci.bed")
    with open(bed, "w") as f:
        for k in range(a.loci):
            name, length = targets[k % len(targets)]
            start = 10_000 + (k // len(targets)) * ((length - 30_000) // max(1, (a.loci + len(targets) - 1) // len(targets)))
            f.write(f"{name}\t{start}\t{start + 2000}\n")
    runs = {"region": [f"{targets[0][0]}:100001-1100000"], "loci": ["-L", bed]}
    res = {"tool": "pull_bench", "reads": info["reads"], "bam_MB": round(info["bytes"] / 1e6, 1), "contig_len": contig_len, "loci": a.loci}
    for what, args in runs.items():
        outs = {}
        for mode in ("device", "host"):
            env = dict(os.environ)
            env.pop("STRL_PULL", None)
            if mode == "host":
                env["STRL_PULL"] = "host"
            out = os.path.join(scratch, f"{what}_{mode}.bam")
            walls = []
            for _ in range(a.repeats):
                r, w = _timed([cli, "pull", "-v", "-o", out, bam] + args, env)
                if r.returncode != 0:
                    sys.stderr.write(r.stderr[-4000:])
                    sys.exit(r.returncode)
                walls.append(round(w, 3))
            outs[mode] = out
            res[f"{what}_{mode}"] = {"wall_s": walls, "says": _says(r.stderr), "out_MB": round(os.path.getsize(out) / 1e6, 2)}
        res[f"{what}_outputs_equal"] = open(outs["device"], "rb").read() == open(outs["host"], "rb").read()
    if a.trace:
        os.makedirs(a.trace, exist_ok=True)
        for what, tag in (("region", "kernel_stats"), ("loci", "kernel_stats_loci")):
            kt = os.path.join(scratch, "kt_" + tag)
            r, w = _timed(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", kt, "-o", "run", "--", cli, "pull", "-o", os.path.join(scratch, "t.bam"), bam] + runs[what])
            f = glob.glob(os.path.join(kt, "**", "run_kernel_stats.csv"), recursive=True)
            if r.returncode != 0 or not f:
                res["trace_" + tag] = {"error": (r.stderr or "no kernel table")[-500:]}
                continue
            shutil.copy(f[0], os.path.join(a.trace, tag + ".csv"))
            rows = list(csv.DictReader(open(f[0])))
            res["trace_" + tag] = {"wall_s": round(w, 3), "kernels_ms": {x["Name"].split("(")[0].split("::")[-1]: round(int(x["TotalDurationNs"]) / 1e6, 3) for x in rows}}
    shutil.rmtree(scratch, ignore_errors=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
