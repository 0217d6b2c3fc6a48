"""`strling fastq` on a shuffled BAM: the device path beside the host path (STRL_FASTQ=host), JSON lines.

    python tools/fastq_bench.py [--pairs N] [--repeats K] [--dir D]

The input is tools/sort_bench.py's: a file of --pairs pairs from bamio.write_bam_slabs (30x geometry, qualities, aux tags), its
records in a random order (default 2^21 pairs: the 4.2e6-read file the sort benchmarks use).  One after the other on one box, one
process at a time, K runs each (the first pays for the page cache and the driver):
  * `strling fastq --verbose -o OUT.fq -s S.fq` on the device: wall time, the step's parts (record kernel, join, layout: HIP-event
    time), and the text kernel's HIP-event time summed over the pieces with the bytes it wrote -> bytes per second of text;
  * `STRL_FASTQ=host strling fastq ...`: wall time.
The two paths' files must be the same bytes.  `samtools fastq` is not on these machines: nothing here compares with it.  No
threshold is asserted."""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import e2e_bench  # noqa: E402
import sort_bench  # noqa: E402


def _run(cmd, env=None):
    t = time.time()
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=1500)
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-4000:])
        sys.exit(r.returncode)
    lines = r.stderr.strip().splitlines()
    return json.loads(lines[-1]), [l for l in lines if "fastq:" in l][-1], round(time.time() - t, 3)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--pairs", type=int, default=2 ** 21)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--dir", default=None)
    a = ap.parse_args()
    t0 = time.time()
    inp = e2e_bench.make_input(a.pairs, d=a.dir, level=1)
    work = tempfile.mkdtemp(prefix="fastq_bench_", dir=os.path.dirname(inp["bam"]))
    src = os.path.join(work, "shuffled.bam")
    n, inflated = sort_bench.shuffled_copy(inp["bam"], src)
    cli = os.path.join(ROOT, "strling_amd", "lib", "strling")
    print(json.dumps({"tool": "fastq_bench", "reads": n, "inflated_bytes": inflated, "bam_bytes": os.path.getsize(src), "input_s": round(time.time() - t0, 1)}), flush=True)
    outs, counts = {}, {}
    for k in range(a.repeats):
        for tag, env in (("device", {}), ("host", {"STRL_FASTQ": "host"})):
            outs[tag] = (os.path.join(work, tag + ".fq"), os.path.join(work, tag + ".singles.fq"))
            says, counts[tag], wall = _run([cli, "fastq", "--verbose", "-o", outs[tag][0], "-s", outs[tag][1], src], dict(os.environ, **env))
            line = {"run": tag, "repeat": k, "wall_s": wall, "says": says}
            if tag == "device" and says.get("text_ms"):
                line["text_kernel_GB_per_s"] = round(says["text_bytes"] / says["text_ms"] / 1e6, 1)
            print(json.dumps(line), flush=True)
    same = all(open(outs["device"][i], "rb").read() == open(outs["host"][i], "rb").read() for i in (0, 1))
    print(json.dumps({"check": "outputs", "device_files_equal_host_files": same, "counts_agree": counts["device"] == counts["host"], "counts": counts["device"],
                      "out_bytes": [os.path.getsize(p) for p in outs["device"]]}), flush=True)
    shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
