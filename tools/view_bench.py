"""`strling view` on a whole BAM: the device path beside the host path (STRL_VIEW=host), JSON lines.

    python tools/view_bench.py [--pairs N] [--repeats K] [--dir D]

The input is the 4 194 304-read set of DESIGN section 24 (e2e_bench.make_input: --pairs pairs from bamio.write_bam_slabs, 30x
geometry, qualities, aux tags; default 2^21 pairs), coordinate-sorted as it is written.  Alternating in one run on one box, one
process at a time, K runs each (the first pays for the page cache and the driver):
  * `strling view --verbose -o OUT.sam` on the device: wall time, the size kernel with its prefix sum and the text kernel (HIP-event
    time summed over the chunks), the bytes of text over them -> bytes per second of text, host_chunks;
  * `STRL_VIEW=host strling view ...`: wall time.
The two paths' files must be the same bytes.  `samtools view` is not on these machines: nothing here compares with it.  No
threshold is asserted; a device path slower in wall clock than the host path is reported as it is."""
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


def _run(cmd, env=None):
    t = time.time()
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=1500)
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-4000:])
        sys.exit(r.returncode)
    return json.loads(r.stderr.strip().splitlines()[-1]), round(time.time() - t, 3)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--pairs", type=int, default=2 ** 21)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--dir", default=None)
    a = ap.parse_args()
    t0 = time.time()
    if a.dir:
        os.makedirs(a.dir, exist_ok=True)
    inp = e2e_bench.make_input(a.pairs, d=a.dir, level=1)
    src = inp["bam"]
    work = tempfile.mkdtemp(prefix="view_bench_", dir=os.path.dirname(src))
    cli = os.path.join(ROOT, "strling_amd", "lib", "strling")
    print(json.dumps({"tool": "view_bench", "pairs": a.pairs, "bam_bytes": os.path.getsize(src), "input_s": round(time.time() - t0, 1)}), flush=True)
    outs, says = {}, {}
    for k in range(a.repeats):
        for tag, env in (("device", {}), ("host", {"STRL_VIEW": "host"})):
            outs[tag] = os.path.join(work, tag + ".sam")
            e = dict(os.environ, **env)
            if tag == "device":
                e.pop("STRL_VIEW", None)
            says[tag], wall = _run([cli, "view", "--verbose", "-h", "-o", outs[tag], src], e)
            line = {"run": tag, "repeat": k, "wall_s": wall, "says": says[tag]}
            if tag == "device" and says[tag].get("text_ms"):
                line["text_kernel_GB_per_s"] = round(says[tag]["text_bytes"] / says[tag]["text_ms"] / 1e6, 1)
                line["size_and_text_GB_per_s"] = round(says[tag]["text_bytes"] / (says[tag]["text_ms"] + says[tag]["size_ms"]) / 1e6, 1)
            print(json.dumps(line), flush=True)
    same = open(outs["device"], "rb").read() == open(outs["host"], "rb").read()
    print(json.dumps({"check": "outputs", "device_file_equals_host_file": same, "counts_agree": all(says["device"][k] == says["host"][k] for k in ("records", "written", "dropped", "text_bytes")),
                      "out_bytes": os.path.getsize(outs["device"])}), flush=True)
    shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
