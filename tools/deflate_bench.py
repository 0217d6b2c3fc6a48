"""The BGZF compressor on the payload `strling pull` writes for tools/pull_bench.py's 1 Mbp region: device, host twin, zlib.

    python tools/deflate_bench.py [--slabs N] [--pairs P] [--repeats R] [--modes fast,dense] [--trace OUTDIR] [--dir D]

The input BAM is pull_bench's (bamio.write_bam_slabs, kept in --dir between runs); the payload is what a default
`strling pull BAM s0chr1:100001-1100000` wrote, inflated.  One after the other on one box, R runs each:
  * strl_bgzf_deflate on one context, host buffers in and out: the copies are inside the time; its kernel time beside it;
  * strl_bgzf_deflate_host on one thread (the same bytes: compared);
  * zlib at its default level, one task per 0xFF00-byte block on 16 threads: what `pull` does without --deflate=device;
  * `strling pull -v` with --deflate=host and --deflate=device, wall time and what the command says itself;
  * --trace: one more `pull --deflate=device` under `rocprofv3 --kernel-trace --stats` (a run of its own), the table copied to
    OUTDIR/kernel_stats.csv.
--modes (default: fast) names the compressor's rules to measure, one after the other in the one run: with `dense` the device, the
twin and `pull --deflate=dense` are measured again under keys that end in _dense, and --trace takes one more run of its own for it
(OUTDIR/kernel_stats_dense.csv).
One JSON line: the times, the output sizes (DEFLATE payload bytes, also of zlib level 1 over the same cuts) and their ratios.
"""
import argparse
import csv
import ctypes as C
import glob
import gzip
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from strling_amd import api, bamio  # noqa: E402

BLK = 0xFF00


def _zlib_blocks(payload, level, threads):
    def one(o):
        c = zlib.compressobj(level, zlib.DEFLATED, -15)
        return len(c.compress(payload[o:o + BLK]) + c.flush())
    with ThreadPoolExecutor(threads) as ex:
        return sum(ex.map(one, range(0, len(payload), BLK)))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--slabs", type=int, default=4)
    ap.add_argument("--pairs", type=int, default=2 ** 18)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--modes", default="fast", help="fast, dense or fast,dense: the compressor's rules to measure")
    ap.add_argument("--trace", default="", help="directory for the kernel table of one more run under rocprofv3 --kernel-trace --stats")
    ap.add_argument("--dir", default=os.path.join(tempfile.gettempdir(), "strling_pull_bench"))
    a = ap.parse_args()
    modes = a.modes.split(",")
    if not modes or any(m not in api.DEFLATE_MODES for m in modes):
        ap.error("--modes takes fast, dense or both")
    forms = ["host"] + [{"fast": "device", "dense": "dense"}[m] for m in modes]
    os.makedirs(a.dir, exist_ok=True)
    bam = os.path.join(a.dir, f"slabs_{a.slabs}_{a.pairs}.bam")
    side = bam + ".json"
    if not (os.path.exists(bam) and os.path.exists(bam + ".bai") and os.path.exists(side)):
        info = bamio.write_bam_slabs(bam, a.slabs, a.pairs)
        json.dump({"reads": info["reads"], "bytes": info["bytes"], "targets": info["targets"]}, open(side, "w"))
    info = json.load(open(side))
    region = f"{info['targets'][0][0]}:100001-1100000"
    cli = os.path.join(ROOT, "strling_amd", "lib", "strling")
    scratch = tempfile.mkdtemp(prefix="deflate_bench_", dir=a.dir)
    res = {"tool": "deflate_bench", "region": region, "block": BLK}

    # ---- the command, both ways (the default run's file gives the payload)
    says = {}
    for form in forms:
        out = os.path.join(scratch, f"{form}.bam")
        walls = []
        for _ in range(a.repeats):
            t = time.time()
            r = subprocess.run([cli, "pull", "-v", "-o", out, bam, region, "--deflate=" + form], capture_output=True, text=True, timeout=900)
            walls.append(round(time.time() - t, 3))
            if r.returncode != 0:
                sys.stderr.write(r.stderr[-4000:])
                sys.exit(r.returncode)
        line = [l for l in r.stderr.split("\n") if l.startswith("[strling] pull: {")]
        says[form] = json.loads(line[-1][len("[strling] pull: "):]) if line else None
        res[f"pull_deflate_{form}"] = {"wall_s": walls, "file_MB": round(os.path.getsize(out) / 1e6, 2),
                                       "says": {k: says[form][k] for k in ("deflate", "deflate_stored_blocks", "deflate_kernel_ms", "seconds")} if says[form] else None}
    payload = gzip.decompress(open(os.path.join(scratch, "host.bam"), "rb").read())
    res["pull_outputs_hold_the_same_bytes"] = all(gzip.decompress(open(os.path.join(scratch, f"{form}.bam"), "rb").read()) == payload for form in forms[1:])
    res["payload_MB"] = round(len(payload) / 1e6, 2)
    n_blocks = (len(payload) + BLK - 1) // BLK
    res["blocks"] = n_blocks

    # ---- the three compressors on that payload
    L = api.load()
    src = np.frombuffer(payload, np.uint8)
    bound = api.bgzf_deflate_bound(src.size, BLK)
    out_d, out_h = np.empty(bound, np.uint8), np.empty(bound, np.uint8)
    nb, stored = C.c_uint64(0), C.c_uint32(0)
    ctx = api.Context(0)
    sizes = {}
    for mode in modes:
        m, tag = api.DEFLATE_MODES[mode], "" if mode == "fast" else "_" + mode
        dev_s, dev_kernel_ms = [], []
        for _ in range(a.repeats + 1):                         # the first call allocates the context's buffers: reported apart
            t = time.time()
            api._check(L.strl_bgzf_deflate_mode(ctx.h, m, src.ctypes.data, src.size, BLK, out_d.ctypes.data, out_d.size, C.byref(nb), None, C.byref(stored)))
            dev_s.append(round(time.time() - t, 4))
            dev_kernel_ms.append(round(ctx.deflate_ms(), 3))
        dev_bytes, dev_stored = nb.value, stored.value
        res["device" + tag] = {"first_call_s": dev_s[0], "s": dev_s[1:], "kernel_ms": dev_kernel_ms[1:], "stored_blocks": dev_stored}
        host_s = []
        for _ in range(a.repeats):
            t = time.time()
            api._check(L.strl_bgzf_deflate_host_mode(m, src.ctypes.data, src.size, BLK, out_h.ctypes.data, out_h.size, C.byref(nb), None, C.byref(stored)))
            host_s.append(round(time.time() - t, 4))
        res["host_twin_one_thread" + tag] = {"s": host_s}
        res["device_equals_twin" + tag] = bool(nb.value == dev_bytes and np.array_equal(out_d[:dev_bytes], out_h[:dev_bytes]))
        sizes[mode] = dev_bytes - 26 * n_blocks
    ctx.close()
    z_s = []
    for _ in range(a.repeats):
        t = time.time()
        z6 = _zlib_blocks(payload, -1, 16)
        z_s.append(round(time.time() - t, 4))
    res["zlib_default_16_threads"] = {"s": z_s}
    z1 = _zlib_blocks(payload, 1, 16)
    res["deflate_bytes"] = {"zlib_level_6": z6, "zlib_level_1": z1, "level_6_over_level_1": round(z6 / z1, 4)}
    for mode, mine in sizes.items():
        tag = "device" if mode == "fast" else "device_" + mode
        res["deflate_bytes"].update({tag: mine, tag + "_over_level_1": round(mine / z1, 4), tag + "_over_level_6": round(mine / z6, 4)})

    if a.trace:
        os.makedirs(a.trace, exist_ok=True)
        for form in forms[1:]:
            tag = "" if form == "device" else "_" + form
            kt = os.path.join(scratch, "kt" + tag)
            r = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", kt, "-o", "run", "--", cli, "pull", "-o", os.path.join(scratch, "t.bam"), bam, region,
                                "--deflate=" + form], capture_output=True, text=True, timeout=900)
            f = glob.glob(os.path.join(kt, "**", "run_kernel_stats.csv"), recursive=True)
            if r.returncode != 0 or not f:
                res["trace" + tag] = {"error": (r.stderr or "no kernel table")[-500:]}
            else:
                shutil.copy(f[0], os.path.join(a.trace, f"kernel_stats{tag}.csv"))
                rows = list(csv.DictReader(open(f[0])))
                res["trace" + tag] = {"kernels_ms": {x["Name"].split("(")[0].split("::")[-1]: round(int(x["TotalDurationNs"]) / 1e6, 3) for x in rows}}
    shutil.rmtree(scratch, ignore_errors=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
