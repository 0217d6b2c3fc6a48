"""`strling bamindex` on a coordinate-sorted BAM: wall clock beside `strling extract` of another build on the same file, one JSON line.

    python tools/bamindex_bench.py [--pairs N] [--parent DIR] [--repeats K] [--trace OUTDIR] [--dir D] [--csi]

The input is the whole-genome BAM `bench.py --full` caches (tools/e2e_bench.py: 2^28 pairs, 57 GB) when its side-car is in the
work directory; else a file of --pairs pairs from the same writer (bamio.write_bam_slabs, zlib level 6, binned qualities, aux
tags), whose size the line states.  One after the other on one box:
  * `strling bamindex -v -o <scratch>.bai BAM`, K runs (the first pays for the page cache and the driver);
  * `strling extract` of the build in --parent (a checkout of the parent commit with `python -m strling_amd.build` run inside it;
    default: this build) on the same file, K runs -- the yardstick: the index pass inflates, checks and scans the same bytes and
    does strictly less behind the scan.  The ratio is reported, no margin asserted;
  * --csi: `strling bamindex --csi -v -o <scratch>.csi BAM` as well, in turn with the two above (the same kernels with the binning
    scheme as an argument, the payload deflated into BGZF blocks: expected within run-to-run noise of the .bai; no threshold);
  * the device-built index against the writer's own .bai, as structures (every virtual offset turned into an offset of the
    inflated stream): bins and chunk lists, linear index, the pseudo-bin's numbers, n_no_coor;
  * --trace: two more `bamindex` runs under `rocprofv3 --kernel-trace --stats` (runs of their own), as shipped and with
    STRL_FRONT_SERIAL=1 (one stream, no kernel beside another): the tables copied to OUTDIR/kernel_stats.csv and
    OUTDIR/kernel_stats_serial.csv, the share of the bai_* kernels beside inflate_kernel in the line.
`samtools index` is not on these machines: its time stays the estimate derived from zlib's rate.
"""
import argparse
import csv
import glob
import json
import os
import shutil
import struct
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
    return r, time.time() - t


def _block_starts(path):
    """file offset of every BGZF block -> offset of its first byte in the inflated stream (26 bytes read per block)"""
    at, o, u = {}, 0, 0
    size = os.path.getsize(path)
    with open(path, "rb") as f:
        while o < size:
            at[o] = u
            f.seek(o + 16)
            bsize = struct.unpack("<H", f.read(2))[0] + 1
            f.seek(o + bsize - 4)
            u += struct.unpack("<I", f.read(4))[0]
            o += bsize
    at[o] = u
    return at


def _bai_abs(path, at):
    d = open(path, "rb").read()
    n_ref = struct.unpack_from("<i", d, 4)[0]
    o, refs = 8, []
    ab = lambda v: at[v >> 16] + (v & 0xffff)
    for _ in range(n_ref):
        n_bin = struct.unpack_from("<i", d, o)[0]; o += 4
        bins = {}
        for _ in range(n_bin):
            b, nc = struct.unpack_from("<Ii", d, o); o += 8
            v = struct.unpack_from(f"<{2 * nc}Q", d, o); o += 16 * nc
            if b == 37450:
                bins[b] = [ab(v[0]), ab(v[1]), v[2], v[3]]
                continue
            ch = []
            for k in range(nc):
                a0, a1 = ab(v[2 * k]), ab(v[2 * k + 1])
                if ch and ch[-1][1] == a0:
                    ch[-1][1] = a1
                else:
                    ch.append([a0, a1])
            bins[b] = ch
        n_intv = struct.unpack_from("<i", d, o)[0]; o += 4
        lin = [ab(x) if x else None for x in struct.unpack_from(f"<{n_intv}Q", d, o)]; o += 8 * n_intv
        refs.append((bins, lin))
    return refs, struct.unpack_from("<Q", d, o)[0]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--pairs", type=int, default=2 ** 22, help="read pairs of the file written when the whole-genome one is not cached (default 2^22: 8.4e6 reads)")
    ap.add_argument("--parent", default="", help="checkout of the parent commit, built: its `strling extract` is the yardstick")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--trace", default="", help="directory for the kernel table of one more run under rocprofv3 --kernel-trace --stats")
    ap.add_argument("--dir", default=None, help="where the input lives (default: e2e_bench's work directory)")
    ap.add_argument("--no-compare", action="store_true", help="skip the structural comparison with the writer's .bai")
    ap.add_argument("--csi", action="store_true", help="also time `bamindex --csi` on the same file, in turn with the .bai")
    a = ap.parse_args()
    full = 2 ** 28
    d = a.dir or e2e_bench.work_dir(full * 2 * 115)
    n_pairs = full if os.path.exists(f"{d}/e2e_{full}_6.input.json") else a.pairs
    inp = e2e_bench.make_input(n_pairs, d=d if n_pairs == full else a.dir)
    bam, bed = inp["bam"], inp["bed"]
    cli = os.path.join(ROOT, "strling_amd", "lib", "strling")
    parent_cli = os.path.join(a.parent, "strling_amd", "lib", "strling") if a.parent else cli
    scratch = tempfile.mkdtemp(prefix="bamindex_bench_", dir=os.path.dirname(bam))
    out_bai, out_bin = os.path.join(scratch, "dev.bai"), os.path.join(scratch, "x.bin")
    res = {"tool": "bamindex_bench", "input": inp.get("input"), "reads": inp["reads"], "bam_MB": inp["bam_MB"], "whole_genome_cache": n_pairs == full,
           "yardstick": "the parent commit's `strling extract`" if a.parent else "THIS build's `strling extract` (no --parent given)"}
    idx, ext, csi = [], [], []
    out_csi = os.path.join(scratch, "dev.csi")
    for k in range(a.repeats):          # alternating, one process at a time
        r, w = _timed([cli, "bamindex", "-v", "-o", out_bai, bam])
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-4000:])
            sys.exit(r.returncode)
        idx.append(round(w, 3))
        res["bamindex_says"] = r.stderr.strip().splitlines()[-1]
        if a.csi:
            r, w = _timed([cli, "bamindex", "--csi", "-v", "-o", out_csi, bam])
            if r.returncode != 0:
                sys.stderr.write(r.stderr[-4000:])
                sys.exit(r.returncode)
            csi.append(round(w, 3))
            res["bamindex_csi_says"] = r.stderr.strip().splitlines()[-1]
        r, w = _timed([parent_cli, "extract", "-g", bed, bam, out_bin])
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-4000:])
            sys.exit(r.returncode)
        ext.append(round(w, 3))
    res["bamindex_wall_s"], res["extract_wall_s"] = idx, ext
    res["ratio_bamindex_to_extract_best"] = round(min(idx) / min(ext), 3)
    res["bai_bytes"] = os.path.getsize(out_bai)
    if a.csi:
        res["bamindex_csi_wall_s"], res["csi_file_bytes"] = csi, os.path.getsize(out_csi)
        res["ratio_csi_to_bai_best"] = round(min(csi) / min(idx), 3)
    if not a.no_compare:
        t = time.time()
        at = _block_starts(bam)
        (ia, na), (ib, nb) = _bai_abs(out_bai, at), _bai_abs(bam + ".bai", at)
        res["equals_writers_index"] = bool(ia == ib and na == nb)
        res["compare_s"] = round(time.time() - t, 1)
    if a.trace:
        os.makedirs(a.trace, exist_ok=True)
        # two runs of their own: as shipped (the index kernels of a chunk run beside the next chunk's inflate, so a kernel's
        # duration includes waiting for a CU), and with STRL_FRONT_SERIAL=1 (every launch on one stream: each kernel its own time)
        for tag, env in (("kernel_stats", None), ("kernel_stats_serial", dict(os.environ, STRL_FRONT_SERIAL="1"))):
            kt = os.path.join(scratch, "kt_" + tag)
            r, w = _timed(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", kt, "-o", "run", "--", cli, "bamindex", "-o", out_bai, bam], env)
            f = glob.glob(os.path.join(kt, "**", "run_kernel_stats.csv"), recursive=True)
            if r.returncode != 0 or not f:
                res["trace_" + tag] = {"error": (r.stderr or "no kernel table")[-500:]}
                continue
            shutil.copy(f[0], os.path.join(a.trace, tag + ".csv"))
            rows = list(csv.DictReader(open(f[0])))
            ns = lambda pat: sum(int(x["TotalDurationNs"]) for x in rows if pat in x["Name"])
            total, infl = sum(int(x["TotalDurationNs"]) for x in rows), ns("inflate")
            res["trace_" + tag] = {"wall_s": round(w, 3), "all_kernels_ms": round(total / 1e6, 3), "inflate_ms": round(infl / 1e6, 3), "crc_ms": round(ns("crc") / 1e6, 3),
                                   "record_scan_ms": round((ns("rec_guess") + ns("rec_walk") + ns("rec_link") + ns("rec_emit")) / 1e6, 3),
                                   "bai_kernels_ms": {x["Name"].split("(")[0].split("::")[-1]: round(int(x["TotalDurationNs"]) / 1e6, 3) for x in rows if "bai_" in x["Name"]},
                                   "bai_share_of_inflate": round(ns("bai_") / infl, 4) if infl else None}
    shutil.rmtree(scratch, ignore_errors=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
