"""`strling sort` on a shuffled BAM: the device path with both --deflate forms beside the host path (STRL_SORT=host), JSON lines.

    python tools/sort_bench.py [--pairs N] [--repeats K] [--trace OUTDIR] [--dir D] [--slab-mb M] [--lanes 16,32,64] [--dense [--parent-cli PATH]]
    python tools/sort_bench.py --write-index [--parent-cli PATH] [--pairs N] [--repeats K] [--trace OUTDIR]

The input is a file of --pairs pairs from bamio.write_bam_slabs (30x geometry, qualities, aux tags), its records put into a random
order (a seeded permutation of the whole file, the header's SO: set to unsorted) and written again at zlib level 1.  One after the
other on one box, one process at a time, K runs each (the first pays for the page cache and the driver):
  * `strling sort -v --deflate=host`, `strling sort -v --deflate=device`, `STRL_SORT=host strling sort -v`; every run's own JSON
    line is kept; the three outputs must inflate to the same stream, and the --deflate=host file must be the host path's file;
  * the gather's rate: stream bytes / the HIP-event time of all gathers, from a run through the ABI (api.Context.bamsort:
    one fetch of the whole stream when it holds less than 4 GiB), for every group size in --lanes (STRL_SORT_GATHER_LANES);
  * one more device run with STRL_ALLOC_TIMING=1: the library's own timing of every hipMalloc of 64 MB and more, the arena's slabs among them;
  * --slab-mb: one more device run with slabs of that size (default 4096), to see what allocating the arena slab by slab costs;
  * --trace: one more run under `rocprofv3 --kernel-trace --stats` (a run of its own): OUTDIR/kernel_stats.csv.
  * --dense: `strling sort -v --deflate=dense` beside the three, and --parent-cli's `sort --deflate=host` (the bar the dense mode is
    measured against), alternating with them; the dense output must inflate to the same stream; the gather runs and the allocation
    run are left out; --trace then traces `sort --deflate=dense` (OUTDIR/kernel_stats_dense.csv).
--write-index measures `sort --write-index` instead, in one call, alternating, K runs each (K >= 5 for a figure), for both --deflate
forms: this build's `sort --write-index`; --parent-cli's (default: this build's) `sort` followed by its `bamindex` of the output,
the two commands' wall times summed; this build's plain `sort` and the parent's side by side, the order swapped every repeat.  The
index must be the bytes `bamindex` wrote.  With --trace the traced run is `sort --write-index --deflate=device`.
    python tools/sort_bench.py --windowed [--window-mb 1300,700,400] [--parent-cli PATH] [--pairs N] [--repeats K] [--trace OUTDIR]
--windowed measures `sort --windowed`: --parent-cli's (default: this build's) resident `sort`, K runs (wall time and read_s); then
`sort --windowed` with every window size of --window-mb (default: the sizes that make 1, 2 and 4 windows of this file) for both
--deflate forms, K runs each: wall time, pass 0's time and the time of a window's pass; the --deflate=host file must be the
resident sort's.  With --trace, runs under the profiler of their own: one window with 16 / 32 / 64 lanes a record of the scatter
(--lanes), then 2 and 4 windows: the time of bsort_scatter_kernel and bsort_dest_kernel, and the scatter's rate in TB/s of stream.
    python tools/sort_bench.py --sam [--parent-cli PATH] [--pairs N] [--repeats K] [--lanes 16,32,64]
--sam measures SAM text as the input: the same shuffled reads printed as SAM, sorted from a file and from a pipe (`cat IN.sam |
strling sort -`), beside --parent-cli's (default: this build's) `sort` of the shuffled BAM and beside STRL_SORT=host on the same SAM;
K runs each: wall time and the read phase.  Then, for every group size of --lanes (STRL_SORT_SAM_LANES), one run whose JSON line
gives the HIP-event time of the chunks' copies and of the three kernels (line scan, size with the sums, encode): GB/s of text each,
and the kernels' time a chunk beside that chunk's copy time.  The SAM outputs must be the BAM's sort with the bin field aside (the
benchmark's BAM writer gives every record bin 4680).
    python tools/sort_bench.py --markdup [--parent-cli PATH] [--pairs N] [--repeats K]
--markdup measures `sort --markdup`: alternating with --parent-cli's (default: this build's) plain `sort` of
the same file, K runs each, for both --deflate forms: wall time, the step's wall time (markdup_s) and the HIP-event time of its five
parts -- the record kernel, the join by name (a sort and the runs kernel), the pairs' and the fragments' chained sorts, the flag
kernel -- and the time added as a share of the parent's command; then STRL_SORT=host with the option.  The device file with
--deflate=host must be the host path's, and the counts must agree.
`samtools sort` is not on these machines: nothing here compares with it.  No threshold is asserted.
"""
import argparse
import glob
import gzip
import json
import os
import shutil
import struct
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import e2e_bench  # noqa: E402


def shuffled_copy(src, dst, seed=7):
    """the records of the BAM at src in a random order -> dst (BGZF level 1); -> (records, inflated bytes)"""
    from strling_amd import bamio
    raw = gzip.decompress(open(src, "rb").read())
    l_text = struct.unpack_from("<i", raw, 4)[0]
    text = raw[8:8 + l_text].decode().replace("SO:coordinate", "SO:unsorted")
    at = 8 + l_text
    n_ref = struct.unpack_from("<i", raw, at)[0]
    r0 = at
    at += 4
    for _ in range(n_ref):
        at += 8 + struct.unpack_from("<i", raw, at)[0]
    head = b"BAM\1" + struct.pack("<i", len(text)) + text.encode() + raw[r0:at]
    offs = []
    while at < len(raw):
        offs.append(at)
        at += 4 + struct.unpack_from("<i", raw, at)[0]
    offs.append(at)
    perm = np.random.default_rng(seed).permutation(len(offs) - 1)
    mv = memoryview(raw)
    out = head + b"".join(mv[offs[i]:offs[i + 1]] for i in perm)
    comp, _ = bamio.bgzf_compress(np.frombuffer(out, np.uint8), 1, 0xFF00)
    with open(dst, "wb") as f:
        f.write(comp.tobytes())
        f.write(bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0]))
    return len(offs) - 1, len(out)


def _run(cmd, env=None):
    t = time.time()
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=1500)
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-4000:])
        sys.exit(r.returncode)
    return json.loads(r.stderr.strip().splitlines()[-1]), round(time.time() - t, 3)


def _timed(cmd):
    t = time.time()
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=1500)
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-4000:])
        sys.exit(r.returncode)
    return r, round(time.time() - t, 3)


def write_index_runs(a, cli, src, work):
    """`sort --write-index` against the parent's `sort` followed by `bamindex`, and plain `sort` against the parent's: alternating"""
    parent = a.parent_cli or cli
    ours, theirs, plain = (os.path.join(work, n) for n in ("ours.bam", "theirs.bam", "plain.bam"))
    for form in ("host", "device"):
        for k in range(a.repeats):
            r, w = _timed([cli, "sort", "--write-index", "-v", f"--deflate={form}", "-o", ours, src])
            print(json.dumps({"run": "sort --write-index", "deflate": form, "repeat": k, "wall_s": w, "says": json.loads(r.stderr.strip().splitlines()[-1])}), flush=True)
            _, ws = _timed([parent, "sort", f"--deflate={form}", "-o", theirs, src])
            _, wi = _timed([parent, "bamindex", theirs])
            print(json.dumps({"run": "parent sort + bamindex", "deflate": form, "repeat": k, "wall_s": round(ws + wi, 3), "sort_wall_s": ws, "bamindex_wall_s": wi}), flush=True)
            for who in (("sort", "parent sort") if k % 2 == 0 else ("parent sort", "sort")):      # side by side, the order swapped every repeat
                _, wp = _timed([cli if who == "sort" else parent, "sort", f"--deflate={form}", "-o", plain, src])
                print(json.dumps({"run": who, "deflate": form, "repeat": k, "wall_s": wp}), flush=True)
        same = open(ours + ".bai", "rb").read() == open(theirs + ".bai", "rb").read() and open(ours, "rb").read() == open(theirs, "rb").read() == open(plain, "rb").read()
        print(json.dumps({"check": "the index is bamindex's, the three BAMs are one", "deflate": form, "ok": same, "index_bytes": os.path.getsize(ours + ".bai")}), flush=True)
    if a.trace:
        os.makedirs(a.trace, exist_ok=True)
        kt = os.path.join(work, "kt")
        r = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", kt, "-o", "run", "--", cli, "sort", "--write-index", "--deflate=device", "-o", ours, src],
                           capture_output=True, text=True, env=dict(os.environ, STRL_TEARDOWN="1"), timeout=900)
        f = glob.glob(os.path.join(kt, "**", "run_kernel_stats.csv"), recursive=True)
        if r.returncode == 0 and f:
            shutil.copy(f[0], os.path.join(a.trace, "kernel_stats_write_index.csv"))
        print(json.dumps({"trace": "kernel_stats_write_index.csv" if (r.returncode == 0 and f) else (r.stderr or "no kernel table")[-500:]}), flush=True)


def _stats_csv(cmd, env, work, dest):
    """cmd under `rocprofv3 --kernel-trace --stats`, a run of its own -> the kernel table copied to dest; its rows by kernel name"""
    kt = os.path.join(work, "kt_" + os.path.basename(dest))
    r = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", kt, "-o", "run", "--", *cmd], capture_output=True, text=True,
                       env=dict(os.environ, STRL_TEARDOWN="1", **env), timeout=900)
    f = glob.glob(os.path.join(kt, "**", "run_kernel_stats.csv"), recursive=True)
    if r.returncode or not f:
        return None, (r.stderr or "no kernel table")[-500:]
    shutil.copy(f[0], dest)
    import csv
    rows = {}
    for row in csv.DictReader(open(dest)):
        rows[row["Name"]] = {"calls": int(row["Calls"]), "total_ms": round(float(row["TotalDurationNs"]) / 1e6, 3)}
    return rows, None


def markdup_runs(a, cli, src, work):
    """`sort --markdup` against the parent's plain `sort` of the same file, alternating; then the host path"""
    parent = a.parent_cli or cli
    ours, theirs, host = (os.path.join(work, n) for n in ("markdup.bam", "parent.bam", "markdup_host.bam"))
    keys = ("markdup_s", "markdup_record_ms", "markdup_join_ms", "markdup_pairs_ms", "markdup_fragments_ms", "markdup_flag_ms", "read_s", "sort_s")
    counts = {}
    for form in ("host", "device"):
        walls = {"sort --markdup": [], "parent sort": []}
        for k in range(a.repeats):
            for who in (("sort --markdup", "parent sort") if k % 2 == 0 else ("parent sort", "sort --markdup")):      # the order swapped every repeat
                if who == "parent sort":
                    _, w = _timed([parent, "sort", f"--deflate={form}", "-o", theirs, src])
                    print(json.dumps({"run": who, "deflate": form, "repeat": k, "wall_s": w}), flush=True)
                else:
                    r, w = _timed([cli, "sort", "--markdup", "-v", f"--deflate={form}", "-o", ours, src])
                    says = json.loads(r.stderr.strip().splitlines()[-1])
                    counts[form] = [l for l in r.stderr.splitlines() if "markdup:" in l][-1]
                    print(json.dumps({"run": who, "deflate": form, "repeat": k, "wall_s": w, **{x: says.get(x) for x in keys}}), flush=True)
                walls[who].append(w)
        med = {who: sorted(v)[len(v) // 2] for who, v in walls.items()}
        print(json.dumps({"summary": "markdup", "deflate": form, "median_wall_s": med,
                          "added_share_of_parent": round((med["sort --markdup"] - med["parent sort"]) / med["parent sort"], 4)}), flush=True)
    r, w = _timed([cli, "sort", "--markdup", "--deflate=host", "-o", ours, src])
    e = dict(os.environ, STRL_SORT="host")
    t = time.time()
    h = subprocess.run([cli, "sort", "--markdup", "-v", "-o", host, src], capture_output=True, text=True, env=e, timeout=3000)
    if h.returncode != 0:
        sys.stderr.write(h.stderr[-4000:])
        sys.exit(h.returncode)
    hc = [l for l in h.stderr.splitlines() if "markdup:" in l][-1]
    print(json.dumps({"run": "STRL_SORT=host sort --markdup", "wall_s": round(time.time() - t, 3), "markdup_s": json.loads(h.stderr.strip().splitlines()[-1]).get("markdup_s")}), flush=True)
    print(json.dumps({"check": "markdup", "device_file_equals_host_file": open(ours, "rb").read() == open(host, "rb").read(), "counts_agree": counts.get("host") == hc == counts.get("device"),
                      "counts": hc}), flush=True)


def windowed_runs(a, cli, src, work, inflated):
    """`sort --windowed` with the windows --window-mb names (default: P = 1, 2, 4 from the inflated size) for both --deflate forms,
    beside --parent-cli's (default: this build's) resident `sort`; and the scatter's group size, each under the profiler once"""
    parent = a.parent_cli or cli
    res, win = os.path.join(work, "resident.bam"), os.path.join(work, "windowed.bam")
    for k in range(a.repeats):
        says, wall = _run([parent, "sort", "-v", "--deflate=host", "-o", res, src])
        print(json.dumps({"run": "parent resident sort", "deflate": "host", "repeat": k, "wall_s": wall, "read_s": says["read_s"], "says": says}), flush=True)
    piece = (128 << 20) // 0xFF00 * 0xFF00           # the CLI's default piece: a window is a whole number of them

    def mb_for(p):
        """MiB of the smallest window limit that cuts this file's stream into p windows (the stream is the input and a few header bytes)"""
        share = -(-(inflated + 4096) // p)
        return -(-share // piece) * piece / 1048576.0

    sizes = [float(x) for x in a.window_mb.split(",") if x] if a.window_mb else [mb_for(p) for p in (1, 2, 4)]
    for form in ("host", "device"):
        for mb in sizes:
            for k in range(a.repeats):
                says, wall = _run([cli, "sort", "--windowed", "-v", f"--deflate={form}", "-o", win, src], dict(os.environ, STRL_SORT_WINDOW_KB=str(mb * 1024)))
                print(json.dumps({"run": "sort --windowed", "deflate": form, "window_mb": mb, "windows": says["windows"], "repeat": k, "wall_s": wall, "pass0_s": says["read_s"],
                                  "per_window_pass_s": round(says["window_s"] / max(1, says["windows"]), 4), "says": says}), flush=True)
            if form == "host":
                print(json.dumps({"check": "the windowed file is the resident sort's", "window_mb": mb, "ok": open(win, "rb").read() == open(res, "rb").read()}), flush=True)
    if a.trace:
        os.makedirs(a.trace, exist_ok=True)
        one = str(mb_for(1) * 1024)
        for lanes in [x for x in a.lanes.split(",") if x]:
            name = "kernel_stats.csv" if lanes == "16" else f"kernel_stats_lanes{lanes}.csv"
            rows, err = _stats_csv([cli, "sort", "--windowed", "--deflate=device", "-o", win, src], {"STRL_SORT_WINDOW_KB": one, "STRL_SORT_GATHER_LANES": lanes}, work,
                                   os.path.join(a.trace, name))
            pick = {k.split("(")[0]: v for k, v in (rows or {}).items() if "bsort_scatter" in k or "bsort_dest" in k}
            for v in pick.values():
                v["TB_per_s_of_stream"] = round(inflated / (v["total_ms"] / 1e3) / 1e12, 3) if v["total_ms"] else None
            print(json.dumps({"trace": name, "windows": 1, "lanes_per_record": int(lanes), "kernels": pick, "error": err}), flush=True)
        for p in (2, 4):
            name = f"kernel_stats_p{p}.csv"
            rows, err = _stats_csv([cli, "sort", "--windowed", "--deflate=device", "-o", win, src], {"STRL_SORT_WINDOW_KB": str(mb_for(p) * 1024)}, work, os.path.join(a.trace, name))
            pick = {k.split("(")[0]: v for k, v in (rows or {}).items() if "bsort_scatter" in k or "bsort_dest" in k}
            print(json.dumps({"trace": name, "windows": p, "kernels": pick, "error": err}), flush=True)


def sam_copy(src, dst):
    """the BAM at src printed as SAM text -> dst; -> text bytes.  Table look-ups a record, not a loop a base"""
    raw = gzip.decompress(open(src, "rb").read())
    l_text = struct.unpack_from("<i", raw, 4)[0]
    at = 8 + l_text
    n_ref = struct.unpack_from("<i", raw, at)[0]
    at += 4
    names = []
    for _ in range(n_ref):
        l = struct.unpack_from("<i", raw, at)[0]
        names.append(raw[at + 4:at + 4 + l - 1])
        at += 8 + l
    code = b"=ACMGRSVTWYHKDBN"
    two = np.array([code[b >> 4] | code[b & 15] << 8 for b in range(256)], np.uint16)
    ops = b"MIDNSHP=X"
    mv = memoryview(raw)
    fixed = struct.Struct("<iiiBBHHHiiii")
    sizes = {67: ("B", 1), 99: ("b", 1), 83: ("H", 2), 115: ("h", 2), 73: ("I", 4), 105: ("i", 4)}
    total = 0
    with open(dst, "wb", buffering=1 << 24) as f:
        f.write(raw[8:8 + l_text])
        total += l_text
        while at < len(raw):
            bs, tid, pos, l_name, mapq, _, n_cig, flag, l_seq, mtid, mpos, tlen = fixed.unpack_from(raw, at)
            q = at + 36
            qname = raw[q:q + l_name - 1]; q += l_name
            cig = b"".join(b"%d%c" % (v >> 4, ops[v & 15]) for v in struct.unpack_from(f"<{n_cig}I", raw, q)) or b"*"; q += 4 * n_cig
            seq = two[np.frombuffer(mv[q:q + (l_seq + 1) // 2], np.uint8)].tobytes()[:l_seq] or b"*"; q += (l_seq + 1) // 2
            ql = np.frombuffer(mv[q:q + l_seq], np.uint8); q += l_seq
            qual = b"*" if not l_seq or ql[0] == 255 else (ql + 33).tobytes()
            tags = []
            end = at + 4 + bs
            while q < end:
                t = raw[q + 2]
                if t in sizes:
                    fmt, sz = sizes[t]
                    tags.append(b"%s:i:%d" % (raw[q:q + 2], struct.unpack_from("<" + fmt, raw, q + 3)[0])); q += 3 + sz
                elif t == 90 or t == 72:
                    e = raw.index(b"\0", q + 3)
                    tags.append(raw[q:q + 2] + (b":Z:" if t == 90 else b":H:") + raw[q + 3:e]); q = e + 1
                elif t == 65:
                    tags.append(raw[q:q + 2] + b":A:" + raw[q + 3:q + 4]); q += 4
                elif t == 102:
                    tags.append(b"%s:f:%s" % (raw[q:q + 2], repr(float(np.float32(struct.unpack_from("<f", raw, q + 3)[0]))).encode())); q += 7
                else:
                    raise ValueError(f"tag type {chr(t)} is not printed here")
            line = b"\t".join([qname, b"%d" % flag, names[tid] if tid >= 0 else b"*", b"%d" % (pos + 1), b"%d" % mapq, cig,
                               b"*" if mtid < 0 else b"=" if mtid == tid else names[mtid], b"%d" % (mpos + 1), b"%d" % tlen, seq, qual] + tags) + b"\n"
            f.write(line)
            total += len(line)
            at = end
    return total


def _zero_bins(path):
    """the file's inflated stream with every record's bin field zeroed"""
    raw = bytearray(gzip.decompress(open(path, "rb").read()))
    at = 8 + struct.unpack_from("<i", raw, 4)[0]
    n_ref = struct.unpack_from("<i", raw, at)[0]
    at += 4
    for _ in range(n_ref):
        at += 8 + struct.unpack_from("<i", raw, at)[0]
    while at < len(raw):
        raw[at + 14:at + 16] = b"\0\0"
        at += 4 + struct.unpack_from("<i", raw, at)[0]
    return bytes(raw)


def sam_runs(a, cli, src, work):
    """SAM text from a file and from a pipe beside the BAM's sort and the host path; the kernels' rates for every group size"""
    parent = a.parent_cli or cli
    t0 = time.time()
    sam = os.path.join(work, "shuffled.sam")
    text_bytes = sam_copy(src, sam)
    print(json.dumps({"sam_text_bytes": text_bytes, "print_s": round(time.time() - t0, 1)}), flush=True)
    out = {t: os.path.join(work, t + ".bam") for t in ("sam_file", "sam_pipe", "bam_parent", "sam_host")}
    keys = ("seconds", "read_s", "sort_s", "gather_s", "deflate_s", "write_s", "lines", "text_bytes", "host_finished", "sam_copy_ms", "sam_scan_ms", "sam_size_ms", "sam_encode_ms")
    for k in range(a.repeats):
        says, wall = _run([cli, "sort", "-v", "-o", out["sam_file"], sam])
        print(json.dumps({"run": "SAM from a file", "repeat": k, "wall_s": wall, "says": {x: says.get(x) for x in keys}}), flush=True)
        t = time.time()
        r = subprocess.run(f"cat {sam} | {cli} sort -v -o {out['sam_pipe']} -", shell=True, capture_output=True, text=True, timeout=1500)
        if r.returncode:
            sys.stderr.write(r.stderr[-2000:]); sys.exit(r.returncode)
        says = json.loads(r.stderr.strip().splitlines()[-1])
        print(json.dumps({"run": "SAM from a pipe", "repeat": k, "wall_s": round(time.time() - t, 3), "says": {x: says.get(x) for x in keys}}), flush=True)
        says, wall = _run([parent, "sort", "-v", "-o", out["bam_parent"], src])
        print(json.dumps({"run": "parent sort of the BAM", "repeat": k, "wall_s": wall, "says": {x: says.get(x) for x in keys[:6]}}), flush=True)
    says, wall = _run([cli, "sort", "-v", "-o", out["sam_host"], sam], dict(os.environ, STRL_SORT="host"))
    print(json.dumps({"run": "STRL_SORT=host on the SAM", "wall_s": wall, "says": {x: says.get(x) for x in keys}}), flush=True)
    same = open(out["sam_file"], "rb").read() == open(out["sam_pipe"], "rb").read() == open(out["sam_host"], "rb").read()
    print(json.dumps({"check": "file, pipe and host path write one file", "ok": same,
                      "the BAM's sort with the bin field aside": _zero_bins(out["sam_file"]) == _zero_bins(out["bam_parent"])}), flush=True)
    for lanes in [x for x in a.lanes.split(",") if x]:
        runs = []
        for k in range(2):
            says, wall = _run([cli, "sort", "-v", "-o", out["sam_file"], sam], dict(os.environ, STRL_SORT_SAM_LANES=lanes))
            runs.append(says)
        s = runs[-1]
        chunks = max(1, -(-s["text_bytes"] // (32 << 20)))
        gbs = lambda ms: round(s["text_bytes"] / ms / 1e6, 1) if ms else None
        print(json.dumps({"kernels": "HIP-event time over all chunks, second run", "lanes_per_line": int(lanes), "text_bytes": s["text_bytes"], "read_s": s["read_s"],
                          "copy_ms": s["sam_copy_ms"], "scan_ms": s["sam_scan_ms"], "size_ms": s["sam_size_ms"], "encode_ms": s["sam_encode_ms"],
                          "GB_per_s_of_text": {"copy": gbs(s["sam_copy_ms"]), "scan": gbs(s["sam_scan_ms"]), "size": gbs(s["sam_size_ms"]), "encode": gbs(s["sam_encode_ms"])},
                          "per_chunk_ms": {"kernels": round((s["sam_scan_ms"] + s["sam_size_ms"] + s["sam_encode_ms"]) / chunks, 3), "copy": round(s["sam_copy_ms"] / chunks, 3)}}), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--pairs", type=int, default=2 ** 20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--trace", default="")
    ap.add_argument("--dir", default=None)
    ap.add_argument("--slab-mb", default="")
    ap.add_argument("--lanes", default="16,32,64")
    ap.add_argument("--write-index", action="store_true")
    ap.add_argument("--parent-cli", default="")
    ap.add_argument("--windowed", action="store_true")
    ap.add_argument("--dense", action="store_true", help="the plain runs with --deflate=dense (and --parent-cli's --deflate=host) beside them")
    ap.add_argument("--sam", action="store_true", help="SAM text as the input, from a file and from a pipe, beside the BAM's sort")
    ap.add_argument("--markdup", action="store_true", help="`sort --markdup` beside --parent-cli's plain sort: the step's times and the time added")
    ap.add_argument("--window-mb", default="", help="with --windowed: comma-separated window sizes in MiB (default: the sizes that give 1, 2 and 4 windows)")
    a = ap.parse_args()
    t0 = time.time()
    inp = e2e_bench.make_input(a.pairs, d=a.dir, level=1)
    work = tempfile.mkdtemp(prefix="sort_bench_", dir=os.path.dirname(inp["bam"]))
    src = os.path.join(work, "shuffled.bam")
    n, inflated = shuffled_copy(inp["bam"], src)
    cli = os.path.join(ROOT, "strling_amd", "lib", "strling")
    base = {"tool": "sort_bench", "reads": n, "inflated_bytes": inflated, "bam_bytes": os.path.getsize(src), "input_s": round(time.time() - t0, 1)}
    print(json.dumps(base), flush=True)
    if a.write_index:
        write_index_runs(a, cli, src, work)
        shutil.rmtree(work, ignore_errors=True)
        return
    if a.markdup:
        markdup_runs(a, cli, src, work)
        shutil.rmtree(work, ignore_errors=True)
        return
    if a.sam:
        sam_runs(a, cli, src, work)
        shutil.rmtree(work, ignore_errors=True)
        return
    if a.windowed:
        windowed_runs(a, cli, src, work, inflated)
        shutil.rmtree(work, ignore_errors=True)
        return
    outs = {}
    forms = [("device_zlib", cli, ["--deflate=host"], {}), ("device_core", cli, ["--deflate=device"], {}), ("host_zlib", cli, ["--deflate=host"], {"STRL_SORT": "host"})]
    if a.dense:
        forms.insert(2, ("device_dense", cli, ["--deflate=dense"], {}))
        if a.parent_cli:
            forms.insert(0, ("parent_device_zlib", a.parent_cli, ["--deflate=host"], {}))
    for k in range(a.repeats):
        for tag, exe, opts, env in forms:
            outs[tag] = os.path.join(work, tag + ".bam")
            says, wall = _run([exe, "sort", "-v", *opts, "-o", outs[tag], src], dict(os.environ, **env))
            print(json.dumps({"run": tag, "repeat": k, "wall_s": wall, "says": says}), flush=True)
    same_file = open(outs["device_zlib"], "rb").read() == open(outs["host_zlib"], "rb").read()
    same_stream = gzip.decompress(open(outs["device_core"], "rb").read()) == gzip.decompress(open(outs["host_zlib"], "rb").read())
    print(json.dumps({"check": "outputs", "device_zlib_file_equals_host_file": same_file, "device_core_stream_equals_host_stream": same_stream,
                      "out_bytes": {t: os.path.getsize(p) for t, p in outs.items()}}), flush=True)
    if a.dense:
        same = gzip.decompress(open(outs["device_dense"], "rb").read()) == gzip.decompress(open(outs["host_zlib"], "rb").read())
        print(json.dumps({"check": "dense", "device_dense_stream_equals_host_stream": same}), flush=True)
        if a.trace:
            os.makedirs(a.trace, exist_ok=True)
            rows, err = _stats_csv([cli, "sort", "--deflate=dense", "-o", outs["device_dense"], src], {}, work, os.path.join(a.trace, "kernel_stats_dense.csv"))
            print(json.dumps({"trace": "kernel_stats_dense.csv" if rows else err}), flush=True)
        shutil.rmtree(work, ignore_errors=True)
        return
    # what allocating the arena costs: the library's own timing of every hipMalloc of 64 MB and more (STRL_ALLOC_TIMING)
    r = subprocess.run([cli, "sort", "-v", "-o", outs["device_zlib"], src], capture_output=True, text=True, env=dict(os.environ, STRL_ALLOC_TIMING="1"), timeout=1500)
    print(json.dumps({"run": "device_zlib", "STRL_ALLOC_TIMING": 1, "hipMalloc": [x for x in r.stderr.splitlines() if "hipMalloc" in x], "says": json.loads(r.stderr.strip().splitlines()[-1])}), flush=True)
    if a.slab_mb:
        says, wall = _run([cli, "sort", "-v", "-o", outs["device_zlib"], src], dict(os.environ, STRL_SORT_SLAB_MB=a.slab_mb))
        print(json.dumps({"run": "device_zlib", "STRL_SORT_SLAB_MB": a.slab_mb, "wall_s": wall, "says": says}), flush=True)
    # the gather alone, through the ABI: one process per group size (the variable is read once)
    code = f"""
import sys, json
sys.path.insert(0, {ROOT!r})
from strling_amd import api
c = api.Context(0)
s, i, p = c.bamsort({src!r}, keep_open=True)
n = min(i['stream_bytes'], (1 << 32) - 65536)
for k in range(3):
    b = c.bamsort_info()['gather_ms']
    c.bamsort_fetch(0, n)
    g = c.bamsort_info()['gather_ms'] - b
    print(json.dumps({{'gather_ms': round(g, 3), 'bytes': n, 'GB_per_s': round(n / g / 1e6, 1), 'sort_ms': round(i['sort_ms'], 3), 'layout_ms': round(i['layout_ms'], 3)}}))
c.bamsort_end()
"""
    if inflated < (1 << 32) - 65536:
        for lanes in [x for x in a.lanes.split(",") if x]:
            r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, STRL_SORT_GATHER_LANES=lanes), timeout=900)
            lines = [json.loads(x) for x in r.stdout.strip().splitlines() if x.startswith("{")]
            print(json.dumps({"gather": "one fetch of the whole stream, three times", "lanes_per_record": int(lanes), "runs": lines, "error": r.stderr[-300:] if r.returncode else None}), flush=True)
    if a.trace:
        os.makedirs(a.trace, exist_ok=True)
        kt = os.path.join(work, "kt")
        r = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", kt, "-o", "run", "--", cli, "sort", "--deflate=device", "-o", outs["device_core"], src],
                           capture_output=True, text=True, env=dict(os.environ, STRL_TEARDOWN="1"), timeout=900)
        f = glob.glob(os.path.join(kt, "**", "run_kernel_stats.csv"), recursive=True)
        if r.returncode == 0 and f:
            shutil.copy(f[0], os.path.join(a.trace, "kernel_stats.csv"))
        print(json.dumps({"trace": "kernel_stats.csv" if (r.returncode == 0 and f) else (r.stderr or "no kernel table")[-500:]}), flush=True)
    shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
