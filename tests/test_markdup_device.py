"""`strling sort --markdup` on the GPU (strling_amd/csrc/markdup.hip): every case of tests/markdup_cases.py byte for byte against the
host path's file (which tests/test_markdup_cases.py holds against the Python reference), again with mates in different arena slabs
and records across chunk seams; the device compressor's modes and SAM input by their inflated streams; the join's refusal of more
than 512 records under one hash; different names under one hash (STRL_MARKDUP_HASH_BITS=4); and the ABI's calls in and out of order."""
import os
import subprocess

import numpy as np
import pytest

import markdup_cases as M
import sort_bam_cases as S
from strling_amd import api, build

pytestmark = pytest.mark.gpu
CLI = build.CLI
NAMES = [name for name, _ in M.cases()]


def _sort(src, out, *opts, **env):
    e = dict(os.environ)
    e.pop("STRL_SORT", None)
    e.update({k: str(v) for k, v in env.items()})
    return subprocess.run([CLI, "sort", *opts, "-o", out, src], capture_output=True, text=True, env=e)


@pytest.fixture(scope="module")
def paths(tmp_path_factory):
    return M.case_dir(tmp_path_factory)


@pytest.fixture(scope="module")
def host_files(paths, tmp_path_factory):
    """the STRL_SORT=host --markdup file of every case, --deflate=host, and the counts it reported"""
    d = tmp_path_factory.mktemp("markdup_host")
    out = {}
    for name, p in paths.items():
        o = os.path.join(str(d), name + ".bam")
        r = _sort(p, o, "--markdup", STRL_SORT="host")
        assert r.returncode == 0, (name, r.stderr)
        out[name] = (open(o, "rb").read(), M.counts_of(r.stderr))
    return out


def _inflated(data):
    return b"".join(raw for _, raw in S.members(data))


# mates in different slabs and records across pushes: chunks of one block, slabs of 0.15 MB (two one-block chunks share one)
SETTINGS = {"defaults": {}, "chunk1_slabs": dict(STRL_CHUNK_BLOCKS=1, STRL_SORT_SLAB_MB=0.15, STRL_SORT_PIECE_KB=1)}


@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("name", NAMES)
def test_device_file_is_the_host_file(name, setting, paths, host_files, tmp_path):
    o = str(tmp_path / "dev.bam")
    r = _sort(paths[name], o, "--markdup", "-v", **SETTINGS[setting])
    assert r.returncode == 0, r.stderr
    assert '"path": "device"' in r.stderr
    want, counts = host_files[name]
    assert M.counts_of(r.stderr) == counts
    assert open(o, "rb").read() == want
    if setting == "chunk1_slabs" and name.startswith(("pairs_", "copies_")):
        assert int(r.stderr.split('"slabs": ')[1].split(",")[0]) >= 3, r.stderr


@pytest.mark.parametrize("mode", ["device", "dense"])
def test_device_compressor_modes_inflate_to_the_same_stream(mode, paths, host_files, tmp_path):
    o = str(tmp_path / "core.bam")
    r = _sort(paths["pairs_2049"], o, "--markdup", f"--deflate={mode}")
    assert r.returncode == 0, r.stderr
    assert _inflated(open(o, "rb").read()) == _inflated(host_files["pairs_2049"][0])


def test_write_index_is_the_host_paths(paths, tmp_path):
    a, b = str(tmp_path / "host.bam"), str(tmp_path / "dev.bam")
    ra, rb = _sort(paths["pairs_2049"], a, "--markdup", "--write-index", STRL_SORT="host"), _sort(paths["pairs_2049"], b, "--markdup", "--write-index")
    assert ra.returncode == 0 and rb.returncode == 0, ra.stderr + rb.stderr
    assert open(a, "rb").read() == open(b, "rb").read() and open(a + ".bai", "rb").read() == open(b + ".bai", "rb").read()


def test_sam_input(paths, tmp_path):
    """the same lines through the device's SAM encoder and through the host's: one stream"""
    recs = dict(M.cases())["random_600"]
    text = "@HD\tVN:1.6\tSO:unsorted\n" + "".join(f"@SQ\tSN:{n}\tLN:{l}\n" for n, l in M.TG)
    for r in recs:
        qual = "".join(chr(33 + q) for q in r["qual"])
        text += "\t".join([r["name"], str(r["flag"]), M.TG[r["tid"]][0], str(r["pos"] + 1), "30", r["cigar"], "=", str(r["pos"] + 1), "0", "A" * r["l_seq"], qual]) + "\n"
    p, a, b = str(tmp_path / "in.sam"), str(tmp_path / "host.bam"), str(tmp_path / "dev.bam")
    open(p, "w").write(text)
    ra, rb = _sort(p, a, "--markdup", STRL_SORT="host"), _sort(p, b, "--markdup", "-v")
    assert ra.returncode == 0 and rb.returncode == 0, ra.stderr + rb.stderr
    assert '"path": "device"' in rb.stderr and '"input": "sam"' in rb.stderr
    assert M.counts_of(ra.stderr) == M.counts_of(rb.stderr) and M.counts_of(rb.stderr)["dup_pairs"] > 0
    assert _inflated(open(a, "rb").read()) == _inflated(open(b, "rb").read())


def test_513_records_under_one_name_are_refused(tmp_path):
    p, o = str(tmp_path / "in.bam"), str(tmp_path / "o.bam")
    M.write_case(p, M.one_name(513))
    r = _sort(p, o, "--markdup")
    assert r.returncode == 1 and not os.path.exists(o) and not [f for f in os.listdir(str(tmp_path)) if ".tmp." in f], r.stderr
    assert "513" in r.stderr and "STRL_SORT=host" in r.stderr and "status -9" in r.stderr, r.stderr
    r = _sort(p, o, "--markdup", STRL_SORT="host")             # the host path has no such limit
    assert r.returncode == 0 and M.counts_of(r.stderr)["fragments"] == 513


@pytest.mark.parametrize("name", ["random_600", "unclip_fr", "two_first_reads", "three_under_a_name"])
def test_different_names_under_one_hash(name, paths, host_files, tmp_path):
    o = str(tmp_path / "dev.bam")
    r = _sort(paths[name], o, "--markdup", STRL_MARKDUP_HASH_BITS=4)
    assert r.returncode == 0, r.stderr
    assert M.counts_of(r.stderr) == host_files[name][1]
    assert open(o, "rb").read() == host_files[name][0]


def test_a_record_that_does_not_fit_its_block_size_is_refused(paths, tmp_path):
    p, o = str(tmp_path / "big.bam"), str(tmp_path / "o.bam")
    M.oversized(paths["unclip_fr"], p, 5)
    r = _sort(p, o, "--markdup")
    assert r.returncode == 1 and not os.path.exists(o), r.stderr
    assert "record 5" in r.stderr and "block_size" in r.stderr and "status -6" in r.stderr, r.stderr


# ---- the ABI through api.py ---------------------------------------------------------------------------------------------------------
def _begin_and_push(ctx, path, windowed=False, markdup=True):
    B = ctx._bam_blocks(path)
    if windowed:
        ctx.bamsort_begin_windowed(B["n_ref"], B["first_off"])
    else:
        ctx.bamsort_begin(B["n_ref"], B["first_off"])
        if markdup:
            ctx.bamsort_markdup_mode(True)
    cb = B["blocks"][B["b0"]:]
    lo, hi = cb[0][0], cb[-1][0] + cb[-1][1]
    comp = np.ascontiguousarray(B["data"][lo:hi])
    tabs = (np.array([b[0] - lo for b in cb], np.uint64), np.array([b[1] for b in cb], np.uint32), np.array([b[2] for b in cb], np.uint32), np.array([b[3] for b in cb], np.uint32))
    ctx.bamsort_push(comp, *tabs)
    return api.bamsort_header(B["header_raw"]), (comp, tabs)


def test_abi_counts_and_stream(ctx, paths, host_files):
    stream, info, _ = ctx.bamsort(paths["pairs_2048"], markdup=True)
    assert stream == _inflated(host_files["pairs_2048"][0])
    assert {k: info["markdup"]["n_" + k] for k in M.COUNT_KEYS} == host_files["pairs_2048"][1]
    assert ctx.bamsort(paths["pairs_2048"])[0] == S.reference_stream(paths["pairs_2048"])[0], "without the step the context sorts as before"


def test_abi_refuses_the_call_out_of_order(ctx, paths, host_files):
    def refused():
        with pytest.raises(api.StrlingError) as e:
            ctx.bamsort_markdup()
        assert e.value.code == -3                               # STRL_ERR_ARG
    p = paths["unclip_fr"]
    try:
        header, keep = _begin_and_push(ctx, p)
        refused()                                               # before the finish
        with pytest.raises(api.StrlingError):
            ctx.bamsort_markdup_mode(True)                      # behind the first push
        info = ctx.bamsort_finish(header)
        got = ctx.bamsort_markdup()
        assert {k: got["n_" + k] for k in M.COUNT_KEYS} == host_files["unclip_fr"][1]
        refused()                                               # twice
        assert ctx.bamsort_fetch(0, info["stream_bytes"]) == _inflated(host_files["unclip_fr"][0])
    finally:
        ctx.bamsort_end()
    try:
        header, keep = _begin_and_push(ctx, p)
        info = ctx.bamsort_finish(header)
        ctx.bamsort_fetch(0, 100)
        refused()                                               # after a fetch
        assert ctx.bamsort_fetch(0, info["stream_bytes"]) == S.reference_stream(p)[0]
    finally:
        ctx.bamsort_end()
    try:
        header, keep = _begin_and_push(ctx, p, windowed=True)
        with pytest.raises(api.StrlingError):
            ctx.bamsort_markdup_mode(True)
        ctx.bamsort_finish(header)
        refused()                                               # a windowed sort holds no records
    finally:
        ctx.bamsort_end()
