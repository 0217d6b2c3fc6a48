"""`strling fastq` on the GPU (strling_amd/csrc/fastq.hip): every case of tests/fastq_cases.py byte for byte against the host path's
files (which tests/test_fastq_cases.py holds against the Python reference), again with mates in different arena slabs and records
across chunk seams; through the ABI every stream whole and in pieces that cut entries at every offset relative to the 16-byte words;
different names under one hash (STRL_FASTQ_HASH_BITS=4); the join's refusal of more than 512 records under one hash; small pieces
and stdout through the CLI; and the ABI's calls in and out of order."""
import os
import subprocess

import numpy as np
import pytest

import fastq_cases as Q
from strling_amd import api, build

pytestmark = pytest.mark.gpu
CLI = build.CLI
CASES = {name: (recs, opts, sam) for name, recs, opts, sam in Q.cases()}
NAMES = list(CASES)
PIECES = (1, 7, 15, 16, 17, 64, 4096)


def _fastq(src, out_dir, opts, stdout=False, **env):
    e = dict(os.environ)
    e.pop("STRL_FASTQ", None)
    e.update({k: str(v) for k, v in env.items()})
    args, files = Q.cli_options(opts, out_dir, stdout=stdout)
    r = subprocess.run([CLI, "fastq", "--verbose", *args, src], capture_output=True, env=e)
    return r, files


@pytest.fixture(scope="module")
def paths(tmp_path_factory):
    return Q.case_dir(tmp_path_factory)


@pytest.fixture(scope="module")
def host_files(paths, tmp_path_factory):
    """the STRL_FASTQ=host files of every case, and the counts it reported"""
    d = tmp_path_factory.mktemp("fastq_host")
    out = {}
    for name, p in paths.items():
        od = os.path.join(str(d), name)
        os.mkdir(od)
        r, files = _fastq(p, od, CASES[name][1], STRL_FASTQ="host")
        assert r.returncode == 0, (name, r.stderr)
        out[name] = ({k: open(f, "rb").read() for k, f in files.items()}, Q.counts_of(r.stderr.decode()))
    return out


# mates in different slabs and records across pushes: chunks of one block, slabs of 0.15 MB, pieces that cut entries
SETTINGS = {"defaults": {}, "chunk1_slabs": dict(STRL_CHUNK_BLOCKS=1, STRL_SORT_SLAB_MB=0.15, STRL_FASTQ_PIECE_KB=3)}


@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("name", NAMES)
def test_device_files_are_the_host_files(name, setting, paths, host_files, tmp_path):
    r, files = _fastq(paths[name], str(tmp_path), CASES[name][1], **SETTINGS[setting])
    err = r.stderr.decode()
    assert r.returncode == 0, err
    assert '"path": "device"' in err
    want, counts = host_files[name]
    assert Q.counts_of(err) == counts
    for k, f in files.items():
        assert open(f, "rb").read() == want[k], k
    if setting == "chunk1_slabs" and name.startswith("random_"):
        assert int(err.split('"slabs": ')[1].split(",")[0]) >= 2, err      # (a shuffled file over two slabs: about half the pairs have their mates in different ones)


@pytest.mark.parametrize("name", ["random_3000", "flags", "names", "flags_filter_0"])
def test_different_names_under_one_hash(name, paths, host_files, tmp_path):
    r, files = _fastq(paths[name], str(tmp_path), CASES[name][1], STRL_FASTQ_HASH_BITS=4)
    assert r.returncode == 0, r.stderr
    assert Q.counts_of(r.stderr.decode()) == host_files[name][1]
    for k, f in files.items():
        assert open(f, "rb").read() == host_files[name][0][k], k


def test_sam_input(paths, host_files, tmp_path):
    r, files = _fastq(paths["random_3000"][:-4] + ".sam", str(tmp_path), CASES["random_3000"][1])
    err = r.stderr.decode()
    assert r.returncode == 0 and '"path": "device"' in err and '"input": "sam"' in err, err
    for k, f in files.items():
        assert open(f, "rb").read() == host_files["random_3000"][0][k], k


def test_small_pieces_and_stdout(paths, host_files, tmp_path):
    """pieces of 100 bytes, and -o - read from the pipe"""
    opts = dict(CASES["lengths"][1], singles=False)
    r, _ = _fastq(paths["lengths"], str(tmp_path), opts, stdout=True, STRL_FASTQ_PIECE_KB=0.1)
    assert r.returncode == 0, r.stderr
    assert r.stdout == host_files["lengths"][0]["p1"]
    c = Q.counts_of(r.stderr.decode())
    assert c["singles_unwritten"] == c["singles"] == host_files["lengths"][1]["singles"] > 0


def test_512_records_under_one_name_pass_and_513_are_refused(paths, host_files, tmp_path):
    assert host_files["one_name_512"][1]["singles"] == 512      # (the 512 have passed in test_device_files_are_the_host_files)
    p = str(tmp_path / "in.bam")
    Q.write_case(p, Q.one_name(513))
    r, files = _fastq(p, str(tmp_path), Q.DEFAULTS)
    err = r.stderr.decode()
    assert r.returncode == 1 and not [f for f in os.listdir(str(tmp_path)) if f != "in.bam"], err
    assert "513" in err and "STRL_FASTQ=host" in err and "status -9" in err, err
    r, files = _fastq(p, str(tmp_path), Q.DEFAULTS, STRL_FASTQ="host")      # the host path has no such limit
    assert r.returncode == 0 and Q.counts_of(r.stderr.decode())["singles"] == 513


def test_a_record_that_does_not_fit_its_block_size_is_refused(paths, tmp_path):
    """a read of 255 bases said to have 295: its bases still fit its block_size, so the front end's record scan passes it, and
    its qualities do not"""
    p = str(tmp_path / "big.bam")
    Q.oversized(paths["lengths"], p, 50)
    r, files = _fastq(p, str(tmp_path), Q.DEFAULTS)
    err = r.stderr.decode()
    assert r.returncode == 1 and not [f for f in os.listdir(str(tmp_path)) if f != "big.bam"], err
    assert "record 50" in err and "block_size" in err and "status -6" in err, err


# ---- the ABI through api.py ---------------------------------------------------------------------------------------------------------
def _begin_and_push(ctx, path, windowed=False, fastq=True, markdup=False):
    B = ctx._bam_blocks(path)
    if windowed:
        ctx.bamsort_begin_windowed(B["n_ref"], B["first_off"])
    else:
        ctx.bamsort_begin(B["n_ref"], B["first_off"])
        if markdup:
            ctx.bamsort_markdup_mode(True)
        if fastq:
            ctx.bamsort_fastq_mode(True)
    cb = B["blocks"][B["b0"]:]
    if cb:
        lo, hi = cb[0][0], cb[-1][0] + cb[-1][1]
        comp = np.ascontiguousarray(B["data"][lo:hi])
        tabs = (np.array([b[0] - lo for b in cb], np.uint64), np.array([b[1] for b in cb], np.uint32), np.array([b[2] for b in cb], np.uint32), np.array([b[3] for b in cb], np.uint32))
        ctx.bamsort_push(comp, *tabs)
    return api.bamsort_header(B["header_raw"])


@pytest.mark.parametrize("name", ["lengths", "lengths_split", "names_suffix", "flags_filter_0", "order_split", "random_3000"])
def test_abi_streams_whole_and_in_pieces(name, ctx, paths):
    """each stream fetched whole, then in pieces of 1 .. 4096 bytes from lo = 0 and lo = 5: the pieces cut entries at every byte
    offset relative to the 16-byte words of the piece; a canary on both sides of the destination stays untouched"""
    recs, opts, _ = CASES[name]
    want, counts = Q.reference(recs, opts)
    try:
        header = _begin_and_push(ctx, paths[name])
        ctx.bamsort_finish(header)
        info = ctx.bamsort_fastq(**Q.abi_options(opts))
        assert {k: info["n_" + k] for k in Q.COUNT_KEYS} == counts
        for s, key in enumerate(("p1", "p2", "s")):
            total = info["stream_bytes"][s]
            assert total == len(want[key]), key
            assert ctx.bamsort_fastq_fetch(s, 0, total, canary=64) == want[key], key
            for piece in PIECES:
                if name == "random_3000" and piece < 64:
                    continue                                    # (tens of thousands of tiny fetches: the small cases cover them)
                for lo0 in (0, 5):
                    got = [want[key][:lo0]] + [ctx.bamsort_fastq_fetch(s, lo, min(piece, total - lo), canary=32) for lo in range(lo0, total, piece)]
                    assert b"".join(got)[:total] == want[key], (key, piece, lo0)
        assert ctx.bamsort_fastq_info()["text_bytes"] > 0
    finally:
        ctx.bamsort_end()


def test_abi_refuses_the_calls_out_of_order(ctx, paths):
    def refused(call, *a, **kw):
        with pytest.raises(api.StrlingError) as e:
            call(*a, **kw)
        assert e.value.code == -3                               # STRL_ERR_ARG
    p = paths["flags"]
    o = Q.abi_options(Q.DEFAULTS)
    try:
        header = _begin_and_push(ctx, p)
        refused(ctx.bamsort_fastq, **o)                         # before the finish
        refused(ctx.bamsort_fastq_mode, True)                   # behind the first push
        info = ctx.bamsort_finish(header)
        refused(ctx.bamsort_fastq_fetch, 0, 0, 1)               # before the plan
        got = ctx.bamsort_fastq(**o)
        refused(ctx.bamsort_fastq, **o)                         # twice
        refused(ctx.bamsort_fastq_fetch, 3, 0, 1)               # no such stream
        refused(ctx.bamsort_fastq_fetch, 0, got["stream_bytes"][0], 1)      # past the end
        refused(ctx.bamsort_fastq_fetch, 1, 0, 1)               # interleaved: p2 is empty
        assert ctx.bamsort_fastq_fetch(0, got["stream_bytes"][0], 0) == b""
        assert len(ctx.bamsort_fetch(0, info["stream_bytes"])) == info["stream_bytes"], "the sorted stream is still there"
    finally:
        ctx.bamsort_end()
    try:
        header = _begin_and_push(ctx, p, fastq=False)
        ctx.bamsort_finish(header)
        refused(ctx.bamsort_fastq, **o)                         # without the mode
    finally:
        ctx.bamsort_end()
    try:
        B = ctx._bam_blocks(p)
        ctx.bamsort_begin(B["n_ref"], B["first_off"])
        ctx.bamsort_markdup_mode(True)
        refused(ctx.bamsort_fastq_mode, True)                   # not together with markdup
        ctx.bamsort_markdup_mode(False)
        ctx.bamsort_fastq_mode(True)
        refused(ctx.bamsort_markdup_mode, True)
    finally:
        ctx.bamsort_end()


def test_a_windowed_sort_is_refused(ctx, paths):
    try:
        B = ctx._bam_blocks(paths["flags"])
        ctx.bamsort_begin_windowed(B["n_ref"], B["first_off"])
        with pytest.raises(api.StrlingError) as e:
            ctx.bamsort_fastq_mode(True)
        assert e.value.code == -3
    finally:
        ctx.bamsort_end()
    try:
        header = _begin_and_push(ctx, paths["flags"], windowed=True)
        ctx.bamsort_finish(header)
        with pytest.raises(api.StrlingError) as e:
            ctx.bamsort_fastq(**Q.abi_options(Q.DEFAULTS))
        assert e.value.code == -3
    finally:
        ctx.bamsort_end()
