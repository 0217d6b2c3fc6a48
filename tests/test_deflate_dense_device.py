"""The dense mode of the BGZF compressor on the device (strl_bgzf_deflate_mode, csrc/deflate.hip: deflate_dense_kernel) against its
host twin, byte for byte, over the inputs of tests/test_deflate_dense_cases.py (which checks the twin against zlib and a model of
the rule), the 19-block payload and a call with more blocks than workgroups; its output through the device inflate; and
`strling pull` / `strling sort --deflate=dense` against the host path's files."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import deflate_cases as D
import sort_index_cases as X
from strling_amd import api, bamio, build
from test_deflate_dense_cases import dense_inputs
from test_pull import bgzf_payload, run_pull

pytestmark = pytest.mark.gpu
CLI = build.CLI
MANY = 513 * 256 + 100          # 514 blocks of 256 bytes, the last one short: more than the 512 workgroups of a launch


def _many_blocks():
    r = np.random.default_rng(31)
    return bytes(r.choice(np.frombuffer(b"ACGT", np.uint8), MANY))


@pytest.fixture(scope="module")
def twin():
    """the dense twin's output for every input, for the fixture and for the many blocks, made once"""
    res = {name: api.bgzf_deflate_host(data, block, mode="dense") for name, data, block in dense_inputs()}
    res["fixture"] = api.bgzf_deflate_host(D.fixture_payload(), mode="dense")
    res["many_blocks"] = api.bgzf_deflate_host(_many_blocks(), 256, mode="dense")
    return res


def _same(got, want):
    assert got[0] == want[0] and np.array_equal(got[1], want[1]) and got[2] == want[2]


@pytest.mark.parametrize("case", dense_inputs(), ids=[c[0] for c in dense_inputs()])
def test_device_equals_twin(ctx, twin, case):
    name, data, block = case
    _same(ctx.bgzf_deflate(data, block, mode="dense"), twin[name])


def test_the_fixture_and_more_blocks_than_workgroups(ctx, twin):
    _same(ctx.bgzf_deflate(D.fixture_payload(), mode="dense"), twin["fixture"])
    assert twin["many_blocks"][1].size == 514
    _same(ctx.bgzf_deflate(_many_blocks(), 256, mode="dense"), twin["many_blocks"])       # a workgroup compresses several blocks in turn


def test_repeated_and_interleaved_calls_and_a_second_context(ctx, twin):
    """no table left over from the call before, whichever mode it ran in; no dependence on the order the workgroups run in"""
    p = D.fixture_payload()
    fast = api.bgzf_deflate_host(p)
    for _ in range(2):
        _same(ctx.bgzf_deflate(p, mode="dense"), twin["fixture"])
    _same(ctx.bgzf_deflate(p), fast)
    _same(ctx.bgzf_deflate(b"\0" * D.BLK, mode="dense"), twin["zeros_full_block"])
    _same(ctx.bgzf_deflate(p, mode="fast"), fast)
    _same(ctx.bgzf_deflate(p, mode="dense"), twin["fixture"])
    assert ctx.deflate_ms() > 0
    other = api.Context(0)
    try:
        _same(other.bgzf_deflate(p, mode="dense"), twin["fixture"])
    finally:
        other.close()


def test_device_inflate_reads_what_the_dense_mode_wrote(ctx):
    streams, sizes, want = [], [], []
    for name, data, block in dense_inputs() + (("fixture", D.fixture_payload(), D.BLK),):
        if name == "small_blocks":
            data = data[:40 * 256]
        out, csize, _ = ctx.bgzf_deflate(data, block, mode="dense")
        for k, m in enumerate(D.members_of(out, csize)):
            streams.append(m[18:-8])
            want.append(data[k * block:(k + 1) * block])
            sizes.append(len(want[-1]))
    got = ctx.inflate_blocks(streams, sizes)
    assert len(got) == len(want) and all(g == w for g, w in zip(got, want))


def test_refusals_leave_the_buffer_alone(ctx):
    data = D.fixture_payload()[:100_000]
    out = np.full(D.bound(len(data), D.BLK) + 64, 0xA5, np.uint8)
    got, _, _ = ctx.bgzf_deflate(data, D.BLK, out=out, mode="dense")
    assert len(got) < len(data) and (out[len(got):] == 0xA5).all()
    out[:] = 0xA5
    with pytest.raises(api.StrlingError) as e:
        ctx.bgzf_deflate(data, D.BLK, out=out[:D.bound(len(data), D.BLK) - 1], mode="dense")
    assert e.value.code == -4 and (out == 0xA5).all()
    for block, mode in ((0, "dense"), (0xFF01, "dense"), (D.BLK, 2), (D.BLK, -1)):
        with pytest.raises(api.StrlingError) as e:
            ctx.bgzf_deflate(data, block, out=out, mode=mode)
        assert e.value.code == -3 and (out == 0xA5).all()


# ---- the commands --------------------------------------------------------------------------------------------------------------
def _pull_stats(stderr):
    m = re.search(r"\[strling\] pull: (\{.*\})", stderr)
    assert m, stderr
    return json.loads(m.group(1))


def test_pull_deflate_dense(tmp_path):
    from test_pull_device import REGIONS, _records
    path = str(tmp_path / "in.bam")
    bamio.write_bam(path, _records())
    outs = {}
    for tag, mode, env in (("host_path", "host", {}), ("device", None, {}), ("split", None, {"STRL_DEFLATE_BATCH_MB": "0.25"})):
        outs[tag] = str(tmp_path / f"{tag}.bam")
        os.environ.update(env)
        try:
            r = run_pull(["-v", "-o", outs[tag], path] + REGIONS + ["--deflate=dense"], mode=mode)
        finally:
            for k in env:
                os.environ.pop(k, None)
        assert r.returncode == 0, r.stderr
        s = _pull_stats(r.stderr)
        assert s["deflate"] == ("core-host-dense" if tag == "host_path" else "device-dense"), r.stderr
        assert (s["deflate_kernel_ms"] > 0) == (tag != "host_path")
    want = open(outs["host_path"], "rb").read()
    assert len(bgzf_payload(outs["host_path"], max_block=0xFF00)) > (1 << 19), "the payload must be cut into several calls of four blocks"
    assert open(outs["device"], "rb").read() == want and open(outs["split"], "rb").read() == want


def _sort(src, out, *opts, **env):
    e = dict(os.environ)
    e.pop("STRL_SORT", None)
    e.update({k: str(v) for k, v in env.items()})
    return subprocess.run([CLI, "sort", "--deflate=dense", "--write-index", "-v", *opts, "-o", out, src], capture_output=True, text=True, env=e)


@pytest.mark.parametrize("windowed", [False, True])
@pytest.mark.parametrize("name", ["uniform_shuffle", "one_300kb_record"])
def test_sort_deflate_dense(name, windowed, tmp_path_factory, tmp_path):
    """resident and --windowed, each with --write-index: the host path's dense file and index, byte for byte, and bamindex's index"""
    src = X.case_dir(tmp_path_factory)[name]
    dev, host, ref = str(tmp_path / "dev.bam"), str(tmp_path / "host.bam"), str(tmp_path / "ref.bai")
    opts, env = (["--windowed"], dict(STRL_SORT_WINDOW_KB=192, STRL_SORT_PIECE_KB=64, STRL_CHUNK_BLOCKS=2)) if windowed else ([], {})
    r = _sort(src, dev, *opts, **env)
    assert r.returncode == 0, r.stderr
    info = json.loads(r.stderr.strip().splitlines()[-1])
    assert info["path"] == "device" and info["deflate"] == "device-dense" and (info["windows"] >= 2) == windowed, r.stderr
    h = _sort(src, host, STRL_SORT="host")
    assert h.returncode == 0 and json.loads(h.stderr.strip().splitlines()[-1])["deflate"] == "core-host-dense", h.stderr
    assert open(dev, "rb").read() == open(host, "rb").read()
    assert open(dev + ".bai", "rb").read() == open(host + ".bai", "rb").read()
    b = subprocess.run([CLI, "bamindex", "-o", ref, dev], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    assert open(dev + ".bai", "rb").read() == open(ref, "rb").read()
