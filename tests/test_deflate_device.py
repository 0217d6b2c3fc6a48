"""The BGZF compressor on the device (strl_bgzf_deflate, csrc/deflate.hip) against its host twin, byte for byte, over the inputs of
tests/deflate_cases.py and the 19-block payload; its output through the device inflate; and `strling pull --deflate=device`."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import deflate_cases as D
from strling_amd import api, bamio
from test_pull import CLI, bgzf_payload, run_pull

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def twin():
    """the host twin's output for every case and for the fixture, made once"""
    res = {name: api.bgzf_deflate_host(data, block) for name, data, block in D.cases()}
    res["fixture"] = api.bgzf_deflate_host(D.fixture_payload())
    return res


def _same(got, want):
    assert got[0] == want[0] and np.array_equal(got[1], want[1]) and got[2] == want[2]


@pytest.mark.parametrize("case", D.cases(), ids=[c[0] for c in D.cases()])
def test_device_equals_twin(ctx, twin, case):
    name, data, block = case
    got = ctx.bgzf_deflate(data, block)
    _same(got, twin[name])
    D.check_members(data, block, *got)


def test_repeated_calls_and_a_second_context_give_the_same_bytes(ctx, twin):
    """no table left over from the call before, no dependence on the order the workgroups run in"""
    p = D.fixture_payload()
    for _ in range(3):
        _same(ctx.bgzf_deflate(p), twin["fixture"])
    _same(ctx.bgzf_deflate(b"\0" * D.BLK), twin["zeros"])                  # another shape in between: the buffers are reused
    _same(ctx.bgzf_deflate(p), twin["fixture"])
    other = api.Context(0)
    try:
        _same(other.bgzf_deflate(p), twin["fixture"])
    finally:
        other.close()
    assert twin["fixture"][2] == 0 and ctx.deflate_ms() > 0


def test_device_inflate_reads_what_the_device_wrote(ctx, twin):
    """dynamic blocks zlib did not write, with one and with no distance code among them, through inflate_wave.h"""
    streams, sizes, want = [], [], []
    for name, data, block in D.cases() + (("fixture", D.fixture_payload(), D.BLK),):
        out, csize, _ = ctx.bgzf_deflate(data, block)
        for k, m in enumerate(D.members_of(out, csize)):
            streams.append(m[18:-8])
            want.append(data[k * block:(k + 1) * block])
            sizes.append(len(want[-1]))
    got = ctx.inflate_blocks(streams, sizes)
    assert len(got) == len(want) and all(g == w for g, w in zip(got, want))


def test_refusals_leave_the_buffer_alone(ctx):
    data = D.fixture_payload()[:100_000]
    out = np.full(D.bound(len(data), D.BLK) + 64, 0xA5, np.uint8)
    got, _, _ = ctx.bgzf_deflate(data, D.BLK, out=out)
    assert len(got) < len(data) and (out[len(got):] == 0xA5).all()
    out[:] = 0xA5
    with pytest.raises(api.StrlingError) as e:
        ctx.bgzf_deflate(data, D.BLK, out=out[:D.bound(len(data), D.BLK) - 1])
    assert e.value.code == -4 and (out == 0xA5).all()
    for block in (0, 0xFF01):
        with pytest.raises(api.StrlingError) as e:
            ctx.bgzf_deflate(data, block, out=out)
        assert e.value.code == -3 and (out == 0xA5).all()


# ---- the command -------------------------------------------------------------------------------------------------------------
def _stats(stderr):
    m = re.search(r"\[strling\] pull: (\{.*\})", stderr)
    assert m, stderr
    return json.loads(m.group(1))


@pytest.fixture(scope="module")
def bam(tmp_path_factory):
    from test_pull_device import _records
    d = tmp_path_factory.mktemp("pulldeflate")
    path = str(d / "in.bam")
    bamio.write_bam(path, _records())
    return d, path


def test_pull_deflate_device(bam):
    from test_pull_device import REGIONS
    d, path = bam
    outs = {}
    for tag, extra, env in (("host", [], {}), ("device", ["--deflate=device"], {}), ("split", ["--deflate=device"], {"STRL_DEFLATE_BATCH_MB": "0.25"})):
        outs[tag] = str(d / f"{tag}.bam")
        os.environ.update(env)
        try:
            r = run_pull(["-v", "-o", outs[tag], path] + REGIONS + extra)
        finally:
            for k in env:
                os.environ.pop(k, None)
        assert r.returncode == 0, r.stderr
        s = _stats(r.stderr)
        assert s["deflate"] == ("zlib" if tag == "host" else "device"), r.stderr
        if tag != "host":
            assert s["deflate_kernel_ms"] > 0 and s["deflate_stored_blocks"] == 0
    want = bgzf_payload(outs["host"], max_block=0xFF00)
    assert len(want) > (1 << 19), "the payload must be cut into several calls of four blocks"
    assert bgzf_payload(outs["device"], max_block=0xFF00) == want
    assert open(outs["split"], "rb").read() == open(outs["device"], "rb").read()
    assert open(outs["device"], "rb").read() == api.bgzf_deflate_host(want)[0] + D.EOF_BLOCK
    a = subprocess.run([CLI, "_dump", outs["device"]], capture_output=True, text=True)
    b = subprocess.run([CLI, "_dump", outs["host"]], capture_output=True, text=True)
    assert a.returncode == 0 and a.stdout == b.stdout and a.stdout.count("\n") > 1000
