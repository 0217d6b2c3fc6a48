"""`strling pull --deflate=device|host` without a device (STRL_PULL=host): the option's forms, the host twin writing the output
(every member checked on its own), the same records as the default run, and the default run unchanged.
tests/test_deflate_device.py has the run on the device."""
import json
import os
import re

import pytest

import deflate_cases as D
from strling_amd import api
from test_pull import bgzf_payload, check_output, pull_expected, run_pull, sample, TARGETS  # noqa: F401  (sample: the fixture)

REGIONS = ["chrA", "chr:B:1-60000"]


def _stats(stderr):
    m = re.search(r"\[strling\] pull: (\{.*\})", stderr)
    assert m, stderr
    return json.loads(m.group(1))


@pytest.fixture(scope="module")
def runs(sample):
    res = {}
    for tag, extra in (("default", []), ("default2", []), ("host", ["--deflate=host"]), ("device", ["--deflate=device"]), ("device_sep", ["--deflate", "device"])):
        out = str(sample["dir"] / f"deflate_{tag}.bam")
        r = run_pull(["-v", "-o", out, sample["bam"]] + REGIONS + extra, mode="host")
        assert r.returncode == 0, r.stderr
        res[tag] = (out, r, open(out, "rb").read())
    return res


def test_the_default_is_the_host_s_zlib_and_has_not_changed(runs, sample):
    a, b, h = runs["default"][2], runs["default2"][2], runs["host"][2]
    assert a == b == h
    s = _stats(runs["default"][1].stderr)
    assert s["deflate"] == "zlib" and s["deflate_stored_blocks"] == 0 and s["deflate_kernel_ms"] == 0
    exp = pull_expected(sample["header"], sample["recs"], len(TARGETS), [(0, 0, 2**31 - 1), (1, 0, 60_000)])[0]
    check_output(runs["default"][0], exp, sample["n_hdr"])


def test_deflate_device_without_a_device_runs_the_twin(runs, sample):
    out, r, data = runs["device"]
    want = bgzf_payload(runs["default"][0], max_block=0xFF00)
    assert bgzf_payload(out, max_block=0xFF00) == want
    exp = pull_expected(sample["header"], sample["recs"], len(TARGETS), [(0, 0, 2**31 - 1), (1, 0, 60_000)])[0]
    check_output(out, exp, sample["n_hdr"])
    # the file is the twin's members and the EOF block, each member valid on its own
    members, csize, stored = api.bgzf_deflate_host(want)
    assert data == members + D.EOF_BLOCK and csize.size >= 2
    D.check_members(want, D.BLK, data[:-28], csize, stored)
    s = _stats(r.stderr)
    assert s["deflate"] == "core-host" and s["deflate_stored_blocks"] == stored and s["deflate_kernel_ms"] == 0
    assert "[strling] pull: deflating the output on the host (STRL_PULL=host)" in r.stderr
    assert runs["device_sep"][2] == data
    assert len(data) > len(runs["default"][2]), "zlib's default level parses harder than the device form's greedy parse"


def test_several_calls_write_the_bytes_of_one(runs, sample):
    """STRL_DEFLATE_BATCH_MB cuts the payload on whole blocks (here one block a call): the seam between two calls"""
    out = str(sample["dir"] / "deflate_cut.bam")
    os.environ["STRL_DEFLATE_BATCH_MB"] = "0.07"
    try:
        r = run_pull(["-o", out, sample["bam"]] + REGIONS + ["--deflate=device"], mode="host")
    finally:
        del os.environ["STRL_DEFLATE_BATCH_MB"]
    assert r.returncode == 0, r.stderr
    assert open(out, "rb").read() == runs["device"][2]


def test_other_values_are_usage_errors(sample):
    for bad in ("--deflate=zip", "--deflate=", "--deflate=Device"):
        r = run_pull(["-o", str(sample["dir"] / "bad.bam"), sample["bam"], "chrA", bad], mode="host")
        assert r.returncode != 0 and "--deflate must be host or device" in r.stderr and "Usage:" in r.stderr, r.stderr


def test_the_usage_text_names_the_option():
    r = run_pull(["--help"])
    assert r.returncode == 0 and "--deflate=host|device" in r.stdout and "level" in r.stdout
