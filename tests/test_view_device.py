"""`strling view` on the GPU (strling_amd/csrc/view.hip): every case of tests/view_cases.py byte for byte against the host path's
output (which tests/test_view_cases.py holds against the Python reference), at the defaults and again with one BGZF block a chunk, so
that records cross chunk seams and chunks drop to zero text bytes; strl_view_records with a canary on both sides of its room;
host_chunks == 0 wherever no float is hard -- the condition that keeps the host fallback from hiding the kernels -- and exactly the
chunks that hold a hard float otherwise; the regions; the refusals in the host's words, with the context usable afterwards; and the
ABI's calls out of order."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import view_cases as V
from strling_amd import api, build

pytestmark = pytest.mark.gpu
CLI = build.CLI
CASES = V.cases()
GOOD = [n for n in CASES if not CASES[n]["refused"]]
BAD = [n for n in CASES if CASES[n]["refused"]]
REF_NAMES = [n for n, _ in V.TG]
SETTINGS = {"defaults": {}, "chunk1": dict(STRL_CHUNK_BLOCKS=1)}


def _view(args, **env):
    e = dict(os.environ)
    e.pop("STRL_VIEW", None)
    e.update({k: str(v) for k, v in env.items()})
    return subprocess.run([CLI, "view", "--verbose", *args], capture_output=True, env=e)


def _field(err, key):
    return int(re.search(r'"%s": (\d+)' % key, err).group(1))


@pytest.fixture(scope="module")
def paths(tmp_path_factory):
    return V.case_dir(tmp_path_factory)


@pytest.fixture(scope="module")
def host_text(paths):
    out = {}
    for name in GOOD:
        r = _view(V.cli_options(CASES[name]["opts"]) + [paths[name]], STRL_VIEW="host")
        assert r.returncode == 0 and b'"path": "host"' in r.stderr, (name, r.stderr)
        out[name] = (r.stdout, _field(r.stderr.decode(), "written"), _field(r.stderr.decode(), "dropped"))
    return out


@pytest.fixture(scope="module")
def regions_bam(tmp_path_factory):
    return V.regions_bam(str(tmp_path_factory.mktemp("view_regions")), CLI)


@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("name", GOOD)
def test_device_text_is_the_host_text(name, setting, paths, host_text, tmp_path):
    c = CASES[name]
    o = str(tmp_path / "out.sam")
    r = _view(V.cli_options(c["opts"]) + ["-o", o, paths[name]], **SETTINGS[setting])
    err = r.stderr.decode()
    assert r.returncode == 0, err
    assert '"path": "device"' in err
    want, written, dropped = host_text[name]
    assert open(o, "rb").read() == want
    assert (_field(err, "written"), _field(err, "dropped"), _field(err, "text_bytes")) == (written, dropped, len(want))
    hard_chunks = 0 if not c["hard"] else 1 if setting == "defaults" else V.chunks_with(c["recs"], c["block"], set(c["hard"]))
    assert _field(err, "host_chunks") == hard_chunks, "the kernels wrote every chunk without a hard float, the host twin exactly the others"
    if setting == "chunk1" and c["recs"]:
        assert _field(err, "chunks") >= 2 or len(V.raw_bam(c["recs"])) <= c["block"]


def test_the_float_case_has_hard_and_plain_chunks():
    c = CASES["floats_hard"]
    n_blocks = -(-len(V.raw_bam(c["recs"])) // c["block"])
    assert 2 <= V.chunks_with(c["recs"], c["block"], set(c["hard"])) < n_blocks - 1


@pytest.mark.parametrize("name", GOOD)
def test_records_entry_writes_inside_its_room_only(ctx, name, host_text):
    c = CASES[name]
    want = host_text[name][0]
    text, info, before, behind = ctx.view_records(b"".join(c["recs"]), REF_NAMES, cap=len(want), guard=64, **V.abi_options(c["opts"]))
    assert text == want and before == b"\xa5" * 64 and behind == b"\xa5" * 64
    assert info["written"] == host_text[name][1] and info["host_chunks"] == (1 if c["hard"] else 0)
    if want:
        with pytest.raises(api.StrlingError) as e:
            ctx.view_records(b"".join(c["recs"]), REF_NAMES, cap=len(want) - 1, guard=64, **V.abi_options(c["opts"]))
        assert e.value.code == -4
        assert ctx.view_records(b"".join(c["recs"]), REF_NAMES, **V.abi_options(c["opts"]))[0] == want, "the need comes back and is enough"


def test_the_library_streams_a_file(ctx, paths, host_text):
    for chunk_blocks in (16384, 1, 3):
        text, info = ctx.view(paths["random_3000"], chunk_blocks=chunk_blocks)
        assert text == host_text["random_3000"][0] and info["host_chunks"] == 0 and info["written"] == 3000
        assert info["size_ms"] > 0 and info["text_ms"] > 0


@pytest.mark.parametrize("regions", V.REGIONS, ids=["+".join(r) for r in V.REGIONS])
def test_regions_against_the_host_path(regions, regions_bam):
    host = _view([regions_bam] + regions, STRL_VIEW="host")
    dev = _view([regions_bam] + regions)
    assert host.returncode == 0 and dev.returncode == 0, dev.stderr
    assert b'"path": "device"' in dev.stderr and dev.stdout == host.stdout
    assert dev.stdout == V.regions_reference(V.region_records(), V.DEFAULTS, regions)[0]
    assert _field(dev.stderr.decode(), "host_chunks") == 0


@pytest.mark.parametrize("batch", [1, 3])
def test_regions_in_small_batches(batch, regions_bam):
    """a region fed a few records at a time (as a region larger than a batch is): the same text, the same counts, through the kernels"""
    for regions in V.REGIONS:
        want, written = V.regions_reference(V.region_records(), V.DEFAULTS, regions)
        dev = _view([regions_bam] + regions, STRL_VIEW_BATCH_RECORDS=batch)
        assert dev.returncode == 0 and b'"path": "device"' in dev.stderr and dev.stdout == want, dev.stderr
        assert _field(dev.stderr.decode(), "host_chunks") == 0 and _field(dev.stderr.decode(), "written") == written
        cnt = _view(["-c", regions_bam] + regions, STRL_VIEW_BATCH_RECORDS=batch)
        assert cnt.stdout == b"%d\n" % written and _field(cnt.stderr.decode(), "text_bytes") == 0


def test_count_only_runs_no_text_kernel(ctx, paths, host_text):
    """-c: the size kernel's counts; neither text kernel time nor text bytes, also where a chunk holds a hard float"""
    for name in ("random_3000", "filter_q", "floats_hard", "no_record"):
        for setting in SETTINGS.values():
            r = _view(V.cli_options(CASES[name]["opts"]) + ["-c", paths[name]], **setting)
            err = r.stderr.decode()
            assert r.returncode == 0 and r.stdout == b"%d\n" % host_text[name][1], err
            assert '"path": "device"' in err and _field(err, "text_bytes") == 0 and '"text_ms": 0.000' in err
    c = CASES["tags"]
    with pytest.raises(api.StrlingError) as e:
        ctx.view_records(b"".join(c["recs"]), REF_NAMES, cap=0)
    assert e.value.code == -4


def test_a_refusal_in_a_later_batch_names_the_ordinal_in_the_call_sequence(ctx):
    recs = CASES["tag_unknown"]["recs"]                        # record 1 is refused
    names, off = api._sam_names(REF_NAMES)
    raw = np.frombuffer(recs[1], np.uint8)
    o, info, need = api._view_opts(), api.ViewInfo(), C.c_uint64(0)
    rc = ctx.L.strl_view_records_at(ctx.h, raw.ctypes.data, raw.size, names.ctypes.data, off.ctypes.data, len(REF_NAMES), C.byref(o), 41, None, 0, C.byref(need), C.byref(info))
    assert rc == -6 and ("record 41: " + V.REFUSALS["tag_type"]).encode() in ctx.L.strl_last_error()


@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("name", BAD)
def test_refusals_in_the_hosts_words(name, setting, paths, tmp_path):
    o = str(tmp_path / "out.sam")
    host = _view(["-o", o, paths[name]], STRL_VIEW="host")
    dev = _view(["-o", o, paths[name]], **SETTINGS[setting])
    assert host.returncode == 1 and dev.returncode == 1 and os.listdir(str(tmp_path)) == []
    words = [l for l in host.stderr.decode().splitlines() if "malformed BAM record" in l]
    assert len(words) == 1 and words[0] in dev.stderr.decode(), dev.stderr


def test_the_context_is_usable_after_a_refusal(ctx, paths, host_text):
    for name in BAD:
        ordinal, key = CASES[name]["refused"]
        with pytest.raises(api.StrlingError) as e:
            ctx.view_records(b"".join(CASES[name]["recs"]), REF_NAMES)
        assert e.value.code == -6 and "record %d: %s" % (ordinal, V.REFUSALS[key]) in str(e.value)
        with pytest.raises(api.StrlingError) as e:
            ctx.view(paths[name], chunk_blocks=1)
        assert e.value.code == -6 and "record %d: %s" % (ordinal, V.REFUSALS[key]) in str(e.value)
    assert ctx.view_records(b"".join(CASES["tags"]["recs"]), REF_NAMES)[0] == host_text["tags"][0]
    assert ctx.view(paths["tags"])[0] == host_text["tags"][0]


def test_a_cut_record_is_refused_behind_an_earlier_refusal(ctx):
    recs = CASES["numbers"]["recs"]
    raw = b"".join(recs)
    with pytest.raises(api.StrlingError) as e:
        ctx.view_records(raw[:-3], REF_NAMES)
    assert e.value.code == -6 and "record %d: %s" % (len(recs) - 1, V.REFUSALS["size"]) in str(e.value)
    with pytest.raises(api.StrlingError) as e:
        ctx.view_records(b"".join(CASES["tag_unknown"]["recs"]) + raw[:-3], REF_NAMES)
    assert "record 1: " + V.REFUSALS["tag_type"] in str(e.value)


def test_abi_refuses_the_calls_out_of_order(ctx, paths, host_text):
    L, h = ctx.L, ctx.h
    text, nb, info = C.c_void_p(), C.c_uint64(0), api.ViewInfo()
    one = (C.c_uint8 * 1)(0)
    L.strl_view_end(h)
    assert L.strl_view_push(h, one, 1, None, None, None, None, 0, C.byref(text), C.byref(nb)) == -3, "a push without a begin"
    assert L.strl_view_finish(h, C.byref(text), C.byref(nb), C.byref(info)) == -3, "a finish without a begin"
    assert L.strl_view_reserve(h, 16, 1 << 20) == -3
    names, off = api._sam_names(REF_NAMES)
    o = api._view_opts()
    assert L.strl_view_begin(h, len(REF_NAMES), 0, names.ctypes.data, off.ctypes.data, C.byref(o)) == 0
    assert L.strl_view_begin(h, -1, 0, names.ctypes.data, off.ctypes.data, C.byref(o)) == -3
    assert L.strl_view_finish(h, C.byref(text), C.byref(nb), C.byref(info)) == 0 and nb.value == 0 and info.records == 0, "a file without a chunk"
    assert L.strl_view_finish(h, C.byref(text), C.byref(nb), C.byref(info)) == -3, "a second finish"
    assert L.strl_view_push(h, one, 1, None, None, None, None, 0, C.byref(text), C.byref(nb)) == -3, "a push behind the finish"
    assert L.strl_view_end(h) == 0 and L.strl_view_end(h) == 0
    assert ctx.view(paths["quals"])[0] == host_text["quals"][0]
