"""The record scan of the device front end (front.hip) on the files of tests/scan_cases.py: decoy records in aux arrays, records
longer than a segment, chunk seams on chosen bytes, every record shape the parse must read.

front.hip promises that "a wrong guess costs time, never a result".  Here the guesses ARE wrong, by construction and by the
model's word (tests/test_scan_cases.py shows that on any machine), and the results are held to
  the oracle's treads, field by field, with qnames, fragment words and chunk counts (helpers.check_front_extract);
  the model's record count of every chunk, and its count of wrongly guessed segments against scan_slow_segments;
  the Python writer's .bai, for the device-built index of `bamindex` and of extract's own pass;
  the oracle's .bin, byte for byte, through the CLI with the device front end and with the host reader (whose own
  guess-and-verify meets the same decoys).
Run with -s for one line of figures per chunk."""
import os
import re
import subprocess
import time

import numpy as np
import pytest

import scan_cases as sc
from helpers import FRONT_FIELDS, check_front_extract
from strling_amd import api, bamio, build, synth
from test_bamindex import _bai_abs, _block_starts

pytestmark = pytest.mark.gpu

CLI = build.CLI
INDEXED = [("a", "decoy"), ("b", "decoy"), ("d", "plain"), ("d", "decoy"), ("k", "uniform")]
EXTRACTED = [f for f in sc.files() if f != ("l", "huge", 4)]


@pytest.fixture(scope="module")
def built(tmp_path_factory, oracle):
    """every file once (those of INDEXED with the Python writer's .bai beside them), and per case the oracle's treads"""
    d = tmp_path_factory.mktemp("scan")
    out = {}
    for name, fn in sc.CASES.items():
        case = fn()
        frag = synth.frag_hist(case.rec)
        exp = oracle.extract(case.rec, case.genome, oracle.make_opts(oracle.median(frag), 0.8, 40))
        assert len(exp) > 20
        files = {}
        for label in case.variants:
            path = str(d / f"{name}_{label}.bam")
            files[label] = (path, case.write(path, label, index=(name, label) in INDEXED))
        out[name] = dict(case=case, exp=exp, frag=frag, files=files)
    return out


def _scan_figures(name, label, cb, got, model):
    """per chunk: the device's record count is the model's; segments walked twice = segments the model calls wrongly guessed
    (a wrongly guessed segment holds a record start, so the exact chain arrives in it, somewhere else than at its guess: it is
    walked again; a stray guess is only cleared, a clean chunk is linked without the sequential lane)"""
    assert len(got["chunks"]) == len(model), (len(got["chunks"]), len(model))
    for k, (c, m) in enumerate(zip(got["chunks"], model)):
        print(f"{name}/{label} chunk_blocks={cb} chunk {k}: records {c['n_records']} (model {m['n_records']}), carry in front {m['carry']}, "
              f"segments walked twice {c['scan_slow_segments']}, model: wrong {m['wrong']} stray {m['stray']}")
    for k, (c, m) in enumerate(zip(got["chunks"], model)):
        assert c["n_records"] == m["n_records"], k
        if m["wrong"]:
            assert c["scan_slow_segments"] >= 1, k
        if m["clean"]:
            assert c["scan_slow_segments"] == 0, k
        assert c["scan_slow_segments"] == len(m["wrong"]), k


@pytest.mark.parametrize("name,label,cb", EXTRACTED)
def test_extract_is_the_oracles_and_the_repair_ran_where_the_model_says(ctx, built, name, label, cb):
    b = built[name]
    path = b["files"][label][0]
    model = sc.scan_model(path, cb)
    t0 = time.perf_counter()
    got = check_front_extract(ctx, b["case"].rec, b["case"].genome, path, cb, b["exp"])
    print(f"{name}/{label} chunk_blocks={cb}: {time.perf_counter() - t0:.3f} s on the device path")
    _scan_figures(name, label, cb, got, model)
    v = b["case"].variants[label]
    if name in "abcgn" and not v.control_of:
        assert sum(c["scan_slow_segments"] for c in got["chunks"]) >= 1        # the repair path ran in this test


@pytest.mark.parametrize("name,label", INDEXED)
@pytest.mark.parametrize("cb", [16384, 3])
def test_the_index_is_the_python_writers(ctx, built, oracle, name, label, cb):
    """recoff and the parse's `end` column, directly: every virtual offset and bin of `bamindex` and of extract's own index pass"""
    b = built[name]
    rec, path = b["case"].rec, b["files"][label][0]
    at = _block_starts(path)
    want = _bai_abs(open(path + ".bai", "rb").read(), at)
    bai, info = ctx.bamindex(path, chunk_blocks=cb)
    assert _bai_abs(bai, at) == want
    assert info["n_records"] == rec.n and info["n_no_coor"] == int((rec.tid < 0).sum())
    ctx.set_opts(0.8, 40, oracle.median(b["frag"]))
    ctx.set_genome(b["case"].genome)
    got, bai2, info2, refused = ctx.extract_bam_device_indexed(path, chunk_blocks=cb)
    assert refused is None and _bai_abs(bai2, at) == want and info2["n_records"] == rec.n
    for f in FRONT_FIELDS:
        assert np.array_equal(got["treads"][f], b["exp"][f]), f
    model = sc.scan_model(path, cb)
    assert [c["scan_slow_segments"] for c in got["chunks"]] == [len(m["wrong"]) for m in model]


@pytest.mark.parametrize("front", ["device", "host"])
@pytest.mark.parametrize("name,label", [("a", "decoy"), ("d", "decoy"), ("k", "uniform")])
def test_cli_bin_is_the_oracles(built, oracle, tmp_path, name, label, front):
    b = built[name]
    rec, (path, hdr) = b["case"].rec, b["files"][label]
    bed, out = str(tmp_path / "ref.fa.str"), str(tmp_path / "o.bin")
    bamio.write_genome_bed(bed, b["case"].genome, rec.targets)
    env = dict(os.environ, STRL_CHUNK_BLOCKS="3")
    if front == "host":
        env["STRL_FRONT"] = "host"
    r = subprocess.run([CLI, "extract", "-g", bed, "-v", path, out], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr
    exp = oracle.bin_write(0.8, 40, b["frag"], hdr.rstrip("\0"), b["exp"], rec.qname_off, rec.qnames)
    assert open(out, "rb").read() == exp
    if front == "device":
        assert "repeating the extraction" not in r.stderr, r.stderr
        twice = re.search(r"(\d+) scan segments walked twice", r.stderr)
        assert twice, r.stderr
        if name == "a":
            assert int(twice.group(1)) >= 3


def test_a_carry_of_more_than_a_megabyte_is_a_status(ctx, built, oracle, tmp_path):
    """case (l) in chunks of four blocks: carry_out_kernel copies nothing (the length it stores is 0), rec_link_kernel raises
    FRONT_ERR_CARRY, the ABI answers STRL_ERR_FORMAT; the CLI hands the file to the host reader, which has no such limit"""
    b = built["l"]
    rec, (path, hdr) = b["case"].rec, b["files"]["huge"]
    ctx.set_opts(0.8, 40, oracle.median(b["frag"]))
    ctx.set_genome(b["case"].genome)
    with pytest.raises(api.StrlingError) as e:
        ctx.extract_bam_device(path, chunk_blocks=4)
    assert "error -6:" in str(e.value) and "BAM record of more than" in str(e.value)
    bed, out = str(tmp_path / "ref.fa.str"), str(tmp_path / "l.bin")
    bamio.write_genome_bed(bed, b["case"].genome, rec.targets)
    r = subprocess.run([CLI, "extract", "-g", bed, path, out], capture_output=True, text=True, env=dict(os.environ, STRL_CHUNK_BLOCKS="4"))
    assert r.returncode == 0, r.stderr
    assert "BAM record of more than" in r.stderr and "repeating the extraction with the host reader" in r.stderr
    assert open(out, "rb").read() == oracle.bin_write(0.8, 40, b["frag"], hdr.rstrip("\0"), b["exp"], rec.qname_off, rec.qnames)
    # ... and the context takes the next file
    check_front_extract(ctx, rec, b["case"].genome, path, 16384, b["exp"])


@pytest.mark.parametrize("blocks", ["3", "0"])
def test_a_file_cut_inside_its_last_record_gets_the_host_readers_verdict(built, tmp_path, blocks):
    """the inflated stream ends 50 bytes into the last record, every BGZF block valid.  The host reader is the reference: same
    exit status through the device front end, and no .bin where the host reader writes none (the device path used to drop the
    partial record and write one)"""
    b = built["a"]
    rec = b["case"].rec
    cut = str(tmp_path / "cut.bam")
    sc.cut_inside_last_record(b["files"]["control"][0], cut)
    bed = str(tmp_path / "ref.fa.str")
    bamio.write_genome_bed(bed, b["case"].genome, rec.targets)
    res = {}
    for front in ("host", "device"):
        out = str(tmp_path / f"{front}.bin")
        env = dict(os.environ, STRL_CHUNK_BLOCKS=blocks)
        if front == "host":
            env["STRL_FRONT"] = "host"
        r = subprocess.run([CLI, "extract", "-g", bed, cut, out], capture_output=True, text=True, env=env)
        res[front] = (r.returncode, os.path.exists(out), r.stderr)
        print(front, r.returncode, os.path.exists(out), r.stderr.strip().splitlines()[-1:])
    assert res["host"][0] >= 0 and res["device"][0] >= 0, res                   # an exit status, not a signal
    assert res["device"][:2] == res["host"][:2], res
    assert res["host"][0] != 0 and not res["host"][1], res                      # (the host reader does refuse the file)
    assert "ends inside a record" in res["device"][2], res["device"][2]
