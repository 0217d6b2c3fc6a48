"""CSI indexes built on the device: strl_bamindex_begin_csi / strl_front_index_begin_csi through api.py and the CLI
(`bamindex --csi`, `extract --write-index --csi`, `call --make-index`) against the Python writer and the brute-force model of
tests/test_csi.py, then by use -- region reads, shares, `call`, `pull` -- with only the device-built .csi beside the file, and the
refusals.  The .bai path is checked again here against bamio.write_bai: it must not have moved.
"""
import os
import shutil
import struct

import numpy as np
import pytest

from strling_amd import api, bamio, synth
from strling_amd.records import RecordBatch
from test_csi import (FILES, HUMANLIKE_REGIONS, P29, _backfilled, _bai_abs, _bgzf_inflate, _bin_first_window, _check_model, _csi_abs, _csi_file_payload, _run,
                      huge_regions, make_file, regions_match, run_pull)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def built(tmp_path_factory, ctx):
    """every case once: the file with the Python writer's .csi, and the device's payload (api) of the same pushes"""
    d = tmp_path_factory.mktemp("csi_device")
    out = {}
    for name in FILES:
        f = make_file(d, name)
        f["payload"], f["info"] = ctx.bamindex(f["bam"], chunk_blocks=f["per_push"], csi=f["asked"])
        out[name] = f
    return out


@pytest.fixture(scope="module")
def bare(tmp_path_factory):
    """huge and humanlike without any index, and a genome BED for `extract`"""
    d = tmp_path_factory.mktemp("csi_bare")
    out = {name: make_file(d, name, index=None) for name in ("huge", "humanlike")}
    rec, g = synth.synth_wgs(2500, seed=31, n_contigs=3, contig_len=200_000)
    out["humanlike"]["bed"] = str(d / "humanlike.str")
    bamio.write_genome_bed(out["humanlike"]["bed"], g, rec.targets)
    out["huge"]["bed"] = str(d / "huge.str")
    open(out["huge"]["bed"], "w").write("huge\t1000\t1040\tAC\n")
    return out


@pytest.mark.parametrize("name", list(FILES))
def test_device_payload_equals_the_python_writers(built, name):
    f = built[name]
    dev, py = _csi_abs(f["payload"], f["at"]), _csi_abs(_csi_file_payload(f["bam"] + ".csi"), f["at"])
    assert dev[:2] == py[:2] == f["scheme"]
    assert len(dev[2]) == len(py[2]) == len(f["rec"].targets)
    for t, (a, b) in enumerate(zip(dev[2], py[2])):
        assert a == b, t                                   # bins, loffsets, chunk lists, the pseudo-bin's four numbers
    n_no_coor = int((f["rec"].tid < 0).sum())
    assert dev[3] == py[3] == n_no_coor
    assert f["info"]["n_records"] == f["rec"].n and f["info"]["n_no_coor"] == n_no_coor
    assert f["info"]["n_chunks"] <= f["info"]["n_runs"] <= max(1, f["rec"].n)


@pytest.mark.parametrize("name", list(FILES))
def test_device_payload_meets_the_model(built, name):
    f = built[name]
    _check_model(_csi_abs(f["payload"], f["at"]), f["rec"], f["off"], f["stop"], f["scheme"])


def test_header_only_payload_bytes(built):
    assert built["header_only"]["payload"] == b"CSI\1" + struct.pack("<iiii", 14, 1, 0, 2) + bytes(8) + bytes(8)


@pytest.mark.parametrize("bad", [(7, 5), (25, 5), (14, 9)])
def test_schemes_outside_the_range_are_an_argument_error(built, ctx, bad):
    with pytest.raises(api.StrlingError) as e:
        ctx.bamindex(built["depth0"]["bam"], csi=bad)
    assert "min_shift" in str(e.value) and "-3" in str(e.value)


def test_bai_has_not_moved(built, ctx, tmp_path):
    """the .bai of humanlike: api and CLI give the same bytes, which parse to what bamio.write_bai writes; and the (14, 5) CSI of the
    device holds the same bins and chunks, its loffsets the .bai's linear index filled from behind"""
    f = make_file(tmp_path, "humanlike", index="bai")
    got, info = ctx.bamindex(f["bam"])
    out = str(tmp_path / "cli.bai")
    r = _run(["bamindex", "-o", out, f["bam"]])
    assert r.returncode == 0, r.stderr
    assert open(out, "rb").read() == got
    dev, py = _bai_abs(got, f["at"]), _bai_abs(open(f["bam"] + ".bai", "rb").read(), f["at"])
    assert dev == py and info["n_records"] == f["rec"].n
    m, depth, refs, no_coor = _csi_abs(built["humanlike_as_bai"]["payload"], f["at"])
    assert (m, depth) == (14, 5) and no_coor == dev[1]
    for bins, (bbins, lin) in zip(refs, dev[0]):
        assert {k: v[1] for k, v in bins.items()} == bbins
        fill = _backfilled({w: v for w, v in enumerate(lin) if v is not None})
        assert all(loff == fill(_bin_first_window(k, 5)) for k, (loff, _) in bins.items() if k != 37450)


def test_cli_small_pushes_equal_one_push(built, tmp_path):
    f = built["huge_small_blocks"]
    outs = []
    for k, blocks in enumerate(("3", "4096")):
        out = str(tmp_path / f"o{k}.csi")
        r = _run(["bamindex", "--csi", "-v", "-o", out, f["bam"]], env=dict(os.environ, STRL_CHUNK_BLOCKS=blocks))
        assert r.returncode == 0 and "records" in r.stderr, r.stderr
        outs.append(_csi_abs(_csi_file_payload(out), f["at"]))
        assert sorted(os.listdir(tmp_path)) == [f"o{j}.csi" for j in range(k + 1)]        # no temporary file stays
    assert outs[0] == outs[1] == _csi_abs(f["payload"], f["at"])


def test_cli_min_shift(built, tmp_path):
    f = built["m12"]
    out = str(tmp_path / "m12.csi")
    r = _run(["bamindex", "--csi", "-m", "12", "-o", out, f["bam"]])
    assert r.returncode == 0, r.stderr
    assert _csi_abs(_csi_file_payload(out), f["at"]) == _csi_abs(f["payload"], f["at"])


@pytest.mark.parametrize("name", ["humanlike", "huge"])
def test_extract_write_index_csi(bare, tmp_path, name):
    f = bare[name]
    bam = str(tmp_path / "x.bam")
    shutil.copy(f["bam"], bam)
    plain, with_idx, ref = str(tmp_path / "plain.bin"), str(tmp_path / "idx.bin"), str(tmp_path / "ref.csi")
    r0 = _run(["extract", "-g", f["bed"], bam, plain])
    r1 = _run(["extract", "-g", f["bed"], "-v", "--write-index", "--csi", bam, with_idx])
    assert r0.returncode == 0 and r1.returncode == 0, (r0.stderr, r1.stderr)
    assert "index not written" not in r1.stderr and os.path.exists(bam + ".csi") and not os.path.exists(bam + ".bai"), r1.stderr
    assert open(plain, "rb").read() == open(with_idx, "rb").read()
    r2 = _run(["bamindex", "--csi", "-o", ref, bam])
    assert r2.returncode == 0, r2.stderr
    assert _csi_abs(_csi_file_payload(bam + ".csi"), f["at"]) == _csi_abs(_csi_file_payload(ref), f["at"])
    assert sorted(os.listdir(tmp_path)) == ["idx.bin", "plain.bin", "ref.csi", "x.bam", "x.bam.csi"]


def test_front_index_payload_equals_bamindex_bytes(built, ctx):
    ctx.set_opts(0.8, 40, 350)
    ctx.set_genome(None)
    for name, per_push in (("huge_small_blocks", 3), ("m12", 1)):
        f = built[name]
        ref, ref_info = ctx.bamindex(f["bam"], chunk_blocks=per_push, csi=f["asked"])
        res, got, info, refused = ctx.extract_bam_device_indexed(f["bam"], chunk_blocks=per_push, csi=f["asked"])
        assert refused is None, refused
        assert got == ref and info == ref_info
        assert _csi_abs(got, f["at"]) == _csi_abs(f["payload"], f["at"])


def test_the_device_built_csi_works(bare, tmp_path):
    """only the device-built .csi beside the files: region reads, the record count, `extract --gpus 2` cut into shares"""
    for name in ("huge", "humanlike"):
        f = bare[name]
        bam = str(tmp_path / f"{name}.bam")
        shutil.copy(f["bam"], bam)
        r = _run(["bamindex", "--csi", bam])
        assert r.returncode == 0 and os.path.exists(bam + ".csi") and not os.path.exists(bam + ".bai"), r.stderr
        g = dict(f, bam=bam)
        assert regions_match(g, huge_regions() if name == "huge" else HUMANLIKE_REGIONS) >= (18 if name == "huge" else 4)
        r = _run(["_indexed_records", bam])
        assert r.returncode == 0 and r.stdout.strip() == str(f["rec"].n)
    one, two = str(tmp_path / "one.bin"), str(tmp_path / "two.bin")
    r1 = _run(["extract", "-g", bare["humanlike"]["bed"], "-v", bam, one])
    r2 = _run(["extract", "-g", bare["humanlike"]["bed"], "-v", "--gpus", "2", bam, two])
    assert r1.returncode == 0 and r2.returncode == 0, (r1.stderr, r2.stderr)
    assert "in turn" not in r2.stderr and "a contiguous share of the file each" in r2.stderr, r2.stderr
    assert open(one, "rb").read() == open(two, "rb").read()


def test_call_with_csi_equals_call_with_bai(bare, tmp_path):
    f = bare["humanlike"]
    d_csi, d_bai = tmp_path / "csi", tmp_path / "bai"
    outs = {}
    for d, flags in ((d_csi, ["--csi"]), (d_bai, [])):
        d.mkdir()
        bam, binp = str(d / "s.bam"), str(d / "s.bin")
        shutil.copy(f["bam"], bam)
        assert _run(["bamindex"] + flags + [bam]).returncode == 0
        assert _run(["extract", "-g", f["bed"], bam, binp]).returncode == 0
        r = _run(["call", "-o", str(d / "out"), bam, binp])
        assert r.returncode == 0, r.stderr
        outs[d] = {n: open(d / n, "rb").read() for n in sorted(os.listdir(d)) if n.startswith("out")}
    assert os.path.exists(d_csi / "s.bam.csi") and not os.path.exists(d_csi / "s.bam.bai")
    assert len(outs[d_csi]) == 3 and outs[d_csi] == outs[d_bai]


def test_call_make_index(bare, tmp_path):
    """a reference longer than 2^29 in the header: <bam>.csi; else the .bai as before"""
    for name, made_ext, other in (("huge", ".csi", ".bai"), ("humanlike", ".bai", ".csi")):
        f = bare[name]
        bam, binp = str(tmp_path / f"{name}.bam"), str(tmp_path / f"{name}.bin")
        shutil.copy(f["bam"], bam)
        assert _run(["extract", "-g", f["bed"], bam, binp]).returncode == 0
        r = _run(["call", "-v", "--make-index", "-o", str(tmp_path / f"{name}_out"), bam, binp])
        assert r.returncode == 0 and "--make-index" in r.stderr, r.stderr
        assert os.path.exists(bam + made_ext) and not os.path.exists(bam + other)
        assert len([n for n in os.listdir(tmp_path) if n.startswith(f"{name}_out")]) == 3
    m, depth, _, _ = _csi_abs(_csi_file_payload(str(tmp_path / "huge.bam.csi")), bare["huge"]["at"])
    assert (m, depth) == (14, 6)


def test_device_pull_beyond_2p29(built, tmp_path):
    f = built["huge"]
    out_d, out_h = str(tmp_path / "d.bam"), str(tmp_path / "h.bam")
    region = f"huge:{P29 + 1}-{P29 + 100_000}"
    d = run_pull(["-v", "-o", out_d, f["bam"], region], None)
    h = run_pull(["-o", out_h, f["bam"], region], "host")
    assert d.returncode == 0 and h.returncode == 0, (d.stderr, h.stderr)
    assert open(out_d, "rb").read() == open(out_h, "rb").read()
    assert len(_bgzf_inflate(open(out_d, "rb").read())) > 5000


def _tiny(rows, targets):
    n = len(rows)
    return RecordBatch.from_fields([r[0] for r in rows], [r[1] for r in rows], [r[0] for r in rows], [r[1] for r in rows], [0x1] * n, [60] * n, ["50M"] * n, ["ACGTA" * 10] * n,
                                   [f"q{i}" for i in range(n)], [0] * n, targets)


@pytest.mark.parametrize("what", ["shuffled", "end_2p31", "far_past_l_ref", "plain_on_huge"])
def test_refusals(bare, tmp_path, what):
    """exit 1 with a message that names the cause, no partial output"""
    bam = str(tmp_path / "x.bam")
    flags = ["--csi"]
    if what == "shuffled":
        rec, _ = synth.synth_wgs(800, seed=37, n_contigs=2, contig_len=60_000)
        order = np.random.default_rng(37).permutation(rec.n)[:300]
        bamio.write_bam(bam, _tiny([(int(rec.tid[i]), int(rec.pos[i])) for i in order], rec.targets), index=False)
        want = ["not coordinate sorted"]
    elif what == "end_2p31":
        bamio.write_bam(bam, _tiny([(0, 100), (0, (1 << 31) - 30)], [("max", (1 << 31) - 1)]), index=False)
        want = ["2^31", "record 1 "]
    elif what == "far_past_l_ref":
        bamio.write_bam(bam, _tiny([(0, 100), (0, 5_000_000)], [("short", 1000)]), index=False)
        want = ["past the end of its reference"]
    else:
        shutil.copy(bare["huge"]["bam"], bam)
        flags, want = [], ["2^29", "CSI", "--csi"]
    r = _run(["bamindex"] + flags + [bam])
    assert r.returncode == 1, (r.returncode, r.stderr)
    for w in want:
        assert w in r.stderr, r.stderr
    assert os.listdir(tmp_path) == ["x.bam"]
