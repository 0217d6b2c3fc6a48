"""`strling sort --write-index` on the GPU (strl_bamsort_index; csrc/bamindex.hip's per-record step over the sort's records): every
case of tests/sort_bam_cases.py and tests/sort_index_cases.py.  The device path's index equals
  * the host path's file byte for byte (--deflate=host: the two paths write the same members);
  * reference 2, the bytes `strling bamindex [--csi] OUT.bam` writes for the same sorted file -- the builder behind the record scan,
    with its own chunking -- or, where bamindex refuses the file, its status and its words from `record N` on;
  * reference 1 as a structure (--deflate=device, where the members and so the virtual offsets are others).
The same with records in many slabs and members written piece by piece, with launches of 64 / 257 / 1000 records, through the
ABI (api.bamsort_index), and by use (`extract --gpus 2` with only the sort-built index beside the file)."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import sort_index_cases as X
from strling_amd import api, bamio, build, synth

pytestmark = pytest.mark.gpu
CLI = build.CLI
NAMES = [name for name, _, _ in X.all_cases()]


def _run(args, **env):
    e = dict(os.environ)
    e.pop("STRL_SORT", None)
    e.update({k: str(v) for k, v in env.items()})
    return subprocess.run([CLI] + args, capture_output=True, text=True, env=e)


@pytest.fixture(scope="module")
def paths(tmp_path_factory):
    return X.case_dir(tmp_path_factory)


def _from_record(text):
    return text[text.index("record "):].strip()


def _one(name, csi, src, d, env, deflate="host"):
    """sort --write-index on the device, on the host, and bamindex of the device's output -> the three index paths (None: refused
    alike), after the comparisons every case gets.  A case in X.REFUSED must be refused and every other must not: the set is asserted
    case by case"""
    opts = ["--csi"] if csi else []
    ext = ".csi" if csi else ".bai"
    dev, host, ref2 = os.path.join(d, "dev.bam"), os.path.join(d, "host.bam"), os.path.join(d, "ref2" + ext)
    r = _run(["sort", "--write-index", f"--deflate={deflate}", "-v", *opts, "-o", dev, src], **env)
    assert '"path": "device"' in r.stderr or r.returncode, r.stderr
    h = _run(["sort", "--write-index", f"--deflate={deflate}", *opts, "-o", host, src], STRL_SORT="host")
    if name == "pos_2p31_minus_2" and not csi:                   # refused before anything is read, for its 2^31 - 1 contig
        assert r.returncode == h.returncode == 1 and "--csi" in r.stderr and r.stderr == h.stderr and os.listdir(d) == []
        return None
    assert os.path.exists(dev) and os.path.exists(host), (r.stderr, h.stderr)
    if deflate == "host":
        assert open(dev, "rb").read() == open(host, "rb").read()
    b = _run(["bamindex", *opts, "-o", ref2, dev])
    if name in X.REFUSED:
        assert r.returncode == h.returncode == b.returncode == 1, (r.stderr, h.stderr, b.stderr)
        assert "sorted file written; index refused: " in r.stderr.strip().splitlines()[-1]
        assert _from_record(r.stderr.strip().splitlines()[-1]) == _from_record(h.stderr) == _from_record(b.stderr)
        assert sorted(os.listdir(d)) == ["dev.bam", "host.bam"], "the sorted files are kept, no index, no temporary file"
        return None
    assert r.returncode == 0 and h.returncode == 0 and b.returncode == 0, (r.stderr, h.stderr, b.stderr)
    got = open(dev + ext, "rb").read()
    if deflate == "host":
        assert got == open(host + ext, "rb").read(), "the host path's index, byte for byte"
    assert got == open(ref2, "rb").read(), "bamindex's bytes for the same file"
    assert not [f for f in os.listdir(d) if ".tmp." in f]
    return dev, dev + ext


@pytest.mark.parametrize("name", NAMES)
def test_device_index_equals_host_and_bamindex(name, paths, tmp_path):
    _one(name, False, paths[name], str(tmp_path), {})


@pytest.mark.parametrize("name", NAMES)
def test_csi_with_records_in_many_slabs_and_members_piece_by_piece(name, paths, tmp_path):
    _one(name, True, paths[name], str(tmp_path), X.SEAM_ENV)


@pytest.mark.parametrize("name", ["uniform_shuffle", "bins_of_every_level", "one_300kb_record", "record_ends_on_member_boundary", "stream_ends_on_member_boundary",
                                  "header_longer_than_a_member", "placed_unmapped_and_pos_minus1"])
def test_bai_with_records_in_many_slabs_and_members_piece_by_piece(name, paths, tmp_path):
    _one(name, False, paths[name], str(tmp_path), X.SEAM_ENV)


@pytest.mark.parametrize("tile", [64, 257, 1000])
@pytest.mark.parametrize("name", ["n2047", "n2048", "n2049", "bins_of_every_level"])
def test_launches_of_a_few_records(name, tile, paths, tmp_path):
    """the wave edge, the block edge, and the last record carried from one launch to the next"""
    _one(name, False, paths[name], str(tmp_path), dict(STRL_SORT_INDEX_TILE=tile))
    for f in os.listdir(tmp_path):
        os.remove(tmp_path / f)
    _one(name, True, paths[name], str(tmp_path), dict(STRL_SORT_INDEX_TILE=tile))


@pytest.mark.parametrize("name", ["uniform_shuffle", "bins_of_every_level", "one_300kb_record", "stream_ends_on_member_boundary", "n_ref_0", "no_record"])
def test_deflate_device(name, paths, tmp_path):
    """the compressor's members have other sizes: against bamindex's bytes, and against the Python writer as a structure"""
    dev, idx = _one(name, False, paths[name], str(tmp_path), {}, deflate="device")
    assert X.index_structure(idx, dev, "bai") == X.reference_index(dev, "bai")
    for f in os.listdir(tmp_path):
        os.remove(tmp_path / f)
    dev, idx = _one(name, True, paths[name], str(tmp_path), {}, deflate="device")
    assert X.index_structure(idx, dev, ("csi", 14)) == X.reference_index(dev, ("csi", 14))


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------------
def test_abi_index_of_members_deflated_by_the_caller(ctx, paths, tmp_path):
    for index, kind in (("bai", "bai"), (("csi", 12, None), ("csi", 12))):
        stream, info, perm, (data, got, idx_info) = ctx.bamsort(paths["bins_of_every_level"], chunk_blocks=3, index=index)
        bam = str(tmp_path / "abi.bam")
        open(bam, "wb").write(data)
        assert gzip.decompress(data) == stream and idx_info["n_records"] == info["n_records"]
        _, _, at = X.walk(bam)
        assert (X.bai_abs(got, at) if kind == "bai" else X.csi_abs(got, at)) == X.reference_index(bam, kind)


def test_abi_refuses_a_bad_member_table_and_stays_usable(ctx, paths):
    """a wrong-length table and one that does not ascend are STRL_ERR_ARG; a refusal of the records' leaves the context usable"""
    p = paths["uniform_shuffle"]
    stream, info, perm = ctx.bamsort(p, keep_open=True)
    try:
        body = api.bgzf_deflate_host(stream)[0]
        tab = api.bamsort_members(body, 0) + [len(body)]
        l_ref = [1 << 20] * 3
        assert len(tab) >= 4
        for bad in (tab[:-1], tab + [tab[-1] + 28], [tab[1], tab[0]] + tab[2:], tab[:-1] + [1 << 48], []):
            with pytest.raises(api.StrlingError) as e:
                ctx.bamsort_index(bad, l_ref)
            assert e.value.code == -3, bad[:3]
        good, _ = ctx.bamsort_index(tab, l_ref)
        again, _ = ctx.bamsort_index(tab, l_ref)                   # (a second index of the same sort replaces the first)
        assert again == good and good[:4] == b"BAI\1"
    finally:
        ctx.bamsort_end()
    with pytest.raises(api.StrlingError):
        ctx.bamsort_index(tab, l_ref)                              # no sort open
    with pytest.raises(api.StrlingError) as e:
        ctx.bamsort(paths["placed_unmapped_and_pos_minus1"], index="bai")
    assert e.value.code == -6 and "negative position" in str(e.value)
    out = ctx.bamsort(p, index="bai")                              # a second sort with an index on the same context
    assert out[3][1] == good


# ---- by use ------------------------------------------------------------------------------------------------------------------------------
def test_the_index_works(tmp_path):
    """only the sort-built .bai beside the sorted file: the record count through the index, and `extract --gpus 2` cut into shares"""
    rec, g = synth.synth_wgs(5000, seed=3, n_contigs=3, contig_len=200_000)
    src, bam, bed = str(tmp_path / "in.bam"), str(tmp_path / "r.bam"), str(tmp_path / "ref.str")
    bamio.write_bam(src, rec, index=False)
    bamio.write_genome_bed(bed, g, rec.targets)
    r = _run(["sort", "--write-index", "-o", bam, src])
    assert r.returncode == 0 and os.path.exists(bam + ".bai"), r.stderr
    os.remove(src)
    r = _run(["_indexed_records", bam])
    assert r.returncode == 0 and r.stdout.strip() == str(rec.n)
    stop = np.array([int(rec.pos[i]) + bamio._ref_len(rec, i) for i in range(rec.n)])
    for tid, beg, end in ((0, 0, 500), (2, 199_000, 200_500), (1, 16_300, 16_400), (0, 100_000, 140_000)):
        q = _run(["_region", bam, str(tid), str(beg), str(end)])
        assert q.returncode == 0 and len(q.stdout.splitlines()) == int(((rec.tid == tid) & (rec.pos < end) & (stop > beg)).sum()), (tid, beg, end)
    one, two = str(tmp_path / "one.bin"), str(tmp_path / "two.bin")
    r1 = _run(["extract", "-g", bed, "-v", bam, one])
    r2 = _run(["extract", "-g", bed, "-v", "--gpus", "2", bam, two])
    assert r1.returncode == 0 and r2.returncode == 0, (r1.stderr, r2.stderr)
    assert "in turn" not in r2.stderr and "a contiguous share of the file each" in r2.stderr, r2.stderr
    assert open(one, "rb").read() == open(two, "rb").read()
