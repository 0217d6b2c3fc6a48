"""`strling extract --write-index`: the .bai written from extract's own pass over the BAM.

The index is compared with the file `strling bamindex` writes for the same BAM byte for byte (test_extract_index_device.py
asserts the premise: `bamindex` gives the same bytes however the blocks are grouped into pushes; both commands here use the same
STRL_CHUNK_BLOCKS anyway).  What is decided before a context is needed -- --gpus N, a CRAM, STRL_FRONT=host -- is checked
without a device.
"""
import os

import pytest

from strling_amd import bamio, build, synth
from strling_amd.records import RecordBatch

CLI = build.CLI


def _run(args, env=None):
    import subprocess
    return subprocess.run([CLI] + args, capture_output=True, text=True, env=dict(os.environ, **(env or {})))


# ---- without a device ------------------------------------------------------------------------------------------------------
def _small_bam(tmp_path):
    rec, g = synth.synth_wgs(200, seed=61, n_contigs=2, contig_len=30_000)
    bam, bed = str(tmp_path / "s.bam"), str(tmp_path / "ref.str")
    bamio.write_bam(bam, rec, index=False)
    bamio.write_genome_bed(bed, g, rec.targets)
    return bam, bed


def test_usage_names_the_flag():
    r = _run(["extract"])
    assert r.returncode == 0 and "--write-index" in r.stdout and "--index-out" in r.stdout


def test_refused_with_several_gpus(tmp_path):
    bam, bed = _small_bam(tmp_path)
    r = _run(["extract", "-g", bed, "--write-index", "--gpus", "2", bam, str(tmp_path / "s.bin")])
    assert r.returncode == 1 and "--write-index cannot be combined with --gpus N" in r.stderr and "need the index beforehand" in r.stderr, r.stderr
    assert sorted(os.listdir(tmp_path)) == ["ref.str", "s.bam"]


def test_refused_for_a_cram(tmp_path):
    cram = str(tmp_path / "x.cram")
    open(cram, "wb").write(b"CRAM\x03\x00" + bytes(64))
    r = _run(["extract", "--write-index", cram, str(tmp_path / "x.bin")])
    assert r.returncode == 1 and ".crai" in r.stderr and "out of scope" in r.stderr, r.stderr
    assert os.listdir(tmp_path) == ["x.cram"]


@pytest.mark.parametrize("var", ["STRL_FRONT", "STRL_PAIR"])
def test_refused_with_the_host_front_end(tmp_path, var):
    bam, bed = _small_bam(tmp_path)
    r = _run(["extract", "-g", bed, "--write-index", bam, str(tmp_path / "s.bin")], env={var: "host"})
    assert r.returncode == 1 and "needs the device front end" in r.stderr, r.stderr
    assert sorted(os.listdir(tmp_path)) == ["ref.str", "s.bam"]


def test_index_out_needs_the_flag(tmp_path):
    bam, bed = _small_bam(tmp_path)
    r = _run(["extract", "-g", bed, "--index-out", str(tmp_path / "o.bai"), bam, str(tmp_path / "s.bin")])
    assert r.returncode == 1 and "--index-out needs --write-index" in r.stderr


# ---- on the device ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sample(tmp_path_factory):
    """one sorted sample (small blocks; STRL_CHUNK_BLOCKS=5 below puts records and runs across many pushes), `extract` without the
    flag and `strling bamindex` of it"""
    d = tmp_path_factory.mktemp("write_index")
    rec, g = synth.synth_wgs(1500, seed=62, n_contigs=2, contig_len=30_000)
    bam, bed = str(d / "s.bam"), str(d / "ref.str")
    bamio.write_bam(bam, rec, block=4099, index=False)
    bamio.write_genome_bed(bed, g, rec.targets)
    env = {"STRL_CHUNK_BLOCKS": "5"}
    r = _run(["extract", "-g", bed, bam, str(d / "plain.bin")], env=env)
    assert r.returncode == 0, r.stderr
    assert not os.path.exists(bam + ".bai")
    r = _run(["bamindex", "-o", str(d / "ref.bai"), bam], env=env)
    assert r.returncode == 0, r.stderr
    return dict(d=d, rec=rec, bam=bam, bed=bed, env=env, plain=open(d / "plain.bin", "rb").read(), ref=open(d / "ref.bai", "rb").read())


@pytest.mark.gpu
def test_write_index_equals_bamindex_and_leaves_the_bin_alone(sample):
    d, bam = sample["d"], sample["bam"]
    r = _run(["extract", "-g", sample["bed"], "-v", "--write-index", bam, str(d / "with.bin")], env=sample["env"])
    assert r.returncode == 0, r.stderr
    assert open(bam + ".bai", "rb").read() == sample["ref"]
    assert open(d / "with.bin", "rb").read() == sample["plain"]
    line = [l for l in r.stderr.splitlines() if l.startswith("[strling] index:")]
    assert len(line) == 1 and f"{sample['rec'].n} records" in line[0] and "runs" in line[0] and "chunks" in line[0] and f"{len(sample['ref'])} bytes" in line[0], r.stderr
    assert not [f for f in os.listdir(d) if ".tmp." in f]
    # one block per chunk: every block's file offset reaches the index through a staged chunk's table of its own
    r = _run(["extract", "-g", sample["bed"], "--write-index", "--index-out", str(d / "one.bai"), bam, str(d / "one.bin")], env={"STRL_CHUNK_BLOCKS": "1"})
    assert r.returncode == 0, r.stderr
    assert open(d / "one.bai", "rb").read() == sample["ref"] and open(d / "one.bin", "rb").read() == sample["plain"]
    # `call` on that index writes the same three files as on bamindex's
    outs = {}
    for tag, bai in (("a", None), ("b", sample["ref"])):
        if bai is not None:
            open(bam + ".bai", "wb").write(bai)
        rc = _run(["call", "-o", str(d / tag), bam, str(d / "with.bin")])
        assert rc.returncode == 0, rc.stderr
        outs[tag] = {f[len(tag):]: open(d / f, "rb").read() for f in sorted(os.listdir(d)) if f.startswith(tag + "-")}
    assert len(outs["a"]) == 3 and outs["a"] == outs["b"], (sorted(outs["a"]), sorted(outs["b"]))
    os.remove(bam + ".bai")


@pytest.mark.gpu
def test_index_out_and_an_existing_index_is_replaced(sample):
    d, bam = sample["d"], sample["bam"]
    out = str(d / "elsewhere.bai")
    open(out, "wb").write(b"an old index")
    r = _run(["extract", "-g", sample["bed"], "--write-index", "--index-out", out, bam, str(d / "io.bin")], env=sample["env"])
    assert r.returncode == 0, r.stderr
    assert open(out, "rb").read() == sample["ref"] and not os.path.exists(bam + ".bai")
    assert open(d / "io.bin", "rb").read() == sample["plain"]
    assert not [f for f in os.listdir(d) if ".tmp." in f]


@pytest.mark.gpu
@pytest.mark.parametrize("old_index", [False, True])
def test_unsorted_bam(tmp_path, old_index):
    """exit 0, the .bin of a run without the flag, one line on stderr, no index and no temporary file; an index that was there stays"""
    rec, g = synth.synth_wgs(1500, seed=63, n_contigs=1, contig_len=60_000, interchrom_frac=0.0, unmapped_frac=0.0)
    pos = rec.pos.copy()
    k = next(i for i in range(3, 20) if pos[i - 1] > 0)
    pos[k] = pos[k - 1] - 1
    rec = RecordBatch(rec.tid, pos, rec.mtid, rec.mpos, rec.flag, rec.mapq, rec.cigar_off, rec.cigar, rec.seq_off, rec.l_seq, rec.seq4, rec.qname_off, rec.qnames,
                      rec.isize, rec.targets)
    bam, bed = str(tmp_path / "u.bam"), str(tmp_path / "ref.str")
    bamio.write_bam(bam, rec, block=4099, index=False)
    bamio.write_genome_bed(bed, g, rec.targets)
    env = {"STRL_CHUNK_BLOCKS": "5", "STRL_NO_INDEX_COUNT": "1"}
    assert _run(["extract", "-g", bed, bam, str(tmp_path / "plain.bin")], env=env).returncode == 0
    ref = _run(["bamindex", "-o", str(tmp_path / "never.bai"), bam], env=env)
    assert ref.returncode == 1 and f"not coordinate sorted: record {k} " in ref.stderr
    if old_index:
        open(bam + ".bai", "wb").write(b"an old index")
    r = _run(["extract", "-g", bed, "--write-index", bam, str(tmp_path / "with.bin")], env=env)
    assert r.returncode == 0, r.stderr
    msg = [l for l in r.stderr.splitlines() if "index not written:" in l]
    assert len(msg) == 1 and f"not coordinate sorted: record {k} " in msg[0], r.stderr
    assert open(tmp_path / "with.bin", "rb").read() == open(tmp_path / "plain.bin", "rb").read()
    assert sorted(os.listdir(tmp_path)) == sorted(["u.bam", "ref.str", "plain.bin", "with.bin"] + (["u.bam.bai"] if old_index else []))
    if old_index:
        assert open(bam + ".bai", "rb").read() == b"an old index"
