"""`strling call --sweep`: the flag in the usage text (CPU), and on a device the three output files of a run with the flag
against the same run without it -- with -b and with -l, with the default chunks and with chunks small enough to put bounds on
seams, with STRL_CALL_EVIDENCE=sweep in the flag's place, and on CRAM input, where the flag is ignored."""
import os
import re
import subprocess

import numpy as np
import pytest

import test_call as tc
from strling_amd import bamio, build, cramio, synth

CLI = build.CLI
FILES = ("-bounds.txt", "-genotype.txt", "-unplaced.txt")


def _run(args, env=None):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([CLI] + args, capture_output=True, text=True, env=e)


def test_help_lists_sweep():
    r = _run(["call", "--help"])
    assert r.returncode == 0
    lines = r.stdout.splitlines()
    at = [k for k, l in enumerate(lines) if l.lstrip().startswith("--sweep")]
    mk = [k for k, l in enumerate(lines) if l.lstrip().startswith("--make-index")]
    assert len(at) == 1 and len(mk) == 1 and 0 < at[0] - mk[0] <= 3, r.stdout      # next to --make-index
    assert "STRL_CALL_EVIDENCE=sweep" in r.stdout


def test_the_flag_is_parsed_before_any_file_is_opened(tmp_path):
    """--sweep is an option of `call` like the others: with it the command still fails on a missing bam with the usual message,
    and an option `call` does not have is still refused"""
    r = _run(["call", "--sweep", "-o", str(tmp_path / "x"), str(tmp_path / "none.bam"), str(tmp_path / "none.bin")])
    assert r.returncode == 1 and "couldn't open bam" in r.stderr, r.stderr
    r = _run(["call", "--sweeps", "-o", str(tmp_path / "x"), str(tmp_path / "none.bam"), str(tmp_path / "none.bin")])
    assert r.returncode != 0 and "couldn't open bam" not in r.stderr


@pytest.fixture(scope="module")
def inputs(tmp_path_factory, oracle):
    d = tmp_path_factory.mktemp("sweepcli")
    rec, g = tc._sample(n_pairs=9000, seed=21, n_contigs=3, contig_len=40_000)
    bam, bedg, binp = str(d / "s.bam"), str(d / "ref.str"), str(d / "s.bin")
    bamio.write_bam(bam, rec, block=6000)
    bamio.write_genome_bed(bedg, g, rec.targets)
    r = _run(["extract", "-g", bedg, bam, binp])
    assert r.returncode == 0, r.stderr
    frag = synth.frag_hist(rec)
    t = oracle.extract(rec, g, oracle.make_opts(oracle.median(frag), 0.8, 40))
    base_b, _, _ = oracle.call(t, rec, frag, min_support=3)
    rows = ["\t".join(l.split("\t")[:11]) for l in base_b.splitlines()[1:]]
    assert len(rows) >= 4
    pb, pl = str(d / "in-bounds.txt"), str(d / "loci.bed")
    open(pb, "w").write("#header line\n" + "\n".join(rows[:-1]) + "\n")
    open(pl, "w").write(tc._loci_from_bounds(rows, rec.targets, np.random.default_rng(2)))
    return dict(dir=d, rec=rec, g=g, bam=bam, bin=binp, bounds=pb, loci=pl, bed=bedg)


def _call(prefix, inputs, extra, env=None, bam=None):
    r = _run(["call", "-v", "-m", "3", "-o", prefix] + extra + [bam or inputs["bam"], inputs["bin"]], env)
    assert r.returncode == 0, r.stderr
    return [open(prefix + s).read() for s in FILES], r.stderr


def _swept(stderr):
    m = re.search(r"\[strling\] sweep: bounds answered by the sweep (\d+), seam bounds (\d+), passed on .*? (\d+), chunks (\d+),", stderr)
    assert m, stderr
    return tuple(int(x) for x in m.groups())


@pytest.mark.gpu
@pytest.mark.parametrize("given", ["-b", "-l", "none"])
def test_files_equal_the_run_without_the_flag(inputs, given):
    d = inputs["dir"]
    extra = {"-b": ["-b", inputs["bounds"]], "-l": ["-l", inputs["loci"]], "none": []}[given]
    tag = given.strip("-")
    plain, err0 = _call(str(d / f"plain_{tag}"), inputs, extra)
    assert "[strling] sweep:" not in err0 and plain[0].count("\n") >= 4
    one, err1 = _call(str(d / f"one_{tag}"), inputs, extra + ["--sweep"])
    assert one == plain
    answered, seam, passed, chunks = _swept(err1)
    assert answered > 0 and chunks == 1 and seam == 0
    # chunks of two 6000-byte blocks hold fewer records than a query spans: bounds fall on seams and take the default path;
    # chunks of 64 blocks leave bounds inside a chunk too.  The files stay what they were
    total, seams, inside = answered + seam + passed, 0, 0
    for blocks in ("2", "64"):
        small, err2 = _call(str(d / f"small{blocks}_{tag}"), inputs, extra + ["--sweep"], {"STRL_CHUNK_BLOCKS": blocks})
        assert small == plain, blocks
        answered2, seam2, passed2, chunks2 = _swept(err2)
        assert chunks2 > 5 and answered2 + seam2 + passed2 == total, (blocks, err2)
        seams += seam2
        inside += answered2
    assert seams > 0 and inside > 0
    if given == "-b":
        env, err3 = _call(str(d / "env_b"), inputs, extra, {"STRL_CALL_EVIDENCE": "sweep"})
        assert env == plain and _swept(err3)[0] == answered


@pytest.mark.gpu
def test_fallbacks(inputs, tmp_path):
    """CRAM input and STRL_CALL_REGIONS=host ignore the flag (one line says why)"""
    rec = inputs["rec"]
    refs = cramio.make_reference(rec, seed=2)
    fa, cram = str(tmp_path / "ref.fa"), str(tmp_path / "s.cram")
    cramio.write_fasta(fa, rec.targets, refs)
    cramio.write_cram(cram, rec, refs, records_per_slice=211, slices_per_container=2)
    plain, _ = _call(str(tmp_path / "cram_plain"), inputs, ["-f", fa], bam=cram)
    swept, err = _call(str(tmp_path / "cram_sweep"), inputs, ["-f", fa, "--sweep"], bam=cram)
    assert swept == plain and plain[0].count("\n") >= 4
    assert "--sweep ignored: the input is a CRAM" in err and "[strling] sweep:" not in err
    host, err = _call(str(tmp_path / "host"), inputs, ["--sweep"], {"STRL_CALL_REGIONS": "host"})
    bam_plain, _ = _call(str(tmp_path / "bam_plain"), inputs, [])
    assert host == bam_plain and "--sweep ignored: STRL_CALL_REGIONS=host" in err and "[strling] sweep:" not in err
