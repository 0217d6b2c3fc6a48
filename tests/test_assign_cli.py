"""STRL_ASSIGN=device on the command line: `call` with -b / -l and `merge` with -l write the same bytes whether the given loci take
their reads through the host function or through strl_assign_reads_loci_device, and only the variable brings the -v line."""
import os
import subprocess

import numpy as np
import pytest

from strling_amd import bamio, build, synth
from test_call import _loci_from_bounds

pytestmark = pytest.mark.gpu
CLI = build.CLI
LINE = "loci take their reads on the device"


def _run(args, device=False):
    env = {k: v for k, v in os.environ.items() if k != "STRL_ASSIGN"}
    if device:
        env["STRL_ASSIGN"] = "device"
    r = subprocess.run([CLI] + args, capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr
    return r.stderr


@pytest.fixture(scope="module")
def samples(tmp_path_factory):
    """two synthetic samples of test_call.py's kind, extracted; the first one's own bounds (call -m 3) and loci made from them"""
    d = tmp_path_factory.mktemp("assign_cli")
    bams, bins = [], []
    for k, seed in enumerate((21, 22)):
        rec, g = synth.synth_wgs(9000, seed=seed, n_contigs=3, contig_len=40_000)
        bam, bed, binp = (str(d / f"s{k}{x}") for x in (".bam", ".str", ".bin"))
        bamio.write_bam(bam, rec)
        bamio.write_genome_bed(bed, g, rec.targets)
        _run(["extract", "-g", bed, bam, binp])
        bams.append(bam); bins.append(binp)
    _run(["call", "-m", "3", "-o", str(d / "base"), bams[0], bins[0]])
    rows = ["\t".join(l.split("\t")[:11]) for l in open(str(d / "base-bounds.txt")).read().splitlines()[1:]]
    assert len(rows) >= 4
    bounds, loci = str(d / "in-bounds.txt"), str(d / "loci.bed")
    open(bounds, "w").write("#header line\n" + "\n".join(rows[:-1]) + "\n")
    open(loci, "w").write(_loci_from_bounds(rows, rec.targets, np.random.default_rng(2)))
    return d, bams, bins, bounds, loci


@pytest.mark.parametrize("how", ["bounds", "loci", "both", "bounds_sweep"])
def test_call_writes_the_same_files(samples, how):
    d, bams, bins, bounds, loci = samples
    args = {"bounds": ["-b", bounds], "loci": ["-l", loci], "both": ["-b", bounds, "-l", loci], "bounds_sweep": ["-b", bounds, "--sweep"]}[how]
    out = {}
    for device in (False, True):
        prefix = str(d / f"{how}_{int(device)}")
        err = _run(["call", "-v", "-m", "3", "-o", prefix] + args + [bams[0], bins[0]], device)
        assert (LINE in err) == device, err
        out[device] = [open(prefix + x, "rb").read() for x in ("-bounds.txt", "-genotype.txt", "-unplaced.txt")]
    assert out[True] == out[False] and out[True][0].count(b"\n") >= 4
    assert out[True][0] != open(str(d / "base-bounds.txt"), "rb").read()          # the given loci changed the rows


def test_merge_writes_the_same_file(samples):
    d, bams, bins, bounds, loci = samples
    out = {}
    for device in (False, True):
        prefix = str(d / f"joint_{int(device)}")
        err = _run(["merge", "-v", "-m", "2", "-l", loci, "-o", prefix] + bins, device)
        assert (LINE in err) == device, err
        out[device] = open(prefix + "-bounds.txt", "rb").read()
    assert out[True] == out[False] and out[True].count(b"locus") >= 2
    quiet = _run(["merge", "-m", "2", "-l", loci, "-o", str(d / "joint_q")] + bins, True)
    assert LINE not in quiet                                                      # (the line belongs to -v)
