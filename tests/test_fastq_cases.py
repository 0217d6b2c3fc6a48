"""`strling fastq` on the CPU: every case of tests/fastq_cases.py through the host path (STRL_FASTQ=host), from BAM and from SAM text,
against the Python reference's three streams and counts; the library's host entry; the rule as a stand-alone program
(tests/emu/fastq_core_main.cpp, also under the sanitizers), which holds every (first, count) window of every entry against the whole
entry; and the refusals.  tests/test_fastq_device.py runs the same cases on the GPU and compares byte for byte.

One case, quals_beyond_sam, runs from BAM only: qualities past 93 and a 0xFF behind a valid first byte cannot be written as SAM text."""
import gzip
import os
import subprocess

import pytest

import fastq_cases as Q
import sort_bam_cases as S
from strling_amd import api, build

HERE = os.path.dirname(os.path.abspath(__file__))
CLI = build.CLI
CASES = {name: (recs, opts, sam) for name, recs, opts, sam in Q.cases()}
NAMES = list(CASES)
INPUTS = [(name, kind) for name in NAMES for kind in (("bam", "sam") if CASES[name][2] else ("bam",))]


def _fastq(src, args, stdin=None, **env):
    e = dict(os.environ, STRL_FASTQ="host")
    e.update({k: str(v) for k, v in env.items()})
    return subprocess.run([CLI, "fastq", *args, src], capture_output=True, env=e, input=stdin)


@pytest.fixture(scope="module")
def paths(tmp_path_factory):
    return Q.case_dir(tmp_path_factory)


@pytest.fixture(scope="module")
def refs():
    return {name: Q.reference(recs, opts) for name, (recs, opts, _) in CASES.items()}


@pytest.mark.parametrize("name,kind", INPUTS)
def test_host_path_equals_the_reference(name, kind, paths, refs, tmp_path):
    args, files = Q.cli_options(CASES[name][1], str(tmp_path))
    r = _fastq(paths[name][:-4] + "." + kind, args)
    err = r.stderr.decode()
    assert r.returncode == 0, err
    want, counts = refs[name]
    for k, f in files.items():
        assert open(f, "rb").read() == want[k], k
    assert sorted(os.listdir(str(tmp_path))) == sorted(os.path.basename(f) for f in files.values()), "no other file, no temporary name left"
    assert Q.counts_of(err) == counts
    assert len([l for l in err.splitlines() if "fastq:" in l]) == 1, "one line gives the counts"


def test_the_cases_reach_what_they_were_made_for(refs):
    def entries(name, key):
        t = refs[name][0][key].split(b"\n")
        return {t[i][1:]: (t[i + 1], t[i + 3]) for i in range(0, len(t) - 1, 4)}
    s = entries("lengths", "s")
    for l in Q.LENGTHS:
        fwd, rev = [r for r in CASES["lengths"][0] if r["name"] == b"rev%d" % l][0], s[b"rev%d" % l]
        assert len(rev[0]) == l and rev[0].decode() == "".join(Q._COMPLEMENT[c] for c in reversed(fwd["seq"])) and rev[1] == bytes(min(q, 93) + 33 for q in reversed(fwd["qual"]))
    assert refs["lengths"][1] == dict(kept=66, filtered=0, empty=0, pairs=22, singles=22, singles_unwritten=0)
    assert refs["l_seq_0"][1] == dict(kept=3, filtered=0, empty=3, pairs=1, singles=1, singles_unwritten=0), "a pair whose R2 is empty leaves its R1 a single"
    a = entries("all_codes", "s")
    assert a[b"c17"][0] == b"=ACMGRSVTWYHKDBNA" and a[b"c17r"][0] == b"TNVHMDRWABSYCKGT=" and a[b"c17r"][1] == bytes(33 + q for q in range(16, -1, -1))
    assert a[b"c15r"][0] == b"NVHMDRWABSYCKGT"
    q = entries("quals", "s")
    assert q[b"absent"][1] == b'"""""' and q[b"q0"][1] == b"!!!" and q[b"q93"][1] == b"~~~"
    q = entries("quals_beyond_sam", "s")
    assert q[b"q94"][1] == b"~~~" and q[b"q254"][1] == b"~~~~" and q[b"later_ff"][1] == b"+~5~~" and q[b"later_ff_rev"][1] == b"~~5~+"
    assert entries("absent_default_40", "s")[b"absent"][1] == b"IIIII" and entries("absent_default_200", "s")[b"absent"][1] == b"~~~~~"
    n = entries("names", "p1")
    assert b"x" in n and b"n" * 100 + b"/" + b"m" * 153 in n and b"a/1" in n and refs["names"][1]["pairs"] == 3 and set(entries("names", "s")) == {b"a/2", b"/", b"y"}
    assert refs["names"][0]["p1"].startswith(b"@x\nACGT\n+\n????\n@x\nTTGA\n+\n@@@@\n@" + b"n" * 100), "x first: its first record comes first; the R1 of the long name before its R2"
    n = refs["names_suffix"][0]
    assert n["p1"].startswith(b"@x/1\nACGT") and b"@a/1/1\nA\n+\n&\n@a/1/2\nG\n" in n["p1"] and b"@a/2/2\n" in n["s"] and b"@//" not in n["s"] and b"@/\nT\n" in n["s"]
    f = refs["flags"]
    assert f[1] == dict(kept=17, filtered=2, empty=0, pairs=4, singles=9, singles_unwritten=0)
    assert [l[1:] for l in f[0]["p1"].split(b"\n")[::4] if l] == [b"sup", b"sup", b"sec", b"sec", b"unpaired_bits", b"unpaired_bits", b"unmapped", b"unmapped"]
    assert refs["flags_filter_0"][1] == dict(kept=19, filtered=0, empty=0, pairs=2, singles=15, singles_unwritten=0), "three under sup and under sec: all singles"
    assert refs["flags_filter_0x904"][1]["filtered"] == 5 and refs["flags_filter_0x904"][1]["pairs"] == 2
    assert refs["flags_no_singles"][1]["singles_unwritten"] == 9 and refs["flags_no_singles"][0]["s"] == b""
    assert b"@r1/1\n" in refs["flags_suffix"][0]["s"] and b"@r3\n" in refs["flags_suffix"][0]["s"] and b"@r0\n" in refs["flags_suffix"][0]["s"]
    o = refs["order"][0]
    assert [l[1:] for l in o["p1"].split(b"\n")[::4] if l][:4] == [b"far", b"far", b"near", b"near"], "the pair stands where its earlier record stood"
    assert [l[1:] for l in o["s"].split(b"\n")[::4] if l] == [b"s0", b"s1", b"s2", b"mid", b"last"]
    far = [r for r in CASES["order"][0] if r["name"] == b"far"]
    assert far[0]["flag"] & 0x80 and o["p1"].split(b"\n")[1].decode() == far[1]["seq"], "R2 came first in the input, R1 is written first"
    assert refs["no_record"] == (dict(p1=b"", p2=b"", s=b""), dict.fromkeys(Q.COUNT_KEYS, 0))
    assert refs["pairs_only"][1]["singles"] == 0 and refs["singles_only"][1]["pairs"] == 0 and refs["singles_only"][0]["p1"] == b""
    assert refs["nothing_kept"][1] == dict(kept=0, filtered=20, empty=1, pairs=0, singles=0, singles_unwritten=0)
    assert refs["random_3000"][1]["pairs"] == 1200 and refs["random_3000"][1]["singles"] == 600
    s = refs["lengths_split"][0]
    assert s["p1"].count(b"\n") == s["p2"].count(b"\n") == 4 * 22 and refs["lengths"][0]["p1"].count(b"\n") == 8 * 22
    assert refs["one_name_512"][1] == dict(kept=512, filtered=0, empty=0, pairs=0, singles=512, singles_unwritten=0)


def test_without_s_the_singles_are_counted_and_absent(paths, refs, tmp_path):
    o = str(tmp_path / "pairs.fq")
    r = _fastq(paths["flags"], ["-o", o])
    err = r.stderr.decode()
    assert r.returncode == 0, err
    assert Q.counts_of(err) == refs["flags_no_singles"][1] and Q.counts_of(err)["singles_unwritten"] == 9
    assert open(o, "rb").read() == refs["flags"][0]["p1"] and os.listdir(str(tmp_path)) == ["pairs.fq"]


def test_stdout_and_stdin(paths, refs):
    r = _fastq("-", ["-o", "-"], stdin=open(paths["order"][:-4] + ".sam", "rb").read())
    assert r.returncode == 0, r.stderr
    assert r.stdout == refs["order"][0]["p1"]


# ---- the refusals ---------------------------------------------------------------------------------------------------------------------
def test_cram_is_refused(tmp_path):
    p = str(tmp_path / "in.cram")
    open(p, "wb").write(b"CRAM\3\0" + b"\0" * 64)
    r = _fastq(p, ["-o", str(tmp_path / "o.fq")])
    assert r.returncode == 1 and b"is a CRAM" in r.stderr and b"out of scope" in r.stderr and not os.path.exists(str(tmp_path / "o.fq"))


def test_output_options_are_checked(paths, tmp_path):
    a, b, o = str(tmp_path / "a.fq"), str(tmp_path / "b.fq"), str(tmp_path / "o.fq")
    r = _fastq(paths["flags"], ["-o", o, "-1", a, "-2", b])
    assert r.returncode == 1 and b"one or the other" in r.stderr
    r = _fastq(paths["flags"], ["-1", a])
    assert r.returncode == 1 and b"-1 and -2 go together" in r.stderr
    r = _fastq(paths["flags"], ["-2", b])
    assert r.returncode == 1 and b"-1 and -2 go together" in r.stderr
    r = _fastq(paths["flags"], [])
    assert r.returncode == 1 and b"is required" in r.stderr
    r = _fastq(paths["flags"], ["-o", o, "-F", "abc"])
    assert r.returncode == 1 and b"--filter must be an integer" in r.stderr
    assert os.listdir(str(tmp_path)) == []


def test_a_record_that_does_not_fit_its_block_size_is_refused(paths, tmp_path):
    p, o = str(tmp_path / "big.bam"), str(tmp_path / "o.fq")
    Q.oversized(paths["flags"], p, 5)
    r = _fastq(p, ["-o", o, "-s", str(tmp_path / "s.fq")])
    assert r.returncode == 1 and os.listdir(str(tmp_path)) == ["big.bam"], r.stderr
    assert b"record 5" in r.stderr and b"block_size" in r.stderr and b"status -6" in r.stderr, r.stderr


def test_sort_is_not_moved(paths, tmp_path):
    """the driver the command shares still sorts as before"""
    o = str(tmp_path / "o.bam")
    r = subprocess.run([CLI, "sort", "-o", o, paths["order"]], capture_output=True, text=True, env=dict(os.environ, STRL_SORT="host"))
    assert r.returncode == 0 and "fastq" not in r.stderr, r.stderr
    S.check_file(o, S.reference_stream(paths["order"])[0])


# ---- the rule through the library ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["lengths", "lengths_split", "flags_suffix", "flags_filter_0", "flags_no_singles", "quals_beyond_sam", "absent_default_40", "no_record", "random_3000"])
def test_library_host_entry(name, refs):
    recs, opts, _ = CASES[name]
    streams, counts = api.fastq_host(b"".join(Q.pack(r) for r in recs), **Q.abi_options(opts))
    assert dict(zip(("p1", "p2", "s"), streams)) == refs[name][0]
    assert counts == {"n_" + k: v for k, v in refs[name][1].items()}


def test_library_host_entry_refuses_a_record_that_does_not_fit():
    recs = [bytearray(Q.pack(r)) for r in CASES["flags"][0]]
    recs[2][16] = 200                                           # 200 CIGAR operations in a record of none
    with pytest.raises(api.StrlingError) as e:
        api.fastq_host(b"".join(bytes(r) for r in recs))
    assert e.value.code == -6 and "record 2" in str(e.value)


# ---- the rule as a stand-alone program, plain and under the sanitizers ---------------------------------------------------------------
def _program(sanitize):
    out = os.path.join(HERE, "emu", "fastq_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "fastq_core_main" + ("_san" if sanitize else ""))
    src = os.path.join(HERE, "emu", "fastq_core_main.cpp")
    cores = [os.path.join(HERE, "..", "strling_amd", "csrc", h) for h in ("fastq_core.h", "markdup_core.h")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(f) for f in [src] + cores):
        flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
        subprocess.check_call(["g++", "-std=c++17", *flags, "-o", exe, src])
    return exe


@pytest.fixture(scope="module", params=[False, True], ids=["plain", "asan_ubsan"])
def core_main(request):
    return _program(request.param)


def test_standalone_program_checks(core_main):
    r = subprocess.run([core_main], capture_output=True, text=True)
    assert r.returncode == 0 and "all cases passed" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


@pytest.mark.parametrize("name", NAMES)
def test_standalone_program_windows_and_streams(core_main, name, paths, refs, tmp_path):
    """every (first, count) window of every kept record's entry equals the whole entry's bytes there; the host rule's streams"""
    recs, opts, _ = CASES[name]
    raw, out = str(tmp_path / "in.raw"), str(tmp_path / "out")
    open(raw, "wb").write(gzip.decompress(open(paths[name], "rb").read()))
    r = subprocess.run([core_main, raw, out, hex(opts["F"]), str(int(opts["N"])), str(opts["v"]), str(int(not opts["split"])), str(int(opts["singles"]))], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    want, counts = refs[name]
    lines = r.stdout.split("\n")
    assert lines[0] == "counts " + " ".join(str(counts[k]) for k in Q.COUNT_KEYS)
    lens = [len(e) for e in (Q._entry(Q.pack(x), opts) for x in recs if not x["flag"] & opts["F"] and x["seq"])]
    assert lines[1] == "windows %d" % sum(l * (l + 1) // 2 for l in lens)
    for k in ("p1", "p2", "s"):
        assert open(out + "." + k, "rb").read() == want[k], k


def test_standalone_program_refuses_a_record_that_does_not_fit(core_main, paths, tmp_path):
    p = str(tmp_path / "big.bam")
    Q.oversized(paths["flags"], p, 5)
    raw = str(tmp_path / "in.raw")
    open(raw, "wb").write(gzip.decompress(open(p, "rb").read()))
    r = subprocess.run([core_main, raw, str(tmp_path / "out"), "0x900", "0", "1", "1", "1"], capture_output=True, text=True)
    assert r.returncode == 3 and "record 5" in r.stderr, r.stderr[-2000:]
