"""`strling view` on the CPU: every case of tests/view_cases.py through the host path (STRL_VIEW=host) by the command against the
Python reference; the library's host entry with room exact to the byte and one byte short; every refusal's words; -h, -H, -c;
regions; the round trip SAM text -> `strling sort` -> `strling view`; and the rule as a stand-alone program
(tests/emu/view_core_main.cpp, also under the sanitizers), which writes every line through the kernels' sinks into a buffer of exactly
its bytes and holds view_float_g against snprintf("%g").  tests/test_view_device.py runs the same cases on the GPU."""
import gzip
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import sam_cases
import sort_bam_cases
import view_cases as V
from strling_amd import api, build

HERE = os.path.dirname(os.path.abspath(__file__))
CLI = build.CLI
CASES = V.cases()
NAMES = list(CASES)
GOOD = [n for n in NAMES if not CASES[n]["refused"]]
BAD = [n for n in NAMES if CASES[n]["refused"]]
REF_NAMES = [n for n, _ in V.TG]


def _view(args, **env):
    e = dict(os.environ, STRL_VIEW="host")
    e.update({k: str(v) for k, v in env.items()})
    return subprocess.run([CLI, "view", *args], capture_output=True, env=e)


@pytest.fixture(scope="module")
def paths(tmp_path_factory):
    return V.case_dir(tmp_path_factory)


@pytest.fixture(scope="module")
def refs():
    return {n: V.reference(c["recs"], c["opts"]) for n, c in CASES.items()}


@pytest.fixture(scope="module")
def regions_bam(tmp_path_factory):
    return V.regions_bam(str(tmp_path_factory.mktemp("view_regions")), CLI)


@pytest.mark.parametrize("name", GOOD)
def test_host_path_equals_the_reference(name, paths, refs, tmp_path):
    o = str(tmp_path / "out.sam")
    r = _view(V.cli_options(CASES[name]["opts"]) + ["--verbose", "-o", o, paths[name]])
    assert r.returncode == 0, r.stderr
    assert open(o, "rb").read() == refs[name][0]
    assert os.listdir(str(tmp_path)) == ["out.sam"], "no temporary name left"
    line = r.stderr.decode()
    assert '"path": "host"' in line and '"written": %d,' % refs[name][1] in line and '"dropped": %d,' % refs[name][2] in line


@pytest.mark.parametrize("option", list("fFGq"))
def test_every_filter_drops_the_first_the_last_and_every_record_of_a_chunk(option, refs):
    c = CASES["filter_" + option]
    assert [k for k, v in c["opts"].items() if v] == [option], "the option alone"
    assert V.filter_shape(c["recs"], c["block"], c["opts"]) == (True, True, True)
    assert 0 < refs["filter_" + option][1] < len(c["recs"])


def test_the_cases_reach_what_they_were_made_for(refs):
    lines = {n: refs[n][0].split(b"\n")[:-1] for n in GOOD}
    # SEQ starts at every offset modulo 16 for every length
    starts = {}
    for l in lines["lengths"]:
        f = l.split(b"\t")
        starts.setdefault(len(f[9]) if f[9] != b"*" else 0, set()).add(sum(len(x) + 1 for x in f[:9]) % 16)
    assert sorted(starts) == list(V.L_SEQS) and all(len(v) == 16 for v in starts.values())
    assert lines["padding_nibble"][-1].split(b"\t")[9] == b"=ACMGRSVTWYHKDBNA"
    assert [l.split(b"\t")[0] for l in lines["no_name"]] == [b"*", b"*", b"x"]
    n = {l.split(b"\t")[0]: l.split(b"\t") for l in lines["numbers"]}
    assert [n[b"f%d" % f][1] for f in (0, 9, 10, 99, 100, 65535)] == [b"0", b"9", b"10", b"99", b"100", b"65535"]
    assert n[b"pos_m1"][3] == b"0" and n[b"pos_max"][3] == b"2147483647" and n[b"pos_max"][7] == b"2147483647" and n[b"pos_max"][6] == b"="
    assert n[b"tlen_min"][8] == b"-2147483648" and n[b"tlen_max"][8] == b"2147483647"
    assert n[b"tagints"][11:] == [b"I0:i:-128", b"I1:i:-32768", b"I2:i:-2147483648", b"I3:i:255", b"I4:i:65535", b"I5:i:4294967295"]
    c = [l.split(b"\t")[5] for l in lines["cigars"]]
    assert c[0] == b"*" and c[1] == b"268435455M" and len(re.findall(rb"\d+[MIDNSHP=X]", c[2])) == 16 and len(re.findall(rb"\d+[MIDNSHP=X]", c[3])) == 17 and c[4] == b"1X"
    assert len(re.findall(rb"\d+[MIDNSHP=X]", lines["cigar_65535"][1].split(b"\t")[5])) == 65535
    r = [(l.split(b"\t")[2], l.split(b"\t")[6]) for l in lines["references"]]
    assert r == [(b"*", b"*"), (b"chrTwo", b"="), (b"t0", b"chrTwo"), (b"empty3", b"t0"), (b"*", b"empty3"), (b"chrTwo", b"*")]
    q = [l.split(b"\t")[10] for l in lines["quals"]]
    assert q == [b"*", b"+~5~~", b"~~!}", b"~" * 20 + b"*" * 20, b"*"]
    t = lines["tags"][0].split(b"\t")[11:]
    assert b"XE:Z:" in t and b"XH:H:1AE301" in t and b"XA:A:!" in t and b"Bc:B:c" in t and b"bS:B:S,65535" in t and b"XG:d:-100000" in t and len([x for x in t if x.startswith(b"L")]) == 7
    assert all(x.count(b",") == 17 for x in t if x.startswith(b"L"))
    f = lines["floats_device"]
    assert [l.split(b"\t")[11] for l in f[:-1]] == [("fl:f:" + s).encode() for _, s in V.DEVICE_FLOATS]
    assert f[-1].split(b"\t")[11:] == [b"d0:d:0.5", b"d1:d:1.00002e+06", b"d2:d:-0"]
    h = {l.split(b"\t")[0]: l.split(b"\t")[11] for l in lines["floats_hard"]}
    assert [h[b"h%d" % i] for i in range(4)] == [("fl:f:" + s).encode() for _, s in V.HARD_FLOATS] and h[b"dbl"] == b"d0:d:0.1" and h[b"tiny"] == b"fl:f:7.5e-06"
    assert refs["filter_drops_everything"][:2] == (b"", 0) and refs["no_record"] == (b"", 0, 0) and refs["filter_first_and_last"][2] == 4
    assert len(CASES["random_3000"]["recs"]) == 3000 > 2048, "more than one tile of the prefix sum"


@pytest.mark.parametrize("name", BAD)
def test_refusals_in_words_and_no_output_file(name, paths, tmp_path):
    ordinal, key = CASES[name]["refused"]
    assert V.reference(CASES[name]["recs"], CASES[name]["opts"]) == (None, ordinal, key)
    o = str(tmp_path / "out.sam")
    r = _view(["-o", o, paths[name]])
    assert r.returncode == 1 and os.listdir(str(tmp_path)) == [], r.stderr
    assert ("malformed BAM record %d: %s (status -6)" % (ordinal, V.REFUSALS[key])).encode() in r.stderr, r.stderr
    with pytest.raises(api.StrlingError) as e:
        api.view_host(b"".join(CASES[name]["recs"]), REF_NAMES)
    assert e.value.code == -6 and "record %d: %s" % (ordinal, V.REFUSALS[key]) in str(e.value)


def test_a_refused_record_that_is_not_kept_is_passed_over(paths, tmp_path):
    """the op code, the references and the tags are held against kept records only"""
    recs = CASES["cigar_op_9"]["recs"]
    bad = bytearray(recs[2])
    struct.pack_into("<H", bad, 18, 0x400)
    text, info = api.view_host(b"".join(recs[:2]) + bytes(bad), REF_NAMES, exclude=0x400)
    assert text == V.reference(recs[:2], V.DEFAULTS)[0] and info["dropped"] == 1


def test_a_record_that_does_not_fit_its_block_size_is_refused_kept_or_not(tmp_path):
    recs = [bytearray(r) for r in CASES["filter_f"]["recs"][:8]]
    struct.pack_into("<i", recs[5], 20, 4000)                    # l_seq past the record; the record's flag does not pass -f 1
    p = str(tmp_path / "big.bam")
    V.write_case(p, [bytes(r) for r in recs])
    r = _view(["-f", "1", p])
    assert r.returncode == 1 and b"malformed BAM record 5: its name, CIGAR, bases and qualities do not fit its block_size" in r.stderr and r.stdout == b""


@pytest.mark.parametrize("name", GOOD)
def test_library_host_entry_exact_and_one_short(name, refs):
    c = CASES[name]
    raw = b"".join(c["recs"])
    want, written, dropped = refs[name]
    text, info = api.view_host(raw, REF_NAMES, cap=len(want), **V.abi_options(c["opts"]))
    assert text == want and (info["records"], info["written"], info["dropped"], info["text_bytes"]) == (len(c["recs"]), written, dropped, len(want))
    if want:
        with pytest.raises(api.StrlingError) as e:
            api.view_host(raw, REF_NAMES, cap=len(want) - 1, **V.abi_options(c["opts"]))
        assert e.value.code == -4 and e.value.need == len(want)


def test_header_options_and_count(paths, refs):
    p = paths["filter_q"]
    body = refs["filter_q"][0]
    assert _view(["-q", "20", p]).stdout == body
    assert _view(["-h", "-q", "20", p]).stdout == V.HEADER_TEXT.encode() + body
    assert _view(["-H", p]).stdout == V.HEADER_TEXT.encode()
    assert _view(["-c", "-q", "20", p]).stdout == b"%d\n" % refs["filter_q"][1]
    assert _view(["-c", paths["no_record"]]).stdout == b"0\n" and _view(["-h", paths["no_record"]]).stdout == V.HEADER_TEXT.encode()
    assert _view(["-o", "-", "-q", "20", p]).stdout == body


def test_what_the_command_does_not_do_is_refused_in_the_usage_words(paths, tmp_path):
    for args in (["-b"], ["-@", "4"], ["-C"], ["-r", "grp"], ["-d", "NM"], ["-M"]):
        r = _view(args + [paths["numbers"]])
        assert r.returncode == 1 and b"is not one of this command's" in r.stderr and b"-b and every other output format" in r.stderr and b"read-group and tag" in r.stderr, args
    sam = str(tmp_path / "in.sam")
    open(sam, "w").write(V.HEADER_TEXT + "r\t4\t*\t0\t0\t*\t*\t0\t0\tA\t*\n")
    r = _view([sam])
    assert r.returncode == 1 and b"SAM text is not read by this command" in r.stderr
    cram = str(tmp_path / "in.cram")
    open(cram, "wb").write(b"CRAM\3\0" + b"\0" * 64)
    r = _view([cram])
    assert r.returncode == 1 and b"is a CRAM" in r.stderr
    r = _view(["-f", "x", paths["numbers"]])
    assert r.returncode == 1 and b"-f must be an integer" in r.stderr
    assert b"Usage:" in subprocess.run([CLI, "view"], capture_output=True).stdout


# ---- regions ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regions", V.REGIONS, ids=["+".join(r) for r in V.REGIONS])
def test_regions_on_the_host_path(regions, regions_bam):
    recs = V.region_records()
    want, written = V.regions_reference(recs, V.DEFAULTS, regions)
    r = _view([regions_bam] + regions)
    assert r.returncode == 0 and r.stdout == want, r.stderr
    assert _view(["-c", regions_bam] + regions).stdout == b"%d\n" % written


@pytest.mark.parametrize("batch", [1, 3])
def test_regions_in_small_batches(batch, regions_bam):
    """a region fed a few records at a time (as a region larger than a batch is) gives the same text and counts"""
    recs = V.region_records()
    for regions in V.REGIONS:
        want, written = V.regions_reference(recs, V.DEFAULTS, regions)
        assert _view([regions_bam] + regions, STRL_VIEW_BATCH_RECORDS=batch).stdout == want
        assert _view(["-c", regions_bam] + regions, STRL_VIEW_BATCH_RECORDS=batch).stdout == b"%d\n" % written


def test_the_regions_reach_what_they_were_made_for():
    recs = V.region_records()
    one = [l.split(b"\t")[0] for l in V.regions_reference(recs, V.DEFAULTS, ["t0:1001-2000"])[0].split(b"\n")[:-1]]
    assert one == [b"reaches_beg_1", b"deletion_reaches", b"no_ref_len_in", b"flag4_with_pos", b"both", b"last_in"]
    two = [l.split(b"\t")[0] for l in V.regions_reference(recs, V.DEFAULTS, ["t0:1001-2000", "t0:1901-2500"])[0].split(b"\n")[:-1]]
    assert two == one + [b"both", b"last_in", b"first_out"], "a record that overlaps two given regions is written once for each"
    assert V.regions_reference(recs, V.DEFAULTS, ["empty3"]) == (b"", 0)


def test_regions_with_filters_and_the_library(regions_bam):
    recs = V.region_records()
    opts = dict(V.DEFAULTS, F=4)
    want, _ = V.regions_reference(recs, opts, ["t0:1001-2000"])
    assert _view(["-F", "4", regions_bam, "t0:1001-2000"]).stdout == want and b"flag4_with_pos" not in want
    text, info = api.view_host(b"".join(recs), REF_NAMES, **V.abi_options(opts, V.parse_region("t0:1001-2000")))
    assert text == want and info["written"] == 5 and info["dropped"] == len(recs) - 5


def test_a_region_needs_the_index_and_a_known_reference(paths, regions_bam):
    r = _view([paths["numbers"], "t0"])
    assert r.returncode == 1 and b"index" in r.stderr
    r = _view([regions_bam, "nowhere:1-5"])
    assert r.returncode == 1 and b"view: unknown reference in region nowhere:1-5" in r.stderr


# ---- the round trip ---------------------------------------------------------------------------------------------------------------------
def _float_spellings_survive(line):
    """False: a float of the line is not spelled as %g spells the float32 it becomes (more than six digits, another form)"""
    for f in line.decode("latin-1").split("\t")[11:]:
        tag, typ, val = f.split(":", 2)
        vals = [val] if typ == "f" else val.split(",")[1:] if typ == "B" and val.startswith("f") else []
        for v in vals:
            if "%g" % np.float32(v) != v:
                return False
    return True


SAM_CASES = dict(sam_cases.cases())


def _canonical(line):
    """the line as a BAM record can give it back: SAM text spells three things in more than one way and the record keeps the value
    only -- bases in lower case and letters outside the sixteen codes (stored as N), a `+` in front of an integer (TLEN, PNEXT, i tags, B elements),
    and an RNEXT that names RNAME's reference (`=`).  Nothing else is touched."""
    f = line.split(b"\t")
    f[9] = f[9].upper() if f[9] == b"*" else bytes(c if c in b"=ACMGRSVTWYHKDBN" else ord("N") for c in f[9].upper())
    if f[6] == f[2] and f[2] != b"*":
        f[6] = b"="
    plus = lambda x: x[1:] if re.fullmatch(rb"\+\d+", x) else x
    f[3], f[7], f[8] = plus(f[3]), plus(f[7]), plus(f[8])
    for k in range(11, len(f)):
        tag, typ, val = f[k].split(b":", 2)
        if typ == b"i":
            f[k] = tag + b":i:" + plus(val)
        elif typ == b"B" and val[:1] in b"cCsSiI":
            f[k] = tag + b":B:" + b",".join([val.split(b",")[0]] + [plus(x) for x in val.split(b",")[1:]])
    return b"\t".join(f)


@pytest.mark.parametrize("name", list(SAM_CASES))
def test_round_trip_from_sam_text(name, tmp_path):
    """SAM text in coordinate order -> `strling sort` (host) -> `strling view` gives the alignment lines back (lines whose floats
    need more than six digits or another form than %g's are passed over; _canonical says what else SAM text cannot keep)"""
    text = SAM_CASES[name]
    text = text if isinstance(text, bytes) else text.encode("latin-1")
    header, lines = sam_cases.split_text(text)
    n_ref = len(sam_cases.header_refs(header))
    recs = sam_cases.reference(text)[4]
    keys = [sort_bam_cases.ref_key(r, n_ref) for r in recs]
    lines = [lines[i] for i in sorted(range(len(lines)), key=lambda i: keys[i])]      # (stable, like the sort: the order of equal keys stays)
    src, bam = str(tmp_path / "in.sam"), str(tmp_path / "sorted.bam")
    open(src, "wb").write(header + b"".join(l + b"\n" for l in lines))
    r = subprocess.run([CLI, "sort", "-o", bam, src], capture_output=True, env=dict(os.environ, STRL_SORT="host"))
    assert r.returncode == 0, r.stderr
    r = _view([bam])
    assert r.returncode == 0, r.stderr
    got = r.stdout.split(b"\n")[:-1]
    assert len(got) == len(lines)
    for g, w in zip(got, lines):
        if _float_spellings_survive(w):
            assert g == _canonical(w)


# ---- the rule as a stand-alone program, plain and under the sanitizers ---------------------------------------------------------------
def _program(sanitize):
    out = os.path.join(HERE, "emu", "view_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "view_core_main" + ("_san" if sanitize else ""))
    src = os.path.join(HERE, "emu", "view_core_main.cpp")
    cores = [os.path.join(HERE, "..", "strling_amd", "csrc", h) for h in ("view_core.h", "markdup_core.h")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(f) for f in [src] + cores):
        flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
        subprocess.check_call(["g++", "-std=c++17", *flags, "-o", exe, src])
    return exe


@pytest.fixture(scope="module", params=[False, True], ids=["plain", "asan_ubsan"])
def core_main(request):
    return _program(request.param)


def test_standalone_program_floats(core_main):
    """200 000 seeded random float bit patterns: identical to snprintf("%g") or "not mine", "not mine" only outside the stated range"""
    r = subprocess.run([core_main], capture_output=True, text=True)
    assert r.returncode == 0 and "all cases passed" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    answered, passed_on = (int(x) for x in re.search(r"floats answered (\d+) passed on (\d+)", r.stdout).groups())
    assert answered > 100000 and passed_on > 10000


@pytest.mark.parametrize("name", NAMES)
def test_standalone_program_lines_exact_to_the_byte(core_main, name, paths, refs, tmp_path):
    c = CASES[name]
    raw, out = str(tmp_path / "in.raw"), str(tmp_path / "out.sam")
    open(raw, "wb").write(gzip.decompress(open(paths[name], "rb").read()))
    o = c["opts"]
    r = subprocess.run([core_main, raw, out, str(o["f"]), str(o["F"]), str(o["G"]), str(o["q"])], capture_output=True, text=True)
    if c["refused"]:
        assert r.returncode == 3 and "record %d: %s" % (c["refused"][0], V.REFUSALS[c["refused"][1]]) in r.stderr, r.stderr[-2000:]
        return
    assert r.returncode == 0, r.stderr[-4000:]
    want, written, dropped = refs[name]
    assert r.stdout == "counts %d %d %d %d\n" % (len(c["recs"]), written, dropped, len(want)) and open(out, "rb").read() == want


def test_standalone_program_region(core_main, tmp_path):
    recs = V.region_records()
    raw, out = str(tmp_path / "in.raw"), str(tmp_path / "out.sam")
    open(raw, "wb").write(V.raw_bam(recs))
    tid, beg, end = V.parse_region("t0:1001-2000")
    r = subprocess.run([core_main, raw, out, "0", "0", "0", "0", str(tid), str(beg), str(end)], capture_output=True, text=True)
    assert r.returncode == 0 and open(out, "rb").read() == V.regions_reference(recs, V.DEFAULTS, ["t0:1001-2000"])[0], r.stderr
