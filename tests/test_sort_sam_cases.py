"""`strling sort` over SAM text on the CPU: every case of tests/sam_cases.py through the host path (STRL_SORT=host), from a file and
from stdin, byte for byte against the stream a Python encoder written from the SAM specification and Python's stable sorted() give;
the indexes as structures against bamio; the library's host entries (api.sam_encode / sam_header) line by line; every refusal with
its line number and its words; the round trip BAM -> SAM text -> sort against the sort of the BAM; and the rule as a stand-alone
program under the sanitizers (tests/emu/sam_core_main.cpp).  tests/test_sort_sam_device.py runs the same cases on the GPU."""
import gzip
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import sam_cases as C
import sort_bam_cases as S
import sort_index_cases as I
from strling_amd import api, bamio, build

HERE = os.path.dirname(os.path.abspath(__file__))
CLI = build.CLI
CASES = C.cases()
NAMES = [n for n, _ in CASES]
REFUSALS = C.refusals()


def _sort(src, out, *opts, stdin=None, **env):
    e = dict(os.environ, STRL_SORT="host")
    e.update({k: str(v) for k, v in env.items()})
    return subprocess.run([CLI, "sort", *opts, "-o", out, src], capture_output=True, input=stdin, env=e)


def _info(r):
    return json.loads(r.stderr.decode().strip().splitlines()[-1])


@pytest.fixture(scope="module")
def texts(tmp_path_factory):
    d = tmp_path_factory.mktemp("sam_cases")
    out = {}
    for name, text in CASES:
        p = os.path.join(str(d), name + ".sam")
        open(p, "wb").write(text)
        out[name] = (p, text)
    return out


@pytest.fixture(scope="module")
def refs():
    return {name: C.reference(text) for name, text in CASES}


@pytest.mark.parametrize("name", NAMES)
def test_host_sort_of_a_file_equals_the_reference(name, texts, refs, tmp_path):
    stream, n, no_ref, in_order, _ = refs[name]
    o = str(tmp_path / "o.bam")
    r = _sort(texts[name][0], o, "-v")
    assert r.returncode == 0, r.stderr
    S.check_file(o, stream)
    info = _info(r)
    assert info["path"] == "host" and info["input"] == "sam" and info["records"] == n == info["lines"] and info["no_reference"] == no_ref
    assert info["stream_bytes"] == len(stream) and info["already_sorted"] is in_order
    header = C.split_text(texts[name][1])[0]
    assert len(texts[name][1]) - len(header) <= info["text_bytes"] <= len(texts[name][1]) - len(header) + 1, "the alignment lines' bytes (a newline added behind a last line without one)"
    assert not [f for f in os.listdir(str(tmp_path)) if ".tmp." in f]


@pytest.mark.parametrize("name", NAMES)
def test_host_sort_of_stdin_equals_the_reference(name, texts, refs, tmp_path):
    o = str(tmp_path / "o.bam")
    r = _sort("-", o, stdin=texts[name][1], STRL_SAM_CHUNK_KB=0.5)      # (and chunks of a line or two)
    assert r.returncode == 0, r.stderr
    S.check_file(o, refs[name][0])


def test_the_cases_reach_what_they_were_made_for(refs):
    lens = {len(l) for l in C.split_text(dict(CASES)["line_lengths_every_residue"])[1]}
    assert {l % 256 for l in lens} == set(range(256)) and {l % 16 for l in lens} == set(range(16))
    first = C.split_text(dict(CASES)["tab_on_16_byte_boundary"])[1][0]
    assert first[16:17] == b"\t" and first[32:33] == b"\t"
    recs = refs["i_tags"][4]
    assert [chr(r[36 + 3 + 2]) for r in recs] == list("iissccCCSSIIII"), "the smallest type in htslib's order"
    assert max(len(r) for r in refs["line_400kb"][4]) > 300_000 and max(len(l) for l in C.split_text(dict(CASES)["line_400kb"])[1]) > 400_000
    assert struct.unpack_from("<H", refs["cigars"][4][1], 16)[0] == 65535
    bins = {r[36:r.index(b"\0", 36)].decode(): struct.unpack_from("<H", r, 14)[0] for r in refs["cigars"][4]}
    assert bins["unmapped_with_cigar"] == 4681 + 1 and bins["mapped_long"] == 585 and bins["reflen0"] == 4681 + 1
    assert struct.unpack_from("<H", refs["integer_ends"][4][0], 14)[0] == 4680, "pos -1"
    assert C.fnv(C.colliding_names()[0]) & 7 == C.fnv(C.colliding_names()[1]) & 7 == C.fnv(C.colliding_names()[2]) & 7
    assert refs["header_only"][1] == 0 and refs["no_header_star_refs"][2] == 40


# ---- the indexes ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["bai", "csi", "csi_m12"])
@pytest.mark.parametrize("name", ["shuffle_3000", "refs_256", "name_prefixes", "header_only"])
def test_write_index_is_the_index_of_the_written_file(name, kind, texts, tmp_path):
    """the index from the sort's pass against `strling bamindex`'s host-side twin of the file just written: bamio's reader walks both"""
    o = str(tmp_path / "o.bam")
    opts = {"bai": ["--write-index"], "csi": ["--write-index", "--csi"], "csi_m12": ["--write-index", "--csi", "-m", "12"]}[kind]
    r = _sort(texts[name][0], o, *opts, "-v")
    assert r.returncode == 0, r.stderr
    idx = o + (".bai" if kind == "bai" else ".csi")
    assert os.path.exists(idx) and _info(r)["index"] == ("bai" if kind == "bai" else "csi")
    # the same records sorted from a BAM give the same index bytes: the index step does not know where the records came from
    raw = gzip.decompress(open(o, "rb").read())
    b = str(tmp_path / "same.bam")
    open(b, "wb").write(bamio.bgzf_bytes(raw))
    o2 = str(tmp_path / "o2.bam")
    r2 = subprocess.run([CLI, "sort", *opts, "-o", o2, b], capture_output=True, env=dict(os.environ, STRL_SORT="host"))
    assert r2.returncode == 0, r2.stderr
    assert open(o2, "rb").read() == open(o, "rb").read()
    assert open(o2 + (".bai" if kind == "bai" else ".csi"), "rb").read() == open(idx, "rb").read()
    KIND = {"bai": "bai", "csi": ("csi", 14), "csi_m12": ("csi", 12)}[kind]
    assert I.index_structure(idx, o, KIND) == I.reference_index(o, KIND)


# ---- the rule through the library -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_library_encodes_every_line_as_the_reference(name, refs):
    text = dict(CASES)[name]
    header, lines = C.split_text(text)
    raw, names, lens = api.sam_header(text)
    assert raw == C.bam_header(header)
    assert [(n.encode(), l) for n, l in zip(names, lens)] == C.header_refs(header)
    step = max(1, len(lines) // 300)
    for k in range(0, len(lines), step):
        assert api.sam_encode(lines[k], names) == refs[name][4][k], (name, k)
    if lines:
        assert api.sam_encode(lines[0] + b"\r\n", names) == refs[name][4][0]


@pytest.mark.parametrize("name,text,line,words", [r for r in REFUSALS if r[2] is not None], ids=[r[0] for r in REFUSALS if r[2] is not None])
def test_library_refuses_the_line(name, text, line, words):
    header, lines = C.split_text(text)
    names = [n.decode() for n, _ in C.header_refs(header)]
    with pytest.raises(api.StrlingError) as e:
        api.sam_encode(lines[line - 1], names)
    assert e.value.code == -6 and words in str(e.value)
    assert len(api.sam_encode(lines[0], names)) > 36


def test_library_refuses_headers():
    for text, words in ((b"@SQ\tSN:a\tLN:5\n@SQ\tSN:a\tLN:6\n", "SN a occurs twice"), (b"@SQ\tLN:5\n", "has no SN"), (b"@SQ\tSN:a\n", "LN"), (b"@SQ\tSN:a\tLN:0\n", "LN"),
                        (b"@SQ\tSN:a\tLN:2147483648\n", "LN")):
        with pytest.raises(api.StrlingError) as e:
            api.sam_header(text)
        assert e.value.code == -6 and words in str(e.value), text


# ---- refusals: one line, exit 1, no file ------------------------------------------------------------------------------------------------
def _refused(r, out, *words):
    err = r.stderr.decode()
    assert r.returncode == 1 and not os.path.exists(out), (r.returncode, err)
    assert not [f for f in os.listdir(os.path.dirname(out)) if ".tmp." in f], "no temporary file is left"
    assert all(w in err for w in words), err
    assert len(err.strip().splitlines()) == 1, err
    return err


@pytest.mark.parametrize("how", ["file", "stdin"])
@pytest.mark.parametrize("name,text,line,words", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusal_names_the_line_and_the_field(name, text, line, words, how, tmp_path):
    o = str(tmp_path / "o.bam")
    if how == "file":
        p = str(tmp_path / "in.sam")
        open(p, "wb").write(text)
        r = _sort(p, o)
    else:
        r = _sort("-", o, stdin=text, STRL_SAM_CHUNK_KB=0.25)
    _refused(r, o, "status -6", words, *([f"SAM line {line}: "] if line is not None else ["SAM header"]))


def test_windowed_with_sam_is_refused(texts, tmp_path):
    o = str(tmp_path / "o.bam")
    for e in ({"STRL_SORT": "host"}, {"STRL_SORT": ""}):
        _refused(_sort(texts["one_line"][0], o, "--windowed", **e), o, "--windowed", "SAM")


def test_gzip_on_stdin_is_refused(tmp_path):
    o = str(tmp_path / "o.bam")
    _refused(_sort("-", o, stdin=bamio.bgzf_bytes(b"BAM\1" + bytes(8))), o, "a BAM on stdin is not read; write it to a file")
    _refused(_sort("-", o, stdin=b""), o, "stdin holds no SAM text")


def test_a_line_longer_than_8_mib_is_refused(tmp_path):
    o = str(tmp_path / "o.bam")
    text = C.HD3.encode() + (C.mk("a") + "\n").encode() + (C.mk("b", seq="A" * (5 << 20), qual="I" * (5 << 20)) + "\n").encode() + (C.mk("c") + "\n").encode()
    _refused(_sort("-", o, stdin=text), o, "SAM line 2: line: more than 8388608 bytes", "status -6")


# ---- round trip: a BAM printed as SAM sorts to the bytes the BAM sorts to ---------------------------------------------------------------
def _mask_bins(raw):
    """bamio.write_bam gives every record bin 4680; the rule computes reg2bin(pos, end).  The two agree only for pos = -1, so the
    round trip is compared with the bin field of every record zeroed"""
    text, refs_bytes, n_ref, recs = S.split_stream(raw)
    head = len(raw) - sum(len(r) for r in recs)
    out = bytearray(raw)
    at = head
    for r in recs:
        out[at + 14:at + 16] = b"\0\0"
        at += len(r)
    return bytes(out)


def _round_trip(bam, tmp_path):
    raw = gzip.decompress(open(bam, "rb").read())
    sam = str(tmp_path / "rt.sam")
    open(sam, "wb").write(C.bam_to_sam(raw))
    a, b = str(tmp_path / "from_bam.bam"), str(tmp_path / "from_sam.bam")
    ra = subprocess.run([CLI, "sort", "-o", a, bam], capture_output=True, env=dict(os.environ, STRL_SORT="host"))
    rb = _sort(sam, b)
    assert ra.returncode == 0 and rb.returncode == 0, (ra.stderr, rb.stderr)
    sa, sb = gzip.decompress(open(a, "rb").read()), gzip.decompress(open(b, "rb").read())
    assert _mask_bins(sa) == _mask_bins(sb)
    return sb


# (header_empty_text is a BAM whose references stand in the binary list alone: without @SQ lines it has no spelling as SAM text)
@pytest.mark.parametrize("name", [n for n, _, _ in S.cases() if n != "header_empty_text"])
def test_round_trip_of_the_bam_cases(name, tmp_path):
    rec, text = {n: (r, t) for n, r, t in S.cases()}[name]
    bam = str(tmp_path / "in.bam")
    S.write_case(bam, rec, text)
    _round_trip(bam, tmp_path)


def test_round_trip_with_qualities_and_tags(tmp_path):
    tid, pos, flag = S._shuffled(500, 3, 77)
    rec = S.batch(tid, pos, flag, S.targets(3), seed=77)
    rng = np.random.default_rng(3)
    quals = [bytes(int(x) for x in rng.integers(0, 60, int(rec.l_seq[i]))) for i in range(rec.n)]
    extra = [b"NMC" + bytes([i % 200]) + b"XSs" + struct.pack("<h", -300 - i) + b"MDZ" + b"10A5\0" + b"XFf" + struct.pack("<f", i / 7) + b"XAAq" +
             b"XBBS" + struct.pack("<i3H", 3, 256, 1, 65535) + b"XHH1A\0" + b"XII" + struct.pack("<I", 70000 + i) for i in range(rec.n)]
    bam = str(tmp_path / "in.bam")
    bamio.write_bam(bam, rec, index=False, quals=quals, extra=extra)
    sb = _round_trip(bam, tmp_path)
    assert b"XFf" in sb and b"MDZ10A5" in sb


# ---- the rule as a stand-alone program under the sanitizers -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def core_main():
    out = os.path.join(HERE, "emu", "sam_core_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "sam_core_main")
    src = os.path.join(HERE, "emu", "sam_core_main.cpp")
    csrc = os.path.join(HERE, "..", "strling_amd", "csrc")
    deps = [src] + [os.path.join(csrc, f) for f in ("sam_core.h", "bamindex_core.h", "bamsort_core.h", "bam_rec.h")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(f) for f in deps):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, src])
    return exe


def test_standalone_program_under_asan_and_ubsan(core_main):
    r = subprocess.run([core_main], capture_output=True, text=True)
    assert r.returncode == 0 and "all cases passed" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


@pytest.mark.parametrize("name", NAMES)
def test_standalone_program_encodes_the_cases(core_main, name, texts, refs, tmp_path):
    """header function and encoder over the same case files, every record in a buffer exact to the byte"""
    out = str(tmp_path / "out.stream")
    r = subprocess.run([core_main, texts[name][0], out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    header = C.split_text(texts[name][1])[0]
    assert open(out, "rb").read() == C.bam_header(header) + b"".join(refs[name][4])


@pytest.mark.parametrize("name,text,line,words", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_standalone_program_refuses(core_main, name, text, line, words, tmp_path):
    p = str(tmp_path / "in.sam")
    open(p, "wb").write(text)
    r = subprocess.run([core_main, p, str(tmp_path / "o")], capture_output=True, text=True)
    assert r.returncode == 1 and words in r.stderr and (line is None or f"SAM line {line}: " in r.stderr), r.stderr[-3000:]
