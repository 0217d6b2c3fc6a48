"""`strling sort --markdup` on the CPU: every case of tests/markdup_cases.py through the host path (STRL_SORT=host) and through the
rule as a stand-alone program (tests/emu/markdup_core_main.cpp, also under the sanitizers) -- the flag word of every record, the
counts, and every other byte against plain sort's --, the library's host entry, the refusals and the index.
tests/test_markdup_device.py runs the same cases on the GPU and compares byte for byte."""
import gzip
import os
import struct
import subprocess

import pytest

import markdup_cases as M
import sort_bam_cases as S
from strling_amd import api, build

HERE = os.path.dirname(os.path.abspath(__file__))
CLI = build.CLI
NAMES = [name for name, _ in M.cases()]


def _sort(src, out, *opts, **env):
    e = dict(os.environ, STRL_SORT="host")
    e.update({k: str(v) for k, v in env.items()})
    return subprocess.run([CLI, "sort", *opts, "-o", out, src], capture_output=True, text=True, env=e)


@pytest.fixture(scope="module")
def paths(tmp_path_factory):
    return M.case_dir(tmp_path_factory)


@pytest.fixture(scope="module")
def refs(paths):
    return {name: M.reference(p) for name, p in paths.items()}


@pytest.fixture(scope="module")
def marked(paths, tmp_path_factory):
    """every case through the host path once"""
    d = tmp_path_factory.mktemp("markdup_host")
    out = {}
    for name, p in paths.items():
        o = os.path.join(str(d), name + ".bam")
        r = _sort(p, o, "--markdup")
        assert r.returncode == 0, (name, r.stderr)
        out[name] = (o, r.stderr)
    return out


@pytest.mark.parametrize("name", NAMES)
def test_host_path_equals_the_reference(name, refs, marked):
    stream, counts, _ = refs[name]
    path, err = marked[name]
    S.check_file(path, stream)             # every record's flag word, and every other byte as plain sort writes it
    assert M.counts_of(err) == counts
    assert len([l for l in err.splitlines() if "markdup:" in l]) == 1, "one line gives the counts"


def test_without_the_option_nothing_changes(paths, tmp_path):
    o = str(tmp_path / "plain.bam")
    r = _sort(paths["incoming_dup_cleared"], o)
    assert r.returncode == 0 and "markdup" not in r.stderr
    S.check_file(o, S.reference_stream(paths["incoming_dup_cleared"])[0])


def test_the_cases_reach_what_they_were_made_for(refs, paths):
    def dup(name):
        recs = S.split_stream(gzip.decompress(open(paths[name], "rb").read()))[3]
        return {(r[36:36 + r[12] - 1].decode(), struct.unpack_from("<H", r, 18)[0] & 0xc0): bool(f & 0x400) for r, f in zip(recs, refs[name][2])}
    d = dup("unclip_fr")
    assert d[("a", 0x40)] and d[("a", 0x80)] and not d[("b", 0x40)] and not d[("c", 0x40)] and not d[("d", 0x40)], "5S45M at 105 is 50M at 100"
    d = dup("reverse_clips")
    assert [d[(n, 0x80)] for n in "abcde"] == [True, True, False, False, True], "c has the best score of a, b, c, e; d ends elsewhere"
    d = dup("hard_and_soft")
    assert not d[("a", 0x40)] and d[("b", 0x40)] and d[("c", 0x40)]
    d = dup("u_negative")
    assert d[("a", 0x40)] and not d[("b", 0x40)] and d[("c", 0x40)] and not d[("d", 0x40)], "u = -8 three times, -7 once"
    d = dup("equal_signatures")
    assert d[("a", 0x40)] and not d[("b", 0x40)] and not d[("c", 0x40)]
    d = dup("two_references")
    assert d[("a", 0x40)] and d[("a", 0x80)] and not d[("b", 0x40)] and not d[("c", 0x40)]
    assert refs["other_strand"][1]["dup_pairs"] == 0
    d = dup("threshold_14_15")
    assert d[("a", 0x40)] and not d[("b", 0x40)] and d[("c", 0x40)], "15 counts, 14 does not"
    d = dup("quals_ff")
    assert d[("a", 0x40)] and not d[("b", 0x40)] and d[("c", 0x40)], "0xFF counts as 0"
    d = dup("score_ties")
    assert d[("a", 0x40)] and not d[("b", 0x40)] and d[("c", 0x40)], "the 0x40 record of b comes first"
    d = dup("fragment_at_pair_end")
    assert d[("f1", 0)] and d[("f2", 0)] and d[("f3", 0)] and not d[("f4", 0)] and not d[("a", 0x40)]
    d = dup("fragments_alone")
    assert [d[(f"f{k}", 0)] for k in range(1, 7)] == [True, False, True, True, False, True], "f2 before f3 by ordinal; f5 ends where f4 ends, with more bases"
    c = refs["mate_unmapped"][1]
    assert (c["pairs"], c["fragments"], c["dup_fragments"], c["ineligible"]) == (0, 4, 2, 2)
    c = refs["three_under_a_name"][1]
    assert (c["pairs"], c["dup_pairs"], c["fragments"], c["dup_fragments"]) == (2, 1, 3, 3)
    c = refs["two_first_reads"][1]
    assert (c["pairs"], c["dup_pairs"], c["fragments"], c["dup_fragments"]) == (2, 1, 2, 2)
    c = refs["ineligible_keep_their_words"][1]
    assert c["ineligible"] == 9 and c["pairs"] == 2 and c["dup_pairs"] == 1
    recs = S.split_stream(gzip.decompress(open(paths["ineligible_keep_their_words"], "rb").read()))[3]
    kept = [(struct.unpack_from("<H", r, 18)[0], f) for r, f in zip(recs, refs["ineligible_keep_their_words"][2]) if struct.unpack_from("<H", r, 18)[0] & 0xb04]
    assert len(kept) == 9 and all(a == b for a, b in kept) and sum(1 for a, _ in kept if a & 0x400) == 5
    d = dup("incoming_dup_cleared")
    assert not d[("a", 0x40)] and d[("b", 0x40)] and not d[("c", 0x40)] and not d[("f", 0)]
    for n in (2047, 2048, 2049):
        c = refs[f"pairs_{n}"][1]
        assert c["pairs"] == n and 0 < c["dup_pairs"] < n and c["fragments"] == 64 and 0 < c["dup_fragments"] < 64
    c = refs["copies_3000"][1]
    assert (c["pairs"], c["dup_pairs"]) == (3000, 2999)
    c = refs["one_name_512"][1]
    assert (c["pairs"], c["fragments"]) == (0, 512) and c["dup_fragments"] == 512 - 3
    assert refs["no_record"][1] == dict.fromkeys(M.COUNT_KEYS, 0)
    assert refs["no_eligible_record"][1] == dict(dict.fromkeys(M.COUNT_KEYS, 0), ineligible=40)


def test_windowed_with_markdup_is_refused(paths, tmp_path):
    o = str(tmp_path / "o.bam")
    r = _sort(paths["unclip_fr"], o, "--windowed", "--markdup")
    assert r.returncode == 1 and not os.path.exists(o) and not [f for f in os.listdir(str(tmp_path)) if ".tmp." in f]
    assert "the records are not resident; sort without --windowed or mark with samtools" in r.stderr


@pytest.mark.parametrize("csi", [False, True])
def test_write_index_gives_plain_sorts_index(csi, paths, tmp_path):
    """the index step does not look at 0x400: it is plain sort's index of the same records.  (An index names compressed offsets, and
    the members of a file with other flag bytes deflate to other sizes, so plain sort's index of the UNMARKED input differs in its
    virtual offsets; the file to compare with is plain sort's of the marked records, which is the marked file itself.)"""
    a, b = str(tmp_path / "a.bam"), str(tmp_path / "b.bam")
    opts = ["--write-index"] + (["--csi"] if csi else [])
    ra = _sort(paths["pairs_2049"], a, "--markdup", *opts)
    rb = _sort(a, b, *opts)
    assert ra.returncode == 0 and rb.returncode == 0, ra.stderr + rb.stderr
    ext = ".csi" if csi else ".bai"
    assert open(a, "rb").read() == open(b, "rb").read()
    assert open(a + ext, "rb").read() == open(b + ext, "rb").read()


def test_a_record_that_does_not_fit_its_block_size_is_refused(paths, tmp_path):
    p, o = str(tmp_path / "big.bam"), str(tmp_path / "o.bam")
    M.oversized(paths["unclip_fr"], p, 5)
    r = _sort(p, o, "--markdup")
    assert r.returncode == 1 and not os.path.exists(o) and not [f for f in os.listdir(str(tmp_path)) if ".tmp." in f]
    assert "record 5" in r.stderr and "block_size" in r.stderr and "status -6" in r.stderr, r.stderr
    assert _sort(p, o).returncode == 0, "plain sort does not look inside the record"


def test_sam_input_equals_bam_input(paths, refs, tmp_path):
    """the same records as SAM text: the same flags"""
    recs = dict(M.cases())["unclip_fr"]
    text = "@HD\tVN:1.6\tSO:unsorted\n" + "".join(f"@SQ\tSN:{n}\tLN:{l}\n" for n, l in M.TG)
    for r in recs:
        qual = "".join(chr(33 + q) for q in r["qual"])
        text += "\t".join([r["name"], str(r["flag"]), M.TG[r["tid"]][0], str(r["pos"] + 1), "30", r["cigar"], "=", str(r["pos"] + 1), "0", "A" * r["l_seq"], qual]) + "\n"
    p, o = str(tmp_path / "in.sam"), str(tmp_path / "o.bam")
    open(p, "w").write(text)
    r = _sort(p, o, "--markdup")
    assert r.returncode == 0, r.stderr
    assert M.counts_of(r.stderr) == refs["unclip_fr"][1]
    got = S.split_stream(b"".join(raw for _, raw in S.members(open(o, "rb").read())))[3]
    want = S.split_stream(refs["unclip_fr"][0])[3]
    assert [(g[36:36 + g[12]], struct.unpack_from("<H", g, 18)[0]) for g in got] == [(w[36:36 + w[12]], struct.unpack_from("<H", w, 18)[0]) for w in want]


# ---- the rule through the library ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["unclip_fr", "pairs_2049", "one_name_512", "no_record", "ineligible_keep_their_words"])
def test_library_host_entry(name, paths, refs):
    recs = S.split_stream(gzip.decompress(open(paths[name], "rb").read()))[3]
    flags, counts = api.markdup_host(b"".join(recs))
    assert [int(f) for f in flags] == refs[name][2]
    assert counts == {"n_" + k: v for k, v in refs[name][1].items()}


def test_library_host_entry_refuses_a_record_that_does_not_fit(paths):
    recs = S.split_stream(gzip.decompress(open(paths["unclip_fr"], "rb").read()))[3]
    bad = bytearray(recs[2])
    struct.pack_into("<H", bad, 16, 200)                        # 200 CIGAR operations in a record of 2
    with pytest.raises(api.StrlingError) as e:
        api.markdup_host(b"".join(recs[:2]) + bytes(bad) + b"".join(recs[3:]))
    assert e.value.code == -6 and "record 2" in str(e.value)


# ---- the rule as a stand-alone program, plain and under the sanitizers ---------------------------------------------------------------
def _program(sanitize):
    out = os.path.join(HERE, "emu", "markdup_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "markdup_core_main" + ("_san" if sanitize else ""))
    src = os.path.join(HERE, "emu", "markdup_core_main.cpp")
    core = os.path.join(HERE, "..", "strling_amd", "csrc", "markdup_core.h")
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(f) for f in (src, core)):
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
def test_standalone_program_marks_the_cases(core_main, name, paths, refs, tmp_path):
    raw, out = str(tmp_path / "in.raw"), str(tmp_path / "out.txt")
    open(raw, "wb").write(gzip.decompress(open(paths[name], "rb").read()))
    r = subprocess.run([core_main, raw, out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = open(out).read().split("\n")
    assert lines[0] == "counts " + " ".join(str(refs[name][1][k]) for k in M.COUNT_KEYS)
    assert [int(x) for x in lines[1:] if x] == refs[name][2]


def test_standalone_program_refuses_a_record_that_does_not_fit(core_main, paths, tmp_path):
    p = str(tmp_path / "big.bam")
    M.oversized(paths["unclip_fr"], p, 5)
    raw = str(tmp_path / "in.raw")
    open(raw, "wb").write(gzip.decompress(open(p, "rb").read()))
    r = subprocess.run([core_main, raw, str(tmp_path / "out.txt")], capture_output=True, text=True)
    assert r.returncode == 3 and "record 5" in r.stderr, r.stderr[-2000:]
