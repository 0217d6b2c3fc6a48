"""`strling sort` on the CPU: every case of tests/sort_bam_cases.py through the host path (STRL_SORT=host) -- the header rule, the
records and their order against Python's stable sorted(), the members and the EOF block --, the library's host entries
(api.bamsort_key / bamsort_header), the refusals, and the rule as a stand-alone program under the sanitizers
(tests/emu/bamsort_core_main.cpp).  tests/test_sort_bam_device.py runs the same cases on the GPU and compares byte for byte."""
import gzip
import json
import os
import struct
import subprocess

import pytest

import sort_bam_cases as S
from strling_amd import api, build

HERE = os.path.dirname(os.path.abspath(__file__))
CLI = build.CLI
NAMES = [name for name, _, _ in S.cases()]


def _sort(src, out, *opts, **env):
    e = dict(os.environ, STRL_SORT="host")
    e.update({k: str(v) for k, v in env.items()})
    return subprocess.run([CLI, "sort", *opts, "-o", out, src], capture_output=True, text=True, env=e)


@pytest.fixture(scope="module")
def paths(tmp_path_factory):
    return S.case_dir(tmp_path_factory)


@pytest.fixture(scope="module")
def refs(paths):
    return {name: S.reference_stream(p) for name, p in paths.items()}


@pytest.fixture(scope="module")
def sorted_files(paths, tmp_path_factory):
    """every case sorted once on the host, with -v"""
    d = tmp_path_factory.mktemp("sorted_host")
    out = {}
    for name, p in paths.items():
        o = os.path.join(str(d), name + ".sorted.bam")
        r = _sort(p, o, "-v")
        assert r.returncode == 0, (name, r.stderr)
        out[name] = (o, json.loads(r.stderr.strip().splitlines()[-1]))
    return out


@pytest.mark.parametrize("name", NAMES)
def test_host_sort_equals_the_reference(name, refs, sorted_files):
    stream, n, no_ref, in_order, _ = refs[name]
    path, info = sorted_files[name]
    S.check_file(path, stream)             # members of 0xFF00 bytes, each valid alone and at most 64 KiB, the EOF block, the bytes
    assert info["path"] == "host" and info["records"] == n and info["no_reference"] == no_ref and info["stream_bytes"] == len(stream)
    assert info["already_sorted"] is in_order and info["deflate"] == "zlib"
    assert not [f for f in os.listdir(os.path.dirname(path)) if ".tmp." in f], "the temporary name is gone"


def test_the_cases_reach_what_they_were_made_for(refs, paths):
    assert refs["already_sorted"][3] and not refs["reverse_sorted"][3] and not refs["uniform_shuffle"][3]
    assert refs["no_record"][1] == 0 and refs["one_record"][1] == 1 and refs["no_reference_scattered"][2] == 225
    text, _, n_ref, recs = S.split_stream(refs["one_position_both_strands"][0])
    at = [(struct.unpack_from("<ii", r, 4), struct.unpack_from("<H", r, 18)[0] & 16, r[36:36 + 7]) for r in recs]
    same = [a for a in at if a[0] == (1, 777)]
    assert len(same) > 500
    fwd = [a[2] for a in same if not a[1]]
    rev = [a[2] for a in same if a[1]]
    assert len(fwd) > 100 and len(rev) > 100 and [a[2] for a in same] == fwd + rev, "forward before reverse"
    assert fwd == sorted(fwd) and rev == sorted(rev), "input order (the names count up) inside a strand"
    _, _, _, recs = S.split_stream(refs["no_reference_scattered"][0])
    tail = [r for r in recs if struct.unpack_from("<i", r, 4)[0] < 0]
    assert recs[-len(tail):] == tail and [r[36:43] for r in tail] == sorted(r[36:43] for r in tail)
    _, _, _, recs = S.split_stream(refs["placed_unmapped_and_pos_minus1"][0])
    pos0 = [struct.unpack_from("<i", r, 8)[0] for r in recs if struct.unpack_from("<i", r, 4)[0] == 0]
    assert pos0[0] == -1 and pos0 == sorted(pos0), "pos -1 first within its reference"
    assert max(len(r) for r in S.split_stream(refs["one_300kb_record"][0])[3]) > 300_000
    for name, want in (("header_hd_unsorted_go", "@HD\tVN:1.5\tSO:coordinate\n@SQ"), ("header_hd_without_so", "@HD\tVN:1.6\tSO:coordinate\n@SQ"),
                       ("header_hd_ss_and_other_fields", "@HD\tVN:1.6\tXY:kept\tSO:coordinate\n@SQ"), ("header_no_hd", "@HD\tVN:1.6\tSO:coordinate\n@SQ"),
                       ("header_empty_text", "@HD\tVN:1.6\tSO:coordinate\n")):
        assert S.split_stream(refs[name][0])[0].startswith(want), name
    co = S.split_stream(refs["header_co_lines"][0])[0]
    assert co.startswith("@HD\tVN:1.6\tSO:coordinate\n") and co.endswith("@CO\tSO:unsorted is only a comment here\n@CO\t@HD\tGO:query\n")


@pytest.mark.parametrize("name", ["uniform_shuffle", "one_300kb_record", "header_co_lines", "no_record", "n2049"])
def test_pieces_of_one_block_write_the_same_file(name, paths, sorted_files, tmp_path):
    """pieces cut records, block_size words and the header; the cuts of the members do not move"""
    o = str(tmp_path / "p.bam")
    r = _sort(paths[name], o, STRL_SORT_PIECE_KB=1)
    assert r.returncode == 0, r.stderr
    assert open(o, "rb").read() == open(sorted_files[name][0], "rb").read()


def test_deflate_device_without_a_device_is_the_twin(paths, refs, tmp_path):
    o = str(tmp_path / "core.bam")
    r = _sort(paths["uniform_shuffle"], o, "--deflate=device", "-v")
    assert r.returncode == 0, r.stderr
    assert json.loads(r.stderr.strip().splitlines()[-1])["deflate"] == "core-host"
    stream = refs["uniform_shuffle"][0]
    data = S.check_file(o, stream)
    twin, _, _ = api.bgzf_deflate_host(stream)
    assert data == twin + S.EOF_BLOCK


def test_sorting_the_output_again_changes_nothing(sorted_files, tmp_path):
    src, _ = sorted_files["uniform_shuffle"]
    o = str(tmp_path / "again.bam")
    r = _sort(src, o, "-v")
    assert r.returncode == 0 and json.loads(r.stderr.strip().splitlines()[-1])["already_sorted"] is True
    assert open(o, "rb").read() == open(src, "rb").read()


# ---- the rule through the library ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["uniform_shuffle", "n_ref_0", "n_ref_256", "pos_2p31_minus_2", "placed_unmapped_and_pos_minus1"])
def test_library_key_and_header(name, paths):
    raw = gzip.decompress(open(paths[name], "rb").read())
    text, refs_bytes, n_ref, recs = S.split_stream(raw)
    for r in recs[:400]:
        assert api.bamsort_key(r[4:24], n_ref) == S.ref_key(r, n_ref)
    assert api.bamsort_key_bits(n_ref) == 33 + n_ref.bit_length()
    t = S.ref_header_text(text).encode()
    assert api.bamsort_header(raw) == b"BAM\1" + struct.pack("<i", len(t)) + t + refs_bytes


def test_library_refuses_a_refid_outside_the_header():
    body = struct.pack("<iiBBHHHi", 3, 0, 2, 0, 0, 0, 0, 0)
    with pytest.raises(api.StrlingError) as e:
        api.bamsort_key(body, 3)
    assert e.value.code == -6                                   # STRL_ERR_FORMAT
    with pytest.raises(api.StrlingError):
        api.bamsort_key(struct.pack("<iiBBHHHi", -2, 0, 2, 0, 0, 0, 0, 0), 3)
    with pytest.raises(api.StrlingError):
        api.bamsort_header(b"BAM\1\xff\0\0\0abc")


# ---- refusals: one line, exit 1, nothing written ---------------------------------------------------------------------------------------
def _refused(r, out, *words):
    assert r.returncode == 1 and not os.path.exists(out), (r.returncode, r.stderr)
    assert not [f for f in os.listdir(os.path.dirname(out)) if ".tmp." in f], "no temporary file is left"
    assert all(w in r.stderr for w in words), r.stderr
    return r.stderr


def test_refuses_a_cram(tmp_path):
    p = str(tmp_path / "x.cram")
    open(p, "wb").write(b"CRAM\3\0" + bytes(64))
    err = _refused(_sort(p, str(tmp_path / "o.bam")), str(tmp_path / "o.bam"), "is a CRAM")
    assert len(err.strip().splitlines()) == 1


def test_refuses_a_truncated_file(paths, tmp_path):
    data = open(paths["uniform_shuffle"], "rb").read()
    for cut, what in ((len(data) * 2 // 3, "mid-block"), (len(data) - 28 - 1, "the last byte of the last data block")):
        p = str(tmp_path / "cut.bam")
        open(p, "wb").write(data[:cut])
        err = _refused(_sort(p, str(tmp_path / "o.bam")), str(tmp_path / "o.bam"), "status")
        assert len(err.strip().splitlines()) == 1, what


def test_refuses_a_file_that_ends_inside_a_record(paths, tmp_path):
    raw = gzip.decompress(open(paths["n2047"], "rb").read())
    from strling_amd import bamio
    p = str(tmp_path / "inside.bam")
    open(p, "wb").write(bamio.bgzf_bytes(raw[:-5]))
    _refused(_sort(p, str(tmp_path / "o.bam")), str(tmp_path / "o.bam"), "status")


def test_refuses_a_refid_outside_the_header(paths, tmp_path):
    raw = bytearray(gzip.decompress(open(paths["n2047"], "rb").read()))
    text, refs_bytes, n_ref, recs = S.split_stream(bytes(raw))
    at = len(raw) - sum(len(r) for r in recs) + sum(len(r) for r in recs[:1234])
    struct.pack_into("<i", raw, at + 4, n_ref)
    from strling_amd import bamio
    p = str(tmp_path / "tid.bam")
    open(p, "wb").write(bamio.bgzf_bytes(bytes(raw)))
    _refused(_sort(p, str(tmp_path / "o.bam")), str(tmp_path / "o.bam"), "record 1234", "refID", "status -6")


def test_missing_output_option_and_file(paths, tmp_path):
    r = subprocess.run([CLI, "sort", paths["one_record"]], capture_output=True, text=True, env=dict(os.environ, STRL_SORT="host"))
    assert r.returncode == 1 and "-o OUT.bam is required" in r.stderr
    _refused(_sort(str(tmp_path / "absent.bam"), str(tmp_path / "o.bam")), str(tmp_path / "o.bam"), "couldn't open bam")
    r = _sort(paths["one_record"], str(tmp_path / "o.bam"), "--deflate=fast")
    assert r.returncode == 1 and not os.path.exists(str(tmp_path / "o.bam"))


def test_a_failed_run_leaves_an_older_output_alone(paths, tmp_path):
    o = str(tmp_path / "o.bam")
    open(o, "wb").write(b"older")
    p = str(tmp_path / "cut.bam")
    open(p, "wb").write(open(paths["uniform_shuffle"], "rb").read()[:5000])
    r = _sort(p, o)
    assert r.returncode == 1 and open(o, "rb").read() == b"older"
    assert not [f for f in os.listdir(str(tmp_path)) if ".tmp." in f]


# ---- the rule as a stand-alone program under the sanitizers --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def core_main():
    out = os.path.join(HERE, "emu", "bamsort_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "bamsort_core_main")
    src = os.path.join(HERE, "emu", "bamsort_core_main.cpp")
    core = os.path.join(HERE, "..", "strling_amd", "csrc", "bamsort_core.h")
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(f) for f in (src, core)):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, src])
    return exe


def test_standalone_program_under_asan_and_ubsan(core_main):
    r = subprocess.run([core_main], capture_output=True, text=True)
    assert r.returncode == 0 and "all cases passed" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


@pytest.mark.parametrize("name", NAMES)
def test_standalone_program_sorts_the_cases(core_main, name, paths, refs, tmp_path):
    """header function, key and piece arithmetic over the same cases: pieces of 1000 bytes in buffers exact to the byte"""
    raw = str(tmp_path / "in.raw")
    open(raw, "wb").write(gzip.decompress(open(paths[name], "rb").read()))
    out = str(tmp_path / "out.stream")
    r = subprocess.run([core_main, raw, out, "1000"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    assert open(out, "rb").read() == refs[name][0]
