"""`strling sort` over SAM text on the GPU (strling_amd/csrc/samparse.hip): every case of tests/sam_cases.py byte for byte against
the host path's file -- again with chunks of one to three lines, chunks that end exactly on a newline, several arena slabs, pieces
of one BGZF block and every lanes-per-line setting the kernels are instantiated for --, the device compressor's members against the
twin's, the index against the host path's and `strling bamindex`'s, the refusals in the host path's words, and the context after
a refusal."""
import json
import os
import subprocess

import numpy as np
import pytest

import sam_cases as C
import sort_bam_cases as S
from strling_amd import api, build

pytestmark = pytest.mark.gpu
CLI = build.CLI
CASES = C.cases()
NAMES = [n for n, _ in CASES]
REFUSALS = C.refusals()


def _sort(src, out, *opts, stdin=None, **env):
    e = dict(os.environ)
    e.pop("STRL_SORT", None)
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
def host_files(texts, tmp_path_factory):
    """the STRL_SORT=host file of every case, --deflate=host"""
    d = tmp_path_factory.mktemp("sorted_host")
    out = {}
    for name, (p, _) in texts.items():
        o = os.path.join(str(d), name + ".bam")
        r = _sort(p, o, STRL_SORT="host")
        assert r.returncode == 0, (name, r.stderr)
        out[name] = open(o, "rb").read()
    return out


def _line_kb(text, lines_per_chunk):
    """STRL_SAM_CHUNK_KB under which a chunk takes `lines_per_chunk` of the case's longest lines at most, and one at least"""
    longest = max([len(l) + 2 for l in C.split_text(text)[1]] + [32])
    return max(1, lines_per_chunk * longest) / 1024.0 if lines_per_chunk > 1 else 1 / 1024.0


def _settings(text):
    body = text[len(C.split_text(text)[0]):]
    # a chunk size that is exactly where a line ends (the third line's end where there are three, else the first's)
    ends = [i + 1 for i, c in enumerate(body) if c == 10]
    exact = ends[min(2, len(ends) - 1)] if ends else 64
    return {"defaults": {},
            "one_line_chunks": dict(STRL_SAM_CHUNK_KB=1 / 1024.0),                        # every chunk is one line
            "few_line_chunks_slabs_pieces": dict(STRL_SAM_CHUNK_KB=_line_kb(text, 3), STRL_SORT_SLAB_MB=0.004 if len(body) < 100_000 else 0.15, STRL_SORT_PIECE_KB=1),
            "chunk_ends_on_a_newline": dict(STRL_SAM_CHUNK_KB=exact / 1024.0),
            "lanes_32": dict(STRL_SORT_SAM_LANES=32, STRL_SAM_CHUNK_KB=8),
            "lanes_64": dict(STRL_SORT_SAM_LANES=64)}


SETTING_NAMES = ["defaults", "one_line_chunks", "few_line_chunks_slabs_pieces", "chunk_ends_on_a_newline", "lanes_32", "lanes_64"]


@pytest.mark.parametrize("setting", SETTING_NAMES)
@pytest.mark.parametrize("name", NAMES)
def test_device_file_is_the_host_file(name, setting, texts, host_files, tmp_path):
    p, text = texts[name]
    env = _settings(text)[setting]
    o = str(tmp_path / "dev.bam")
    if name == "shuffle_3000" and setting == "one_line_chunks":
        env = dict(STRL_SAM_CHUNK_KB=2)            # (3000 chunks of a line each say nothing more than the smaller cases' do)
    r = _sort(p, o, "-v", **env) if setting != "lanes_64" else _sort("-", o, "-v", stdin=text, **env)
    assert r.returncode == 0, r.stderr
    info = _info(r)
    n = len(C.split_text(text)[1])
    assert info["path"] == "device" and info["input"] == "sam" and info["records"] == n == info["lines"]
    assert open(o, "rb").read() == host_files[name]
    if setting == "few_line_chunks_slabs_pieces" and name in ("shuffle_3000", "refs_256"):
        assert info["slabs"] >= 3, info
    if name == "f_all_host":
        assert info["host_finished"] == n
    if name == "f_edges":
        assert 0 < info["host_finished"] == len(C.F_HOST)
    if name in ("shuffle_3000", "i_tags", "lines_64"):
        assert info["host_finished"] == 0


@pytest.mark.parametrize("name", ["shuffle_3000", "line_400kb", "one_line", "header_only"])
def test_deflate_device_members_are_the_twin_s(name, texts, tmp_path):
    o = str(tmp_path / "core.bam")
    r = _sort(texts[name][0], o, "--deflate=device", "-v", STRL_SORT_PIECE_KB=64)
    assert r.returncode == 0, r.stderr
    assert _info(r)["deflate"] == "device"
    stream = C.reference(texts[name][1])[0]
    data = S.check_file(o, stream)
    twin, _, _ = api.bgzf_deflate_host(stream)
    assert data == twin + S.EOF_BLOCK


@pytest.mark.parametrize("opts", [["--write-index"], ["--write-index", "--csi"]], ids=["bai", "csi"])
@pytest.mark.parametrize("name", ["shuffle_3000", "refs_256", "header_only"])
def test_write_index_is_the_host_path_s_and_bamindex_s(name, opts, texts, tmp_path):
    ext = ".csi" if "--csi" in opts else ".bai"
    o, h = str(tmp_path / "dev.bam"), str(tmp_path / "host.bam")
    r = _sort(texts[name][0], o, *opts, STRL_SAM_CHUNK_KB=16)
    assert r.returncode == 0, r.stderr
    rh = _sort(texts[name][0], h, *opts, STRL_SORT="host")
    assert rh.returncode == 0, rh.stderr
    assert open(o, "rb").read() == open(h, "rb").read()
    import gzip
    unz = (lambda b: gzip.decompress(b)) if ext == ".csi" else (lambda b: b)
    assert unz(open(o + ext, "rb").read()) == unz(open(h + ext, "rb").read())
    again = str(tmp_path / ("again" + ext))
    rb = subprocess.run([CLI, "bamindex", *(["--csi"] if ext == ".csi" else []), "-o", again, o], capture_output=True)
    assert rb.returncode == 0, rb.stderr
    assert unz(open(again, "rb").read()) == unz(open(o + ext, "rb").read())


def test_pull_reads_the_result(texts, tmp_path):
    o = str(tmp_path / "dev.bam")
    r = _sort(texts["shuffle_3000"][0], o, "--write-index")
    assert r.returncode == 0, r.stderr
    out = str(tmp_path / "pulled.bam")
    rp = subprocess.run([CLI, "pull", "-o", out, o, "t1:20000-40000"], capture_output=True)
    assert rp.returncode == 0, rp.stderr
    import gzip
    _, _, _, recs = S.split_stream(gzip.decompress(open(out, "rb").read()))
    want = [r for r in C.reference(texts["shuffle_3000"][1])[4] if r[4:8] == b"\1\0\0\0"]
    assert recs and all(r in want for r in recs)


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def _refused(r, out):
    err = r.stderr.decode()
    assert r.returncode == 1 and not os.path.exists(out), (r.returncode, err)
    assert not [f for f in os.listdir(os.path.dirname(out)) if ".tmp." in f], "no temporary file is left"
    assert len(err.strip().splitlines()) == 1, err
    return err


@pytest.mark.parametrize("name,text,line,words", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusal_is_the_host_path_s(name, text, line, words, tmp_path):
    p = str(tmp_path / "in.sam")
    open(p, "wb").write(text)
    o = str(tmp_path / "o.bam")
    host = _refused(_sort(p, o, STRL_SORT="host"), o)
    for env in ({}, dict(STRL_SAM_CHUNK_KB=0.1, STRL_SORT_SAM_LANES=64)):
        assert _refused(_sort(p, o, **env), o) == host
    assert words in host and (line is None or f"SAM line {line}: " in host)


def test_refusal_in_chunk_3_of_5_leaves_no_file(tmp_path):
    ok = C.mk("fine", 0, "t0", 5, cigar="4M", seq="ACGT", qual="IIII") + "\n"
    per = 20
    lines = [ok] * (5 * per)
    lines[2 * per + 7] = C.mk("bad", 0, "t0", 5, mapq=300) + "\n"
    lines[4 * per + 1] = C.mk("later", 0, "nowhere", 5) + "\n"
    text = (C.HD3 + "".join(lines)).encode()
    o = str(tmp_path / "o.bam")
    err = _refused(_sort("-", o, stdin=text, STRL_SAM_CHUNK_KB=per * len(ok) / 1024.0), o)
    assert f"SAM line {2 * per + 8}: MAPQ:" in err and "status -6" in err


def test_a_line_longer_than_8_mib_is_refused(tmp_path):
    o = str(tmp_path / "o.bam")
    text = C.HD3.encode() + (C.mk("a") + "\n").encode() + (C.mk("b", seq="A" * (5 << 20), qual="I" * (5 << 20)) + "\n").encode() + (C.mk("c") + "\n").encode()
    assert "SAM line 2: line: more than 8388608 bytes" in _refused(_sort("-", o, stdin=text), o)


# ---- the context ---------------------------------------------------------------------------------------------------------------------
def test_context_sorts_again_after_a_refusal(ctx, texts, tmp_path):
    name, text, line, words = next(r for r in REFUSALS if r[0] == "unknown_rname")
    with pytest.raises(api.StrlingError) as e:
        ctx.bamsort_sam(text, chunk_bytes=64)
    assert e.value.code == -6 and f"SAM line {line}: " in str(e.value) and words in str(e.value)
    stream, info, perm = ctx.bamsort_sam(texts["shuffle_3000"][1], chunk_bytes=50_000)
    ref = C.reference(texts["shuffle_3000"][1])
    assert stream == ref[0] and info["lines"] == info["n_records"] == 3000 and info["chunks"] > 10 and info["host_finished"] == 0
    keys = np.array([S.ref_key(r, 3) for r in ref[4]], np.uint64)
    assert np.array_equal(perm, np.argsort(keys, kind="stable").astype(np.uint32))
    bam = str(tmp_path / "b.bam")
    rec, htext = {n: (r, t) for n, r, t in S.cases()}["uniform_shuffle"]
    S.write_case(bam, rec, htext)
    got, _, _ = ctx.bamsort(bam)
    assert got == S.reference_stream(bam)[0]
    stream, info, _ = ctx.bamsort_sam(texts["f_edges"][1])
    assert stream == C.reference(texts["f_edges"][1])[0] and info["host_finished"] == len(C.F_HOST)


def test_push_of_a_chunk_without_a_final_newline_is_an_argument_error(ctx, texts):
    text = texts["lines_64"][1]
    raw, names, _ = api.sam_header(text)
    body = text[int.from_bytes(raw[4:8], "little"):]
    half = body.index(b"\n", len(body) // 2) + 1
    ctx.bamsort_sam_begin(names)
    try:
        ctx.bamsort_sam_reserve(len(body))
        with pytest.raises(api.StrlingError) as e:
            ctx.bamsort_push_sam(body[:half - 1])
        assert e.value.code == -3                                   # STRL_ERR_ARG, and the sort goes on
        ctx.bamsort_push_sam(body[:half])
        ctx.bamsort_push_sam(body[half:])
        info = ctx.bamsort_finish(api.bamsort_header(raw))
        assert ctx.bamsort_fetch(0, info["stream_bytes"]) == C.reference(text)[0]
    finally:
        ctx.bamsort_end()
