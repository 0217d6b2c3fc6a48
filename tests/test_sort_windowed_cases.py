"""`strling sort --windowed` on the CPU: the option on the host path (STRL_SORT=host holds the file in host memory anyway, so the
file and the index are the ones written without it), the rule of the windows (bsort_window_plan) against a model written out
here, and the scatter's rule and the completeness condition of strling_amd/csrc/bamsort_core.h as a stand-alone program under
the sanitizers (tests/emu/bamsort_window_main.cpp) over every case of tests/sort_bam_cases.py.
tests/test_sort_windowed_device.py runs the windows on the GPU."""
import gzip
import os
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


# ---- the option on the host path ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_windowed_on_the_host_path_writes_the_same_file(name, paths, refs, tmp_path):
    plain, win = str(tmp_path / "plain.bam"), str(tmp_path / "win.bam")
    r = _sort(paths[name], plain)
    assert r.returncode == 0, r.stderr
    r = _sort(paths[name], win, "--windowed", "-v")
    assert r.returncode == 0, r.stderr
    assert '"path": "host"' in r.stderr and '"windows": 0' in r.stderr and '"window_bytes": 0' in r.stderr
    assert open(win, "rb").read() == open(plain, "rb").read()
    S.check_file(win, refs[name][0])


@pytest.mark.parametrize("csi", [False, True])
def test_windowed_write_index_on_the_host_path(csi, paths, tmp_path):
    opts = ["--write-index"] + (["--csi"] if csi else [])
    ext = ".csi" if csi else ".bai"
    plain, win = str(tmp_path / "plain.bam"), str(tmp_path / "win.bam")
    for o, more in ((plain, []), (win, ["--windowed"])):
        r = _sort(paths["uniform_shuffle"], o, *opts, *more)
        assert r.returncode == 0 and os.path.exists(o + ext), r.stderr
    assert open(win, "rb").read() == open(plain, "rb").read()
    assert open(win + ext, "rb").read() == open(plain + ext, "rb").read()


def test_usage_names_the_option():
    r = subprocess.run([CLI, "sort"], capture_output=True, text=True)
    assert "--windowed" in r.stdout + r.stderr and "second read of the output" in r.stdout + r.stderr


# ---- the rule of the windows ---------------------------------------------------------------------------------------------------------
def _model(stream, limit, piece):
    w = max(piece, limit // piece * piece)
    return w, -(-stream // w)


@pytest.mark.parametrize("piece", [S.BLK, 3 * S.BLK, 2056 * S.BLK])
def test_window_plan_against_the_model(piece, window_main):
    limits = [0, 1, piece - 1, piece, piece + 1, 2 * piece - 1, 2 * piece, 5 * piece + piece // 2, 7 * piece + 1, (200 << 30) + 12345]
    for limit in limits:
        w = _model(0, limit, piece)[0]
        assert w % piece == 0 and w >= piece and (w <= limit or w == piece)
        for stream in (0, 1, w - 1, w, w + 1, 2**40 + 3):
            want = _model(stream, limit, piece)
            assert api.bamsort_window_plan(stream, limit, piece) == want, (stream, limit, piece)
            if limit in (0, piece - 1, 5 * piece + piece // 2):
                r = subprocess.run([window_main, "plan", str(stream), str(limit), str(piece)], capture_output=True, text=True)
                assert r.returncode == 0 and tuple(int(x) for x in r.stdout.split()) == want, (r.stdout, r.stderr[-2000:])
            # the windows tile the stream: every one starts on a multiple of the piece, only the last is short
            n = want[1]
            assert (n - 1) * w < stream <= n * w if stream else n == 0


# ---- the scatter's rule as a stand-alone program under the sanitizers ----------------------------------------------------------------
@pytest.fixture(scope="module")
def window_main():
    out = os.path.join(HERE, "emu", "bamsort_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "bamsort_window_main")
    src = os.path.join(HERE, "emu", "bamsort_window_main.cpp")
    core = os.path.join(HERE, "..", "strling_amd", "csrc", "bamsort_core.h")
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(f) for f in (src, core)):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, src])
    return exe


def _raw_and_stream(name, paths, refs, tmp_path):
    raw, stream = str(tmp_path / "in.raw"), str(tmp_path / "want.stream")
    open(raw, "wb").write(gzip.decompress(open(paths[name], "rb").read()))
    open(stream, "wb").write(refs[name][0])
    return raw, stream


@pytest.mark.parametrize("name", NAMES)
def test_standalone_scatter_fills_the_windows(window_main, name, paths, refs, tmp_path):
    """windows of 1 block, 3 blocks and the whole stream x chunks of 1, 2 and all records, every window buffer exact to the byte"""
    raw, stream = _raw_and_stream(name, paths, refs, tmp_path)
    r = subprocess.run([window_main, raw, stream], capture_output=True, text=True)
    assert r.returncode == 0 and "all windows equal" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


@pytest.mark.parametrize("name,k", [("uniform_shuffle", 1234), ("one_record", 0), ("one_300kb_record", 137), ("n2049", 2048)])
def test_standalone_completeness_trips_on_a_withheld_record(window_main, name, k, paths, refs, tmp_path):
    raw, stream = _raw_and_stream(name, paths, refs, tmp_path)
    r = subprocess.run([window_main, raw, stream, "withhold", str(k)], capture_output=True, text=True)
    assert r.returncode == 3 and "incomplete window" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


@pytest.mark.parametrize("name,k", [("uniform_shuffle", 1234), ("one_record", 0), ("one_300kb_record", 137), ("n2049", 0)])
def test_standalone_length_check_trips_on_an_altered_block_size(window_main, name, k, paths, refs, tmp_path):
    raw, stream = _raw_and_stream(name, paths, refs, tmp_path)
    r = subprocess.run([window_main, raw, stream, "alter", str(k)], capture_output=True, text=True)
    assert r.returncode == 4 and r.stdout.strip() == f"the input changed between passes: record {k}", r.stdout[-2000:] + r.stderr[-4000:]
