"""`strling sort --windowed` on the GPU (strling_amd/csrc/bamsort.hip: bsort_dest_kernel, bsort_scatter_kernel, strl_bamsort_window_*):
every case of tests/sort_bam_cases.py, and the header longer than a member of tests/sort_index_cases.py, byte for byte against the
host path's file with windows of one block, of three blocks and of the whole stream; the file the resident sort refuses; the
device compressor's members; the index behind the rename against `strling bamindex`'s bytes; the ABI through the Python mirror; an
input that changes between the passes; and dest[] and the scatter's parts beyond 2^32 (strl_bamsort_window_probe)."""
import gzip
import json
import os
import subprocess

import numpy as np
import pytest

import sort_bam_cases as S
import sort_index_cases as X
from strling_amd import api, build

pytestmark = pytest.mark.gpu
CLI = build.CLI
NAMES = [name for name, _, _ in S.cases()] + ["header_longer_than_a_member"]


def _run(args, **env):
    e = dict(os.environ)
    e.pop("STRL_SORT", None)
    e.update({k: str(v) for k, v in env.items()})
    return subprocess.run([CLI] + args, capture_output=True, text=True, env=e)


def _sort(src, out, *opts, **env):
    return _run(["sort", *opts, "-o", out, src], **env)


def _info(r):
    return json.loads(r.stderr.strip().splitlines()[-1])


@pytest.fixture(scope="module")
def paths(tmp_path_factory):
    return {k: v for k, v in X.case_dir(tmp_path_factory).items() if k in NAMES}


@pytest.fixture(scope="module")
def host_files(paths, tmp_path_factory):
    """the STRL_SORT=host file of every case, --deflate=host, without --windowed"""
    d = tmp_path_factory.mktemp("sorted_host")
    out = {}
    for name, p in paths.items():
        o = os.path.join(str(d), name + ".bam")
        r = _sort(p, o, STRL_SORT="host")
        assert r.returncode == 0, (name, r.stderr)
        out[name] = open(o, "rb").read()
    return out


@pytest.fixture(scope="module")
def refs(paths):
    return {name: S.reference_stream(p) for name, p in paths.items()}


# windows of one 0xFF00 block: their edges cut records, block_size words and the header, the 300 KB record spans five, the long
# header fills windows that hold no record | three blocks, chunks of two | one window over the whole stream (the default piece)
SETTINGS = {"window1_piece1_chunk1": (dict(STRL_SORT_WINDOW_KB=1, STRL_SORT_PIECE_KB=1, STRL_CHUNK_BLOCKS=1), S.BLK),
            "window3_chunk2": (dict(STRL_SORT_WINDOW_KB=192, STRL_SORT_PIECE_KB=1, STRL_CHUNK_BLOCKS=2), 3 * S.BLK),
            "one_window": (dict(STRL_SORT_WINDOW_KB=1 << 20), (1 << 30) // (2056 * S.BLK) * 2056 * S.BLK)}


@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("name", NAMES)
def test_windowed_file_is_the_host_file(name, setting, paths, host_files, refs, tmp_path):
    env, W = SETTINGS[setting]
    o = str(tmp_path / "dev.bam")
    r = _sort(paths[name], o, "--windowed", "-v", **env)
    assert r.returncode == 0, r.stderr
    info = _info(r)
    stream, n, no_ref, in_order, _ = refs[name]
    assert info["path"] == "device" and info["records"] == n and info["no_reference"] == no_ref and info["stream_bytes"] == len(stream)
    assert info["already_sorted"] is in_order and info["slabs"] == 0
    assert info["window_bytes"] == W and info["windows"] == -(-len(stream) // W)
    assert open(o, "rb").read() == host_files[name]
    assert not [f for f in os.listdir(str(tmp_path)) if ".tmp." in f]
    if setting == "window1_piece1_chunk1":
        if name == "one_300kb_record":
            big = max(len(r) for r in S.split_stream(stream)[3])
            assert big > 4 * S.BLK and info["windows"] >= 6, "the long record spans five windows"
        if name == "header_longer_than_a_member":
            assert len(stream) - sum(len(r) for r in S.split_stream(stream)[3]) > S.BLK, "the first window holds no record"
    if setting == "one_window":
        assert info["windows"] == 1


def _three_mb(path):
    n = 3000
    t, p, f = S._shuffled(n, 3, 41)
    S.write_case(path, S.batch(t, p, f, S.targets(3), l_seq=[650] * n, seed=41), None)


def test_the_file_the_resident_sort_refuses(tmp_path):
    big = str(tmp_path / "big.bam")
    _three_mb(big)
    assert len(gzip.decompress(open(big, "rb").read())) > 3_000_000
    env = dict(STRL_SORT_ARENA_MB=1, STRL_CHUNK_BLOCKS=4, STRL_SORT_SLAB_MB=0.5)
    o, h = str(tmp_path / "o.bam"), str(tmp_path / "h.bam")
    r = _sort(big, o, **env)
    assert r.returncode == 1 and not os.path.exists(o) and "status -10" in r.stderr, r.stderr
    r = _sort(big, o, "--windowed", "-v", STRL_SORT_WINDOW_KB=1024, **env)
    assert r.returncode == 0, r.stderr
    info = _info(r)
    assert info["path"] == "device" and info["windows"] >= 3 and info["slabs"] == 0 and info["records"] == 3000
    assert _sort(big, h, STRL_SORT="host").returncode == 0
    assert open(o, "rb").read() == open(h, "rb").read()


@pytest.mark.parametrize("one_block", [True, False])
@pytest.mark.parametrize("name", ["uniform_shuffle", "one_300kb_record", "one_record", "no_record", "header_co_lines"])
def test_deflate_device_members_are_the_twin_s(name, one_block, paths, refs, tmp_path):
    o = str(tmp_path / "core.bam")
    env = dict(STRL_SORT_WINDOW_KB=1, STRL_SORT_PIECE_KB=1, STRL_CHUNK_BLOCKS=2) if one_block else dict(STRL_SORT_WINDOW_KB=1 << 20)
    r = _sort(paths[name], o, "--deflate=device", "--windowed", "-v", **env)
    assert r.returncode == 0, r.stderr
    info = _info(r)
    stream = refs[name][0]
    assert info["deflate"] == "device" and info["windows"] == (-(-len(stream) // S.BLK) if one_block else 1)
    data = S.check_file(o, stream)
    assert data == api.bgzf_deflate_host(stream)[0] + S.EOF_BLOCK


@pytest.mark.parametrize("csi", [False, True])
def test_write_index_is_bamindex_s_bytes(csi, paths, tmp_path):
    opts = ["--csi"] if csi else []
    ext = ".csi" if csi else ".bai"
    dev, ref2 = str(tmp_path / "dev.bam"), str(tmp_path / ("ref2" + ext))
    r = _sort(paths["uniform_shuffle"], dev, "--windowed", "--write-index", "-v", *opts, STRL_SORT_WINDOW_KB=192, STRL_SORT_PIECE_KB=1, STRL_CHUNK_BLOCKS=2)
    assert r.returncode == 0 and os.path.exists(dev + ext), r.stderr
    info = _info(r)
    assert info["windows"] >= 2 and info["index"] == ("csi" if csi else "bai") and info["index_bytes"] == os.path.getsize(dev + ext)
    b = _run(["bamindex", *opts, "-o", ref2, dev])
    assert b.returncode == 0, b.stderr
    assert open(dev + ext, "rb").read() == open(ref2, "rb").read()
    assert sorted(os.listdir(str(tmp_path))) == sorted(["dev.bam", "dev.bam" + ext, "ref2" + ext])


@pytest.mark.parametrize("csi", [False, True])
def test_a_refused_index_keeps_the_sorted_file(csi, paths, host_files, tmp_path):
    name = "placed_unmapped_and_pos_minus1"
    assert name in X.REFUSED
    dev = str(tmp_path / "dev.bam")
    r = _sort(paths[name], dev, "--windowed", "--write-index", *(["--csi"] if csi else []), STRL_SORT_WINDOW_KB=1, STRL_SORT_PIECE_KB=1)
    assert r.returncode == 1, r.stderr
    lines = r.stderr.strip().splitlines()
    assert len(lines) == 1 and "sorted file written; index refused: " in lines[0] and "record " in lines[0], r.stderr
    assert os.listdir(str(tmp_path)) == ["dev.bam"], "the sorted file is kept: no index, no temporary file"
    assert open(dev, "rb").read() == host_files[name]


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk_blocks", [16384, 1])
@pytest.mark.parametrize("name", NAMES)
def test_abi_windowed_stream(ctx, name, chunk_blocks, paths, refs):
    stream, n, no_ref, in_order, _ = refs[name]
    got, info = ctx.bamsort_windowed(paths[name], 2 * S.BLK, chunk_blocks=chunk_blocks)
    assert got == stream
    assert (info["n_records"], info["n_no_ref"], info["stream_bytes"], bool(info["already_sorted"]), info["n_slabs"], info["arena_bytes"]) == (n, no_ref, len(stream), in_order, 0, 0)
    assert info["window_bytes"] == 2 * S.BLK and info["windows"] == -(-len(stream) // (2 * S.BLK))


def test_abi_fetches_the_calls_it_refuses_and_the_next_sort(ctx, paths, refs):
    stream = refs["uniform_shuffle"][0]
    got, info = ctx.bamsort_windowed(paths["uniform_shuffle"], S.BLK, chunk_blocks=2, keep_open=True)
    try:
        assert got == stream and info["windows"] >= 4
        lo = (info["windows"] - 1) * S.BLK                     # the last window is the current one
        assert 0 < len(stream) - lo <= S.BLK
        for a, b in ((lo, len(stream)), (lo + 1, lo + 2), (lo + 17, len(stream) - 1), (len(stream), len(stream))):
            assert ctx.bamsort_fetch(a, b - a) == stream[a:b], (a, b)
        assert ctx.bamsort_fetch_bgzf(lo, len(stream) - lo)[0] == api.bgzf_deflate_host(stream[lo:])[0]
        for a, nbytes in ((0, 10), (lo - 1, 2), (lo - S.BLK, S.BLK), (lo, len(stream) - lo + 1)):
            with pytest.raises(api.StrlingError) as e:
                ctx.bamsort_fetch(a, nbytes)
            assert e.value.code == -3, (a, nbytes)
        with pytest.raises(api.StrlingError) as e:
            ctx.bamsort_fetch_bgzf(0, S.BLK)
        assert e.value.code == -3
        with pytest.raises(api.StrlingError) as e:
            ctx.bamsort_order(info["n_records"])
        assert e.value.code == -3 and "windowed" in str(e.value)
        with pytest.raises(api.StrlingError) as e:
            ctx.bamsort_index([0, 100], [1 << 20] * 3)
        assert e.value.code == -3 and "windowed" in str(e.value)
        assert ctx.bamsort_window_limit() > 0
        # an earlier window again: the passes may come in any order
        ctx.bamsort_window_begin(S.BLK, 2 * S.BLK)
        chunks = list(ctx._bam_chunks(ctx._bam_blocks(paths["uniform_shuffle"]), 3))      # (kept: the copies are asynchronous)
        for ch in chunks:
            ctx.bamsort_window_push(*ch)
        with pytest.raises(api.StrlingError) as e:
            ctx.bamsort_fetch(S.BLK, 10)                       # not before the window's end
        assert e.value.code == -3
        ctx.bamsort_window_end()
        assert ctx.bamsort_fetch(S.BLK, S.BLK) == stream[S.BLK:2 * S.BLK]
    finally:
        ctx.bamsort_end()
    with pytest.raises(api.StrlingError) as e:
        ctx.bamsort_window_limit()                             # no sort open
    assert e.value.code == -3
    assert ctx.bamsort(paths["n2049"])[0] == refs["n2049"][0]   # a resident sort on the same context


def _rec_lens(path):
    return [len(r) for r in S.split_stream(gzip.decompress(open(path, "rb").read()))[3]]


def test_a_changed_input_between_passes_is_refused(ctx, paths, refs, tmp_path):
    """pass 0 reads A, the windows' passes read B: A with record k's sequence two bases longer, and A without record k.  A refusal
    checked on the data: the lengths of pass 0 against the block_size words of the pass"""
    n, k = 1500, 777
    t, p, f = S._shuffled(n, 3, 77)
    ls = [int(x) for x in np.random.default_rng(77).integers(20, 60, n)]
    longer = list(ls)
    longer[k] += 2
    keep = [i for i in range(n) if i != k]
    A, B1, B2 = (str(tmp_path / x) for x in ("a.bam", "b1.bam", "b2.bam"))
    S.write_case(A, S.batch(t, p, f, S.targets(3), l_seq=ls, seed=77), None)
    S.write_case(B1, S.batch(t, p, f, S.targets(3), l_seq=longer, seed=77), None)
    S.write_case(B2, S.batch(t[keep], p[keep], f[keep], S.targets(3), l_seq=[ls[i] for i in keep], seed=77), None)
    la, l1, l2 = _rec_lens(A), _rec_lens(B1), _rec_lens(B2)
    assert [i for i in range(n) if la[i] != l1[i]] == [k] and len(l2) == n - 1
    first2 = next(i for i in range(n - 1) if la[i] != l2[i])
    assert first2 >= k
    for again, ordinal, window in ((B1, k, 2 * S.BLK), (B2, first2, 2 * S.BLK), (B1, k, 1 << 30), (B2, first2, 1 << 30)):
        with pytest.raises(api.StrlingError) as e:
            ctx.bamsort_windowed(A, window, chunk_blocks=1, again=again)
        assert e.value.code == -6 and f"the input changed between passes: record {ordinal}" in str(e.value), str(e.value)
    # a file with one record fewer whose lengths all agree: the count tells
    same = str(tmp_path / "same.bam")
    short = str(tmp_path / "short.bam")
    S.write_case(same, S.batch(t, p, f, S.targets(3), l_seq=[30] * n, seed=77), None)
    S.write_case(short, S.batch(t[:-1], p[:-1], f[:-1], S.targets(3), l_seq=[30] * (n - 1), seed=77), None)
    with pytest.raises(api.StrlingError) as e:
        ctx.bamsort_windowed(same, 1 << 30, again=short)
    assert e.value.code == -6 and "the input changed between passes" in str(e.value) and f"{n - 1} records" in str(e.value), str(e.value)
    with pytest.raises(api.StrlingError) as e:
        ctx.bamsort_windowed(short, 1 << 30, again=same)
    assert e.value.code == -6 and "the input changed between passes" in str(e.value), str(e.value)
    assert ctx.bamsort_windowed(A, 2 * S.BLK)[0] == S.reference_stream(A)[0]
    assert ctx.bamsort(paths["n2049"])[0] == refs["n2049"][0]


# ---- destinations beyond 2^32 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("base", [2**32 - 100, 2**40 + 3])
@pytest.mark.parametrize("n", [0, 1, 37, 2049, 5000])
def test_probe_dest_and_parts_beyond_2p32(ctx, n, base):
    """dest[] against numpy.cumsum of the lengths in sorted order, scattered through the permutation; the parts against a walk"""
    rng = np.random.default_rng(1000 + n)
    lens = rng.integers(36, 700, n).astype(np.uint32)
    perm = rng.permutation(n).astype(np.uint32)
    off = np.concatenate(([0], np.cumsum(lens[perm], dtype=np.int64))).astype(np.int64) + base
    want = np.zeros(n, np.int64)
    want[perm] = off[:n]
    end = int(off[-1])
    cuts = sorted({0, base - 1, base, base + 1, end - 1, end} | ({int(off[1]) - 1, int(off[1]), int(off[1]) + 1, int(off[n // 2]) + 2, int(off[n - 1])} if n else set()))
    for lo in cuts:
        for hi in cuts:
            if not (0 <= lo < hi <= end):
                continue
            dest, parts = ctx.bamsort_window_probe(lens, perm, base, lo, hi)
            assert np.array_equal(dest.astype(np.int64), want), (n, base)
            s, e = np.maximum(want, lo), np.minimum(want + lens, hi)
            inside = e > s
            assert np.array_equal(parts[:, 2].astype(np.int64), np.where(inside, e - s, 0)), (n, base, lo, hi)
            assert np.array_equal(parts[inside, 0].astype(np.int64), (s - want)[inside]) and np.array_equal(parts[inside, 1].astype(np.int64), (s - lo)[inside])
            assert int(parts[:, 2].sum()) == min(hi, end) - max(lo, base) if hi > base else not inside.any()
