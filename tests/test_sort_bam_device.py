"""`strling sort` on the GPU (strling_amd/csrc/bamsort.hip): every case of tests/sort_bam_cases.py byte for byte against the host
path's file, again with records across chunk seams, several arena slabs and pieces of one BGZF block; the device compressor's
members against the twin's; the permutation against numpy's stable argsort; the layout and the piece search beyond 2^32
(strl_bamsort_probe); the arena's refusal; and the sorted file under `strling bamindex` and `strling pull`."""
import gzip
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import sort_bam_cases as S
from strling_amd import api, bamio, build
from strling_amd.records import RecordBatch

pytestmark = pytest.mark.gpu
CLI = build.CLI
NAMES = [name for name, _, _ in S.cases()]


def _sort(src, out, *opts, **env):
    e = dict(os.environ)
    e.pop("STRL_SORT", None)
    e.update({k: str(v) for k, v in env.items()})
    return subprocess.run([CLI, "sort", *opts, "-o", out, src], capture_output=True, text=True, env=e)


def _info(r):
    return json.loads(r.stderr.strip().splitlines()[-1])


@pytest.fixture(scope="module")
def paths(tmp_path_factory):
    return S.case_dir(tmp_path_factory)


@pytest.fixture(scope="module")
def host_files(paths, tmp_path_factory):
    """the STRL_SORT=host file of every case, --deflate=host"""
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


# chunk seams (records across pushes, the carry), arena slabs (0.15 MB: two one-block chunks share a slab, the rest of it is
# left; 0.25 MB: a three-block chunk has a slab of its own), pieces of one 0xFF00 block (they cut records, block_size words, the header)
SETTINGS = {"defaults": {},
            "chunk1_slabs_pieces": dict(STRL_CHUNK_BLOCKS=1, STRL_SORT_SLAB_MB=0.15, STRL_SORT_PIECE_KB=1),
            "chunk2_pieces": dict(STRL_CHUNK_BLOCKS=2, STRL_SORT_PIECE_KB=1),
            "chunk3_slabs": dict(STRL_CHUNK_BLOCKS=3, STRL_SORT_SLAB_MB=0.25)}


@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("name", NAMES)
def test_device_file_is_the_host_file(name, setting, paths, host_files, refs, tmp_path):
    o = str(tmp_path / "dev.bam")
    r = _sort(paths[name], o, "-v", **SETTINGS[setting])
    assert r.returncode == 0, r.stderr
    info = _info(r)
    stream, n, no_ref, in_order, _ = refs[name]
    assert info["path"] == "device" and info["records"] == n and info["no_reference"] == no_ref and info["stream_bytes"] == len(stream)
    assert info["already_sorted"] is in_order
    assert open(o, "rb").read() == host_files[name]
    if setting == "chunk1_slabs_pieces" and name in ("uniform_shuffle", "one_300kb_record"):
        assert info["slabs"] >= 3, info


@pytest.mark.parametrize("piece", [None, 1])
@pytest.mark.parametrize("name", ["uniform_shuffle", "one_300kb_record", "one_record", "no_record", "header_co_lines"])
def test_deflate_device_members_are_the_twin_s(name, piece, paths, refs, tmp_path):
    o = str(tmp_path / "core.bam")
    env = {} if piece is None else dict(STRL_SORT_PIECE_KB=piece, STRL_CHUNK_BLOCKS=2)
    r = _sort(paths[name], o, "--deflate=device", "-v", **env)
    assert r.returncode == 0, r.stderr
    assert _info(r)["deflate"] == "device"
    stream = refs[name][0]
    data = S.check_file(o, stream)                       # the inflated stream equals the reference (= the host run's)
    twin, _, _ = api.bgzf_deflate_host(stream)
    assert data == twin + S.EOF_BLOCK


@pytest.mark.parametrize("chunk_blocks", [16384, 1])
@pytest.mark.parametrize("name", NAMES)
def test_abi_stream_and_order(ctx, name, chunk_blocks, paths, refs):
    """the ABI through the Python mirror: the stream, the figures, and strl_bamsort_order against numpy's stable argsort"""
    stream, n, no_ref, in_order, _ = refs[name]
    got, info, perm = ctx.bamsort(paths[name], chunk_blocks=chunk_blocks)
    assert got == stream
    assert (info["n_records"], info["n_no_ref"], info["stream_bytes"], bool(info["already_sorted"])) == (n, no_ref, len(stream), in_order)
    text, _, n_ref, recs = S.split_stream(gzip.decompress(open(paths[name], "rb").read()))
    keys = np.array([S.ref_key(r, n_ref) for r in recs], np.uint64)
    assert np.array_equal(perm, np.argsort(keys, kind="stable").astype(np.uint32))


def test_fetches_at_any_offset_and_members_of_a_piece(ctx, paths, refs):
    """pieces that start and end inside the header, inside block_size words and inside records; fetch_bgzf of whole blocks"""
    stream = refs["uniform_shuffle"][0]
    got, info, _ = ctx.bamsort(paths["uniform_shuffle"], chunk_blocks=2, keep_open=True)
    try:
        assert got == stream
        hb = len(stream) - sum(len(r) for r in S.split_stream(stream)[3])
        for lo, hi in ((0, 1), (3, hb - 1), (hb - 2, hb + 2), (hb, hb + 4), (hb + 1, hb + 3), (hb + 17, hb + 100_001), (len(stream) - 1, len(stream)), (len(stream), len(stream)),
                       (S.BLK - 1, 2 * S.BLK + 1)):
            assert ctx.bamsort_fetch(lo, hi - lo) == stream[lo:hi], (lo, hi)
        members, stored = ctx.bamsort_fetch_bgzf(S.BLK, 2 * S.BLK)
        assert members == api.bgzf_deflate_host(stream[S.BLK:3 * S.BLK])[0]
        tail = len(stream) - 4 * S.BLK
        assert 0 < tail < S.BLK
        assert ctx.bamsort_fetch_bgzf(4 * S.BLK, tail)[0] == api.bgzf_deflate_host(stream[4 * S.BLK:])[0]
        for off, nbytes in ((len(stream), 1), (5, len(stream))):
            with pytest.raises(api.StrlingError) as e:
                ctx.bamsort_fetch(off, nbytes)
            assert e.value.code == -3
        with pytest.raises(api.StrlingError) as e:
            ctx.bamsort_fetch_bgzf(S.BLK + 1, 10)
        assert e.value.code == -3
        assert ctx.bamsort_info()["gather_ms"] > 0
    finally:
        ctx.bamsort_end()


def test_probe_layout_and_pieces_beyond_2p32(ctx):
    """offsets past 2^32 without 4 GB of data: the layout against numpy.cumsum, the piece search and the parts against a walk"""
    rng = np.random.default_rng(3)
    for n, base in ((37, 2**32 - 100), (1, 2**32 - 100), (2049, 2**32 - 100), (5000, 2**40 + 3), (0, 77)):
        lens = rng.integers(36, 700, n).astype(np.uint32)
        want = np.concatenate(([0], np.cumsum(lens, dtype=np.uint64))).astype(np.uint64) + np.uint64(base)
        end = int(want[-1])
        cuts = sorted({0, base - 1, base, base + 1, end - 1, end} | ({int(want[1]) - 1, int(want[1]), int(want[1]) + 1, int(want[n // 2]) + 2, int(want[n - 1])} if n else set()))
        for lo in cuts:
            for hi in cuts:
                if not (0 <= lo < hi <= end):
                    continue
                off, (a, b), parts = ctx.bamsort_probe(lens, base, lo, hi)
                assert np.array_equal(off, want)
                touch = [j for j in range(n) if int(want[j + 1]) > lo and int(want[j]) < hi]
                assert list(range(a, b)) == touch, (n, base, lo, hi)
                for j, (skip, dst, nb) in zip(touch, parts.tolist()):
                    s, e = max(lo, int(want[j])), min(hi, int(want[j + 1]))
                    assert (skip, dst, nb) == (s - int(want[j]), s - lo, e - s)


def _three_mb(path):
    n = 3000
    t, p, f = S._shuffled(n, 3, 41)
    S.write_case(path, S.batch(t, p, f, S.targets(3), l_seq=[650] * n, seed=41), None)


def test_arena_limit_refuses_and_the_context_goes_on(ctx, paths, refs, tmp_path):
    big = str(tmp_path / "big.bam")
    _three_mb(big)
    assert len(gzip.decompress(open(big, "rb").read())) > 3_000_000
    o = str(tmp_path / "o.bam")
    r = _sort(big, o, STRL_SORT_ARENA_MB=1, STRL_CHUNK_BLOCKS=4, STRL_SORT_SLAB_MB=0.5)
    assert r.returncode == 1 and not os.path.exists(o) and not [f for f in os.listdir(str(tmp_path)) if ".tmp." in f], r.stderr
    assert "status -10" in r.stderr and "arena holds" in r.stderr and "needs" in r.stderr and "sort this file with samtools, or on a device with more memory" in r.stderr
    assert len(r.stderr.strip().splitlines()) == 1
    # the same through the ABI, then a second and a third sort on the same context
    os.environ["STRL_SORT_SLAB_MB"] = "0.5"
    try:
        with pytest.raises(api.StrlingError) as e:
            ctx.bamsort(big, chunk_blocks=4, arena_limit_bytes=1 << 20)
        assert e.value.code == -10
        ctx.bamsort_end()                                   # (a second end after the error: nothing to do)
        got, info, _ = ctx.bamsort(big, chunk_blocks=4)
        assert got == S.reference_stream(big)[0] and info["n_slabs"] >= 3
    finally:
        del os.environ["STRL_SORT_SLAB_MB"]
    assert ctx.bamsort(paths["n2049"])[0] == refs["n2049"][0]


def test_a_refused_refid_names_the_record_and_the_context_goes_on(ctx, paths, refs, tmp_path):
    raw = bytearray(gzip.decompress(open(paths["n2047"], "rb").read()))
    _, _, n_ref, recs = S.split_stream(bytes(raw))
    at = len(raw) - sum(len(r) for r in recs) + sum(len(r) for r in recs[:1234])
    struct.pack_into("<i", raw, at + 4, n_ref)
    p = str(tmp_path / "tid.bam")
    open(p, "wb").write(bamio.bgzf_bytes(bytes(raw)))
    o = str(tmp_path / "o.bam")
    r = _sort(p, o, STRL_CHUNK_BLOCKS=1)
    assert r.returncode == 1 and not os.path.exists(o) and "record 1234" in r.stderr and "status -6" in r.stderr, r.stderr
    with pytest.raises(api.StrlingError) as e:
        ctx.bamsort(p)
    assert e.value.code == -6 and "record 1234" in str(e.value)
    assert ctx.bamsort(paths["one_record"])[0] == refs["one_record"][0]


def test_refusals_on_the_device_path(paths, tmp_path):
    data = open(paths["uniform_shuffle"], "rb").read()
    o = str(tmp_path / "o.bam")
    p = str(tmp_path / "cut.bam")
    open(p, "wb").write(data[:len(data) * 2 // 3])
    r = _sort(p, o)
    assert r.returncode == 1 and not os.path.exists(o) and "status" in r.stderr and len(r.stderr.strip().splitlines()) == 1, r.stderr
    raw = gzip.decompress(data)
    open(p, "wb").write(bamio.bgzf_bytes(raw[:-5]))
    r = _sort(p, o)
    assert r.returncode == 1 and not os.path.exists(o) and "ends inside a record" in r.stderr, r.stderr
    bad = bytearray(data)
    bad[len(data) // 2] ^= 0x55
    open(p, "wb").write(bytes(bad))
    r = _sort(p, o)
    assert r.returncode == 1 and not os.path.exists(o) and not [f for f in os.listdir(str(tmp_path)) if ".tmp." in f], r.stderr


def test_bamindex_and_pull_accept_the_sorted_file(tmp_path):
    """the sorted file under the project's own readers: `strling bamindex` indexes it, and `strling pull` of a region gives the
    records it gives from a file bamio wrote in order"""
    rng = np.random.default_rng(9)
    n = 2500
    tg = S.targets(3)
    tid, pos, flag = S._shuffled(n, 3, 9, span=50_000)
    seqs = ["".join("ACGT"[c] for c in rng.integers(0, 4, 50)) for _ in range(n)]
    names = [f"q{i:05d}" for i in range(n)]

    def make(order):
        return RecordBatch.from_fields(tid[order], pos[order], tid[order], pos[order], flag[order], [30] * n, ["50M"] * n, [seqs[i] for i in order],
                                       [names[i] for i in order], isize=[0] * n, targets=tg)
    keys = (tid.astype(np.int64) << 33) | ((pos.astype(np.int64) + 1) << 1) | (flag >> 4 & 1)
    order = np.argsort(keys, kind="stable")
    shuffled, in_order = str(tmp_path / "in.bam"), str(tmp_path / "ref.bam")
    bamio.write_bam(shuffled, make(np.arange(n)), index=False, header_text=bamio.sam_header(tg, "unsorted"))
    bamio.write_bam(in_order, make(order), index=True)
    mine = str(tmp_path / "mine.bam")
    r = _sort(shuffled, mine)
    assert r.returncode == 0, r.stderr
    assert subprocess.run([CLI, "bamindex", shuffled], capture_output=True, text=True).returncode == 1, "the input is refused: not coordinate sorted"
    r = subprocess.run([CLI, "bamindex", mine], capture_output=True, text=True)
    assert r.returncode == 0 and os.path.exists(mine + ".bai"), r.stderr
    got = []
    for src in (mine, in_order):
        o = str(tmp_path / "pulled.bam")
        r = subprocess.run([CLI, "pull", "-o", o, src, "t1:10000-30000"], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        got.append(S.split_stream(gzip.decompress(open(o, "rb").read()))[3])
    assert len(got[0]) > 300 and got[0] == got[1]
