"""Every file of tests/scan_cases.py reaches the edge it is named for -- shown with the model alone, on any machine.
tests/test_scan_device.py feeds the same files to the kernels; a case that silently stopped exercising its edge (a decoy that
no longer passes for a record, a seam that moved) would leave that file green and meaningless, so it fails here instead.
Run with -s for one line of the model's counts per file and chunk size."""
import os
import subprocess
import zlib

import numpy as np
import pytest

import scan_cases as sc
from strling_amd import bamio, build, synth

SEG = sc.SEG
CLI = build.CLI


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    """every file once, and the model of it at every chunk size it is pushed with: {(case, label): path}, {(case, label, chunk_blocks): chunks}"""
    d = tmp_path_factory.mktemp("scan_cases")
    paths, models = {}, {}
    for name, label, cb in sc.files():
        if (name, label) not in paths:
            paths[name, label] = str(d / f"{name}_{label}.bam")
            sc.CASES[name]().write(paths[name, label], label)
        models[name, label, cb] = sc.scan_model(paths[name, label], cb)
        print(sc.model_line(name, label, cb, models[name, label, cb]))
    return paths, models


def _total(chunks, key):
    return sum(len(c[key]) for c in chunks)


def _of(models, name, label):
    return [(cb, m) for (n, l, cb), m in models.items() if (n, l) == (name, label)]


def test_every_control_is_clean_and_nothing_else_claims_to_be(built):
    _, models = built
    n = 0
    for (name, label, cb), m in models.items():
        v = sc.CASES[name]().variants[label]
        if v.control_of:
            assert all(c["clean"] for c in m), (name, label, cb)
            assert sum(c["n_records"] for c in m) == sc.CASES[name]().rec.n
            n += 1
    assert n >= 12


@pytest.mark.parametrize("name,at_least", [("a", 3), ("b", 2)])
def test_chains_in_front_of_a_segments_first_record_are_its_guess(built, name, at_least):
    _, models = built
    decoys = sc.CASES[name]().meta["decoys"]
    for cb, m in _of(models, name, "decoy"):
        assert _total(m, "wrong") >= at_least, cb
        guessed = {g for c in m for s, g in c["guess"].items() if s in c["wrong"]}
        assert guessed == set(decoys), cb                             # every chain is taken for the segment's start, at every chunk size
        assert not _total(m, "stray")


def test_b_rejoins_the_true_chain(built):
    paths, _ = built
    stream, _ = sc.inflate(paths["b", "decoy"])
    n_ref, first = sc.bam_header(stream)
    starts = set(sc.truth(stream, first)[:-1])
    for at in sc.CASES["b"]().meta["decoys"]:
        o = at
        for _ in range(4):
            assert o not in starts
            o = sc.plausible(stream, o, len(stream), n_ref)
        assert o in starts and o // SEG >= at // SEG + 2              # the fourth header leads to a record start, two segments on


def test_c_two_chains_stop_in_a_chunk_that_is_not_the_last(built):
    _, models = built
    m = models["c", "decoy", 3]
    stops = sc.CASES["c"]().meta["stops"]
    hit = 0
    for k, c in enumerate(m[:-1]):
        mine = [s for s in stops if c["base"] <= s < c["end"]]
        if not mine:
            continue
        assert len(c["wrong"]) >= 1
        carry_from = m[k + 1]["start0"]
        assert m[k + 1]["carry"] > 0 and all(s < carry_from for s in mine)      # the decoy's stop lies in front of the true one: a minimum over both would be wrong
        hit += 1
    assert hit >= 1
    assert _total(models["c", "decoy", 16384], "wrong") >= 1


def test_d_a_record_over_whole_segments_with_and_without_chains_inside(built):
    _, models = built
    for cb, m in _of(models, "d", "plain"):
        assert _total(m, "no_start") >= 2 and all(c["clean"] for c in m), cb
    for cb, m in _of(models, "d", "decoy"):
        assert _total(m, "no_start") >= 2 and _total(m, "stray") >= 2 and not _total(m, "wrong"), cb


def test_e_the_carry_is_longer_than_a_segment_and_holds_chains(built):
    _, models = built
    m = models["e", "decoy", 3]
    assert any(c["carry"] > SEG and any(s < sc.CARRY_SEGS for s in c["stray"]) for c in m)
    assert any(c["carry"] > SEG for c in models["e", "control", 3])


def test_f_chunks_that_lie_inside_one_record(built):
    _, models = built
    m = models["f", "plain", 1]
    run = best = 0
    for k, c in enumerate(m):
        run = run + 1 if c["n_records"] == 0 else 0
        best = max(best, run)
        if run >= 2:
            assert c["carry"] > m[k - 1]["carry"]                     # ... and the carry grows from chunk to chunk
    assert best >= 3
    assert max(c["carry"] for c in m) > 2 * SEG


def test_g_one_header_and_then_the_data_ends(built):
    _, models = built
    m = models["g", "decoy", 2]
    hits = [c for c in m if c["n_seg"] - 1 in c["wrong"] + c["stray"]]
    assert len(hits) >= 1
    decoys = set(sc.CASES["g"]().meta["decoys"])
    assert any(c["guess"].get(c["n_seg"] - 1) in decoys for c in hits)
    assert _total(models["g", "decoy", 16384], "wrong") >= 1


def test_h_every_seam_offset_is_a_carry_length(built):
    _, models = built
    m = models["h", "seams", 1]
    carries = {c["carry"] for c in m[1:]}
    last_byte = sc.CASES["h"]().meta["last_byte"]
    assert set(sc.SEAM_K) | {last_byte} <= carries and last_byte > 100
    assert 40 <= len(m) <= 48


def test_i_the_first_record_lies_deep_in_its_block_or_in_a_later_block(built):
    _, models = built
    for cb, m in _of(models, "i", "one_block"):
        assert m[0]["base"] == 0 and m[0]["start0"] > 2 * SEG and m[0]["s0"] >= sc.CARRY_SEGS + 2
    for cb, m in _of(models, "i", "two_blocks"):
        assert m[0]["base"] >= sc.BLOCK                               # the first chunk begins with a later block than the file does: b0 >= 1
        assert m[0]["start0"] > m[0]["base"]


def test_j_records_end_on_segment_boundaries_and_at_the_end(built):
    paths, models = built
    m = models["j", "aligned", 1]
    stream, _ = sc.inflate(paths["j", "aligned"])
    ends = set(sc.truth(stream, sc.bam_header(stream)[1])[1:])
    e0, e1, e2 = sc.CASES["j"]().meta["ends"]
    assert {e0, e1, e2} <= ends and not any(e % SEG for e in (e0, e1, e2))
    assert m[0]["end"] == e0 and m[1]["carry"] == 0                   # a record ends exactly at `end`, on a segment boundary
    assert m[1]["base"] == e0 and m[1]["end"] == e2 + 20 and (m[1]["end"] - m[1]["base"]) % SEG == 20      # the last segment holds 20 bytes
    assert m[2]["carry"] == 20
    assert 1 <= m[2]["n_records"] < 4 and m[3]["carry"] > 36


def test_k_every_shape_twice_and_once_as_the_last_record_of_a_chunk(built):
    paths, models = built
    case = sc.CASES["k"]()
    rec = case.rec
    for name, fn in sc.SHAPES.items():
        assert sum(bool(fn(rec, i)) for i in range(rec.n)) >= 2, name
    assert sum(bool(sc.SHAPES["smallest"](rec, i)) for i in range(rec.n)) >= sc.N_SMALLEST
    stream, _ = sc.inflate(paths["k", "cuts"])
    offs = sc.truth(stream, sc.bam_header(stream)[1])
    chunk_ends = {c["end"] for c in models["k", "cuts", 1]}
    for name, fn in sc.SHAPES.items():
        e = case.meta["last"][name]
        assert e in chunk_ends and fn(rec, offs.index(e) - 1), name
    ustream, _ = sc.inflate(paths["k", "uniform"])
    per_segment = np.bincount(np.asarray(sc.truth(ustream, sc.bam_header(ustream)[1])[:-1]) // SEG)
    assert per_segment.max() > 400                                    # the smallest records: more than 400 to a segment


def test_l_a_carry_of_more_than_the_room_in_front_of_a_chunk(built):
    _, models = built
    m = models["l", "huge", 4]
    assert max(c["carry"] for c in m) > 1 << 20 and sum(c["n_records"] == 0 for c in m) >= 3        # ... grown over chunks that lie inside the record
    assert len(models["l", "huge", 16384]) == 1 and _total(models["l", "huge", 16384], "no_start") > 60


def test_n_ordinary_records_are_decoys_enough(built):
    paths, models = built
    assert not sc.CASES["n"]().variants["natural"].kw.get("extra")
    stream, _ = sc.inflate(paths["n", "natural"])
    starts = set(sc.truth(stream, sc.bam_header(stream)[1])[:-1])
    for cb, m in _of(models, "n", "natural"):
        assert _total(m, "wrong") >= 1 and not _total(m, "stray"), cb
        for c in m:
            for s in c["wrong"]:                                      # two bytes in front of the segment's first record
                assert c["guess"][s] + 2 in starts


def test_the_models_truth_is_a_walk_of_the_inflated_file(built):
    """the stream as zlib's gzip reader gives it (member by member, knowing nothing of BGZF), walked by block_size: the layout the
    builders computed, the records the batch has"""
    paths, _ = built
    for (name, label), path in paths.items():
        raw, out = open(path, "rb").read(), []
        while raw:
            z = zlib.decompressobj(31)
            out.append(z.decompress(raw))
            raw = z.unused_data
        stream = b"".join(out)
        assert stream == sc.inflate(path)[0]
        case = sc.CASES[name]()
        kw = case.variants[label].kw
        off, _ = sc.layout(case.rec, kw.get("header_text") or bamio.sam_header(case.rec.targets), kw.get("extra") or {})
        assert sc.truth(stream, sc.bam_header(stream)[1]) == off and off[-1] == len(stream) and len(off) == case.rec.n + 1, (name, label)


def test_a_file_cut_inside_its_last_record(built, tmp_path):
    paths, _ = built
    dst = str(tmp_path / "cut.bam")
    n, last = sc.cut_inside_last_record(paths["a", "control"], dst)
    stream, _ = sc.inflate(dst)
    offs = sc.truth(stream, sc.bam_header(stream)[1])
    assert len(stream) == n and offs[-1] == last and len(offs) == sc.CASES["a"]().rec.n       # all records but the last, and 50 bytes
    assert sc.scan_model(dst, 16384)[0]["n_records"] == len(offs) - 1


def test_the_host_reader_meets_the_same_files(built, tmp_path):
    """cli/bam_reader.cpp guesses a record start per group of blocks and verifies the guesses, as the device scan does per
    segment: with three blocks to a superchunk and four threads it yields the records the sequential reader yields, of every
    file here; a file cut inside its last record is refused by both"""
    paths, _ = built
    env = dict(os.environ, STRL_THREADS="4", STRL_CHUNK_BLOCKS="3")
    for (name, label), path in paths.items():
        a = subprocess.run([CLI, "_dump", path], capture_output=True, text=True)
        b = subprocess.run([CLI, "_dump", path, "stream", "500"], capture_output=True, text=True, env=env)
        assert a.returncode == 0 and b.returncode == 0, (name, label, a.stderr, b.stderr)
        assert a.stdout == b.stdout and a.stdout.count("\n") >= sc.CASES[name]().rec.n + 4, (name, label)
    cut = str(tmp_path / "cut.bam")
    sc.cut_inside_last_record(paths["a", "control"], cut)
    for args in (["_dump", cut], ["_dump", cut, "stream", "500"]):
        r = subprocess.run([CLI] + args, capture_output=True, text=True, env=env)
        assert r.returncode == 1 and "error reading" in r.stderr, (args, r.returncode, r.stderr)


@pytest.mark.parametrize("name", list(sc.CASES))
def test_every_case_has_treads_to_compare(oracle, name):
    case = sc.CASES[name]()
    med = oracle.median(synth.frag_hist(case.rec))
    assert len(oracle.extract(case.rec, case.genome, oracle.make_opts(med, 0.8, 40))) > 20


def test_write_bam_defaults_are_unchanged(tmp_path):
    """extra / quals / cuts left alone: the bytes of before; given: the record grows by exactly the bytes handed over"""
    rec, _ = sc.base_records(50, 1)
    a, b, c = (str(tmp_path / f"{x}.bam") for x in "abc")
    bamio.write_bam(a, rec, index=False)
    bamio.write_bam(b, rec, index=False, extra=None, quals=None, cuts=None)
    assert open(a, "rb").read() == open(b, "rb").read()
    bamio.write_bam(c, rec, index=False, extra={3: sc.aux_array(b"abc")}, quals={3: bytes(int(rec.l_seq[3]))}, cuts=[100, 5000])
    sa, sb = sc.inflate(a), sc.inflate(c)
    oa = sc.truth(sa[0], sc.bam_header(sa[0])[1])
    assert sb[1][:2] == [100, 4900] and len(sb[0]) == len(sa[0]) + 11
    assert sb[0][:oa[3]] == sa[0][:oa[3]] and sb[0][oa[4] + 11:] == sa[0][oa[4]:] and sb[0][oa[4]:oa[4] + 11] == sc.aux_array(b"abc")
