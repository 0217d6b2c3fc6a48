"""The inputs of tests/loop_cases.py reach the edges they are built for (CPU only).

Two things are asserted here, so that tests/test_loop_device.py cannot pass by running kernels whose loops never turn:
  * the ORACLE's skipped flags of every skip-predicate case equal a brute-force all-pairs predicate (two independent statements of
    extract.nim:30-34), and the hand-derived answers of the touching-end reads;
  * under every grid configuration a case is run with, the launch arithmetic (loop_cases.Model: constants and formulas read off the
    kernels' source) takes the case where it is meant to go: several turns per wave, a contig change on a turn's boundary, more
    than JOIN_WIN starts in a span, a turn below the carried window, a stage that fills before the last turn, two turns per
    scorer lane with the named neighbours, 17 lanes with a base that is not ACGT in a wave, two rounds per compaction kernel.
A case that stops reaching its edge (because a constant, a rounding or a grid formula changed) fails here.
"""
import numpy as np
import pytest

import loop_cases as LC

CFGS = ["one", "odd", "split"]


@pytest.fixture(scope="module")
def model():
    return LC.Model()


def _trace(model, name, cfg):
    c = LC.case(name)
    return model.classify_trace(c, LC.CONFIGS[cfg] if cfg else None, ~LC.expected(name)["skipped"])


def test_model_constants_and_partitions(model):
    """what the issue's sizes were chosen for, from the constants found in the source"""
    assert (model.CL_ILP, model.CL_STAGE, model.PR_ILP, model.PR_STAGE, model.JOIN_WIN, model.BIN_SHIFT) == (8, 512, 8, 1024, 8, 12)
    one = model.wave_ranges(LC.N, "C", LC.CONFIGS["one"])
    assert one == [(0, 2304), (2304, 4608), (4608, 6912), (6912, 8269)] and (one[-1][1] - one[-1][0]) % 4 == 1      # the ragged group of the vector variant
    odd = model.wave_ranges(LC.N, "C", LC.CONFIGS["odd"])
    assert len(odd) == 7 and odd[0] == (0, 1280) and odd[-1] == (7680, 8269)
    assert model.wave_ranges(LC.N, "P", LC.CONFIGS["one"])[0] == (0, 2112)
    # unset, the grids are what the batch makes them: one turn per wave, one per lane, one round per block
    assert all(len(it) == 1 for it in model.iterations(LC.N, "C", None)) and all(len(it) == 1 for it in model.iterations(LC.N, "P", None))
    for max_l in (160, 256, 510):
        for stage in "AB":
            g, b = model.score_grid(LC.N3, max_l, stage, None)
            assert g * b >= LC.N3
            assert model.score_grid(LC.N3, max_l, stage, LC.CONFIGS["odd"]) == (3 if stage == "A" else 2, b)       # no clamp on a given grid
    assert (model.score_grid(1 << 25, 256, "A", None), model.score_grid(1 << 25, 510, "A", None)) == ((2048, 256), (4096, 64))
    assert (model.score_grid(LC.N, 256, "A", None), model.score_grid(LC.N, 510, "B", None)) == ((256, 256), (512, 64))
    for k in model.rounds:
        assert model.compaction_rounds(k, 1 << 20, None) == 1


def test_model_names_what_it_cannot_find():
    with pytest.raises(AssertionError, match="the window-reuse test not found"):
        LC._find("if (!(J.valid && J.e[WIN - 1].x >= smax))", r"J\.valid && smin >= J\.lo", "the window-reuse test")


@pytest.mark.parametrize("name", LC.SKIP_CASES)
def test_oracle_skip_flags_equal_the_brute_force_predicate(name):
    c = LC.case(name)
    exp = LC.expected(name)["skipped"]
    brute = LC.brute_force_skipped(c.rec, c.genome)
    assert np.array_equal(exp, brute), np.flatnonzero(exp != brute)[:10]
    if c.genome is not None:
        assert 1000 < int(exp.sum()) < c.rec.n - 1000          # both answers are common
    for i, (sk, what) in c.meta.get("expect", {}).items():
        assert bool(exp[i]) == sk, (i, what, int(c.rec.pos[i]))


def test_nested_reads_answered_by_the_running_max():
    c = LC.case("nested")
    lo, hi = c.meta["long"]
    start, stop = c.rec.pos.astype(np.int64), c.rec.pos.astype(np.int64) + 100
    inner = np.array(c.meta["inner"])
    only_long = (start < hi) & (stop > lo) & ~((inner[None, :, 0] < stop[:, None]) & (inner[None, :, 1] > start[:, None])).any(axis=1)
    later_starts = (inner[None, :, 0] < stop[:, None]).sum(axis=1)          # starts between the long interval's and the read's stop
    assert len(inner) >= 60
    assert int((only_long & (later_starts >= 2 * LC.Model().JOIN_WIN)).sum()) >= 1000
    assert not LC.expected("nested")["skipped"][only_long].any()


@pytest.mark.parametrize("cfg", CFGS)
@pytest.mark.parametrize("name", LC.SKIP_CASES)
def test_skip_case_reaches_its_edge(model, name, cfg):
    rows = _trace(model, name, cfg)
    turns = [len(it) for it in model.iterations(LC.N, "C", LC.CONFIGS[cfg])]
    assert all(t >= 3 for t in turns[:-1]) and turns[-1] >= 2, turns
    later = [r for r in rows if r["turn"] >= 1]
    S = model.CL_STAGE
    if name == "nested":
        assert sum(r["window"] == "reused" for r in later) >= 1 and sum(r["window"] == "loaded" for r in later) >= 3
    elif name == "dense":
        hit = [r for r in later if r["fallback"] and r["uniform"] and r["starts_in_span"] > model.JOIN_WIN]
        assert len(hit) >= 2, "no later turn with more than JOIN_WIN starts between smin's bin and smax"
    elif name == "edges":
        assert any(r["window"] == "reused" and r["at_lo"] for r in later), "no reused window with smin == J.lo"
        sent = [r for r in rows if r.get("all_sentinel")]
        assert sent, "no window loaded behind the last bin"
        assert any(r["wave"] == sent[0]["wave"] and r["turn"] > sent[0]["turn"] and r["window"] == "reused" for r in rows), "the all-sentinel window is not reused"
    elif name == "backwards":
        assert sum(r.get("below", False) and r["window"] == "loaded" for r in later) >= 3, "no turn below the carried window"
    elif name == "contigs":
        c = LC.case(name)
        on = {r["base"] for r in later if r["contig_changed"] and r["uniform"]}
        want = {c.meta["boundaries"]["both"], c.meta["boundaries"]["odd" if cfg == "odd" else "one"]}
        assert want <= on, (want, on)
        assert sum(r["any"] and not r["uniform"] for r in rows) >= 2, "no turn with mixed contigs"
        assert any(not r["any"] and not r["last_turn"] and r["end"] - r["base"] == 64 * model.CL_ILP for r in rows), "no full turn without a candidate"
        tids = {r.get("tid") for r in rows if r["uniform"]}
        assert {0, 1, 2, 3, 4, 5} <= tids                                  # tid 2: no key of the table; tid 3: a key without intervals
        assert any(r.get("tid") == 3 and r.get("all_sentinel") for r in rows)
        assert set(np.unique(c.rec.tid)) >= {-1, 6}
    elif name == "contig_carry":
        fits = {r["base"] for r in later if r["contig_changed"] and r.get("stale_fits")}
        assert set(LC.case(name).meta["changes"]) <= fits, fits
        e = LC.expected(name)["skipped"]
        assert e[:1024].all() and not e[1024:4352].any() and e[4352:].all()
    elif name == "keep_all":
        mid = [r for r in rows if not r["last_turn"]]
        assert mid and all(r["flushed"] and r["cnt_after"] == S for r in mid if r["end"] - r["base"] == S)
    elif name == "keep_half":
        assert any(r["flushed"] and not r["last_turn"] and S < r["cnt_after"] < 2 * S and r["cnt_before"] > 0 for r in rows), \
            [(r["wave"], r["turn"], r["cnt_after"]) for r in rows]
    if name in ("keep_all", "keep_half"):
        assert any(r["flushed"] and not r["last_turn"] for r in rows), "no wave keeps CL_STAGE reads before its last turn"


@pytest.mark.parametrize("name,cfgs", [("hot", ["one", "split"]), ("hot_wide", ["one", "odd", "split"])])
def test_probe_wave_fills_its_stage_before_its_last_turn(model, name, cfgs):
    c, e = LC.case(name), LC.expected(name)
    hit = e["probe_hit"]
    assert hit.mean() >= 0.70 and len(e["treads"]) > 1000
    for cfg in cfgs:
        filled = 0
        for its in model.iterations(c.rec.n, "P", LC.CONFIGS[cfg]):
            assert len(its) >= 3
            cnt = 0
            for a, b in its[:-1]:
                cnt += int(hit[a:b].sum())
                if cnt >= model.PR_STAGE:
                    filled += 1
                    break
        assert filled >= 2, (name, cfg)
    if name == "hot":         # STRL_GRID_P=3: twelve waves of 704 reads, which cannot hold PR_STAGE hits -- what hot_wide is for
        assert max(b - a for a, b in model.wave_ranges(c.rec.n, "P", LC.CONFIGS["odd"])) < model.PR_STAGE


@pytest.mark.parametrize("cfg", CFGS)
@pytest.mark.parametrize("name", ["short_mix", "mid_mix", "long_mix"])
def test_scorer_mix_neighbours_in_consecutive_turns_of_a_lane(model, name, cfg):
    c = LC.case(name)
    attrs, max_l, n = c.meta["attrs"], c.meta["max_l"], c.rec.n
    assert int(c.rec.l_seq.max()) == max_l and int(c.rec.l_seq.min()) == 0
    grid, block = model.score_grid(n, max_l, "A", LC.CONFIGS[cfg])
    stride = grid * block
    assert n >= 2 * stride + block
    kept = np.ones(n, bool)
    for vec in (True, False):
        for order, q in model.queue_orders(n, LC.CONFIGS[cfg], kept, vec).items():
            assert np.array_equal(np.sort(q), np.arange(n))
            a = [attrs[int(i)] for i in q]
            for what, first, then in LC.NEIGHBOURS:
                k = sum(1 for i in range(n - stride) if first(a[i], max_l) and then(a[i + stride], max_l))
                assert k >= 20, (what, order, vec, k)
            has_n = np.array([x["has_n"] for x in a])
            per_wave = np.add.reduceat(has_n.astype(int), np.arange(0, n, 64))
            assert per_wave.max() >= 17 and (per_wave >= 17).sum() >= 10 and per_wave.min() < 16, per_wave
    assert model.score_grid(n, max_l, "A", None)[0] * block >= n          # (unset: one turn)


@pytest.mark.parametrize("cfg", CFGS)
@pytest.mark.parametrize("name", ["clips", "clips_long"])
def test_clip_cases_turn_the_segment_scorers_and_the_compaction_rounds(model, name, cfg):
    c, e = LC.case(name), LC.expected(name)
    env = LC.CONFIGS[cfg]
    n, max_l, items = c.rec.n, c.meta["max_l"], e["items"]
    clipped = len({i for i, _ in items})
    lens = np.array([int(c.rec.cigar[int(c.rec.cigar_off[i])]) >> 4 if s == 0 else int(c.rec.cigar[int(c.rec.cigar_off[i + 1]) - 1]) >> 4 for i, s in items])
    assert lens.min() == 17 and clipped >= 3000
    if name == "clips":
        assert int(c.rec.l_seq.max()) == 160 and set(range(3, 21)) <= set(((lens + 7) >> 3).tolist())       # every length class from 17 bases up
        assert n == LC.N3 and len(items) > 8192 and len(e["treads"]) > 1000
        assert model.compaction_rounds("soft_compact_kernel", n, env) >= 2 and model.compaction_rounds("compact_kernel", n, env) >= 2
        assert model.compaction_rounds("pair_soft_items_kernel", len(items), env) >= 2
        if cfg == "split":       # (the survivor compaction of the segments is only launched beside the split scorer)
            assert model.compaction_rounds("compact_kernel", len(items), env) >= 2
        assert (model.compaction_rounds("soft_compact_kernel", n, LC.CONFIGS["one"]), model.compaction_rounds("compact_kernel", n, LC.CONFIGS["one"])) == (3, 3)
    else:
        assert int(c.rec.l_seq.max()) > 256 and int((lens > 160).sum()) >= 300
        assert model.compaction_rounds("pair_soft_items_kernel", len(items), LC.CONFIGS["one"]) >= 2
    grid, block = model.score_grid(n, max_l, "A", env)
    assert len(items) >= 3 * grid * block and n >= 3 * grid * block         # turns of a lane over the segments and over the whole reads
