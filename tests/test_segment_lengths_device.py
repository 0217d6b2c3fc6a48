"""The segment scorer when the lengths of a wave's segments decide how much of the k = 5, 6 counts and of the literal recount
runs: waves that mix clips of 1 .. 149 bases, waves of one length on the edges of the four-window blocks and 16-base words,
whole reads of one length, the split launches, the long class, and the records' way through the pair logic.  Everything
against the oracle, through the C ABI.  Needs a real MI355X (-m gpu)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from strling_amd import api, synth
from strling_amd.records import RecordBatch, unpack_result
from helpers import oracle_words, soft_items_expected, treads_equal

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
P, Q = 0.8, 40


def _unit(rng, k):
    return "".join(rng.choice(list("ACGT"), k))


def _part(rng, n, kind, unit=None):
    """n bases: 0..5 = a repeat of a (kind + 1)-mer at some phase and purity, 6 = random, 7 = random with N and other codes"""
    if n == 0:
        return ""
    if kind == 6:
        return "".join(rng.choice(list("ACGT"), n))
    if kind == 7:
        return "".join(rng.choice(list("ACGTACGTACGTNNR"), n))
    u = unit or _unit(rng, kind + 1)
    ph = int(rng.integers(0, len(u)))
    s = np.array(list((u * (n // len(u) + 3))[ph:ph + n]))
    pur = float(rng.choice([1.0, 1.0, 0.97, 0.9]))
    hit = rng.random(n) >= pur
    s[hit] = rng.choice(list("ACGT"), int(hit.sum()))
    return "".join(s)


def _batch(seqs, cigars):
    n = len(seqs)
    return RecordBatch.from_fields(tid=[0] * n, pos=list(range(100, 100 + n)), mtid=[0] * n, mpos=[5] * n, flag=[99] * n,
                                   mapq=[60] * n, cigars=cigars, seqs=seqs, qnames=[f"r{i}" for i in range(n)])


def mixed_batch():
    """20 115 reads of 150 bases: every clip length 1 .. 149 on the left, on the right and on both sides, 45 of each, shuffled, so
    that the 64 clipped ends a wave takes are short and long ones side by side.  The clipped parts are k = 1 .. 6 repeats (a
    third of the reads is that repeat throughout, which is what gets a clip of 16 bases or fewer scored at all), random bases
    and N-bearing ones."""
    rng = np.random.default_rng(20261)
    L = 150
    seqs, cigars = [], []
    for rep in range(45):
        for c in range(1, L):
            for side in range(3):
                kind = int(rng.integers(0, 8))
                unit = _unit(rng, kind + 1) if kind < 6 else None
                if side == 2:
                    cl = c
                    cr = int(rng.integers(1, L - cl)) if cl < L - 1 else 0
                    if cr == 0:
                        cl, cr = 1, L - 2
                else:
                    cl, cr = (c, 0) if side == 0 else (0, c)
                if unit and rep % 3 == 0:
                    s = _part(rng, L, kind, unit)
                else:
                    kr = int(rng.integers(0, 8))
                    s = _part(rng, cl, kind, unit) + _part(rng, L - cl - cr, 6) + _part(rng, cr, kr if side == 2 else kind, unit if side != 2 else None)
                seqs.append(s)
                cigars.append((f"{cl}S" if cl else "") + f"{L - cl - cr}M" + (f"{cr}S" if cr else ""))
    order = rng.permutation(len(seqs))
    return _batch([seqs[i] for i in order], [cigars[i] for i in order])


def _check(ctx, oracle, rec, min_items):
    """words, the records (as a multiset: whatever order the device left them in, the entry point sorts by read and side) and the
    counts against the oracle"""
    opts = oracle.make_opts(350, P, Q)
    ctx.set_opts(P, Q, 350)
    ctx.set_genome(None)
    whole, soft, st = ctx.score_reads(rec)
    exp_whole, exp_soft = oracle_words(oracle, rec, None, opts)
    bad = np.nonzero(whole != exp_whole)[0]
    assert bad.size == 0, [(rec.sequence(int(i)), unpack_result(whole[i]), unpack_result(exp_whole[i])) for i in bad[:5]]
    items = soft_items_expected(rec, exp_whole, Q)
    assert len(items) >= min_items, len(items)
    got = sorted(zip(soft["read_side"].tolist(), soft["res_first"].tolist(), soft["res_after"].tolist()))
    exp = sorted(((i << 1) | s, exp_soft[(i, s)][0], exp_soft[(i, s)][1]) for i, s in items)
    assert len(got) == len(exp), (len(got), len(exp))                  # no hole, no duplicate
    diff = [(g, e) for g, e in zip(got, exp) if g != e]
    assert not diff, diff[:5]
    assert soft["read_side"].tolist() == [e[0] for e in exp]          # and in the entry point's order
    assert st.n_reads == rec.n and st.n_skipped == 0 and st.n_scored == rec.n and st.n_soft_items == len(items)
    return whole, soft, exp_soft, items


@pytest.fixture(scope="module")
def mixed(ctx, oracle):
    rec = mixed_batch()
    whole, soft, exp_soft, items = _check(ctx, oracle, rec, 20000)
    return rec, whole, soft, exp_soft, items


def test_waves_that_mix_short_and_long_clips(mixed):
    rec, whole, soft, exp_soft, items = mixed
    assert rec.n > 2 * 8192                         # several compaction rounds and a ragged last one
    lens = np.zeros(150, int)
    k56 = 0
    for i, s in items:
        op = rec.cigar[int(rec.cigar_off[i])] if s == 0 else rec.cigar[int(rec.cigar_off[i + 1]) - 1]
        lens[int(op) >> 4] += 1
        k56 += (exp_soft[(i, s)][1] >> 12) & 7 in (5, 6)
    assert (lens[17:150] > 0).all() and (lens[1:17] > 0).all(), np.nonzero(lens[1:] == 0)[0] + 1
    assert k56 > 500, k56                           # the k = 5, 6 counts and their recount decide results


@pytest.mark.parametrize("L", [4, 5, 6, 19, 20, 21, 24, 25, 29, 30, 31, 96, 100])
def test_waves_of_one_clip_length(ctx, oracle, L):
    """every clipped end of the batch has L bases: the wave's bounds are lo = hi = L, on and around the block edges"""
    rng = np.random.default_rng(100 + L)
    seqs, cigars = [], []
    for i in range(640):
        kind = int(rng.integers(0, 8)) if i % 4 else int(rng.integers(4, 6))
        unit = _unit(rng, kind + 1) if kind < 6 else None
        left = bool(i & 1)
        if unit and (L <= 16 or i % 3 == 0):      # the whole read is the repeat: its clip is scored whatever its length
            s = _part(rng, 150, kind, unit)
        else:
            c = _part(rng, L, kind, unit)
            s = c + _part(rng, 150 - L, 6) if left else _part(rng, 150 - L, 6) + c
        seqs.append(s)
        cigars.append(f"{L}S{150 - L}M" if left else f"{150 - L}M{L}S")
    _check(ctx, oracle, _batch(seqs, cigars), 200)


@pytest.mark.parametrize("L", [100, 101, 149, 150, 151, 160])
def test_whole_reads_of_one_length(ctx, oracle, L):
    """k = 5 and k = 6 repeats that reach stage B, in batches of one read length"""
    rng = np.random.default_rng(200 + L)
    seqs = []
    for i in range(1024):
        kind = [4, 5, 4, 5, 6, int(rng.integers(0, 8))][i % 6]
        seqs.append(_part(rng, L, kind))
    rec = _batch(seqs, [f"{L}M"] * len(seqs))
    whole, _, _, _ = _check(ctx, oracle, rec, 0)
    ks = (whole >> 12) & 7
    assert (ks == 5).sum() > 100 and (ks == 6).sum() > 100


def test_split_launches_on_the_mixed_batch(mixed, tmp_path):
    """STRL_SPLIT_SEGMENTS=1 (read once per process: a child) scores the same soft queue with stage A, the survivors' compaction
    and stage B: the same bytes as the fused launch"""
    rec, whole, soft, _, _ = mixed
    script = (
        "import sys, numpy as np\n"
        "sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "from strling_amd import api\n"
        "from test_segment_lengths_device import mixed_batch\n"
        "c = api.Context(0); c.set_opts(%r, %r, 350); c.set_genome(None)\n"
        "whole, soft, st = c.score_reads(mixed_batch())\n"
        "np.save(sys.argv[1] + '_w.npy', whole); np.save(sys.argv[1] + '_s.npy', soft)\n"
    ) % (os.path.dirname(HERE), HERE, P, Q)
    base = str(tmp_path / "split")
    subprocess.run([sys.executable, "-c", script, base], check=True, env=dict(os.environ, STRL_SPLIT_SEGMENTS="1"))
    assert np.array_equal(np.load(base + "_w.npy"), whole)
    assert np.load(base + "_s.npy").tobytes() == soft.tobytes()


def test_long_class_clips(ctx, oracle):
    """250-base reads with clips of up to 200 bases: the classes above 160 bases (hash-counted k = 5, 6, split launches)"""
    rng = np.random.default_rng(250)
    seqs, cigars = [], []
    for i in range(512):
        c = int(rng.integers(1, 201))
        kind = int(rng.integers(0, 8))
        unit = _unit(rng, kind + 1) if kind < 6 else None
        left = bool(i & 1)
        if unit and i % 3 == 0:
            s = _part(rng, 250, kind, unit)
        else:
            part = _part(rng, c, kind, unit)
            s = part + _part(rng, 250 - c, 6) if left else _part(rng, 250 - c, 6) + part
        seqs.append(s)
        cigars.append(f"{c}S{250 - c}M" if left else f"{250 - c}M{c}S")
    _check(ctx, oracle, _batch(seqs, cigars), 300)


def test_records_through_the_pair_logic(ctx, oracle):
    """extract on the device + resident clustering: the soft-clip records reach the pair logic wherever the scorer left them"""
    rec, g = synth.synth_wgs(30000, seed=4321, contig_len=3_000_000)
    frag = synth.frag_hist(rec)
    med = oracle.median(frag)
    ctx.set_opts(P, Q, med)
    ctx.set_genome(g)
    soa = api.Soa(rec)
    keep = soa.pair_rows()
    ctx.extract_device(soa.c_struct(), api.CPairSoa(keep[0].ctypes.data, keep[1].ctypes.data), int((rec.tid < 0).sum()))
    got, st = ctx.treads_fetch()
    exp = oracle.extract(rec, g, oracle.make_opts(med, P, Q))
    ok, why = treads_equal(got, exp)
    assert ok and len(exp) > 100, why
    window = api.frag_median(frag, 0.99)
    mcd = int(0.5 * api.frag_median(frag, 0.5))
    b, u, _ = ctx.cluster_resident(len(rec.targets), window, min_support=3, max_clip_dist=mcd, pos_bits=24)
    eb, eu = oracle.call_bounds(exp, 1, window, min_support=3, max_clip_dist=mcd)
    assert [api.bounds_row(x, "c") for x in b] == [oracle.bounds_row(x, "c") for x in eb] and len(eb) > 5
    assert [(x["repeat"].decode(), int(x["count"])) for x in u] == [(r, int(k)) for r, k in eu]
