"""Inputs that lay the join items of pair_groups_kernel (strling_amd/csrc/pair.hip) out item by item: which sorted items are
runs of one that cannot emit, which start a run whose replay can, and how many of the latter a 512-item block holds.

A batch is written as a list of qname groups IN JOIN ORDER (`layout_batch`): the builder hashes a pool of names, sorts them the
way the join will (pair_cases.join_order) and hands the groups out in that order.  Every read is hot (150 bases of CAG), so the
join items are exactly the records.  `block_model` restates, from the batch's own qname hashes, what each block should see; the
`*_conditions` functions assert it together with what the ORACLE emits, so that no test compares two empty results by accident.
"""
import functools

import numpy as np

import pair_cases as pc
from oracle import oracle as O
from strling_amd import api
from strling_amd.records import RecordBatch

PG_BLOCK, PG_EMIT, PAIR_MAXM = 512, 256, 15        # restated from pair.hip
HOMO = "A" * 510                                    # scores 510 one-base units: to_tread's doAssert (extract.nim:72)

# kinds of group: ("alt", n)  n records alternating before / after their mate (pair_cases.hot_batch): n // 2 unplaced pairs
#                 ("after", 1) one record that lies after its mate: Cache.add returns at once
#                 ("tail", 1)  one unmapped record in the tail: stored on the first visit, its own mate on the second
#                 ("homo", 1)  one record before its mate whose scorer word counts 510


def lone(n, kind="alt"):
    return [(kind, 1)] * n


def pairs(n):
    return [("alt", 2)] * n


def n_items(spec):
    return sum(n for _, n in spec)


@functools.lru_cache(maxsize=None)
def _name_pool(prefix, n):
    """n names in the order the join puts them; no two share their low 32 hash bits"""
    names = ["%s%05d" % (prefix, i) for i in range(n)]
    probe = RecordBatch.from_fields([0] * n, [0] * n, [0] * n, [0] * n, [99] * n, [60] * n, ["1M"] * n, ["A"] * n, names)
    lo = pc.fmix64(api.qname_hash(probe)) & np.uint64(0xFFFFFFFF)
    assert np.unique(lo).size == n
    return [names[i] for i in np.argsort(lo, kind="stable")]


def layout_batch(spec, prefix="d"):
    """spec: groups in join order -> (RecordBatch, n_tail).  Records are written group by group in NAME order (the file order the
    replay must restore inside a run is the order of the record indices, not the join's), the unmapped tail last."""
    spec = list(spec)
    ordered = _name_pool(prefix, len(spec))
    by_name = sorted(zip(ordered, spec))
    rows, tail = [], []
    for g, (q, (kind, n)) in enumerate(by_name):
        lo_pos, hi_pos = 1000 + g, 900_000 + g
        if kind == "alt":
            for j in range(n):
                rows.append((0, lo_pos, 0, hi_pos, 99, 60, "150M", pc.HOT, q) if j % 2 == 0 else (0, hi_pos, 0, lo_pos, 147, 60, "150M", pc.HOT, q))
        elif kind == "after":
            rows.append((0, hi_pos, 0, lo_pos, 147, 60, "150M", pc.HOT, q))
        elif kind == "homo":
            rows.append((0, lo_pos, 0, hi_pos, 99, 60, "510M", HOMO, q))
        elif kind == "tail":
            tail.append((-1, -1, -1, -1, 77, 0, "*", pc.HOT, q))
        else:
            raise AssertionError(kind)
        assert kind == "alt" or n == 1
    rows += tail
    return RecordBatch.from_fields(*[[r[j] for r in rows] for j in range(9)]), len(tail)


def block_model(rec, qhash, n_tail, asserting=()):
    """what pair_groups_kernel's blocks see -> (run starts, run lengths, per block: dict(items, skipped, heads, long)).
    skipped: runs of one read in front of the tail (and not in `asserting`, the records whose word counts 256 or more): one
    Cache.add that stores or drops the read, nothing to emit; heads: first items of all other runs; long: those of more than
    15 items."""
    lo, starts, lens = pc.join_order(qhash)
    order = np.argsort(lo, kind="stable")                  # the record behind a sorted item: exact for runs of one
    tail_start = rec.n - n_tail
    blocks = [dict(items=min(PG_BLOCK, rec.n - b), skipped=0, heads=0, long=0) for b in range(0, rec.n, PG_BLOCK)]
    for s, m in zip(starts.tolist(), lens.tolist()):
        blk = blocks[s // PG_BLOCK]
        r = int(order[s])
        if m == 1 and r < tail_start and r not in asserting:
            blk["skipped"] += 1
        else:
            blk["heads"] += 1
            blk["long"] += m > PAIR_MAXM
    return starts, lens, blocks


def expect(rec, n_tail, p=0.8, q=40):
    return O.extract(rec, None, O.make_opts(pc.MEDIAN, p, q), n_tail)


def emitted(spec):
    """treads the groups of `spec` emit by the rules in the header (the oracle's count is asserted against it)"""
    return sum(n // 2 * 2 if kind == "alt" else 2 if kind == "tail" else 0 for kind, n in spec)


# ---- the cases: every spec is a whole number of 512-item blocks, so that they can be laid end to end ---------------------------
def spec_lone(kind="alt"):
    return lone(PG_BLOCK, kind)


def spec_pairs():
    return pairs(PG_BLOCK // 2)


def spec_runs15():
    return [("alt", 15)] * 34 + lone(2)


def spec_heads(k):
    """k pairs spread among 512 - 2 k lone reads"""
    n_lone = PG_BLOCK - 2 * k
    out = []
    for _ in range(k):
        out += lone(n_lone // k) + pairs(1)
    return out + lone(n_lone - n_lone // k * k)


HEAD_COUNTS = (1, 63, 64, 65)


def spec_head_counts():
    return [g for k in HEAD_COUNTS for g in spec_heads(k)]


def spec_ends_and_seam():
    """lone items at 0, 511 | 512, 1023 (the array's first and last, and either side of the seam)"""
    return lone(1) + pairs(255) + lone(1, "after") + lone(1) + pairs(255) + lone(1, "after")


def spec_run_at_511():
    """lone at 510, a run of three at 511 .. 513 (two items in the halo), lone at 514"""
    return pairs(255) + lone(1) + [("alt", 3)] + lone(1) + pairs(254) + lone(1, "after")


def spec_tail():
    out = []
    for _ in range(100):
        out += lone(1, "tail") + pairs(2)
    return out + pairs(6)


def spec_homo():
    return lone(100) + lone(1, "homo") + pairs(205) + lone(1)


def spec_long_mixed():
    return [("alt", 20)] + lone(50) + pairs(100) + [("alt", 16)] + lone(26, "after") + pairs(100)


def spec_all():
    """every case but the failing one, end to end: item 0 is lone, the last item is lone"""
    return (spec_lone() + spec_lone("after") + spec_pairs() + spec_runs15() + spec_head_counts() + spec_run_at_511() + spec_tail() + spec_long_mixed()
            + spec_ends_and_seam())


CASES = {
    "lone_before_mate": lambda: spec_lone() + spec_pairs(),
    "lone_after_mate": lambda: spec_lone("after") + spec_pairs(),
    "all_pairs": lambda: spec_pairs() * 2,
    "runs_of_15": lambda: spec_runs15() * 2,
    "head_counts": spec_head_counts,
    "ends_and_seam": spec_ends_and_seam,
    "run_at_511": spec_run_at_511,
    "tail": spec_tail,
    "long_mixed": spec_long_mixed,
    "all": spec_all,
}


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (spec, RecordBatch, n_tail, qname hashes, oracle's treads); built once, shared, never modified"""
    spec = CASES[name]()
    rec, n_tail = layout_batch(spec)
    qh = api.Soa(rec).pair_rows()[1]
    return spec, rec, n_tail, qh, expect(rec, n_tail)


def spec_conditions(spec, rec, n_tail, qh, exp):
    """the layout is the spec's: runs start where the spec puts them, with its lengths; the oracle emits what the spec's groups
    should -> the block model"""
    starts, lens, blocks = block_model(rec, qh, n_tail)
    assert rec.n == n_items(spec) and lens.tolist() == [n for _, n in spec]
    assert starts.tolist() == np.r_[0, np.cumsum([n for _, n in spec])[:-1]].tolist()
    assert n_tail == sum(kind == "tail" for kind, _ in spec)
    assert len(exp) == emitted(spec)
    return starts, lens, blocks


def case_conditions(name):
    spec, rec, n_tail, qh, exp = case(name)
    starts, lens, blocks = spec_conditions(spec, rec, n_tail, qh, exp)
    runs = dict(zip(starts.tolist(), lens.tolist()))
    heads = [b["heads"] for b in blocks]
    skipped = [b["skipped"] for b in blocks]
    if name in ("lone_before_mate", "lone_after_mate"):
        assert heads == [0, 256] and skipped == [512, 0]                 # block 0: no run that can emit
        assert len(exp) == 512 and exp["qname_id"].min() >= 0
        first_block = set(np.argsort(pc.join_order(qh)[0], kind="stable")[:512].tolist())     # the records behind items 0 .. 511
        assert not (set(exp["qname_id"].tolist()) & first_block)
        after = name == "lone_after_mate"
        assert all((rec.pos[r] > rec.mpos[r]) == after for r in first_block)
    elif name == "all_pairs":
        assert heads == [256, 256] and skipped == [0, 0] and 256 % 64 == 0       # four full waves of heads
        assert len(exp) == 1024 and 512 > PG_EMIT                              # every block emits more than its stage holds
    elif name == "runs_of_15":
        assert heads == [34, 34] and skipped == [2, 2] and 34 % 64 != 0          # heads that do not fill a wave
    elif name == "head_counts":
        assert heads == list(HEAD_COUNTS) and skipped == [PG_BLOCK - 2 * k for k in HEAD_COUNTS]
    elif name == "ends_and_seam":
        assert rec.n == 1024 and all(runs[i] == 1 for i in (0, 511, 512, 1023)) and runs[1] == 2 and runs[509] == 2 and runs[513] == 2
        assert heads == [255, 255] and skipped == [2, 2]
    elif name == "run_at_511":
        assert runs[510] == 1 and runs[511] == 3 and runs[514] == 1 and 511 + 3 > PG_BLOCK
        assert rec.n == 1024 and heads == [256, 254] and skipped == [1, 2]
    elif name == "tail":
        assert n_tail == 100 and heads == [100 + 206] and skipped == [0]
        # the reference emits for the lone tail reads, and on their second visit only: both treads carry the read's own index
        t = exp[exp["qname_id"] >= rec.n - n_tail]
        assert len(t) == 200 and (np.bincount(t["qname_id"] - (rec.n - n_tail), minlength=100) == 2).all()
        assert len(expect(rec, 0)) == len(exp) - 200                           # without the second visit they emit nothing
    elif name == "long_mixed":
        assert [b["long"] for b in blocks] == [2] and heads == [202] and skipped == [76]
        assert runs[0] == 20 and runs[270] == 16
    elif name == "all":
        assert len(blocks) == 14 and runs[0] == 1 and runs[rec.n - 1] == 1
        assert rec.n > 2 * PG_BLOCK * 2                                        # STRL_GRID_G=2: some block takes a third tile
        assert heads[:4] == [0, 0, 256, 34] and heads[4:8] == list(HEAD_COUNTS) and sum(b["long"] for b in blocks) == 2
        assert any(b["skipped"] == 512 for b in blocks) and n_tail == 100 and max(heads) == 100 + 206
    else:
        raise AssertionError(name)
    return dict(items=rec.n, blocks=len(blocks), heads=heads, skipped=skipped, treads=len(exp))


@functools.lru_cache(maxsize=None)
def homo_case():
    spec = spec_homo()
    rec, n_tail = layout_batch(spec)
    return spec, rec, n_tail, api.Soa(rec).pair_rows()[1]


def homo_conditions():
    """the one long read is a run of its own in front of the tail, and its scorer word counts 256 or more; without it nothing
    of the batch would be replayed differently"""
    spec, rec, n_tail, qh = homo_case()
    r = int(np.flatnonzero(rec.l_seq == 510)[0])
    wc = O.score_records_packed(rec, None, O.make_opts(pc.MEDIAN, 0.8, 40))[2]
    assert int(wc[r]) >= 256 and int(np.delete(wc, r).max()) < 256 and n_tail == 0
    starts, lens, blocks = block_model(rec, qh, n_tail, asserting={r})
    order = np.argsort(pc.join_order(qh)[0], kind="stable")
    at = int(np.flatnonzero(order == r)[0])
    assert at == 100 and dict(zip(starts.tolist(), lens.tolist()))[at] == 1
    assert [b["heads"] for b in blocks] == [206] and [b["skipped"] for b in blocks] == [101]
    assert rec.pos[r] < rec.mpos[r]                    # before its mate: Cache.add reaches to_tread
    return r


# ---- seeded mixtures ---------------------------------------------------------------------------------------------------------
N_DRAWS = 20


@functools.lru_cache(maxsize=None)
def mixed_case(draw):
    """about 1500 items of lone reads (before / after the mate, in the tail), pairs, triples, runs of 4 .. 15 and of 16 .. 24 in
    proportions drawn per batch -> (spec, rec, n_tail, qname hashes, oracle's treads)"""
    rng = np.random.Generator(np.random.Philox(key=[7919 + draw, 0]))
    w = rng.dirichlet([0.7] * 7) + 0.01
    w /= w.sum()
    spec, total = [], 0
    while total < 1500:
        c = int(rng.choice(7, p=w))
        g = [("alt", 1), ("after", 1), ("tail", 1), ("alt", 2), ("alt", 3), ("alt", int(rng.integers(4, 16))), ("alt", int(rng.integers(16, 25)))][c]
        reps = int(rng.integers(1, max(2, 24 // g[1])))        # short groups come in stretches, so that the shares are shares of ITEMS
        spec += [g] * reps
        total += g[1] * reps
    rec, n_tail = layout_batch(spec, prefix="m%02d_" % draw)
    return spec, rec, n_tail, api.Soa(rec).pair_rows()[1], expect(rec, n_tail)


def mixed_conditions():
    """every draw has the layout of its spec; over the 20 draws every kind of group occurs, the proportion of skippable items
    ranges widely -> per draw (items, skipped, heads, treads)"""
    out, kinds = [], set()
    for d in range(N_DRAWS):
        spec, rec, n_tail, qh, exp = mixed_case(d)
        _, _, blocks = spec_conditions(spec, rec, n_tail, qh, exp)
        kinds |= {(k, min(n, 16)) for k, n in spec}
        out.append(dict(items=rec.n, skipped=sum(b["skipped"] for b in blocks), heads=sum(b["heads"] for b in blocks), treads=len(exp)))
    assert {("alt", 1), ("after", 1), ("tail", 1), ("alt", 2), ("alt", 3), ("alt", 15), ("alt", 16)} <= kinds
    frac = [o["skipped"] / o["items"] for o in out]
    assert min(frac) < 0.1 and max(frac) > 0.5
    assert sum(o["treads"] > 0 for o in out) == N_DRAWS
    return out
