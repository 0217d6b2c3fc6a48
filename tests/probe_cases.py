"""Batches for pair_probe_kernel and the Bloom bitmap's layout (strling_amd/csrc/pair.hip, bloom_layout.h) whose qname-hash column
the test writes itself: fmix64 is a bijection, so a case chooses the MIXED hash of every qname group -- the word of the bitmap and
the bit positions inside it -- and stores its preimage.  Mates share a value, distinct qnames get distinct values, so the device's
join (keyed by the hash) forms the groups the oracle (keyed by the name) forms, and the treads must be the oracle's.

The layout is restated here (word from the low bits, K six-bit fields from bit 32 on); tests/test_bloom_layout.py holds the
restatement against the header's own functions, and every case against the oracle's idea of which groups are hot.  No GPU code.
"""
import collections
import functools

import numpy as np

import loop_cases as LC

K = 4                       # bits per key
WORD_BITS = 64
SMALL_BITS = 1 << 16        # the smallest bitmap: any batch of at most 131 072 reads
SMALL_WORDS = SMALL_BITS // WORD_BITS
M64 = (1 << 64) - 1
SIZES = (2, 63, 64, 65, 513, 2113)
FLUSH_N = LC.N              # the `hot` case's shape: four probe waves of 2112 reads under STRL_GRID_P=1
CONFIGS = {"one": dict(STRL_GRID_P=1)}

Case = collections.namedtuple("Case", "name rec qhash groups hot_design")
Group = collections.namedtuple("Group", "hot word fields clip what")


def fmix64(h):
    h ^= h >> 33; h = h * 0xff51afd7ed558ccd & M64; h ^= h >> 33; h = h * 0xc4ceb9fe1a85ec53 & M64; h ^= h >> 33
    return h


def fmix64_inv(m):
    m ^= m >> 33; m = m * pow(0xc4ceb9fe1a85ec53, -1, 1 << 64) & M64; m ^= m >> 33; m = m * pow(0xff51afd7ed558ccd, -1, 1 << 64) & M64; m ^= m >> 33
    return m


def key(word, fields, uniq):
    """the mixed hash of a group: `word` of the smallest bitmap, the K bit positions, and a number that keeps the hashes (and their
    low 32 bits, which the join sorts by) distinct"""
    assert 0 <= word < SMALL_WORDS and len(fields) == K and all(0 <= f < 64 for f in fields) and 0 <= uniq < (1 << 22)
    m = word | (uniq << 10)
    for j, f in enumerate(fields):
        m |= f << (32 + 6 * j)
    return m


def word_of(m, bits=SMALL_BITS):
    return m & (bits // WORD_BITS - 1)


def pattern_of(m):
    p = 0
    for j in range(K):
        p |= 1 << ((m >> (32 + 6 * j)) & 63)
    return p


def _build(name, groups, lone_first, seed):
    """mates adjacent (the shape of loop_cases._hot); a hot group's reads are tracts, a cold group's random; `clip`: the first read
    of the group is soft-clipped, so that the group brings a hot soft-clip record as well"""
    rng = LC._rng(seed)
    pos, mpos, flag, qn, seqs, cig, grp = [], [], [], [], [], [], []
    if lone_first:                               # an odd batch: a lone cold read in front
        groups = [Group(False, SMALL_WORDS - 1 - 64, (9, 19, 29, 39), False, "lone")] + list(groups)
    for g, G in enumerate(groups):
        for j in range(1 if G.what == "lone" else 2):
            before = j == 0
            pos.append(1000 + g if before else 900_000 + g)
            mpos.append(900_000 + g if before else 1000 + g)
            flag.append(99 if before else 147)
            qn.append("p%05d" % g)
            seqs.append(LC.HOT_SEQ if G.hot else LC._rand(rng, 150))
            cig.append("30S120M" if G.clip and before else "150M")
            grp.append(g)
    n = len(pos)
    rec = LC._batch([0] * n, pos, cig, seqs, flag=flag, mpos=mpos, qnames=qn)
    m = [key(G.word, G.fields, g) for g, G in enumerate(groups)]
    assert len(set(m)) == len(m) and len(set(x & 0xffffffff for x in m)) == len(m)
    qhash = np.array([fmix64_inv(m[g]) for g in grp], np.uint64)
    return Case(name, rec, qhash, groups, np.array([groups[g].hot for g in grp]))


@functools.lru_cache(maxsize=None)
def layout():
    """every edge of the layout in one batch of the smallest bitmap"""
    rng = LC._rng(51)
    hot = [Group(True, 0, (0, 31, 32, 63), False, "bit positions 0, 31, 32, 63, first word"),
           Group(True, SMALL_WORDS - 1, (5, 5, 5, 5), False, "all fields equal, last word"),
           Group(True, 7, (1, 2, 3, 4), True, "two hot keys in one word (a)"),
           Group(True, 7, (10, 20, 30, 40), False, "two hot keys in one word (b)"),
           Group(True, 1, (63, 63, 63, 63), False, "all fields 63"),
           Group(True, 2, (0, 0, 0, 0), True, "all fields 0"),
           Group(True, SMALL_WORDS - 1, (0, 31, 32, 63), False, "bit positions 0, 31, 32, 63, last word"),
           Group(True, 0, (31, 32, 31, 32), False, "the two middle bits, first word")]
    short = [Group(False, 7, (1, 2, 3, 5), False, "one bit short of (a)"),
             Group(False, 7, (10, 20, 30, 41), False, "one bit short of (b)"),
             Group(False, 7, (1, 2, 10, 21), False, "three bits of (a) and (b) together, one short"),
             Group(False, 0, (0, 31, 32, 62), False, "one bit short, first word"),
             Group(False, SMALL_WORDS - 1, (5, 5, 5, 6), False, "one bit short of the single bit, last word"),
             Group(False, 1, (63, 63, 63, 62), False, "one bit short, all fields 63"),
             Group(False, 2, (0, 0, 0, 1), False, "one bit short, all fields 0")]
    away = [Group(False, 100 + j, tuple(int(x) for x in rng.integers(0, 64, K)), False, "word disjoint from every hot key's") for j in range(40)]
    groups = short + away + hot[:-1]
    order = rng.permutation(len(groups))
    return _build("layout", [groups[int(i)] for i in order] + [hot[-1]], False, 52)


def _random_groups(n, p_hot, seed):
    """hot keys in the lower half of the words, cold keys in the upper half: no cold key can pass; the last group is hot"""
    rng = LC._rng(seed)
    n_groups = n // 2
    out = []
    for g in range(n_groups):
        is_hot = g == n_groups - 1 or rng.random() < p_hot
        w = int(rng.integers(0, SMALL_WORDS // 2)) + (0 if is_hot else SMALL_WORDS // 2)
        out.append(Group(is_hot, w, tuple(int(x) for x in rng.integers(0, 64, K)), is_hot and g % 5 == 0, ""))
    return out


@functools.lru_cache(maxsize=None)
def sized(n):
    """n reads, the last one hot: the ends of a wave's range and of a turn (64 lanes, 512 reads) around the clamped loads"""
    return _build("n%d" % n, _random_groups(n, 0.5, 60 + n), n % 2 == 1, 61 + n)


@functools.lru_cache(maxsize=None)
def flush():
    """three groups in four hot: under STRL_GRID_P=1 a wave owns 2112 reads and fills its stage (PR_STAGE hits) before its last turn"""
    return _build("flush", _random_groups(FLUSH_N, 0.78, 71), FLUSH_N % 2 == 1, 72)


ALL = ("layout", "flush") + tuple("n%d" % n for n in SIZES)


def case(name):
    return layout() if name == "layout" else flush() if name == "flush" else sized(int(name[1:]))


@functools.lru_cache(maxsize=None)
def expected(name):
    """the oracle's treads, which reads belong to a hot group (loop_cases.expected's definition), and the join items a probe without
    a spurious hit makes: the reads of the hot groups plus the hot soft-clip records"""
    from oracle import oracle as O
    from helpers import oracle_words, soft_items_expected
    c = case(name)
    opts = O.make_opts(LC.OPTS[2], LC.OPTS[0], LC.OPTS[1])
    whole, soft = oracle_words(O, c.rec, None, opts)
    items = soft_items_expected(c.rec, whole, LC.OPTS[1])
    hot_read = ((whole >> 16) != 0) & ((whole & 0x8000) == 0)
    n_hot_soft = 0
    for i, s in items:
        a, b = soft[(i, s)]
        if (int(a) >> 16) or (int(b) >> 16):
            hot_read[i] = True
            n_hot_soft += 1
    grp = LC.qname_groups(c.rec)
    hot_grp = np.zeros(grp.max() + 1, bool)
    hot_grp[grp[hot_read]] = True
    probe_hit = hot_grp[grp]
    return dict(treads=O.extract(c.rec, None, opts, 0), probe_hit=probe_hit, n_hot_soft=n_hot_soft, items=int(probe_hit.sum()) + n_hot_soft)
