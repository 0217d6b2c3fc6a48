"""Inputs that put the kernels behind `strling pull` (strling_amd/csrc/pull.hip: pull_select_kernel, pull_keys_kernel +
pull_count_kernel, pull_mate_kernel + pull_mate_rows_kernel, pull_copy_kernel) on their edges, and a plain-Python model of what
strl_pull_select and strl_pull_mates must answer.

Plain builders, no GPU code; the builders of tests/region_cases.py (R, records, fill, header_only, patch, Call.add_set) make
the bytes, and its walk() gives the range [s0, s1) a request yields.  A call is one strl_pull_select (its cases are TILES) or
one strl_pull_mates (its cases are WINDOWS with their requests).  A case has a family -- t tile, batches and prefix; w the walk's
LDS window; k keep rule and stop; h hash collisions and the request table; q request rounds and the mate rule; m malformed;
c the copy -- a name and a WITNESS: a predicate over the model's trace that proves the case reaches the edge it is named for.

The model restates, record by record: the walk of pl_walk (batches of 256, the 4 KiB window), select (kept rows in file order
through the per-wave counts and the running prefix), the counts over name bytes, the mates (256 requests a round in a table of
1024 slots, the first match in file order), the rows and the gather (at = align16(at) + (off & 15)).  Each part takes a `mut`
that breaks it the way a wrong kernel would be broken (MUTATIONS; "ge" is `>=` for `>` at an interval's beg, "end_le" `<=` for `<`
at its end, "no_len" the mate rule without its compare of the names' lengths), so that tests/test_pull_cases.py can show on the CPU which
case tells each break apart; tests/test_pull_edges_device.py sends the same calls to the device.
"""
import functools
import struct
import zlib

import numpy as np

import region_cases as rc
from region_cases import FAR, INT32_MAX, R, fill, header_only, patch, records

PL_WIN, PL_BATCH, PL_TAB_REQ, PL_TAB_SLOTS = 4096, 256, 256, 1024
COPY_ROWS = 2048 * 4          # the rows one turn of pull_copy_kernel's grid takes
INT32_MIN = -2 ** 31
M32 = 0xFFFFFFFF
ROW_FIELDS = ("off", "tid", "pos", "mtid", "mpos", "size", "hash", "flag", "l_name", "found", "count")
ZERO_ROW = (0,) * len(ROW_FIELDS)
MUTATIONS = ("no_running", "wcnt_wrong_wave", "win_lt", "no_wrap", "first_hash", "max", "ge", "end_le", "no_len", "l_name", "no_grid_loop", "no_head")


# ---- Nim's hash of a string (MurmurHash3_x86_32, seed 0), one name and many names of one length ---------------------------------
def murmur(b):
    rotl = lambda x, r: ((x << r) | (x >> (32 - r))) & M32      # noqa: E731
    h, n = 0, len(b) & ~3
    for i in range(0, n, 4):
        k = int.from_bytes(b[i:i + 4], "little")
        k = rotl(k * 0xcc9e2d51 & M32, 15) * 0x1b873593 & M32
        h = (rotl(h ^ k, 13) * 5 + 0xe6546b64) & M32
    k = int.from_bytes(b[n:], "little")
    h ^= rotl(k * 0xcc9e2d51 & M32, 15) * 0x1b873593 & M32
    h ^= len(b)
    h ^= h >> 16
    h = h * 0x85ebca6b & M32
    h ^= h >> 13
    h = h * 0xc2b2ae35 & M32
    return h ^ (h >> 16)


def murmur_many(a):
    """a = uint8[n, L] -> uint32[n]"""
    a = np.ascontiguousarray(a, np.uint8)
    n, L = a.shape
    m = np.uint64(M32)
    rotl = lambda x, r: ((x << np.uint64(r)) | (x >> np.uint64(32 - r))) & m      # noqa: E731
    mix = lambda k: (rotl((k * np.uint64(0xcc9e2d51)) & m, 15) * np.uint64(0x1b873593)) & m      # noqa: E731
    h = np.zeros(n, np.uint64)
    for i in range(0, L & ~3, 4):
        k = a[:, i:i + 4].copy().view("<u4")[:, 0].astype(np.uint64)
        h = (rotl(h ^ mix(k), 13) * np.uint64(5) + np.uint64(0xe6546b64)) & m
    k = np.zeros(n, np.uint64)
    for j in range(L - 1, (L & ~3) - 1, -1):
        k = (k << np.uint64(8)) | a[:, j].astype(np.uint64)
    h ^= mix(k)
    h ^= np.uint64(L)
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85ebca6b)) & m
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xc2b2ae35)) & m
    return (h ^ (h >> np.uint64(16))).astype(np.uint32)


def home(h):
    """the home slot of a hash in pull_mate_kernel's table"""
    return ((h * 0x9E3779B1) & M32) >> 22


def _names(prefix, digits, n):
    a = np.empty((n, 1 + digits), np.uint8)
    a[:, 0] = prefix
    i = np.arange(n, dtype=np.int64)
    for d in range(digits):
        a[:, 1 + d] = 48 + (i // 10 ** (digits - 1 - d)) % 10
    return a


@functools.lru_cache(maxsize=None)
def colliding():
    """over 2^20 names "r0000000" .. of 8 bytes and 2^20 names "s00000000" .. of 9: pairs of 8-byte names with one hash, pairs of
    an 8- and a 9-byte name with one hash, and the 8-byte names by home slot"""
    n = 1 << 20
    a8, a9 = _names(ord("r"), 7, n), _names(ord("s"), 8, n)
    h8, h9 = murmur_many(a8), murmur_many(a9)
    order = np.argsort(h8, kind="stable")
    hs = h8[order]
    at = np.flatnonzero(hs[1:] == hs[:-1])
    same = [(a8[order[i]].tobytes(), a8[order[i + 1]].tobytes()) for i in at]
    both, i8, i9 = np.intersect1d(h8, h9, return_indices=True)
    mixed = [(a8[i].tobytes(), a9[j].tobytes()) for i, j in zip(i8, i9)]
    hm = ((h8.astype(np.uint64) * np.uint64(0x9E3779B1)) & np.uint64(M32)) >> np.uint64(22)
    by_home = lambda s: [a8[i].tobytes() for i in np.flatnonzero(hm == s)]      # noqa: E731
    return dict(same=same, mixed=mixed, home1023=by_home(1023), home512=by_home(512))


# ---- a record as pull_rec.h reads it ------------------------------------------------------------------------------------------------
def plausible(u, p, left):
    """pl_plausible"""
    if left < 36:
        return False
    bs = struct.unpack_from("<I", u, p)[0]
    if bs < 32 or bs > 1 << 28 or 4 + bs > left:
        return False
    l_name, n_cig = u[p + 12], struct.unpack_from("<H", u, p + 16)[0]
    l_seq = struct.unpack_from("<i", u, p + 20)[0]
    return l_seq >= 0 and 32 + l_name + 4 * n_cig + (l_seq + 1) // 2 <= bs


class Rec:
    """PlRec"""
    def __init__(self, u, p):
        self.p = p
        self.bs, self.tid, self.pos, self.l_name = struct.unpack_from("<IiiB", u, p)
        self.n_cig, self.flag = struct.unpack_from("<HH", u, p + 16)
        self.mtid, self.mpos = struct.unpack_from("<ii", u, p + 24)
        self.name_len = self.l_name - 1 if self.l_name else 0
        self.name = bytes(u[p + 36:p + 36 + self.name_len])
        rl = 0
        if not self.flag & 4:
            for c in struct.unpack_from(f"<{self.n_cig}I", u, p + 36 + self.l_name):
                if c & 15 in (0, 2, 3, 7, 8):
                    rl += c >> 4
        self.stop = self.pos + (rl or 1)                          # 64-bit in PlRec::stop

    def kept_by(self, T, mut=None):
        tid, beg, end, own_beg, own_end = T
        reach = self.stop >= beg if mut == "ge" else self.stop > beg
        before = self.pos <= end if mut == "end_le" else self.pos < end
        return self.tid == tid and before and not self.flag & 0x900 and own_beg <= self.pos < own_end and reach

    def row(self, h, count=0):
        return (self.p, self.tid, self.pos, self.mtid, self.mpos, 4 + self.bs, h, self.flag, self.l_name, 1, count)


class Walker:
    """pl_walk: the state that outlives a batch (p, w0, w1) and every window loaded: wins = [(w0, w1, p, w1 before)]"""
    def __init__(self, call, s0, s1, wins, mut=None):
        self.call, self.s0, self.s1, self.p, self.w0, self.w1, self.wins, self.mut = call, s0, s1, s0, 0, 0, wins, mut

    def batch(self):
        """-> (the offsets of up to 256 records, status 0 or 2)"""
        u, readable, offs = self.call.padded, (self.call.tot + 64) & ~15, []
        while len(offs) < PL_BATCH and self.p < self.s1:
            p = self.p
            if p + 36 > self.s1:
                return offs, 2
            if p < self.w0 or (p + 36 >= self.w1 if self.mut == "win_lt" else p + 36 > self.w1):
                before = self.w1
                self.w0 = p & ~15
                self.w1 = min(self.w0 + PL_WIN, readable) & ~15
                self.wins.append((self.w0, self.w1, p, before))
                if p + 36 > self.w1:
                    return offs, 2
            if not plausible(u, p, self.s1 - p):
                return offs, 2
            offs.append(p)
            self.p = p + 4 + struct.unpack_from("<I", u, p)[0]
        return offs, 0

    @property
    def more(self):
        return self.p < self.s1


class Trace:
    """what the model did for one tile or window: walk (region_cases.walk's trace of the request), status, s0 and s1, wins (every
    load of the 4 KiB window), batches = [(records, [kept of wave 0..3], more)] (select; of a window: of its first round), recs =
    the records walked, kept (select: the kept records), rounds = [(requests, occupied slots, longest probe of a record, the slots
    a probe that met a request passed)] (mates), folded = answers folded into ans[] before the status was known"""
    def __init__(self):
        self.status, self.s0, self.s1, self.wins, self.batches, self.recs, self.kept, self.rounds, self.folded = 0, 0, 0, [], [], [], [], [], 0


# ---- select ------------------------------------------------------------------------------------------------------------------------
def select_tile(call, req, tile, mut=None):
    """pull_select_kernel for one tile -> (trace, rows without count, or [] with status != 0).  The rows stand where the kernel's
    prefix puts them: place = running + the kept of the waves in front + the kept lanes in front within the wave, written only
    below the count of the first launch; a place no record took stays ZERO_ROW"""
    t = Trace()
    t.walk = rc.walk(call, req)
    t.status = t.walk.status
    if t.status:
        return t, []
    t.s0, t.s1 = s0, s1 = t.walk.keep, t.walk.stop
    W = Walker(call, s0, s1, t.wins, mut)
    running, placed = 0, []
    while True:
        offs, st = W.batch()
        if st:
            t.status = 2
            return t, []
        rs = [Rec(call.padded, p) for p in offs]
        kept = [r.kept_by(tile, mut) for r in rs]
        wcnt = [sum(kept[64 * w:64 * w + 64]) for w in range(4)]
        t.batches.append((len(offs), wcnt, W.more))
        t.recs += rs
        for i, (r, k) in enumerate(zip(rs, kept)):
            if k:
                wave = i >> 6
                front = [wcnt[(w + 1) % 4] for w in range(wave)] if mut == "wcnt_wrong_wave" else wcnt[:wave]
                placed.append(((0 if mut == "no_running" else running) + sum(front) + sum(kept[64 * wave:i]), r))
                t.kept.append(r)
        running += sum(wcnt)
        if not W.more:
            break
    rows = [ZERO_ROW] * running
    for k, r in placed:
        if k < running:
            rows[k] = r.row(murmur(r.name))
    return t, rows


def counted(call, rows, mut=None):
    """pull_count_kernel: count = rows of the call with the same name bytes; mut "l_name": ... with the same l_read_name too"""
    u, keys = call.padded, []
    for r in rows:
        l_name = r[8]
        keys.append((l_name if mut == "l_name" else 0, bytes(u[r[0] + 36:r[0] + 36 + max(0, l_name - 1)])))
    n = {}
    for k in keys:
        n[k] = n.get(k, 0) + 1
    return [r[:10] + (n[k],) for r, k in zip(rows, keys)]


def gather(call, rows, mut=None):
    """pull_gather + pull_copy_kernel: the found rows' records back to back, each at the next multiple of 16 plus its source's
    offset modulo 16 -> (rows with off = the offset in the bytes, the bytes; zeros where nothing is written).  mut "no_grid_loop":
    only the first COPY_ROWS records are copied; "no_head": not the bytes in front of the source's next multiple of 16"""
    at, out, items = 0, [], []
    for r in rows:
        if r[9]:
            at = ((at + 15) & ~15) + (r[0] & 15)
            items.append((r[0], at, r[5]))
            out.append((at,) + r[1:])
            at += r[5]
        else:
            out.append(r)
    data = bytearray(at)
    for i, (src, dst, n) in enumerate(items):
        if mut == "no_grid_loop" and i >= COPY_ROWS:
            break
        head = min((16 - (src & 15)) & 15, n) if mut == "no_head" else 0
        data[dst + head:dst + n] = call.u[src + head:src + n]
    return out, bytes(data)


# ---- mates -------------------------------------------------------------------------------------------------------------------------
def mate_window(call, req, reqs, mut=None):
    """pull_mate_kernel + pull_mate_rows_kernel for one window; reqs = [(hash, beg, end, name, flag)] -> (trace, a row per request).
    The table: 256 requests a round, each from its home slot on to the first free slot (the slots taken do not depend on the
    order); a record goes from its hash's home slot to the first free slot and meets every request on the way"""
    t = Trace()
    t.walk = rc.walk(call, req)
    t.status = t.walk.status
    zero = [ZERO_ROW] * len(reqs)
    if t.status:
        return t, zero
    t.s0, t.s1 = s0, s1 = t.walk.keep, t.walk.stop
    tid, ans = req[3], [None] * len(reqs)
    for r0 in range(0, len(reqs), PL_TAB_REQ):
        slot = [-1] * PL_TAB_SLOTS
        m = min(PL_TAB_REQ, len(reqs) - r0)
        for k in range(m):
            at = home(reqs[r0 + k][0])
            while slot[at] != -1:
                at = (at + 1) & (PL_TAB_SLOTS - 1)
            slot[at] = k
        wins, longest, passed = [], 0, set()
        W = Walker(call, s0, s1, wins, mut)
        while True:
            offs, st = W.batch()
            if st:
                t.status, t.folded = 2, sum(a is not None for a in ans)
                t.wins += wins
                return t, zero
            rs = [Rec(call.padded, p) for p in offs]
            if r0 == 0:
                t.batches.append((len(offs), None, W.more))
                t.recs += rs
            for r in rs:
                if r.flag & 0x900 or r.tid != tid:
                    continue
                h, at, walked, met = murmur(r.name), home(murmur(r.name)), [], False
                while at < PL_TAB_SLOTS and slot[at] >= 0:
                    walked.append(at)
                    k = r0 + slot[at]
                    qh, qbeg, qend, qname, qflag = reqs[k]
                    at = at + 1 if mut == "no_wrap" else (at + 1) & (PL_TAB_SLOTS - 1)
                    if qh != h:
                        continue
                    reach = r.stop >= qbeg if mut == "ge" else r.stop > qbeg
                    before = r.pos <= qend if mut == "end_le" else r.pos < qend
                    same = qname[:r.name_len] == r.name if mut == "no_len" else len(qname) == r.name_len and qname == r.name
                    if (qflag ^ r.flag) & 0x40 and before and reach and same:
                        met = True
                        ans[k] = r.p if ans[k] is None else (max if mut == "max" else min)(ans[k], r.p)
                    if mut == "first_hash":
                        break
                longest = max(longest, len(walked))
                if met:
                    passed |= set(walked)
            if not W.more:
                break
        t.wins += wins
        t.rounds.append((m, {i for i, e in enumerate(slot) if e >= 0}, longest, passed))
    rows = [ZERO_ROW if a is None else Rec(call.padded, a).row(q[0]) for a, q in zip(ans, reqs)]
    return t, rows


# ---- calls -------------------------------------------------------------------------------------------------------------------------
class Case(rc.Case):
    """req = the request of strl_regions_fetch's kind; tile = (tid, beg, end, own_beg, own_end) or reqs = the window's requests"""
    def __init__(self, call, family, name, req, witness, tile=None, reqs=None):
        super().__init__(call, family, name, req, witness)
        self.tile, self.reqs = tile, reqs


class Call(rc.Call):
    kind = None

    def case(self, family, name, req, witness, **kw):
        self.cases.append(Case(self, family, name, tuple(req), witness, **kw))

    def whole_set(self, fb, tid=0):
        """the request that takes every record of the set that begins with block fb, up to its stopper"""
        return (fb, len(self.blocks) - fb, 0, tid, 0, INT32_MAX)

    def lay(self):
        if "_pulled" not in self.__dict__:
            self.isize = [len(b) for b in self.blocks]
            self.uoff = rc.offsets(self.blocks)[:-1]
            self.u = b"".join(self.blocks)
            self.padded = self.u + bytes(64)
            self.streams = [rc.deflate(b) for b in self.blocks]
            self.crcs = [zlib.crc32(b) for b in self.blocks]
            self.requests = [c.req for c in self.cases]
            self.answer = self.model()
            self._pulled = True
        return self


class SelectCall(Call):
    kind = "select"

    def model(self, mut=None):
        """-> dict(traces, status, tile_rows, src (rows with off in the call's bytes), rows (off in the gathered bytes), data)"""
        traces, status, tile_rows, rows = [], [], [0], []
        for c in self.cases:
            t, r = select_tile(self, c.req, c.tile, mut)
            traces.append(t)
            status.append(t.status)
            rows += r
            tile_rows.append(len(rows))
        src = counted(self, rows, mut)
        out, data = gather(self, src, mut)
        return dict(traces=traces, status=status, tile_rows=tile_rows, src=src, rows=out, data=data)


class MateCall(Call):
    kind = "mates"

    def lay(self):
        if "_pulled" not in self.__dict__:
            self.win_off, self.names, self.reqs = [0], b"", []
            for c in self.cases:
                for h, beg, end, name, flag in c.reqs:
                    self.reqs.append((h, beg, end, len(self.names), flag, len(name), 0))
                    self.names += name
                self.win_off.append(len(self.reqs))
        return super().lay()

    def model(self, mut=None):
        traces, status, rows = [], [], []
        for c in self.cases:
            t, r = mate_window(self, c.req, c.reqs, mut)
            traces.append(t)
            status.append(t.status)
            rows += r
        out, data = gather(self, rows, mut)
        return dict(traces=traces, status=status, src=rows, rows=out, data=data)


STOPPER = rc.STOPPER
EVERY = (0, 0, INT32_MAX, INT32_MIN, INT32_MAX)        # the tile that keeps every primary record of reference 0


def _set(C, recs, cuts=(), align=None):
    """records (dicts of R, or ready-made bytes) and the stopper behind them -> (first block, the records' offsets in the call)"""
    pieces = list(recs) if all(isinstance(r, bytes) for r in recs) else records(recs)
    total = sum(len(p) for p in pieces)
    pieces = pieces + records([STOPPER])
    fb, off = C.add_set(pieces, [c for c in cuts if c <= total], align=align)
    base = C.tot - off[-1]
    return fb, [base + o for o in off]


def names_of(t):
    return [r.name for r in t.kept]


def no_name(rec):
    """the record without its name's NUL: l_read_name 0"""
    assert rec[12] == 1
    b = bytearray(rec[:36] + rec[37:])
    struct.pack_into("<I", b, 0, len(b) - 4)
    b[12] = 0
    return bytes(b)


def S(pos, name, flag=0, cigar="2M", **kw):
    """a short record"""
    return R(pos, cigar, name=name, flag=flag, **kw)


# ---- t. a tile's batches and the kept-row prefix ------------------------------------------------------------------------------------
def family_t():
    C = SelectCall("t")
    for n in (0, 1, 255, 256, 257, 512):
        fb, off = _set(C, [S(1000 + i, b"t%d_%d" % (n, i), flag=0x100 if i % 5 == 3 else 0) for i in range(n)], cuts=[1500, 9000], align=(3 * n) % 16)
        C.case("t", f"records-{n}", C.whole_set(fb),
               lambda t, c, n=n: t.status == 0 and [b[0] for b in t.batches] == ([256] * (n // 256) + [n % 256] if n % 256 or not n else [256] * (n // 256))
               and [b[2] for b in t.batches] == [True] * (len(t.batches) - 1) + [False] and len(t.kept) == n - len(range(3, n, 5)), tile=EVERY)
    # wave 0 keeps nothing, wave 3 everything, the two between them one lane in three and all but one lane in seven
    keep = lambda i: i >= 192 or (64 <= i < 128 and i % 3 == 0) or (128 <= i < 192 and i % 7 != 0)      # noqa: E731
    fb, off = _set(C, [S(2000 + i, b"w%d" % i, flag=0 if keep(i) else 0x800) for i in range(256)], cuts=[4000], align=5)
    C.case("t", "wave0-empty-wave3-full", C.whole_set(fb), lambda t, c, keep=keep: t.status == 0 and [b[1] for b in t.batches] == [[sum(keep(i) for i in range(64 * w, 64 * w + 64)) for w in range(4)]]
           and t.batches[0][1][0] == 0 and t.batches[0][1][3] == 64 and len(set(t.batches[0][1])) == 4, tile=EVERY)
    # alternating lanes over three batches, the last one short; every wave's count differs from its neighbour's in the last batch
    keep = lambda i: i % 2 == 1 if i < 512 else (i - 512) % 64 < 10 * ((i - 512) // 64 + 1)      # noqa: E731
    fb, off = _set(C, [S(3000 + i, b"a%d" % i, flag=0 if keep(i) else 0x100) for i in range(700)], cuts=[7000, 7001, 20000], align=9)
    C.case("t", "alternating-three-batches", C.whole_set(fb),
           lambda t, c: t.status == 0 and [b[:2] for b in t.batches] == [(256, [32] * 4), (256, [32] * 4), (188, [10, 20, 30, 0])], tile=EVERY)
    # a first batch that keeps nothing: the second batch's rows start at place 0 with or without the running count
    fb, off = _set(C, [S(4000 + i, b"e%d" % i, flag=0x100 if i < 256 else 0) for i in range(300)], align=1)
    C.case("t", "first-batch-empty", C.whole_set(fb), lambda t, c: t.status == 0 and [b[1] for b in t.batches] == [[0] * 4, [44, 0, 0, 0]], tile=EVERY)
    return C


# ---- w. the walk's LDS window ------------------------------------------------------------------------------------------------------
def family_w():
    C = SelectCall("w")
    for j in range(16):
        fb, off = _set(C, [S(1000 + i, b"m%d_%d" % (j, i) + b"n" * ((i * 5 + j) % 16)) for i in range(6)], align=j)
        C.case("w", f"tile-start-mod16-{j}", C.whole_set(fb),
               lambda t, c, j=j: t.status == 0 and t.s0 % 16 == j and t.wins[0][:3] == (t.s0 - j, t.s0 - j + PL_WIN, t.s0) and len(t.kept) == 6, tile=EVERY)
    # a header that ends d bytes behind the window's end; with d = 0 it ends with the window and is read without a reload
    for d in (0, 1, 35):
        recs = fill(PL_WIN - 36 + d, 1000) + [S(2000, b"X"), S(2010, b"Y")]
        fb, off = _set(C, recs, cuts=[1501], align=0)
        x = off[len(recs) - 2]
        if d:
            wit = lambda t, c, d=d, x=x: t.status == 0 and len(t.wins) == 2 and t.wins[1][2] == x and x + 36 - t.wins[1][3] == d and names_of(t)[-2:] == [b"X", b"Y"]
        else:
            wit = lambda t, c, x=x: t.status == 0 and x + 36 == t.wins[0][1] and all(w[2] != x for w in t.wins) and len(t.wins) == 2 and names_of(t)[-2:] == [b"X", b"Y"]
        C.case("w", f"header-ends-{d}-behind-w1", C.whole_set(fb), wit, tile=EVERY)
    # a record longer than the window: the next header lies behind the window, not across its end
    recs = fill(500, 1000) + [R(2000, "3000M", name=b"X"), S(2010, b"Y")]
    fb, off = _set(C, recs, cuts=[2222], align=7)
    C.case("w", "record-longer-than-window", C.whole_set(fb),
           lambda t, c: t.status == 0 and any(w[2] >= w[3] > 0 for w in t.wins) and max(4 + r.bs for r in t.kept) > PL_WIN and names_of(t)[-2:] == [b"X", b"Y"], tile=EVERY)
    return C


# ---- k. PlRec::kept_by and PlRec::stop ---------------------------------------------------------------------------------------------
def _op9(rec, j, n):
    """CIGAR operation j of the record becomes n x operation 9"""
    return patch(rec, 36 + rec[12] + 4 * j, "<I", (n << 4) | 9)


def family_k():
    C = SelectCall("k")
    recs = [S(970, b"stop-is-beg", cigar="30M"), S(971, b"stop-is-beg-plus-1", cigar="30M"),
            S(970, b"unmapped-with-cigar", cigar="40M", flag=0x4), S(1000, b"unmapped-at-beg", cigar="40M", flag=0x4),
            S(999, b"only-30S", cigar="30S"), S(999, b"only-10I", cigar="10I"), S(1000, b"only-30S-at-beg", cigar="30S")]
    recs += [S(990, b"counts-" + op.encode(), cigar="5M6" + op) for op in "=XDN"]
    recs += [S(990, b"counts-not-" + op.encode(), cigar="9M5" + op) for op in "HPIS"]
    recs = records(recs) + [_op9(records([S(990, b"counts-not-9", cigar="9M5M")])[0], 1, 5)]
    recs += records([S(1400, b"flag-0x100", flag=0x100), S(1400, b"flag-0x800", flag=0x800), S(1400, b"flag-0x400", flag=0x400),
                     S(1499, b"own-beg-minus-1"), S(1500, b"own-beg"), S(1599, b"own-end-minus-1"), S(1600, b"own-end"),
                     S(1999, b"pos-is-end-minus-1"), S(2000, b"pos-is-end")])
    recs.append(patch(records([S(5, b"near-2-to-31", cigar="100M")])[0], 8, "<i", 2 ** 31 - 10))
    fb, off = _set(C, recs, cuts=[700], align=6)
    inside = [b"flag-0x400", b"own-beg-minus-1", b"own-beg", b"own-end-minus-1", b"own-end", b"pos-is-end-minus-1"]
    reach = [b"stop-is-beg-plus-1", b"unmapped-at-beg", b"only-30S-at-beg"] + [b"counts-" + op for op in (b"=", b"X", b"D", b"N")]
    # the tile owns every position, so `pos < end` alone drops pos-is-end: it is of the tile's reference, primary, owned, and reaches beg
    region = (0, 1000, 2000, INT32_MIN, INT32_MAX)

    def by_end_alone(t, name, tile=region):
        tid, beg, end, own_beg, own_end = tile
        r = next(r for r in t.recs if r.name == name)
        return r.pos == end and r.tid == tid and not r.flag & 0x900 and own_beg <= r.pos < own_end and r.stop > beg and r not in t.kept
    C.case("k", "the-region", C.whole_set(fb), lambda t, c, n=len(recs): t.status == 0 and names_of(t) == reach + inside and len(t.recs) == n
           and by_end_alone(t, b"pos-is-end") and next(r for r in t.kept if r.name == b"pos-is-end-minus-1").pos == 1999, tile=region)
    C.case("k", "own-range", C.whole_set(fb), lambda t, c: t.status == 0 and names_of(t) == [b"own-beg", b"own-end-minus-1"], tile=(0, 1000, 2000, 1500, 1600))
    # stop = 2^31 + 90 is behind beg only as a 64-bit number
    C.case("k", "stop-leaves-32-bits", C.whole_set(fb), lambda t, c: t.status == 0 and names_of(t) == [b"near-2-to-31"] and t.kept[0].stop == 2 ** 31 + 90,
           tile=(0, 2 ** 31 - 5, INT32_MAX, INT32_MIN, INT32_MAX))
    C.case("k", "another-reference", C.whole_set(fb), lambda t, c, n=len(recs): t.status == 0 and not t.kept and len(t.recs) == n, tile=(1, 0, INT32_MAX, INT32_MIN, INT32_MAX))
    return C


# ---- h. names with one hash; the request table ---------------------------------------------------------------------------------------
def family_h():
    K = colliding()
    (a, b), (a2, b2), (c8, c9) = K["same"][0], K["same"][1], K["mixed"][0]
    C = SelectCall("h")
    two = lambda t, x, y: murmur(x) == murmur(y) and x != y and {x, y} <= set(names_of(t))      # noqa: E731
    fb, off = _set(C, [S(1000, a), S(1001, b), S(1002, b"other")], align=2)
    C.case("h", "same-length", C.whole_set(fb), lambda t, c: two(t, a, b) and len(a) == len(b), tile=EVERY)
    fb, off = _set(C, [S(1000, c8), S(1001, c9), S(1002, c9), S(1003, c9)], align=3)
    C.case("h", "different-lengths", C.whole_set(fb), lambda t, c: two(t, c8, c9) and (len(c8), len(c9)) == (8, 9), tile=EVERY)
    fb, off = _set(C, [S(1000 + i, (a2, b2)[i % 2]) for i in range(5)], align=4)
    C.case("h", "interleaved-A-B-A-B-A", C.whole_set(fb), lambda t, c: two(t, a2, b2) and names_of(t) == [a2, b2, a2, b2, a2], tile=EVERY)
    # l_read_name 0 and 1 both carry the name "": header_only has no name at all, the two others one NUL / not even that
    recs = [header_only(0, 1000), records([S(1001, b"")])[0], no_name(records([S(1002, b"")])[0]), records([S(1003, b"x")])[0]]
    fb, off = _set(C, recs, align=11)
    C.case("h", "empty-name-l0-and-l1", C.whole_set(fb), lambda t, c: [r.l_name for r in t.kept] == [0, 1, 0, 2] and names_of(t) == [b"", b"", b"", b"x"], tile=EVERY)
    return C


def _ask(name, mpos, flag=0x41):
    """the request of a kept record (flag, mate at mpos): get_mate's interval"""
    return (murmur(name), max(0, mpos - 1), mpos + 1, name, flag)


def family_hm():
    K = colliding()
    (a, b), (c8, c9) = K["same"][2], K["mixed"][1]
    C = MateCall("hm")
    found = lambda t: t.status == 0      # noqa: E731
    # both names of a collision ask in one window; B's mate lies in front of A's
    fb, off = _set(C, [S(1000, b"pad"), S(1010, b, flag=0x81), S(1020, a, flag=0x81), S(1030, c9, flag=0x81), S(1040, c8, flag=0x81)], align=5)
    C.case("h", "both-ask-in-one-window", (fb, len(C.blocks) - fb, 0, 0, 0, FAR),
           lambda t, c: found(t) and murmur(a) == murmur(b) and a != b and murmur(c8) == murmur(c9) and t.rounds[0][2] >= 2,
           reqs=[_ask(a, 1020), _ask(b, 1010), _ask(c8, 1040), _ask(c9, 1030)])
    # only A asks; B's record, with A's hash, is not A's mate
    fb, off = _set(C, [S(1010, b, flag=0x81), S(1011, c9, flag=0x81)], align=6)
    C.case("h", "the-other-name-alone", (fb, len(C.blocks) - fb, 0, 0, 0, FAR), lambda t, c: found(t) and t.rounds[0][2] == 1 and not t.rounds[0][3],
           reqs=[_ask(a, 1010), _ask(c8, 1011)])
    # three requests at home in slot 1023: they take 1023, 0 and 1
    hi = K["home1023"][:3]
    fb, off = _set(C, [S(1100 + i, n, flag=0x81) for i, n in enumerate(hi)], align=7)
    C.case("h", "chain-wraps-1023-to-0", (fb, len(C.blocks) - fb, 0, 0, 0, FAR),
           lambda t, c: found(t) and all(home(murmur(n)) == 1023 for n in hi) and t.rounds[0][1] == {1023, 0, 1} and {1023, 0, 1} <= t.rounds[0][3],
           reqs=[_ask(n, 1100 + i) for i, n in enumerate(hi)])
    # forty requests with one home slot
    mid = K["home512"][:40]
    fb, off = _set(C, [S(1200 + i, n, flag=0x81) for i, n in enumerate(mid)], align=8)
    C.case("h", "forty-at-one-home", (fb, len(C.blocks) - fb, 0, 0, 0, FAR),
           lambda t, c: found(t) and t.rounds[0][1] == set(range(512, 552)) and t.rounds[0][2] == 40, reqs=[_ask(n, 1200 + i) for i, n in enumerate(mid)])
    # one name asks twice, as read 1 and as read 2: each gets the other's record
    fb, off = _set(C, [S(1300, b"twice", flag=0x81), S(1301, b"twice", flag=0x41)], align=9)
    C.case("h", "same-name-both-read1-bits", (fb, len(C.blocks) - fb, 0, 0, 0, FAR), lambda t, c: found(t) and t.rounds[0][2] == 2,
           reqs=[_ask(b"twice", 1300, 0x41), _ask(b"twice", 1301, 0x81)])
    return C


# ---- q. request rounds and the mate rule -------------------------------------------------------------------------------------------
def family_q():
    C = MateCall("q")
    for n, n_rec in ((256, 200), (257, 300), (512, 100)):
        # every third request has no mate in the window; the mates lie in reverse order of the requests
        recs = [S(1000 + i, b"q%d_%d" % (n, (n_rec - 1 - i) * 3 % n), flag=0x81) for i in range(n_rec)]
        fb, off = _set(C, recs, cuts=[5000], align=n % 16)
        reqs = [_ask(b"q%d_%d" % (n, k), 1000 + n_rec // 2) for k in range(n)]
        reqs = [(q[0], 0, FAR, q[3], q[4]) for q in reqs]
        C.case("q", f"requests-{n}", (fb, len(C.blocks) - fb, 0, 0, 0, FAR),
               lambda t, c, n=n, n_rec=n_rec: t.status == 0 and [r[0] for r in t.rounds] == ([256] * (n // 256) + ([n % 256] if n % 256 else []))
               and sum(b[0] for b in t.batches) == n_rec, reqs=reqs)
    # two primaries meet one request: in two waves of one batch, and in two batches
    for name, second in (("two-waves", 100), ("two-batches", 300)):
        recs = [S(2000 + i, b"first" if i in (10, second) else b"f%d" % i, flag=0x81) for i in range(second + 5)]
        fb, off = _set(C, recs, align=3)
        C.case("q", f"first-match-{name}", (fb, len(C.blocks) - fb, 0, 0, 0, FAR),
               lambda t, c, second=second: t.status == 0 and [r.name for r in t.recs].count(b"first") == 2 and len(t.batches) == 1 + second // 256,
               reqs=[(murmur(b"first"), 0, FAR, b"first", 0x41)])
    # the interval's edges, the READ1 bit of a request with neither 0x40 nor 0x80, names of 0, 1 and 254 bytes
    long = b"L" * 253
    recs = records([S(970, b"stop-is-beg", cigar="30M", flag=0x81), S(971, b"stop-is-beg-plus-1", cigar="30M", flag=0x81),
                    S(1001, b"pos-is-end-minus-1", flag=0x81), S(1002, b"pos-is-end", flag=0x81),
                    S(1001, b"no-read-bits", flag=0x81), S(1001, b"no-read-bits", flag=0x1), S(1001, b"no-read-bits", flag=0x41),
                    S(1001, b"same-read1-bit", flag=0x41), S(1001, b"secondary", flag=0x181), S(1001, b"supplementary", flag=0x881)])
    recs += [no_name(records([S(1001, b"", flag=0x81)])[0]), records([S(1001, b"", flag=0x81)])[0]]
    recs += records([S(1001, b"x", flag=0x81), S(1001, long + b"b", flag=0x81), S(1001, long + b"a", flag=0x81), S(1001, long, flag=0x81)])
    fb, off = _set(C, recs, cuts=[600], align=13)
    names = [b"stop-is-beg", b"stop-is-beg-plus-1", b"pos-is-end-minus-1", b"pos-is-end", b"same-read1-bit", b"secondary", b"supplementary", b"", b"x", long + b"a", long]
    C.case("q", "rule-edges", (fb, len(C.blocks) - fb, 0, 0, 0, FAR), lambda t, c, n=len(recs): t.status == 0 and len(t.recs) == n,
           reqs=[(murmur(n), 1000, 1002, n, 0x41) for n in names] + [(murmur(b"no-read-bits"), 1000, 1002, b"no-read-bits", 0x1)])
    # a record of another reference ends the window's bytes: the walk stops there, and the mate behind it is not in them
    recs = [S(1000, b"before", flag=0x81), S(1000, b"behind", flag=0x81, tid=1), S(1001, b"behind", flag=0x81)]
    fb, off = _set(C, recs, align=14)
    C.case("q", "another-reference-ends-the-window", (fb, len(C.blocks) - fb, 0, 0, 0, FAR),
           lambda t, c: t.status == 0 and t.walk.end == "ref" and [r.name for r in t.recs] == [b"before"] and Rec(c.padded, t.s1).name == b"behind",
           reqs=[_ask(b"before", 1000), _ask(b"behind", 1001)])
    return C


# ---- m. bytes that do not parse ------------------------------------------------------------------------------------------------------
BAD = {"block-size-31": lambda r: patch(r, 0, "<I", 31), "l-seq-negative": lambda r: patch(r, 20, "<i", -2), "seq-leaves-record": lambda r: patch(r, 20, "<i", 100_000)}


def _m_sets(C, flag):
    """per malformation: a set whose first record is bad, a set whose record 300 is, and good sets around them"""
    out = []
    for k, (name, bad) in enumerate(BAD.items()):
        for at in (0, 300):
            recs = records([S(1000 + i, b"m%d_%d" % (k, i), flag=flag) for i in range(at + 3)])
            recs[at] = bad(recs[at])
            fb, off = _set(C, recs, cuts=[900], align=(5 * k + at) % 16)
            out.append((f"{name}-{'first-record' if at == 0 else 'second-batch'}", fb, at, k))
        fb, off = _set(C, [S(1000 + i, b"good%d_%d" % (k, i), flag=flag) for i in range(4)], align=k)
        out.append((f"good-tile-{k}", fb, None, k))
    return out


def family_m():
    C = SelectCall("m")
    for name, fb, at, k in _m_sets(C, 0):
        if at is None:
            wit = lambda t, c: t.status == 0 and len(t.kept) == 4      # noqa: E731
        elif k == 0:           # the walk in front of the pull kernels refuses a block_size below 32 itself: status 1
            wit = lambda t, c, at=at: t.status == 1 and t.walk.end == "bad-size" and len(t.walk.recs) == at      # noqa: E731
        else:
            wit = lambda t, c, at=at: t.status == 2 and sum(b[0] for b in t.batches) == at - at % 256 and len(t.batches) == at // 256      # noqa: E731
        C.case("m", name, C.whole_set(fb), wit, tile=EVERY)
    return C


def family_mm():
    C = MateCall("mm")
    for name, fb, at, k in _m_sets(C, 0x81):
        if at is None:
            wit = lambda t, c: t.status == 0      # noqa: E731
            reqs = [_ask(b"good%d_%d" % (k, i), 1000 + i) for i in range(4)]
        else:
            # the answers of the first batch are folded into ans[] before the second batch's bad record is met
            if k == 0:
                wit = lambda t, c: t.status == 1 and t.walk.end == "bad-size"      # noqa: E731
            else:
                wit = lambda t, c, at=at: t.status == 2 and t.folded == (2 if at else 0)      # noqa: E731
            reqs = [_ask(b"m%d_%d" % (k, i), 1000 + i) for i in (1, 2, at + 1)]
        C.case("m", name, (fb, len(C.blocks) - fb, 0, 0, 0, FAR), wit, reqs=reqs)
    return C


# ---- c. the copy -------------------------------------------------------------------------------------------------------------------
def family_c():
    C = SelectCall("c")
    recs = records([S(1000 + i, b"c" * ((i * 11 + i // 16) % 17) + b"%d" % i) for i in range(96)])
    recs[40:40] = [header_only(0, 1040)]
    recs[70:70] = records([R(1070, "1000M", name=b"long")])
    fb, off = _set(C, recs, cuts=[1000, 3001], align=0)

    def wit(t, c):
        src = [(r.p % 16, 4 + r.bs) for r in t.kept]
        tails = {(n - min((16 - a) % 16, n)) % 16 for a, n in src}
        return t.status == 0 and {a for a, _ in src} == set(range(16)) and tails == set(range(16)) and any(n == 36 for _, n in src) and any(n > 1040 + 15 for _, n in src)
    C.case("c", "alignments-tails-and-sizes", C.whole_set(fb), wit, tile=EVERY)
    return C


def family_c_grid():
    """one tile of 8200 short records: the copy's grid of 2048 workgroups of four waves takes a second turn"""
    C = SelectCall("c-grid")
    fb, off = _set(C, [S(1000 + i, b"g%d" % i, cigar="1M") for i in range(COPY_ROWS + 8)], cuts=range(65000, 400000, 65000), align=0)
    C.case("c", "more-rows-than-the-grid", C.whole_set(fb), lambda t, c: t.status == 0 and len(t.kept) == COPY_ROWS + 8 and c.tot < 1_000_000, tile=EVERY)
    return C


def cli_records():
    """the edges of t and h as the records of one coordinate-sorted file, for `strling pull` itself over chr1:1-131072: the
    16 KiB windows 0 .. 5 hold 0, 1, 255, 256, 257 and 512 records (pairs by name, every fifth record secondary, so that some
    names are kept once and ask for a mate that is no primary), window 6 alternating lanes over three batches whose mates do not
    exist, window 7 the names with one hash -- two of one length, an 8- and a 9-byte one, three at home in slot 1023, forty at
    home in slot 512 -- whose mates share one window far behind the region, and A B A B of one hash kept twice each"""
    from evidence_cases import rd
    W, out = 1 << 14, []
    rec = lambda pos, name, flag, mpos: rd(pos, "20M", None, name, flag=flag, tid=0, mtid=0, mpos=mpos)      # noqa: E731
    for w, n in enumerate((0, 1, 255, 256, 257, 512)):
        for i in range(n):
            out.append(rec(w * W + 100 + i, b"t%d_%d" % (n, i // 2), (0x81 if i % 2 else 0x41) | (0x100 if i % 5 == 3 else 0), w * W + 100 + (i ^ 1)))
    for i in range(700):
        out.append(rec(6 * W + 100 + i, b"a%d" % i, 0x41 if i % 2 else 0x141, 40 * W + i))
    K = colliding()
    names = list(K["same"][0]) + list(K["mixed"][0]) + K["home1023"][:3] + K["home512"][:40]
    for i, nm in enumerate(names):
        out += [rec(7 * W + 100 + i, nm, 0x41, 30 * W + 500 - i), rec(30 * W + 500 - i, nm, 0x81, 7 * W + 100 + i)]
    for i in range(4):
        out.append(rec(7 * W + 200 + i, K["same"][1][i % 2], 0x41 if i < 2 else 0x81, 7 * W + 200 + (i + 2) % 4))
    out += [rec(60 * W, b"filler_end", 0x41, 60 * W + 100), rec(60 * W + 100, b"filler_end", 0x81, 60 * W)]      # (the index bounds the mates' window)
    out.append(rd(10, "20M", None, b"stop", tid=1))
    return sorted(out, key=lambda r: (r["tid"], r["pos"])), [(0, 0, 8 * W)], ["chr1:1-131072"]


def cli_fallback_records():
    """a mates' window whose bytes do not parse, in a file `strling pull` itself can still answer: the reads A, B and C of the
    region chr1:1-16384 have their mates far behind it.  A's and B's share the 16 KiB window 20, whose query ends at B's mate + 1;
    a record with l_seq -2 ("bad", written without SEQ and QUAL) lies at B's mate's position behind B's mate, so it is inside the
    window's bytes: pl_walk meets it and answers status 2, while the host, which reads on only until every request is answered,
    never gets to it.  C's mate has window 25 to itself, which the device answers.  -> (records in file order, regions, the
    command's arguments, the bad record's name)"""
    from evidence_cases import rd
    W = 1 << 14
    rec = lambda pos, name, flag, mpos: rd(pos, "20M", None, name, flag=flag, tid=0, mtid=0, mpos=mpos)      # noqa: E731
    out = [rec(100, b"A", 0x41, 20 * W + 100), rec(200, b"B", 0x41, 20 * W + 5000), rec(300, b"C", 0x41, 25 * W + 100),
           rec(20 * W + 100, b"A", 0x81, 100), rec(20 * W + 5000, b"B", 0x81, 200), rec(20 * W + 5000, b"bad", 0x81, 200),
           rec(25 * W + 100, b"C", 0x81, 300),
           rec(60 * W, b"filler_end", 0x41, 60 * W + 100), rec(60 * W + 100, b"filler_end", 0x81, 60 * W)]      # (bounds the windows)
    out.append(rd(10, "20M", None, b"stop", tid=1))
    assert out == sorted(out, key=lambda r: (r["tid"], r["pos"]))
    return out, [(0, 0, W)], ["chr1:1-16384"], b"bad"


def write_cli_fallback(path):
    """cli_fallback_records() as an indexed BAM in blocks of 1500 bytes -> (header text, regions, arguments, the bad record's name)"""
    import evidence_cases as ec
    from strling_amd import bamio
    recs, regions, args, bad = cli_fallback_records()
    b = ec.batch(recs)
    b.l_seq[[r["name"] for r in recs].index(bad)] = -2
    return bamio.write_bam(path, b, block=1500), regions, args, bad


@functools.lru_cache(maxsize=None)
def calls():
    """every call, laid out, with the model's answers"""
    return tuple(c.lay() for c in (family_t(), family_w(), family_k(), family_h(), family_hm(), family_q(), family_m(), family_mm(), family_c(), family_c_grid()))


def call(name):
    return next(c for c in calls() if c.name == name)
