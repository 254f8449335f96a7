"""Shared by test_crossover_host.py and test_gpu_crossover.py: two alignments of one read compared base by
base (include/meshclust_amd.h, mc_nw_msa_crossover) restated in Python twice, host/chimera.hpp ported, and
one seeded set of points, pairs and candidates.

The definition.  For a pair p of a read of la bases, e_p(u) = 1 where base u of the read as written lies in
an '=' column of p's alignment (a minus pair: base i as aligned is base la - 1 - i as written).  For two
pairs x, y of one read, D(s) = sum over u < s of e_x(u) - e_y(u), s = 0 .. la, and the eight values are
ids_x, ids_y, ids_y + max D with its first and last s, ids_x - min D with its first and last s.
Two ways to e: from the operation words nw_trace_cases.align_all gives (e_from_words), and from the rows
msa_cases.block renders (e_from_rows: a read base at a centre column that equals the centre row's byte);
test_crossover_host.py holds them equal.

The points: small reads of every length around the bitmap word (1, 2, 31, 32, 33, 63, 64, 65) against two
targets, two of them against three; a read of 480 bases with more than 64 operation words; reads of 2047,
2048 and 2049 bases (the edges of the scan's chunk of 64 words) -- four pairs above 600 bases in all: the
read of 2048 against two targets (more than 128 words each), the other two against one target each, the
read of 2049 an exact prefix of its target: an '=' run over 65 bitmap words; and planted chimeras: parents
A and B of 120 bases 10 % apart (nw_trace_cases.mutate), six error-free reads A[:cut] + B[cut':] with cut in
[30, 90) and cut' the base of B that descends from A[cut], and pure reads of either parent; last, a read
of no bases against two targets (the loader and mc_nw_msa_begin take one: its alignment is lb 'D')."""
import copy

import numpy as np

import msa_cases as A
import nw_trace_cases as T

RES = 8
NAMES = ["plus", "minus", "mixed"]
SMALL = (1, 2, 31, 32, 33, 63, 64, 65)
THREE = (33, 65)  # the small reads with pairs against three targets


# ---------------------------------------------------------------- the definition, twice
def e_from_words(words, la, minus):
    """One pair's words -> e over the read as written (uint8[la])."""
    e = np.zeros(la, np.uint8)
    i = 0
    for wd in words:
        n, op = int(wd) >> 4, int(wd) & 15
        if op == T.OP_EQ:
            e[i:i + n] = 1
        if op in (T.OP_EQ, T.OP_X, T.OP_I):
            i += n
    assert i == la
    return e[::-1].copy() if minus else e


def e_from_rows(centre_row, row, minus):
    """The same from the pair's row of msa_cases.block and its centre's row."""
    c, r = np.frombuffer(centre_row, np.uint8), np.frombuffer(row, np.uint8)
    has = r != A.GAP
    e = ((c != A.GAP) & has & (r == c))[has].astype(np.uint8)  # per read base as aligned, in row order
    return e[::-1].copy() if minus else e


def crossover(ex, ey):
    """-> the eight values (int32)."""
    D = np.concatenate([[0], np.cumsum(ex.astype(np.int64) - ey.astype(np.int64))])
    hi, lo = int(D.max()), int(D.min())
    at_hi, at_lo = np.nonzero(D == hi)[0], np.nonzero(D == lo)[0]
    ix, iy = int(ex.sum()), int(ey.sum())
    return np.array([ix, iy, iy + hi, at_hi[0], at_hi[-1], ix - lo, at_lo[0], at_lo[-1]], np.int32)


def exchanged(v):
    """The values of (y, x) from those of (x, y)."""
    v = np.asarray(v)
    return v[..., [1, 0, 5, 6, 7, 2, 3, 4]]


# ---------------------------------------------------------------- host/chimera.hpp in Python
def chimera_order(v):
    """-> (xy, best, gain, cut_first, cut_last, ids_left, ids_right)."""
    v = [int(t) for t in v]
    xy = v[2] >= v[5]
    best = v[2] if xy else v[5]
    return (xy, best, best - max(v[0], v[1])) + ((v[3], v[4], v[0], v[1]) if xy else (v[6], v[7], v[1], v[0]))


def chimera_candidates(centres):
    return [j for j in range(1, len(centres)) if centres[j] != centres[0]]


def chimera_pick(cand, res, min_gain):
    """cand: hit indices, ascending; res: their values -> (hit, xy, best, gain, cut_first, cut_last,
    ids_left, ids_right, flag) or None without a candidate."""
    out = None
    for j, v in zip(cand, res):
        c = chimera_order(v)
        if out is None or c[2] > out[3]:
            out = (j,) + c
    return None if out is None else out + (out[3] >= min_gain,)


# ---------------------------------------------------------------- the points
class Cross:
    """codes / segs: the points; a, b: the pairs (read, target); targets; cands: (x, y) pair indices;
    planted: [(candidate, cut)] of the chimeras; pure: the candidates of the pure reads."""

    def __init__(self):
        rng = np.random.default_rng(11)
        self.codes, self.segs = [], []

        def point(c):
            c = np.asarray(c, np.uint8)
            self.codes.append(c)
            self.segs.append([[0, len(c) - 1]] if len(c) else [])
            return len(self.codes) - 1

        def rnd(n):
            return rng.integers(0, 4, n).astype(np.uint8)

        a, b, cands, targets = [], [], [], []
        self.label = []  # per candidate

        def read(r, tg, what):
            """Pairs of read point r against the targets tg; candidates: every couple of them, the earlier as x."""
            k0 = len(a)
            for t in tg:
                a.append(r)
                b.append(t)
            ks = list(range(k0, len(a)))
            for n, x in enumerate(ks):
                for y in ks[n + 1:]:
                    cands.append((x, y))
                    self.label.append(what)
            return ks

        t0 = rnd(70)
        small_t = [point(t0), point(T.mutate(rng, t0, 0.1)), point(T.mutate(rng, t0, 0.1))]
        targets += small_t
        for la in SMALL:  # the left half from one target, the right half from another, then 5 % errors
            mix = np.concatenate([self.codes[small_t[0]][:la // 2], self.codes[small_t[1]][la // 2:]])
            r = point(T.fit(rng, T.mutate(rng, mix, 0.05), la))
            read(r, small_t[:3 if la in THREE else 2], "s%d" % la)
        # more than 64 words below 600 bases
        tm = rnd(500)
        mid_t = [point(tm), point(T.mutate(rng, tm, 0.06))]
        targets += mid_t
        self.mid = read(point(T.fit(rng, T.mutate(rng, tm, 0.09), 480)), mid_t, "mid")
        # the chunk edges: four pairs above 600 bases
        tl = rnd(2100)
        long_t = [point(tl), point(T.mutate(rng, tl, 0.05))]
        targets += long_t
        self.long2048 = read(point(T.fit(rng, T.mutate(rng, tl, 0.06), 2048)), long_t, "l2048")
        self.long2047 = read(point(T.fit(rng, T.mutate(rng, self.codes[long_t[1]], 0.04), 2047)), long_t[1:], "l2047")
        self.long2049 = read(point(tl[:2049].copy()), long_t[:1], "l2049")
        # planted chimeras and pure reads
        # (parents redrawn until either end of 30 bases holds four substitutions: a cut in [30, 90) then has at least
        # four differences on each side, and the two-parent model gains about the smaller of the two counts)
        while True:
            pa = rnd(120)
            replay = copy.deepcopy(rng)
            pb = T.mutate(rng, pa, 0.1)
            hit = replay.random(120) < 0.1  # mutate's own draws again: the bases of A it changed and dropped
            replay.integers(1, 4, int(hit.sum()))
            drop = replay.random(120) < 0.1 / 4
            assert len(pb) == 120 - int(drop.sum())
            if (hit & ~drop)[:30].sum() >= 4 and (hit & ~drop)[90:].sum() >= 4:
                break
        par = [point(pa), point(pb)]
        targets += par
        self.parents = par
        self.planted, self.pure = [], []
        for cut in (30, 41, 52, 63, 74, 89):
            cut_b = cut - int(drop[:cut].sum())
            read(point(np.concatenate([pa[:cut], pb[cut_b:]])), par, "chim%d" % cut)
            self.planted.append((len(cands) - 1, cut))
        for n, r in enumerate((pa.copy(), pb.copy(), pa[5:].copy(), pb[:-7].copy(), pa[3:-4].copy(), pb[6:].copy())):
            read(point(r), par, "pure%d" % n)
            self.pure.append(len(cands) - 1)
        self.empty = read(point(np.zeros(0, np.uint8)), small_t[:2], "empty")
        # x == y
        for k in (0, self.mid[0], self.long2047[0], self.long2049[0], self.long2048[1], self.empty[1]):
            cands.append((k, k))
            self.label.append("same%d" % k)
        self.a, self.b = np.array(a, np.uint32), np.array(b, np.uint32)
        self.targets = np.array(targets, np.uint32)
        self.x = np.array([c[0] for c in cands], np.uint64)
        self.y = np.array([c[1] for c in cands], np.uint64)

    def load_args(self):
        lens = [len(c) for c in self.codes]
        seq_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        seg = np.array([v for s in self.segs for pair in s for v in pair], np.int32)
        seg_off = np.concatenate([[0], np.cumsum([len(s) for s in self.segs])]).astype(np.uint64)
        return np.concatenate(self.codes), seq_off, seg, seg_off

    def la(self, k):
        return len(self.codes[self.a[k]])

    def read(self, k, minus):
        """seq1 of pair k as aligned."""
        c = self.codes[self.a[k]]
        return T.np_minus(c) if minus else c

    def strands(self, name):
        """A flag per pair; mixed: msa_cases' rule, under which neighbours 3n + 1 and 3n + 2 differ."""
        n = len(self.a)
        return {"plus": np.zeros(n, np.uint8), "minus": np.ones(n, np.uint8), "mixed": (np.arange(n) % 3 != 2).astype(np.uint8)}[name]


_cache = {}


def cross():
    if "c" not in _cache:
        _cache["c"] = Cross()
    return _cache["c"]


def aligned():
    """Computed once per process -> (plus, minus): per pair (words, score, columns, '=' count)."""
    if "a" not in _cache:
        q = cross()
        m = len(q.a)
        res = T.align_all([(q.read(k, False), q.codes[q.b[k]]) for k in range(m)] + [(q.read(k, True), q.codes[q.b[k]]) for k in range(m)])
        _cache["a"] = (res[:m], res[m:])
    return _cache["a"]


def bitmaps(name, how="words"):
    """e of every pair for the strands `name`, from the words or from the rendered rows; once per process."""
    if ("e", name, how) not in _cache:
        q = cross()
        am = q.strands(name)
        al = aligned()
        if how == "words":
            out = [e_from_words(al[am[k]][k][0], q.la(k), bool(am[k])) for k in range(len(q.a))]
        else:
            out = [None] * len(q.a)
            for j in q.targets:
                ks = [k for k in range(len(q.a)) if q.b[k] == j]
                _, _, rows = A.block(q.codes[j], [(al[am[k]][k][0], q.read(k, bool(am[k]))) for k in ks])
                for n, k in enumerate(ks):
                    out[k] = e_from_rows(rows[0], rows[1 + n], bool(am[k]))
        _cache[("e", name, how)] = out
    return _cache[("e", name, how)]


def expected(name, how="words"):
    """-> [nc, 8] int32 over cross()'s candidates; computed once per process and left unchanged."""
    if ("x", name, how) not in _cache:
        q = cross()
        e = bitmaps(name, how)
        out = np.array([crossover(e[int(x)], e[int(y)]) for x, y in zip(q.x, q.y)], np.int32).reshape(len(q.x), RES)
        out.setflags(write=False)
        _cache[("x", name, how)] = out
    return _cache[("x", name, how)]
