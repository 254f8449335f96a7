"""Shared by test_nw_trace_host.py and test_gpu_nw_align.py: one set of points and pairs, and a
numpy restatement of GlobAlignE's recurrences (GlobAlignE.cpp:123-291) that records every cell's
predecessor choices and traces them back -- the definition of mc_nw_align_strands' output.

Points come in two halves: point i as written and point NP + i, its minus-strand string (reversed,
digits d -> 3 - d, letters complemented, N kept), so that the expectation for a minus-strand pair
is a plus-strand alignment of a point of its own.
"""
import numpy as np

GO, GE, MATCH, MISMATCH = 2, 1, 1, -1
OP_I, OP_D, OP_EQ, OP_X = 1, 2, 7, 8
OPCH = {OP_I: "I", OP_D: "D", OP_EQ: "=", OP_X: "X"}
_LETTER = {ord("A"): ord("T"), ord("T"): ord("A"), ord("C"): ord("G"), ord("G"): ord("C")}
SMALL = (1, 2, 15, 16, 17, 63, 64, 65)


def np_minus(x):
    x = np.asarray(x, np.uint8)[::-1]
    out = x.copy()
    out[x <= 3] = 3 - x[x <= 3]
    for a, b in _LETTER.items():
        out[x == a] = b
    return out


def mutate(rng, s, rate):
    s = s.copy()
    hit = rng.random(len(s)) < rate
    s[hit] = (s[hit] + rng.integers(1, 4, int(hit.sum()))) % 4
    drop = rng.random(len(s)) < rate / 4
    return s[~drop].astype(np.uint8)


def fit(rng, s, n):
    """s cut or extended with random digits to n bases."""
    if len(s) >= n:
        return s[:n].astype(np.uint8)
    return np.concatenate([s, rng.integers(0, 4, n - len(s))]).astype(np.uint8)


def rows_per_lane(la):
    return 4 if la <= 256 else 8 if la <= 512 else 16


def choice_bytes(la, lb):
    """The choice bytes of a pair: ceil(la / (64 R)) * (lb + 63) * 32 R."""
    r = rows_per_lane(la)
    return (la + 64 * r - 1) // (64 * r) * (lb + 63) * 32 * r


def batch_ends(lens, a, b, am, pairs, nbytes, scratch=0):
    """The batches of host/pairbatch.hpp restated -> one (i1, why) per batch: where it ends and which
    cap ended it ("pairs", "scratch", "bytes"; "end": the list did).  lens: the points' lengths;
    am: a strand flag per pair (None: all plus); scratch 0: no scratch rule (the identities)."""
    out, i0, m = [], 0, len(a)
    while i0 < m:
        i1, uniq, pad, scr, why = i0, set(), 0, 0, "end"
        while i1 < m and why == "end":
            la, lb = lens[a[i1]], lens[b[i1]] if b is not None else 0
            need, string = choice_bytes(la, lb) if scratch else 0, (la + 15) // 16 * 16
            new = am is not None and bool(am[i1]) and int(a[i1]) not in uniq
            if i1 - i0 >= pairs:
                why = "pairs"
            elif scratch and i1 > i0 and scr + need > scratch:
                why = "scratch"
            elif new and uniq and pad + string > nbytes:
                why = "bytes"
            else:
                if new:
                    pad += string
                    uniq.add(int(a[i1]))
                scr += need
                i1 += 1
        out.append((i1, why))
        i0 = i1
    return out


def ident_bytes(lens, a):
    """A value of MC_IDENT_BYTES that puts batch ends inside a list of minus reads a: three times
    the longest one's padded string."""
    return 3 * ((max(lens[i] for i in a) + 15) // 16 * 16)


class Cases:
    """codes: the points (both halves); pairs: name -> (a, b) ids of the first half."""

    def __init__(self):
        rng = np.random.default_rng(2024)
        self.codes, self.segs, self.pairs = [], [], {}

        def point(c, seg=None):
            c = np.asarray(c, np.uint8)
            self.codes.append(c)
            self.segs.append([[0, len(c) - 1]] if seg is None else seg)
            return len(self.codes) - 1

        def rnd(n):
            return rng.integers(0, 4, n).astype(np.uint8)

        for la in SMALL:  # every small length against every small length
            for lb in SMALL:
                if (la + lb) % 2:  # the random side and the mutated copy take turns
                    a = rnd(la)
                    b = fit(rng, mutate(rng, a, 0.1), lb)
                else:
                    b = rnd(lb)
                    a = fit(rng, mutate(rng, b, 0.1), la)
                self.pairs["s%dx%d" % (la, lb)] = (point(a), point(b))
        for la in (255, 256, 257, 511, 512, 513):  # every boundary of the rows-per-lane choice
            a = rnd(la)
            self.pairs["r%d" % la] = (point(a), point(mutate(rng, a, 0.06)))
        wide, narrow = rnd(1100), None
        pw = point(wide)
        for la in (1024, 1025, 1100):  # a second row block
            a = fit(rng, mutate(rng, wide, 0.05), la)
            pa = point(a)
            self.pairs["b%dx1100" % la] = (pa, pw)
            if narrow is None:
                narrow = point(fit(rng, mutate(rng, a[:100], 0.05), 90))
            self.pairs["b%dx90" % la] = (pa, narrow)
        self.pairs["one_x300"] = (point(rnd(1)), point(rnd(300)))
        self.pairs["300x_one"] = (point(rnd(300)), point(rnd(1)))
        s = point(rnd(180))
        self.pairs["self"] = (s, s)
        self.pairs["zeros_ones"] = (point(np.zeros(50, np.uint8)), point(np.ones(47, np.uint8)))
        self.pairs["homopolymers"] = (point(np.full(40, 2, np.uint8)), point(np.full(57, 2, np.uint8)))
        # a 40-base gap at a 16-row group edge (rows 305..320 are one lane's at 16 rows per lane)
        # and at the 1,024-row block edge: the read lacks 40 bases of the centre after its row
        # 320 / 1,024 (a D run in the group's last row), or holds 40 bases the centre lacks in
        # rows 301..340 / 1,005..1,044 (an I run across the edge)
        for name, edge, n in (("g16", 320, 600), ("g1024", 1024, 1100)):
            cen = rnd(n)
            self.pairs[name + "_del"] = (point(np.concatenate([cen[:edge], cen[edge + 40:]])), point(cen))
            self.pairs[name + "_ins"] = (point(np.concatenate([cen[:edge - 20], rnd(40), cen[edge - 20:]])), point(cen))
        a, b = rnd(70), rnd(45)
        g = np.concatenate([a, np.full(6, ord("N"), np.uint8), b])  # a record with an N run
        g2 = np.concatenate([mutate(rng, a, 0.05), np.full(4, ord("N"), np.uint8), b])
        self.pairs["n_run"] = (point(g, [[0, 69], [76, 120]]), point(g2, [[0, len(g2) - 50], [len(g2) - 45, len(g2) - 1]]))
        e = np.frombuffer(b"ACGTNNACCGGTTAGCATNACGTTGCAAGGCT", np.uint8).copy()  # a record without segments
        e2 = np.frombuffer(b"ACGTNACCGTTTAGCATNNACGTTGAAGGCTT", np.uint8).copy()
        self.pairs["raw_letters"] = (point(e, []), point(e2, []))
        reads = []  # the identity test's read families: 13 x 20 reads of 100 .. 300 bases
        for fam in range(13):
            t = rnd(int(rng.integers(140, 290)))
            for i in range(20):
                r = mutate(rng, t, 0.01 + 0.012 * i)
                reads.append(point(r[:max(100, min(300, len(r)))]))
        assert all(100 <= len(self.codes[r]) <= 300 for r in reads)
        for k in range(200):
            a = int(rng.integers(0, len(reads)))
            b = a // 20 * 20 + int(rng.integers(0, 20)) if k % 8 else int(rng.integers(0, len(reads)))
            self.pairs["f%03d" % k] = (reads[a], reads[b])
        self.reads = reads
        self.NP = len(self.codes)
        for i in range(self.NP):  # the second half: every point's minus-strand string
            c = self.codes[i]
            self.codes.append(np_minus(c))
            self.segs.append([[len(c) - 1 - hi, len(c) - 1 - lo] for lo, hi in reversed(self.segs[i])])
        self.names = list(self.pairs)
        self.a = np.array([self.pairs[n][0] for n in self.names], np.uint32)
        self.b = np.array([self.pairs[n][1] for n in self.names], np.uint32)

    def load_args(self):
        lens = [len(c) for c in self.codes]
        seq_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        seg = np.array([v for s in self.segs for pair in s for v in pair], np.int32)
        seg_off = np.concatenate([[0], np.cumsum([len(s) for s in self.segs])]).astype(np.uint64)
        return np.concatenate(self.codes), seq_off, seg, seg_off


def neg_inf(la, lb):
    len1, len2 = la + 1, lb + 1
    shorter, diff = min(len1, len2) - 1, abs(len1 - len2)
    return (-GO - diff * GE if diff >= 1 else 0) + MISMATCH * shorter - 1


def _forward(seqa, seqb):
    """The recurrences on a group of pairs at once, swept by anti-diagonal (arrays indexed
    [pair, row]); sequences are padded with bytes that match nothing, which changes no cell of
    a pair's own matrix.  -> choices [P, LA + 1, LB + 1] (4 bits per cell: 0-1 the state M took
    at (i-1, j-1), 4: X from X, 8: Y from Y) and per pair (score, final state)."""
    P = len(seqa)
    las = np.array([len(x) for x in seqa])
    lbs = np.array([len(x) for x in seqb])
    LA, LB = int(las.max()), int(lbs.max())
    A = np.full((P, LA + 1), 254, np.int32)
    B = np.full((P, LB + 1), 255, np.int32)
    for p in range(P):
        A[p, :las[p]] = seqa[p]
        B[p, :lbs[p]] = seqb[p]
    ninf = np.array([neg_inf(int(x), int(y)) for x, y in zip(las, lbs)], np.int32)[:, None]
    ch = np.zeros((P, LA + 1, LB + 1), np.uint8)
    z = np.zeros((P, LA + 1), np.int32)
    M2, X2, Y2 = z + ninf, z + ninf, z + ninf  # diagonal d - 2, then d - 1
    M2[:, 0], Y2[:, 0] = 0, -GO  # (0, 0)
    M1, X1, Y1 = M2.copy(), X2.copy(), Y2.copy()
    fin = np.zeros((P, 3), np.int64)
    rows = np.arange(P)
    for p in np.nonzero(las + lbs == 0)[0]:
        fin[p] = (0, ninf[p, 0], ninf[p, 0])  # (nw.hip: two empty strings score 0)
    first = True
    for d in range(1, LA + LB + 1):
        if first:
            first = False  # diagonal 0 is both d - 1 and (unused) d - 2
        M0, X0, Y0 = M1.copy(), X1.copy(), Y1.copy()
        if d <= LA:  # column 0
            M0[:, d], Y0[:, d], X0[:, d] = ninf[:, 0], ninf[:, 0], -GO - d * GE
        if d <= LB:  # row 0
            M0[:, 0], X0[:, 0], Y0[:, 0] = ninf[:, 0], ninf[:, 0], -GO - d * GE
        lo, hi = max(1, d - LB), min(LA, d - 1)
        if lo <= hi:
            I, Im = slice(lo, hi + 1), slice(lo - 1, hi)
            ii = np.arange(lo, hi + 1)
            yb, yc = M1[:, I] - (GO + GE), Y1[:, I] - GE
            yy = yb < yc
            Y0[:, I] = np.where(yy, yc, yb)
            xb, xc = M1[:, Im] - (GO + GE), X1[:, Im] - GE
            xx = xb < xc
            X0[:, I] = np.where(xx, xc, xb)
            gM, gX, gY = M2[:, Im], X2[:, Im], Y2[:, Im]
            code = np.where(gM >= np.maximum(gX, gY), 0, np.where(gX >= gY, 1, 2))
            best = np.maximum(gM, np.maximum(gX, gY))
            s = np.where(A[:, lo - 1:hi] == B[:, d - ii - 1], MATCH, MISMATCH)
            M0[:, I] = best + s
            ch[:, ii, d - ii] = (code + 4 * xx + 8 * yy).astype(np.uint8)
        for p in np.nonzero(las + lbs == d)[0]:
            i = las[p]
            fin[p] = (M0[p, i], X0[p, i], Y0[p, i])
        M2, X2, Y2, M1, X1, Y1 = M1, X1, Y1, M0, X0, Y0
    out = []
    for p in range(P):
        m, x, y = (int(v) for v in fin[p])
        sc = max(m, x, y)
        out.append((sc, 0 if sc == m else 1 if sc == x else 2))
    return ch, out


def _traceback(a, b, ch, state):
    """-> (operation words in alignment order, columns, '=' count, reached a boundary)."""
    la, lb = len(a), len(b)
    W = ch.shape[1]
    flat = ch.tobytes()
    a, b = bytes(a), bytes(b)
    i, j, ops = la, lb, []
    cols = ids = 0
    for _ in range(la + lb):
        if i == 0 or j == 0:
            break
        nib = flat[i * W + j]
        cols += 1
        if state == 0:
            eq = a[i - 1] == b[j - 1]
            ops.append(OP_EQ if eq else OP_X)
            ids += eq
            state = nib & 3
            assert state != 3
            i, j = i - 1, j - 1
        elif state == 1:
            ops.append(OP_I)
            state = 1 if nib & 4 else 0
            i -= 1
        else:
            ops.append(OP_D)
            state = 2 if nib & 8 else 0
            j -= 1
    ok = i == 0 or j == 0
    if i == 0:
        ops += [OP_D] * j
        cols += j
    else:
        ops += [OP_I] * i
        cols += i
    ops.reverse()
    words, k = [], 0
    while k < len(ops):
        n = k
        while n < len(ops) and ops[n] == ops[k]:
            n += 1
        words.append((n - k) << 4 | ops[k])
        k = n
    return np.array(words, np.uint32), cols, ids, ok


def align_all(seq_pairs):
    """[(seq1, seq2)] -> [(words, score, columns, '=' count)], the pairs grouped by size."""
    out = [None] * len(seq_pairs)
    groups = {}
    for k, (a, b) in enumerate(seq_pairs):
        n = max(len(a), len(b))
        groups.setdefault(0 if n <= 70 else 1 if n <= 320 else 2 if n <= 520 else 3, []).append(k)
    for ks in groups.values():
        ch, fin = _forward([seq_pairs[k][0] for k in ks], [seq_pairs[k][1] for k in ks])
        for p, k in enumerate(ks):
            a, b = seq_pairs[k]
            la, lb = len(a), len(b)
            score, state = fin[p]
            if la == 0:
                score = neg_inf(0, lb) if lb else 0
            words, cols, ids, ok = _traceback(a, b, np.ascontiguousarray(ch[p, :la + 1, :lb + 1]), state)
            assert ok
            out[k] = (words, score, cols, ids)
    return out


def replay(words, a, b):
    """A CIGAR over two byte strings -> (columns, '=' count, score under 1 / -1 / 2 / 1, bases
    of a, bases of b, every = and X truthful)."""
    i = j = cols = eq = score = 0
    true = True
    for w in words:
        n, op = int(w) >> 4, int(w) & 15
        cols += n
        if op in (OP_EQ, OP_X):
            if i + n > len(a) or j + n > len(b):
                return cols, eq, score, i + n, j + n, False
            same = np.asarray(a[i:i + n]) == np.asarray(b[j:j + n])
            true = true and bool(same.all() if op == OP_EQ else not same.any())
            eq += n if op == OP_EQ else 0
            score += n * (MATCH if op == OP_EQ else MISMATCH)
            i, j = i + n, j + n
        elif op == OP_I:
            score -= GO + n * GE
            i += n
        elif op == OP_D:
            score -= GO + n * GE
            j += n
        else:
            true = False
    return cols, eq, score, i, j, true


def cigar_string(words):
    return "".join("%d%s" % (int(w) >> 4, OPCH[int(w) & 15]) for w in words)


_cache = {}


def cases():
    if "c" not in _cache:
        _cache["c"] = Cases()
    return _cache["c"]


def expected():
    """Computed once per process: name -> result for the plus pairs, and for the same pairs with
    the read's minus-strand string (point NP + a) as seq1."""
    if "e" not in _cache:
        c = cases()
        plus = [(c.codes[a], c.codes[b]) for a, b in zip(c.a, c.b)]
        minus = [(c.codes[c.NP + a], c.codes[b]) for a, b in zip(c.a, c.b)]
        res = align_all(plus + minus)
        _cache["e"] = (res[:len(plus)], res[len(plus):])
    return _cache["e"]
