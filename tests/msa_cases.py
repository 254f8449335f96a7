"""Shared by test_msa_host.py and test_gpu_msa.py: the centre-anchored multiple alignment
(include/meshclust_amd.h, mc_nw_msa_begin / mc_nw_msa_rows) restated in Python, and one set of
points, pairs and targets.

The definition: for a centre of L bytes and its pairs, ins(i, r) is the length of pair i's 'I' run
met with r centre bases consumed; w[r] = max over the pairs of ins(i, r), r = 0 .. L;
col[r] = r + w[0] + .. + w[r]; W = col[L] = L + sum(w).  The centre's row has its characters at
col[r]; a pair's row has '=' / 'X' bases at col[j], nothing at a 'D', and an 'I' run of n at
col[j] - w[j] .. + n; everything else is '-'.

The points: pileup_cases.pile()'s points, pairs and targets as they are, followed by 40 reads on
one centre whose insertions contend for the same widths (slots before the first base and after the
last, five different lengths on one row) and one pair with an 'I' run of 70: a slot run of more than
64 columns.  Expectations of the new pairs come from nw_trace_cases.align_all."""
import numpy as np

import nw_trace_cases as T
import pileup_cases as P

GAP = ord("-")


def char(x):
    return ord("ACGT"[x]) if x <= 3 else int(x)


def ins_runs(words):
    """-> [(row, length)] of the 'I' runs of one alignment."""
    out, j = [], 0
    for w in words:
        n, op = int(w) >> 4, int(w) & 15
        if op == T.OP_I:
            out.append((j, n))
        elif op in (T.OP_D, T.OP_EQ, T.OP_X):
            j += n
    return out


def widths(L, all_words):
    """w[0 .. L] over the alignments all_words of one centre of L bytes."""
    w = np.zeros(L + 1, np.uint32)
    for words in all_words:
        rows = [r for r, _ in ins_runs(words)]
        assert len(set(rows)) == len(rows)  # at most one 'I' run per row
        for r, n in ins_runs(words):
            w[r] = max(w[r], n)
    return w


def columns(w):
    """-> (col[0 .. L], W): col[r] = r + w[0] + .. + w[r], col[L] = W."""
    col = np.arange(len(w), dtype=np.int64) + np.cumsum(w.astype(np.int64))
    return col, int(col[-1])


def block(centre, pairs):
    """centre: its bytes; pairs: [(words, seq1 as aligned)] -> (w, W, rows): the centre's row, then a
    row per pair, each W bytes."""
    L = len(centre)
    w = widths(L, [words for words, _ in pairs])
    col, W = columns(w)
    row = np.full(W, GAP, np.uint8)
    for r in range(L):
        row[col[r]] = char(centre[r])
    rows = [row.tobytes()]
    for words, read in pairs:
        row = np.full(W, GAP, np.uint8)
        i = j = 0
        for wd in words:
            n, op = int(wd) >> 4, int(wd) & 15
            if op in (T.OP_EQ, T.OP_X):
                for t in range(n):
                    row[col[j + t]] = char(read[i + t])
                i, j = i + n, j + n
            elif op == T.OP_D:
                j += n
            else:
                assert op == T.OP_I and n <= w[j]
                for t in range(n):
                    row[col[j] - int(w[j]) + t] = char(read[i + t])
                i += n
        assert (i, j) == (len(read), L)
        rows.append(row.tobytes())
    return w, W, rows


class Msa:
    def __init__(self):
        p = P.pile()
        self.pile = p
        self.codes = list(p.codes)
        self.segs = list(p.segs)

        def point(c):
            c = np.asarray(c, np.uint8)
            self.codes.append(c)
            self.segs.append([[0, len(c) - 1]])
            return len(self.codes) - 1

        a, b, names = list(p.a), list(p.b), list(p.names)
        self.nold = len(a)
        rng = np.random.default_rng(31)
        cen = rng.integers(0, 4, 120).astype(np.uint8)
        reads = [np.concatenate([rng.integers(0, 4, k % 3).astype(np.uint8), cen[:40], rng.integers(0, 4, k % 5 + 1).astype(np.uint8),
                                 cen[40:80], cen[81:], rng.integers(0, 4, k % 4).astype(np.uint8)]) for k in range(40)]
        c2 = rng.integers(0, 4, 100).astype(np.uint8)
        r2 = np.concatenate([c2[:50], rng.integers(0, 4, 70).astype(np.uint8), c2[50:]])
        self.slots = point(cen)
        for k, r in enumerate(reads):
            a.append(point(r))
            b.append(self.slots)
            names.append("s%02d" % k)
        self.long_target = point(c2)
        a.append(point(r2))
        b.append(self.long_target)
        names.append("i70")
        self.a, self.b, self.names = np.array(a, np.uint32), np.array(b, np.uint32), names
        self.targets = np.array(list(p.targets) + [self.slots, self.long_target], np.uint32)
        self.tindex = {int(j): t for t, j in enumerate(self.targets)}
        lens = [len(self.codes[j]) + 1 for j in self.targets]
        self.row_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)

    def load_args(self):
        lens = [len(c) for c in self.codes]
        seq_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        seg = np.array([v for s in self.segs for pair in s for v in pair], np.int32)
        seg_off = np.concatenate([[0], np.cumsum([len(s) for s in self.segs])]).astype(np.uint64)
        return np.concatenate(self.codes), seq_off, seg, seg_off

    def read(self, k, minus):
        """seq1 of pair k as aligned."""
        c = self.codes[self.a[k]]
        return T.np_minus(c) if minus else c

    def strands(self, name):
        """A flag per pair; mixed: pileup_cases.mixed_strands()' rule over the longer list."""
        n = len(self.a)
        return {"plus": np.zeros(n, np.uint8), "minus": np.ones(n, np.uint8), "mixed": (np.arange(n) % 3 != 2).astype(np.uint8)}[name]


_cache = {}


def msa():
    if "m" not in _cache:
        _cache["m"] = Msa()
    return _cache["m"]


def expected():
    """Computed once per process -> (plus, minus): per pair (words, score, columns, '=' count)."""
    if "e" not in _cache:
        q = msa()
        plus, minus = (list(x) for x in P.expected())
        new = range(q.nold, len(q.a))
        res = T.align_all([(q.read(k, False), q.codes[q.b[k]]) for k in new] + [(q.read(k, True), q.codes[q.b[k]]) for k in new])
        _cache["e"] = (plus + res[:len(new)], minus + res[len(new):])
    return _cache["e"]


def blocks(am, pairs=None):
    """The whole alignment for the strands am (a flag per pair) over `pairs` (all) -> per target
    (w, W, rows, ks): ks the target's pairs in list order, rows[0] its centre row, rows[1 + n] pair
    ks[n]'s."""
    q = msa()
    exp = expected()
    out = []
    for j in q.targets:
        ks = [k for k in (range(len(q.a)) if pairs is None else pairs) if q.b[k] == j]
        w, W, rows = block(q.codes[j], [(exp[am[k]][k][0], q.read(k, bool(am[k]))) for k in ks])
        out.append((w, W, rows, ks))
    return out


def named_blocks(name):
    """blocks(strands(name)), computed once per process."""
    if ("b", name) not in _cache:
        _cache[("b", name)] = blocks(msa().strands(name))
    return _cache[("b", name)]


def all_rows(bl, m):
    """-> (rows in mc_nw_msa_rows' order: the nt centre rows, then the m pair rows; width of all
    rows [row_off[-1]]; block widths [nt])."""
    centre = [rows[0] for _, _, rows, _ in bl]
    pair = [None] * m
    for _, _, rows, ks in bl:
        for n, k in enumerate(ks):
            pair[k] = rows[1 + n]
    return centre + pair, np.concatenate([w for w, _, _, _ in bl]).astype(np.uint32), np.array([W for _, W, _, _ in bl], np.uint64)
