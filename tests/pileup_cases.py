"""Shared by test_pileup_host.py and test_gpu_pileup.py: the pile-up table and the consensus
restated in Python, and one set of points, pairs and targets.

The table (include/meshclust_amd.h, mc_nw_pileup_strands): a centre of L bytes has L + 1 rows of 8
counters.  Walking an alignment (the words of mc_nw_align_strands; seq1 the read, seq2 the centre)
with j centre bases consumed: '=' / 'X' add 1 to row j, channel x (the read's byte, 4 if x > 3),
j++; 'D' adds 1 to row j, channel 5, j++; an 'I' run of n adds 1 to row j, channel 6 and n to
channel 7.

The pairs: the whole list of nw_trace_cases (whose expectations test_nw_trace_host.py ties to the
CPU oracle), then what only a pile-up can get wrong: 150 reads on one centre, a pair of more than
64 runs, a planted-truth family whose consensus is known, a target no pair names, and a pair with
a run of more than 64 'X'.  Points are
nw_trace_cases' (both halves) followed by the new ones; a minus pair's expectation is the
alignment of the read's minus-strand string."""
import numpy as np

import nw_trace_cases as T

CH = 8
LETTERS = "ACGTN"


def channel(x):
    return int(x) if x <= 3 else 4


def base_char(x):
    return LETTERS[x] if x <= 3 else chr(x)


def table_from_words(words, read, centre, tab=None):
    """Adds one alignment to tab ([len(centre) + 1, 8] uint32; made if None) -> tab."""
    L = len(centre)
    if tab is None:
        tab = np.zeros((L + 1, CH), np.uint32)
    read = np.asarray(read, np.uint8)
    cls = np.where(read <= 3, read, 4).astype(np.int64)
    i = j = 0
    for w in words:
        n, op = int(w) >> 4, int(w) & 15
        if op in (T.OP_EQ, T.OP_X):
            np.add.at(tab, (np.arange(j, j + n), cls[i:i + n]), 1)
            i, j = i + n, j + n
        elif op == T.OP_D:
            tab[j:j + n, 5] += 1
            j += n
        else:
            assert op == T.OP_I
            tab[j, 6] += 1
            tab[j, 7] += n
            i += n
    assert (i, j) == (len(read), L)
    return tab


def insertion_runs(words, read):
    """-> [(row, the inserted bytes)] of one alignment."""
    out, i, j = [], 0, 0
    for w in words:
        n, op = int(w) >> 4, int(w) & 15
        if op == T.OP_I:
            out.append((j, bytes(bytearray(read[i:i + n]))))
            i += n
        elif op == T.OP_D:
            j += n
        else:
            i, j = i + n, j + n
    return out


def insertion_consensus(runs):
    """runs: the reads' inserted byte strings at one site."""
    count = {}
    for r in runs:
        count[len(r)] = count.get(len(r), 0) + 1
    length = min(count, key=lambda n: (-count[n], n))  # the most frequent length, ties to the shortest
    out = ""
    for t in range(length):
        cls = [0] * 5
        for r in runs:
            if len(r) > t:
                cls[channel(r[t])] += 1
        out += LETTERS[cls.index(max(cls))]  # ties to the lowest class
    return out


def consensus(centre, rows, depth, runs):
    """centre: its bytes; rows: [L + 1, 8]; runs: [(row, bytes)] of every 'I' run of the centre's
    reads -> (sequence, sub, del, ins)."""
    L = len(centre)
    if depth == 0:
        return "".join(base_char(x) for x in centre), 0, 0, 0
    seq, sub, dele, ins = [], 0, 0, 0
    for r in range(L + 1):
        if 2 * int(rows[r][6]) > depth:
            here = [b for row, b in runs if row == r]
            if here:
                seq.append(insertion_consensus(here))
                ins += 1
        if r == L:
            break
        six = [int(v) for v in rows[r][:6]]
        top, own = max(six), channel(centre[r])
        ch = own if six[own] == top else six.index(top)
        if ch == 5:
            dele += 1
            continue
        x = LETTERS[ch]
        sub += x != base_char(centre[r])
        seq.append(x)
    return "".join(seq), sub, dele, ins


def planted(seed):
    """-> (template T, centre, reads): the centre is T with 6 substitutions, one base of T missing
    and two bases T does not have; the reads are T mutated independently at 2 %."""
    rng = np.random.default_rng(seed)
    t = rng.integers(0, 4, 300).astype(np.uint8)
    cen = t.copy()
    for pos in (17, 64, 65, 140, 222, 287):
        cen[pos] = (cen[pos] + 1 + pos % 3) % 4
    cen = np.concatenate([cen[:100], cen[101:200], rng.integers(0, 4, 2).astype(np.uint8), cen[200:]])
    reads = [T.mutate(rng, t, 0.02) for _ in range(30)]
    return t, cen, reads


PLANTED_SEED = 5  # checked by test_pileup_host.py: the consensus is T exactly


class Pile:
    def __init__(self):
        base = T.cases()
        rng = np.random.default_rng(77)
        self.base = base
        self.codes = list(base.codes)
        self.segs = list(base.segs)

        def point(c):
            c = np.asarray(c, np.uint8)
            self.codes.append(c)
            self.segs.append([[0, len(c) - 1]])
            return len(self.codes) - 1

        a, b, names = list(base.a), list(base.b), list(base.names)
        self.nbase = len(a)
        # one centre with 150 reads: many waves add to the same rows and difference entries
        cen = rng.integers(0, 4, 120).astype(np.uint8)
        self.contended = point(cen)
        for k in range(150):
            a.append(point(T.mutate(rng, cen, 0.03)))
            b.append(self.contended)
            names.append("c%03d" % k)
        # a pair of more than 64 runs: the prefix carry crosses word chunks
        x = rng.integers(0, 4, 400).astype(np.uint8)
        y = x.copy()
        hit = rng.random(400) < 0.25
        y[hit] = (y[hit] + rng.integers(1, 4, int(hit.sum()))) % 4
        a.append(point(y))
        b.append(point(x))
        names.append("runs")
        # the planted-truth family
        self.truth, pcen, reads = planted(PLANTED_SEED)
        self.planted = point(pcen)
        for k, r in enumerate(reads):
            a.append(point(r))
            b.append(self.planted)
            names.append("p%02d" % k)
        self.lonely = point(rng.integers(0, 4, 33).astype(np.uint8))  # a target with no pair
        # the one class of runs no pair above has (test_pileup_host.py's census): more than 64 'X'.
        # 70 bases of one letter in a 260-base centre, of another in the read: 95=70X95= on the
        # plus strand, and a run of 71 on the minus strand (the complement differs from it too)
        xc = np.random.default_rng(260).integers(0, 4, 260).astype(np.uint8)
        xc[95:165] = 0
        xr = xc.copy()
        xr[95:165] = 2
        a.append(point(xr))
        b.append(point(xc))
        names.append("x70")
        self.a, self.b, self.names = np.array(a, np.uint32), np.array(b, np.uint32), names
        seen, targets = set(), []
        for j in list(self.b) + [self.lonely]:
            if int(j) not in seen:
                seen.add(int(j))
                targets.append(int(j))
        self.targets = np.array(targets, np.uint32)
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


_cache = {}


def pile():
    if "p" not in _cache:
        _cache["p"] = Pile()
    return _cache["p"]


def expected():
    """Computed once per process -> (plus, minus): per pair (words, score, columns, '=' count)."""
    if "e" not in _cache:
        p = pile()
        plus, minus = (list(x) for x in T.expected())
        new = range(p.nbase, len(p.a))
        res = T.align_all([(p.read(k, False), p.codes[p.b[k]]) for k in new] + [(p.read(k, True), p.codes[p.b[k]]) for k in new])
        _cache["e"] = (plus + res[:len(new)], minus + res[len(new):])
    return _cache["e"]


def pair_tables():
    """-> (plus, minus): per pair its own table, computed once."""
    if "t" not in _cache:
        p = pile()
        exp = expected()
        _cache["t"] = tuple([table_from_words(exp[s][k][0], p.read(k, bool(s)), p.codes[p.b[k]]) for k in range(len(p.a))]
                            for s in (0, 1))
    return _cache["t"]


def expected_table(am, pairs=None):
    """The whole table [row_off[-1], 8] for the strands am (a flag per pair), over `pairs` (all)."""
    p = pile()
    tabs = pair_tables()
    out = np.zeros((int(p.row_off[-1]), CH), np.uint32)
    for k in (range(len(p.a)) if pairs is None else pairs):
        r0 = int(p.row_off[p.tindex[int(p.b[k])]])
        t = tabs[1 if am[k] else 0][k]
        out[r0:r0 + len(t)] += t
    return out


def mixed_strands():
    p = pile()
    return (np.arange(len(p.a)) % 3 != 2).astype(np.uint8)
