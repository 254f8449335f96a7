"""Shared by test_qpileup_host.py and test_gpu_qpileup.py: the weight table of
mc_nw_qpileup_strands and the weighted consensus restated in Python, over the points, pairs and
operation words of tests/pileup_cases.py, with one seeded quality string per point.

The weight table (include/meshclust_amd.h): Qs is the read's quality string in the aligned string's
order -- reversed here for a minus pair, where the device indexes backwards.  Walking the words with
i read bases and j centre bases consumed: '=' / 'X' add Qs[i] to row j, the channel of the read's
byte; a 'D' run adds min(Qs[i - 1] if i > 0, Qs[i] if i < la) to channel 5 of each of its rows; an
'I' run of n adds min(Qs[i : i + n]) to channel 6 of row j.  Channel 7 stays 0."""
import numpy as np

import nw_trace_cases as T
import pileup_cases as P

QMAX = 93
CH = P.CH


def wtable_from_words(words, read, qs, centre, tab=None):
    """Adds one alignment's weights to tab ([len(centre) + 1, 8] uint32; made if None) -> tab.
    read, qs: seq1 and its qualities as aligned."""
    L, la = len(centre), len(read)
    if tab is None:
        tab = np.zeros((L + 1, CH), np.uint32)
    read = np.asarray(read, np.uint8)
    qs = np.asarray(qs, np.uint32)
    assert len(qs) == la
    cls = np.where(read <= 3, read, 4).astype(np.int64)
    i = j = 0
    for w in words:
        n, op = int(w) >> 4, int(w) & 15
        if op in (T.OP_EQ, T.OP_X):
            np.add.at(tab, (np.arange(j, j + n), cls[i:i + n]), qs[i:i + n])
            i, j = i + n, j + n
        elif op == T.OP_D:
            around = ([int(qs[i - 1])] if i > 0 else []) + ([int(qs[i])] if i < la else [])
            tab[j:j + n, 5] += min(around) if around else 0
            j += n
        else:
            assert op == T.OP_I
            tab[j, 6] += int(qs[i:i + n].min())
            i += n
    assert (i, j) == (la, L)
    return tab


def insertion_runs(words, read, qs):
    """-> [(row, the inserted bytes, their qualities)] of one alignment."""
    out, i, j = [], 0, 0
    for w in words:
        n, op = int(w) >> 4, int(w) & 15
        if op == T.OP_I:
            out.append((j, bytes(bytearray(read[i:i + n])), [int(v) for v in qs[i:i + n]]))
            i += n
        elif op == T.OP_D:
            j += n
        else:
            i, j = i + n, j + n
    return out


def pick(w, n, own):
    """The class of the largest weight; ties to the larger count, then to `own` if it is among the
    tied, else to the lowest."""
    top = max(zip(w, n))
    tied = [c for c in range(len(w)) if (w[c], n[c]) == top]
    return own if own in tied else tied[0]


def quality_char(w, win):
    return chr(33 + min(QMAX, max(0, w[win] - (sum(w) - w[win]))))


def insertion_consensus(runs):
    """runs: [(bytes, qualities)] at one site -> (bases, quality characters)."""
    count = {}
    for b, _ in runs:
        count[len(b)] = count.get(len(b), 0) + 1
    length = min(count, key=lambda n: (-count[n], n))  # the most frequent length, ties to the shortest
    seq, qual = "", ""
    for t in range(length):
        w, n = [0] * 5, [0] * 5
        for b, q in runs:
            if len(b) > t:
                w[P.channel(b[t])] += q[t]
                n[P.channel(b[t])] += 1
        win = pick(w, n, None)
        seq += P.LETTERS[win]
        qual += quality_char(w, win)
    return seq, qual


def consensus(centre, rows, wrows, depth, runs):
    """centre: its bytes; rows, wrows: [L + 1, 8] counts and weights; runs: [(row, bytes, qualities)]
    of every 'I' run of the centre's reads -> (sequence, quality string, sub, del, ins)."""
    L = len(centre)
    if depth == 0:
        return "".join(P.base_char(x) for x in centre), "!" * L, 0, 0, 0
    seq, qual, sub, dele, ins = [], [], 0, 0, 0
    for r in range(L + 1):
        if 2 * int(rows[r][6]) > depth:
            here = [(b, q) for row, b, q in runs if row == r]
            if here:
                s, q = insertion_consensus(here)
                seq.append(s)
                qual.append(q)
                ins += 1
        if r == L:
            break
        w, n = [int(v) for v in wrows[r][:6]], [int(v) for v in rows[r][:6]]
        ch = pick(w, n, P.channel(centre[r]))
        if ch == 5:
            dele += 1
            continue
        x = P.LETTERS[ch]
        sub += x != P.base_char(centre[r])
        seq.append(x)
        qual.append(quality_char(w, ch))
    return "".join(seq), "".join(qual), sub, dele, ins


_cache = {}


def qualities():
    """One quality string per point of pileup_cases.pile(), seeded; among the 150 reads of the
    contended centre one is all 0, one all 93 and one a ramp, and the 1,100-base read of the widest
    pair is a ramp too (a reversed index shows in a run the whole wave takes)."""
    if "q" not in _cache:
        p = P.pile()
        rng = np.random.default_rng(93)
        q = [rng.integers(0, QMAX + 1, len(c)).astype(np.uint8) for c in p.codes]
        ks = [k for k in range(len(p.a)) if p.b[k] == p.contended]
        q[p.a[ks[0]]][:] = 0
        q[p.a[ks[1]]][:] = QMAX
        for i in (p.a[ks[2]], p.base.pairs["b1100x1100"][0]):
            q[i] = (np.arange(len(q[i])) % (QMAX + 1)).astype(np.uint8)
        _cache["q"] = q
        _cache["special"] = (int(p.a[ks[0]]), int(p.a[ks[1]]), int(p.a[ks[2]]))
    return _cache["q"]


def special_reads():
    qualities()
    return _cache["special"]


def flat(q):
    return np.concatenate(q).astype(np.uint8)


def aligned_quality(q, k, minus):
    """The qualities of pair k's seq1 in the aligned string's order."""
    x = q[P.pile().a[k]]
    return x[::-1] if minus else x


def pair_wtable(q, k, minus):
    p = P.pile()
    words = P.expected()[1 if minus else 0][k][0]
    return wtable_from_words(words, p.read(k, bool(minus)), aligned_quality(q, k, minus), p.codes[p.b[k]])


def pair_wtables():
    """-> (plus, minus): per pair its own weight table under qualities(), computed once."""
    if "t" not in _cache:
        q = qualities()
        _cache["t"] = tuple([pair_wtable(q, k, s) for k in range(len(P.pile().a))] for s in (0, 1))
    return _cache["t"]


def expected_wtable(am, pairs=None):
    """The whole weight table [row_off[-1], 8] for the strands am (a flag per pair), over `pairs` (all)."""
    p = P.pile()
    tabs = pair_wtables()
    out = np.zeros((int(p.row_off[-1]), CH), np.uint32)
    for k in (range(len(p.a)) if pairs is None else pairs):
        r0 = int(p.row_off[p.tindex[int(p.b[k])]])
        t = tabs[1 if am[k] else 0][k]
        out[r0:r0 + len(t)] += t
    return out


def planted_q():
    """The planted truth of the weighted consensus -> (template, reads, qualities): a 300-base
    template; at three columns two reads carry a wrong base at Q2 against one read with the right
    base at Q40 (every other base Q40)."""
    rng = np.random.default_rng(40)
    t = rng.integers(0, 4, 300).astype(np.uint8)
    reads = [t.copy() for _ in range(3)]
    quals = [np.full(300, 40, np.uint8) for _ in range(3)]
    for col in (31, 150, 268):
        wrong = (t[col] + 1 + col % 3) % 4
        for k in (0, 1):
            reads[k][col] = wrong
            quals[k][col] = 2
    return t, reads, quals
