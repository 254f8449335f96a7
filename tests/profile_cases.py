"""Shared by test_profile_host.py and test_gpu_msa_counts.py: the column profile of the
centre-anchored multiple alignment (include/meshclust_amd.h, mc_nw_msa_counts) restated in Python
over msa_cases.msa()'s points and nw_trace_cases' words, and host/profile.hpp's consensus ported.

The definition, in msa_cases' terms (w, col, W of a centre of L bytes; depth = its pairs; the class
of a byte x is x for x <= 3, else 4).  A block has W columns of 8 counters:
  the column of centre base r (col[r])   channels 0..4 the reads' bytes there by class, 5 the reads
                                         with a 'D', 6 = r, 7 = 0
  slot t of site r (col[r] - w[r] + t)   channels 0..4 the bytes of the 'I' runs at r longer than t,
                                         5 = depth less those, 6 = r, 7 = t + 1
The weights have the same shape: '=' / 'X' / 'I' add the base's quality Qs[i] to its class, a 'D' run
adds min(Qs[i - 1] if i > 0, Qs[i] if i < la) to channel 5 of each of its columns; channel 5 of a
slot and channels 6 and 7 stay 0.

Two ways to the counts: from the words (from_words) and as the per-column histogram of the rows
msa_cases.block renders (from_rows); test_profile_host.py holds them equal."""
import numpy as np

import msa_cases as A
import nw_trace_cases as T
import pileup_cases as P
import qpileup_cases as Q

CH = 8


def from_words(centre, pairs):
    """centre: its bytes; pairs: [(words, seq1 as aligned, its qualities as aligned or None)] ->
    (w, col, W, counts[W, 8], wcounts[W, 8])."""
    L, depth = len(centre), len(pairs)
    w = A.widths(L, [p[0] for p in pairs])
    col, W = A.columns(w)
    counts = np.zeros((W, CH), np.uint32)
    wcounts = np.zeros((W, CH), np.uint32)
    slot = np.zeros(W, bool)
    for r in range(L + 1):
        for t in range(int(w[r])):
            c = int(col[r]) - int(w[r]) + t
            slot[c] = True
            counts[c, 6], counts[c, 7] = r, t + 1
        if r < L:
            counts[col[r], 6] = r
    for words, read, qs in pairs:
        la = len(read)
        i = j = 0
        for wd in words:
            n, op = int(wd) >> 4, int(wd) & 15
            if op in (T.OP_EQ, T.OP_X):
                for t in range(n):
                    ch = P.channel(read[i + t])
                    counts[col[j + t], ch] += 1
                    if qs is not None:
                        wcounts[col[j + t], ch] += int(qs[i + t])
                i, j = i + n, j + n
            elif op == T.OP_D:
                around = [] if qs is None else ([int(qs[i - 1])] if i > 0 else []) + ([int(qs[i])] if i < la else [])
                for t in range(n):
                    counts[col[j + t], 5] += 1
                    wcounts[col[j + t], 5] += min(around) if around else 0
                j += n
            else:
                assert op == T.OP_I and n <= w[j]
                for t in range(n):
                    c = int(col[j]) - int(w[j]) + t
                    ch = P.channel(read[i + t])
                    counts[c, ch] += 1
                    if qs is not None:
                        wcounts[c, ch] += int(qs[i + t])
                i += n
        assert (i, j) == (la, L)
    counts[slot, 5] = depth - counts[slot, :5].sum(axis=1)
    return w, col, W, counts, wcounts


_CLASS = np.full(256, 4, np.uint8)
for _x, _c in zip(b"ACGT", range(4)):
    _CLASS[_x] = _c
_CLASS[A.GAP] = 5


def from_rows(L, w, W, rows):
    """The histogram of the pair rows rows[1:] of msa_cases.block (the centre row rows[0] is not
    counted), channels 6 and 7 from w -> counts[W, 8]."""
    col, W2 = A.columns(w)
    assert W2 == W
    counts = np.zeros((W, CH), np.uint32)
    for row in rows[1:]:
        cls = _CLASS[np.frombuffer(row, np.uint8)]
        counts[np.arange(W), cls] += 1
    for r in range(L + 1):
        for t in range(int(w[r])):
            counts[int(col[r]) - int(w[r]) + t, 6:8] = (r, t + 1)
        if r < L:
            counts[col[r], 6] = r
    return counts


def renders_its_classes(reads):
    """False if a read holds, as a raw byte above 3, one of the characters A C G T -: the rows show
    that character, the profile (like the pile-up) counts class 4, so the histogram of the rows is
    not the profile there."""
    amb = np.zeros(256, bool)
    amb[list(b"ACGT-")] = True
    return not any(amb[np.asarray(r, np.uint8)].any() for r in reads)


_cache = {}


def qualities():
    """One quality string per point of msa_cases.msa(): qpileup_cases.qualities() for pile()'s points,
    seeded values for the rest."""
    if "q" not in _cache:
        q = A.msa()
        old = list(Q.qualities())
        rng = np.random.default_rng(94)
        _cache["q"] = old + [rng.integers(0, Q.QMAX + 1, len(c)).astype(np.uint8) for c in q.codes[len(old):]]
    return _cache["q"]


def profiles(name):
    """Per target of msa_cases.msa() for the strands `name` -> (w, col, W, counts, wcounts), from the
    words under qualities(); computed once per process."""
    if ("p", name) not in _cache:
        q = A.msa()
        am = q.strands(name)
        exp = A.expected()
        ql = qualities()
        out = []
        for j in q.targets:
            ks = [k for k in range(len(q.a)) if q.b[k] == j]
            pairs = []
            for k in ks:
                x = ql[q.a[k]]
                pairs.append((exp[am[k]][k][0], q.read(k, bool(am[k])), x[::-1] if am[k] else x))
            out.append(from_words(q.codes[j], pairs))
        _cache[("p", name)] = out
    return _cache[("p", name)]


def tables(name):
    """-> (col_off[nt + 1], counts, wcounts) of all targets, mc_nw_msa_counts' layout."""
    pr = profiles(name)
    off = np.concatenate([[0], np.cumsum([p[2] for p in pr])]).astype(np.uint64)
    return off, np.concatenate([p[3] for p in pr]), np.concatenate([p[4] for p in pr])


# ---------------------------------------------------------------- host/profile.hpp in Python
def _nongap(counts, c):
    return int(counts[c][:5].sum())


def consensus_from_profile(centre, counts, wcounts=None):
    """centre: its bytes; counts (and wcounts): the W columns of its block -> (sequence, sub, del, ins)
    or, with wcounts, (sequence, quality string, sub, del, ins): pileup_cases.consensus /
    qpileup_cases.consensus from the profile alone.  depth is the sum of channels 0..5 of any
    column."""
    L, W = len(centre), len(counts)
    depth = int(counts[0][:6].sum()) if W else 0
    weighted = wcounts is not None
    if depth == 0:
        s = "".join(P.base_char(x) for x in centre)
        return (s, "!" * L, 0, 0, 0) if weighted else (s, 0, 0, 0)
    seq, qual, sub, dele, ins = [], [], 0, 0, 0
    c = 0
    for r in range(L + 1):
        s0 = c
        while c < W and int(counts[c][7]) != 0:
            assert int(counts[c][6]) == r and int(counts[c][7]) == c - s0 + 1
            c += 1
        wr = c - s0
        if wr and 2 * (depth - int(counts[s0][5])) > depth:
            ng = [_nongap(counts, s0 + t) for t in range(wr)] + [0]
            runs = {t + 1: ng[t] - ng[t + 1] for t in range(wr) if ng[t] - ng[t + 1] > 0}
            length = min(runs, key=lambda n: (-runs[n], n))
            for t in range(length):
                n = [int(v) for v in counts[s0 + t][:5]]
                if weighted:
                    wv = [int(v) for v in wcounts[s0 + t][:5]]
                    win = Q.pick(wv, n, None)
                    qual.append(Q.quality_char(wv, win))
                else:
                    win = n.index(max(n))
                seq.append(P.LETTERS[win])
            ins += 1
        if r == L:
            break
        assert int(counts[c][6]) == r and int(counts[c][7]) == 0
        n = [int(v) for v in counts[c][:6]]
        own = P.channel(centre[r])
        if weighted:
            wv = [int(v) for v in wcounts[c][:6]]
            ch = Q.pick(wv, n, own)
        else:
            ch = own if n[own] == max(n) else n.index(max(n))
        c += 1
        if ch == 5:
            dele += 1
            continue
        x = P.LETTERS[ch]
        sub += x != P.base_char(centre[r])
        seq.append(x)
        if weighted:
            qual.append(Q.quality_char(wv, ch))
    assert c == W
    s = "".join(seq)
    return (s, "".join(qual), sub, dele, ins) if weighted else (s, sub, dele, ins)
