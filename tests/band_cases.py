"""Shared by test_band_host.py and test_gpu_band.py: the certified band of DESIGN.md 3.13 restated
in Python -- the formulas of host/band.hpp, a DP that knows whether a path has left the band, and
nw_trace_cases' recurrences over the banded kernel's region with the sentinel outside it.
"""
import numpy as np

import nw_trace_cases as T

GO, GE, MATCH, MISMATCH = T.GO, T.GE, T.MATCH, T.MISMATCH
BAND_R = 4
BAND_ROWS = 64 * BAND_R
SENT = -(1 << 30)
NEG = -(1 << 40)  # no path at all (the leaving DP only)


def ub(la, lb, w):
    """The best score of a path that leaves the band of width w."""
    return min(la, lb) - abs(lb - la) - 3 * (w + 1) - 4


def above_ninf(la, lb, s):
    return s > T.neg_inf(la, lb) + min(la, lb)


def certified(la, lb, w, s):
    return above_ninf(la, lb, s) and s > ub(la, lb, w)


def need(la, lb, s):
    """w*: the least width at which the exact score s is above the bound."""
    return max(0, (min(la, lb) - abs(lb - la) - 4 - s) // 3)


def limits(la, lb, w):
    d = lb - la
    return min(0, d) - w, max(0, d) + w


def window(la, lb, w, k, rows=BAND_ROWS):
    """The columns (c0, c1) block k sweeps."""
    dlo, dhi = limits(la, lb, w)
    r0, r1 = k * rows + 1, min(la, (k + 1) * rows)
    return max(1, r0 + dlo), min(lb, r1 + dhi)


def band_cols(la, lb, w, rows=BAND_ROWS):
    return min(lb, rows + abs(lb - la) + 2 * w)


def band_choice_bytes(la, lb, w, rows=BAND_ROWS):
    return (la + rows - 1) // rows * (band_cols(la, lb, w, rows) + 63) * (rows // 2)


def plan(la, lb, s):
    """The planned width of a pair whose exact score is s (-1: the full record)."""
    if la == 0 or lb == 0 or not above_ninf(la, lb, s):
        return -1
    w = need(la, lb, s)
    return -1 if band_choice_bytes(la, lb, w) >= T.choice_bytes(la, lb) else w


def best_leaving(a, b, w):
    """The best score of a path (0, 0) -> (la, lb) through the recurrences' graph that visits a cell
    outside the band of width w (NEG: there is none).  Only real paths: the boundary states the
    reference holds at its finite "-infinity" start none."""
    la, lb = len(a), len(b)
    dlo, dhi = limits(la, lb, w)
    # [state M, X, Y][flag: has left][i][j]
    V = [[[[NEG] * (lb + 1) for _ in range(la + 1)] for _ in range(2)] for _ in range(3)]

    def out(i, j):
        return 0 if dlo <= j - i <= dhi else 1

    V[0][0][0][0] = 0
    for i in range(1, la + 1):
        V[1][out(i, 0) | (1 if any(out(k, 0) for k in range(1, i)) else 0)][i][0] = -GO - i * GE
    for j in range(1, lb + 1):
        V[2][out(0, j) | (1 if any(out(0, k) for k in range(1, j)) else 0)][0][j] = -GO - j * GE
    for i in range(1, la + 1):
        for j in range(1, lb + 1):
            o = out(i, j)
            s = MATCH if a[i - 1] == b[j - 1] else MISMATCH
            for f in (0, 1):
                g = f | o
                m = max(V[0][f][i - 1][j - 1], V[1][f][i - 1][j - 1], V[2][f][i - 1][j - 1])
                if m > NEG:
                    V[0][g][i][j] = max(V[0][g][i][j], m + s)
                x = max(V[0][f][i - 1][j] - (GO + GE), V[1][f][i - 1][j] - GE)
                if x > NEG // 2:
                    V[1][g][i][j] = max(V[1][g][i][j], x)
                y = max(V[0][f][i][j - 1] - (GO + GE), V[2][f][i][j - 1] - GE)
                if y > NEG // 2:
                    V[2][g][i][j] = max(V[2][g][i][j], y)
    return max(V[s][1][la][lb] for s in range(3))


def region(la, lb, w, rows=BAND_ROWS):
    """bool [la + 1, lb + 1]: the cells whose states the banded kernel holds as computed or real
    boundary values; every other cell is the sentinel.  Row 0 is real for block 0's columns, column 0
    for the rows of the blocks that start at column 1."""
    reg = np.zeros((la + 1, lb + 1), bool)
    reg[0, 0] = True
    for k in range((la + rows - 1) // rows):
        c0, c1 = window(la, lb, w, k, rows)
        r0, r1 = k * rows + 1, min(la, (k + 1) * rows)
        reg[r0:r1 + 1, c0:c1 + 1] = True
        if c0 == 1:
            reg[r0:r1 + 1, 0] = True
        if k == 0:
            reg[0, 1:c1 + 1] = True
    return reg


def forward_banded(seqa, seqb, ws, rows=BAND_ROWS):
    """nw_trace_cases._forward over each pair's region at its width: every state of a cell outside
    the region is SENT.  -> choices [P, LA + 1, LB + 1] and per pair (score, final state)."""
    P = len(seqa)
    las = np.array([len(x) for x in seqa])
    lbs = np.array([len(x) for x in seqb])
    assert las.min() >= 1 and lbs.min() >= 1
    LA, LB = int(las.max()), int(lbs.max())
    A = np.full((P, LA + 1), 254, np.int32)
    B = np.full((P, LB + 1), 255, np.int32)
    reg = np.zeros((P, LA + 1, LB + 1), bool)
    for p in range(P):
        A[p, :las[p]] = seqa[p]
        B[p, :lbs[p]] = seqb[p]
        reg[p, :las[p] + 1, :lbs[p] + 1] = region(int(las[p]), int(lbs[p]), int(ws[p]), rows)
    ninf = np.array([T.neg_inf(int(x), int(y)) for x, y in zip(las, lbs)], np.int32)[:, None]
    ch = np.zeros((P, LA + 1, LB + 1), np.uint8)
    z = np.zeros((P, LA + 1), np.int32)
    M2, X2, Y2 = z + ninf, z + ninf, z + ninf  # diagonal d - 2, then d - 1
    M2[:, 0], Y2[:, 0] = 0, -GO  # (0, 0)
    M1, X1, Y1 = M2.copy(), X2.copy(), Y2.copy()
    fin = np.zeros((P, 3), np.int64)
    for d in range(1, LA + LB + 1):
        M0, X0, Y0 = M1.copy(), X1.copy(), Y1.copy()
        if d <= LA:  # column 0
            real = reg[:, d, 0]
            M0[:, d] = np.where(real, ninf[:, 0], SENT)
            Y0[:, d] = np.where(real, ninf[:, 0], SENT)
            X0[:, d] = np.where(real, -GO - d * GE, SENT)
        if d <= LB:  # row 0
            real = reg[:, 0, d]
            M0[:, 0] = np.where(real, ninf[:, 0], SENT)
            X0[:, 0] = np.where(real, ninf[:, 0], SENT)
            Y0[:, 0] = np.where(real, -GO - d * GE, SENT)
        lo, hi = max(1, d - LB), min(LA, d - 1)
        if lo <= hi:
            I, Im = slice(lo, hi + 1), slice(lo - 1, hi)
            ii = np.arange(lo, hi + 1)
            inside = reg[:, ii, d - ii]
            yb, yc = M1[:, I] - (GO + GE), Y1[:, I] - GE
            yy = yb < yc
            xb, xc = M1[:, Im] - (GO + GE), X1[:, Im] - GE
            xx = xb < xc
            gM, gX, gY = M2[:, Im], X2[:, Im], Y2[:, Im]
            code = np.where(gM >= np.maximum(gX, gY), 0, np.where(gX >= gY, 1, 2))
            best = np.maximum(gM, np.maximum(gX, gY))
            s = np.where(A[:, lo - 1:hi] == B[:, d - ii - 1], MATCH, MISMATCH)
            Y0[:, I] = np.where(inside, np.where(yy, yc, yb), SENT)
            X0[:, I] = np.where(inside, np.where(xx, xc, xb), SENT)
            M0[:, I] = np.where(inside, best + s, SENT)
            ch[:, ii, d - ii] = np.where(inside, code + 4 * xx + 8 * yy, 0).astype(np.uint8)
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


def align_banded(seq_pairs, ws, rows=BAND_ROWS):
    """[(seq1, seq2)], a width each -> [(words, score, reached a boundary)] from the banded record."""
    ch, fin = forward_banded([a for a, _ in seq_pairs], [b for _, b in seq_pairs], ws, rows)
    out = []
    for p, (a, b) in enumerate(seq_pairs):
        score, state = fin[p]
        try:
            words, _, _, ok = T._traceback(a, b, np.ascontiguousarray(ch[p, :len(a) + 1, :len(b) + 1]), state)
        except AssertionError:  # (a choice word that names no state: only outside a certified band)
            words, ok = np.zeros(0, np.uint32), False
        out.append((words, score, ok))
    return out


def seeded_pairs(rng, n, lo, hi):
    """n pairs of lengths lo .. hi: 30 % unrelated, 10 % homopolymers, 60 % copies with up to four
    indels of 1 .. 4 bases or substitutions."""
    out = []
    for _ in range(n):
        kind = rng.random()
        la = int(rng.integers(lo, hi + 1))
        if kind < 0.3:
            a = rng.integers(0, 4, la).astype(np.uint8)
            b = rng.integers(0, 4, int(rng.integers(lo, hi + 1))).astype(np.uint8)
        elif kind < 0.4:
            c = int(rng.integers(0, 4))
            a = np.full(la, c, np.uint8)
            b = np.full(int(rng.integers(lo, hi + 1)), c, np.uint8)
        else:
            a = rng.integers(0, 4, la).astype(np.uint8)
            b = list(a)
            for _ in range(int(rng.integers(0, 5))):
                at = int(rng.integers(0, len(b) + 1))
                what = int(rng.integers(0, 3))
                n_b = int(rng.integers(1, 5))
                if what == 0:
                    b[at:at] = [int(v) for v in rng.integers(0, 4, n_b)]
                elif what == 1:
                    del b[at:at + n_b]
                elif at < len(b):
                    b[at] = (b[at] + 1 + int(rng.integers(0, 3))) % 4
            b = np.array(b[:hi] if len(b) >= lo else list(a), np.uint8)
        out.append((a, b))
    return out
