"""The certified band without a GPU: the bound on paths that leave the band, the
equality of the certified banded chain with the full matrix's, and host/band.hpp against the Python
formulas (tests/native/band_check.cpp, a stand-alone program that includes the header alone)."""
import os
import subprocess

import numpy as np

import band_cases as Bc
import fixtures
import nw_trace_cases as T

ROOT = fixtures.HERE.rsplit(os.sep, 1)[0]
HOST_SRC = os.path.join(ROOT, "meshclust_amd", "csrc", "host")
SRC = os.path.join(fixtures.HERE, "native", "band_check.cpp")
WIDTHS = (0, 1, 2, 3, 5, 8)


def test_leaving_paths_stay_below_the_bound():
    rng = np.random.default_rng(11)
    pairs = Bc.seeded_pairs(rng, 600, 1, 14)
    cases = tight = 0
    for a, b in pairs:
        for w in range(6):
            best = Bc.best_leaving(a, b, w)
            if best == Bc.NEG:  # (the band holds the whole matrix: no path leaves it)
                assert Bc.region(len(a), len(b), w, 1).all()
                continue
            cases += 1
            assert best <= Bc.ub(len(a), len(b), w), (list(a), list(b), w, best)
            tight += best == Bc.ub(len(a), len(b), w)
    assert cases >= 1000 and tight >= 100, (cases, tight)  # the bound is reached: it is tight


def _chain_census(rows, n_pairs, seed):
    rng = np.random.default_rng(seed)
    pairs = Bc.seeded_pairs(rng, n_pairs, 1, 30)
    full = T.align_all(pairs)
    cases = [(k, w) for k in range(len(pairs)) for w in WIDTHS]
    band = Bc.align_banded([pairs[k] for k, _ in cases], [w for _, w in cases], rows)
    cert = differ = 0
    for (k, w), (words, score, ok) in zip(cases, band):
        a, b = pairs[k]
        fw, fs = full[k][0], full[k][1]
        same = ok and score == fs and np.array_equal(words, fw)
        assert score <= fs  # monotone: a banded value never exceeds the full one
        if Bc.certified(len(a), len(b), w, score):
            cert += 1
            assert same, (list(a), list(b), w, score, fs)
            assert Bc.need(len(a), len(b), fs) <= w  # the width the pair needs is no more than a certified one
        else:
            differ += not same
    return len(cases), cert, differ


def test_certified_chain_is_the_full_chain_kernel_windows():
    """The kernel's own BAND_ROWS: at these lengths a pair is one block, whose window is every column
    (r1 + dhi >= lb), so the banded record is the full one whether certified or not."""
    n, cert, differ = _chain_census(Bc.BAND_ROWS, 1000, 5)
    assert 2 * cert >= n and differ == 0, (n, cert, differ)


def test_certified_chain_is_the_full_chain_small_blocks():
    """The same geometry at 4 rows per block, so that every block's left edge, the sentinel above a
    block and the untouched column 0 all occur at these lengths."""
    n, cert, differ = _chain_census(4, 3000, 6)
    assert 2 * cert >= n and differ >= 100, (n, cert, differ)


def test_certified_chain_two_real_blocks():
    """Pairs of more than BAND_ROWS rows: the real windows of a second and third block."""
    rng = np.random.default_rng(8)
    pairs = []
    for la in (257, 300, 520):
        a = rng.integers(0, 4, la).astype(np.uint8)
        pairs.append((a, T.mutate(rng, a, 0.03)))
        cut = int(rng.integers(100, la - 60))
        pairs.append((a, np.concatenate([a[:cut], a[cut + 30:]])))
        pairs.append((np.concatenate([a[:cut], a[cut + 30:]]), a))
    full = T.align_all(pairs)
    ws = [Bc.need(len(a), len(b), full[k][1]) for k, (a, b) in enumerate(pairs)]
    band = Bc.align_banded(pairs, ws)
    for k, (words, score, ok) in enumerate(band):
        a, b = pairs[k]
        assert Bc.certified(len(a), len(b), ws[k], score), k
        assert ok and score == full[k][1] and np.array_equal(words, full[k][0]), k
    assert any(w > 0 for w in ws) and any(not Bc.region(len(a), len(b), w).all() for (a, b), w in zip(pairs, ws))


def test_band_native(tmp_path):
    exe = str(tmp_path / "band_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", HOST_SRC, SRC, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.endswith("OK\n"), r.stdout[-2000:] + r.stderr
    grid = plans = 0
    for line in r.stdout.splitlines():
        if line[0] == "R":
            assert [int(v) for v in line.split()[1:]] == [Bc.BAND_R, Bc.BAND_ROWS, Bc.SENT]
            continue
        if line == "OK":
            continue
        key, val = line.split(" : ")
        kind, la, lb, x = key.split()
        la, lb, x, val = int(la), int(lb), int(x), [int(v) for v in val.split()]
        if kind == "G":
            w, nblk = x, (la + Bc.BAND_ROWS - 1) // Bc.BAND_ROWS
            cols = Bc.band_cols(la, lb, w)
            want = [Bc.ub(la, lb, w), int(w >= max(la, lb)), cols, cols + 63, Bc.band_choice_bytes(la, lb, w),
                    3 * (cols + 1) if la > Bc.BAND_ROWS else 0, nblk]
            for k in range(nblk):
                want += list(Bc.window(la, lb, w, k))
            assert val == want, line
            grid += 1
        else:
            s = x
            want = [T.neg_inf(la, lb), int(Bc.above_ninf(la, lb, s)), Bc.need(la, lb, s), Bc.plan(la, lb, s), T.choice_bytes(la, lb)]
            want += [int(Bc.certified(la, lb, w, s)) for w in (0, 1, 7, 64)]
            assert val == want, line
            plans += 1
    assert grid >= 2000 and plans >= 3000, (grid, plans)
