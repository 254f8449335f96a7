"""mc_revcomp_rows / mc_assign_strands / meshclust-assign --both-strands: reads on either strand.

Every value is compared with ==, and every expectation comes from code that existed before the
strands did: the histograms of reverse-complemented records loaded as points of their own
(mc_get_histograms), and mc_assign on those points combined in numpy by the rule of the header
(minus wins only with a strictly larger combo 0, the counts add).

Points: the 1000 a1k reads (ids 0..999), the reverse complements of reads 100..360 (ids
1000..1260), and four hand-made records: two segments around an N gap (G) and its mirror (GM),
a record without any segment (E: its row is all pseudocounts), and a reverse-palindromic
record s + RC(s) (P: its row equals its own permutation).
"""
import os
import subprocess

import numpy as np
import pytest

import fixtures
import meshclust_amd as M
import oracle_lib as O

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
N_READS, RC0, RC1 = 1000, 100, 361  # reads RC0 .. RC1 - 1 are also loaded reverse-complemented
G, GM, E, P = (N_READS + (RC1 - RC0) + i for i in range(4))
N_POINTS = P + 1
ASSIGN_BIN = os.path.join(os.path.dirname(M.BIN), "meshclust-assign")


def partner(ids):
    """The point holding the reverse complement of each point (only for ids that have one)."""
    ids = np.asarray(ids, np.int64)
    out = np.full(len(ids), -1, np.int64)
    fwd = (ids >= RC0) & (ids < RC1)
    rev = (ids >= N_READS) & (ids < G)
    out[fwd] = ids[fwd] - RC0 + N_READS
    out[rev] = ids[rev] - N_READS + RC0
    for a, b in ((G, GM), (GM, G), (E, E), (P, P)):
        out[ids == a] = b
    assert (out >= 0).all()
    return out.astype(np.uint32)


# 264 queries (more than one workgroup of the short form): forward reads, reverse-complemented
# points, the palindrome, the gapped record and the empty one
QUERIES = np.concatenate([np.arange(RC0, RC1, 2), np.arange(N_READS + 1, G, 2), [P, G, E]]).astype(np.uint32)
# centres: forward reads, the palindrome, one reverse-complemented point; SET_B repeats id 3
SET_A = np.concatenate([np.arange(23), [P, N_READS + 5]]).astype(np.uint32)
SET_B = np.array([0, 1, 2, 3, 4, 5, 6, 3, P], np.uint32)


@pytest.fixture(scope="module")
def eng(built):
    e = M.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def points():
    """(codes per point, segments per point, lengths)."""
    recs = fixtures.synth_records(*fixtures.manifest()["e2e"]["a1k"]["generator"])
    assert len(recs) == N_READS
    codes = [c.astype(np.uint8) for _, c, _ in recs]
    segs = [[[0, len(c) - 1]] for c in codes]
    for i in range(RC0, RC1):
        codes.append((3 - codes[i][::-1]).astype(np.uint8))
        segs.append([[0, len(codes[i]) - 1]])
    rng = np.random.default_rng(7)
    a, b = rng.integers(0, 4, 70).astype(np.uint8), rng.integers(0, 4, 45).astype(np.uint8)
    gap = np.full(6, ord("N"), np.uint8)
    codes.append(np.concatenate([a, gap, b]))  # G: segments [0, 69] and [76, 120]
    segs.append([[0, 69], [76, 120]])
    codes.append(np.concatenate([3 - b[::-1], gap, 3 - a[::-1]]).astype(np.uint8))  # GM: its mirror
    segs.append([[0, 44], [51, 120]])
    codes.append(np.full(30, ord("N"), np.uint8))  # E: no segment at all
    segs.append([])
    s = rng.integers(0, 4, 250).astype(np.uint8)
    codes.append(np.concatenate([s, 3 - s[::-1]]).astype(np.uint8))  # P = s + RC(s)
    segs.append([[0, 499]])
    assert len(codes) == N_POINTS
    return codes, segs, np.array([len(c) for c in codes], np.uint64)


_state = {}


def setup(eng, points, k, width, cls=None):
    codes, segs, lens = points
    if _state.get("eng") is not eng:
        _state.clear()
        _state["eng"] = eng
        seq_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        seg = np.array([v for s in segs for pair in s for v in pair], np.int32)
        seg_off = np.concatenate([[0], np.cumsum([len(s) for s in segs])]).astype(np.uint64)
        eng.load_sequences(np.concatenate(codes), seq_off, seg, seg_off)
    if _state.get("kw") != (k, width):
        assert eng.kmer_max(k) < (1 << (8 * width))
        eng.kmer_build(k, width)
        _state["kw"] = (k, width)
    if cls is None:
        cls = O.classifier_from_golden(np.load(fixtures.golden("train_a1k.npz")))
    eng.set_classifier(cls)


# ---------------------------------------------------------------- 1. the permutation
@pytest.mark.parametrize("k,width", [(1, 1), (3, 1), (4, 1), (5, 1), (6, 1), (3, 2), (4, 2)])
def test_revcomp_rows_are_the_histograms_of_the_other_strand(eng, points, k, width):
    """A row smaller than one 16-byte chunk (k = 1), the 4- and 16-chunk rows, rows wider than
    the short form (k = 5, 6), 16-bit bins, and the odd k where rc has no fixed point."""
    setup(eng, points, k, width)
    h, _ = eng.histograms()
    assert h.shape == (N_POINTS, 4 ** k)
    ids = np.concatenate([np.arange(RC0, RC1), np.arange(N_READS, G), [G, GM, E, P]]).astype(np.uint32)
    got = eng.revcomp_rows(ids)
    assert got.dtype == h.dtype and got.shape == (len(ids), 4 ** k)
    assert np.array_equal(got, h[partner(ids)])
    assert (h[E] == 1).all()  # no segment: pseudocounts only
    assert np.array_equal(eng.revcomp_rows([P])[0], h[P])  # the palindrome is its own permutation
    assert not np.array_equal(h[RC0], h[N_READS]) and not np.array_equal(h[G], h[GM])  # (the check can fail)
    assert np.array_equal(eng.revcomp_rows([RC0, RC0])[1], h[N_READS])  # a repeated id
    assert eng.revcomp_rows([]).shape == (0, 4 ** k)


# ---------------------------------------------------------------- 2. equality with mc_assign
def combine(plus, minus):
    """The header's rule on two mc_assign results -> (best, best_val, strand, n_similar)."""
    (jp, vp, n_p, _), (jm, vm, n_m, _) = plus, minus
    win = (jm != NONE) & ((jp == NONE) | (vm > vp))
    return np.where(win, jm, jp), np.where(win, vm, vp), win.astype(np.uint8), (n_p + n_m).astype(np.uint32)


CONFIGS = {"short_k4": (4, 1, None), "general_k4": (4, 1, "general"), "k4_u16": (4, 2, None), "k5_u8": (5, 1, None)}


@pytest.mark.parametrize("tile", ["7", None], ids=["tile7", "tile_default"])
@pytest.mark.parametrize("config", list(CONFIGS))
def test_assign_strands_equals_mc_assign(eng, points, config, tile, monkeypatch):
    k, width, form = CONFIGS[config]
    setup(eng, points, k, width)
    for name, val in (("MC_ASSIGN_TILE", tile), ("MC_ASSIGN_FORM", form)):
        if val:
            monkeypatch.setenv(name, val)
        else:
            monkeypatch.delenv(name, raising=False)
    seen = dict(minus_wins=False, plus_wins=False, unassigned=False, both_strands=False, gated=False)
    for centres in (SET_A, SET_B):
        for sim in (0.0, 0.9):
            plus = eng.assign(centres, QUERIES, sim)
            minus = eng.assign(centres, partner(QUERIES), sim)
            assert int(plus[3][0]) == int(minus[3][0])  # the gate does not depend on the strand
            got = eng.assign_strands(centres, QUERIES, sim, M.MC_STRAND_PLUS)
            for x, y in zip((got[0], got[1], got[3]), plus[:3]):
                assert np.array_equal(x, y)
            assert not got[2].any() and int(got[4][0]) == int(plus[3][0]) and int(got[4][1]) == int(plus[3][1])
            got = eng.assign_strands(centres, QUERIES, sim, M.MC_STRAND_MINUS)
            for x, y in zip((got[0], got[1], got[3]), minus[:3]):
                assert np.array_equal(x, y)
            assert (got[2] == 1).all() and int(got[4][0]) == int(minus[3][0]) and int(got[4][1]) == int(minus[3][1])
            want = combine(plus, minus)
            got = eng.assign_strands(centres, QUERIES, sim)
            for x, y in zip(got[:4], want):
                assert x.dtype == y.dtype and np.array_equal(x, y)
            assert int(got[4][0]) == int(plus[3][0])  # pairs after the gate, counted once
            assert int(got[4][1]) == int(plus[3][1]) + int(minus[3][1])  # fall-backs per (pair, strand)
            seen["minus_wins"] |= bool((want[2] == 1).any())
            seen["plus_wins"] |= bool(((want[2] == 0) & (want[0] != NONE)).any())
            seen["unassigned"] |= bool((want[0] == NONE).any())
            seen["both_strands"] |= bool(((plus[2] > 0) & (minus[2] > 0)).any())
            seen["gated"] |= int(plus[3][0]) < len(QUERIES) * len(centres)
    assert all(seen.values()), seen


# ---------------------------------------------------------------- 3. the strand tie
@pytest.mark.parametrize("form", [None, "general"], ids=["short", "general"])
def test_palindrome_ties_and_goes_to_plus(eng, points, form, monkeypatch):
    setup(eng, points, 4, 1)
    monkeypatch.delenv("MC_ASSIGN_TILE", raising=False)
    if form:
        monkeypatch.setenv("MC_ASSIGN_FORM", form)
    else:
        monkeypatch.delenv("MC_ASSIGN_FORM", raising=False)
    q = np.array([P], np.uint32)
    plus = eng.assign(SET_A, q)
    minus = eng.assign(SET_A, partner(q))
    assert plus[0][0] != NONE and plus[0][0] == minus[0][0] and plus[1][0] == minus[1][0]  # an exact tie
    assert SET_A[plus[0][0]] == P
    best, val, strand, nsim, _ = eng.assign_strands(SET_A, q)
    assert best[0] == plus[0][0] and val[0] == plus[1][0] and strand[0] == 0 and nsim[0] == 2 * plus[2][0]


# ---------------------------------------------------------------- 4. error codes
def test_assign_strands_errors(eng, points):
    setup(eng, points, 4, 1)
    for strands in (0, 4):
        with pytest.raises(M.MCError) as e:
            eng.assign_strands(SET_A, QUERIES, 0.0, strands)
        assert e.value.code == M.ERR_ARG
    best, val, strand, nsim, stats = eng.assign_strands(SET_A, [])  # M = 0
    assert len(best) == 0 and len(strand) == 0 and int(stats[0]) == 0
    al = O.Classifier()
    al.n_single, al.n_combo = 1, 1
    al.lookup[0], al.is_sim[0], al.mins[0], al.maxs[0] = M.FEAT_ALIGN, 1, 0.0, 1.0
    al.combo_kind[0], al.combo_len[0], al.combo_idx[0][0] = M.COMBO_SELF, 1, 0
    al.weights[0], al.weights[1] = -0.5, 1.0
    setup(eng, points, 4, 1, al)
    with pytest.raises(M.MCError) as e:
        eng.assign_strands(SET_A, QUERIES)
    assert e.value.code == M.ERR_UNSUPPORTED
    setup(eng, points, 3, 4)  # 32-bit bins
    for call in (lambda: eng.assign_strands(SET_A, QUERIES), lambda: eng.revcomp_rows(SET_A)):
        with pytest.raises(M.MCError) as e:
            call()
        assert e.value.code == M.ERR_UNSUPPORTED


# ---------------------------------------------------------------- 5. end to end
_RC = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def read_fasta(path):
    recs = []
    with open(path, "rb") as f:
        for ln in f.read().splitlines():
            if ln.startswith(b">"):
                recs.append([ln, b""])
            else:
                recs[-1][1] += ln
    return recs


def write_fasta(path, recs):
    with open(path, "wb") as f:
        for h, s in recs:
            f.write(h + b"\n" + s + b"\n")


def run_assign(model, cen, reads, tsv, extra=(), env=None):
    e = dict(os.environ, **(env or {}))
    for name in ("MC_ASSIGN_FORM", "MC_ASSIGN_TILE", "MC_ASSIGN_PAIRS"):
        if not env or name not in env:
            e.pop(name, None)
    r = subprocess.run([ASSIGN_BIN, "--model", str(model), "--centres", str(cen), str(reads), "--output", str(tsv),
                        "--quiet"] + list(extra), capture_output=True, text=True, timeout=300, env=e)
    return r


def test_cli_both_strands(eng, tmp_path):
    fa, flags = fixtures.e2e_input("a1k", tmp_path)
    model, cen = tmp_path / "a1k.model", tmp_path / "a1k.centres.fa"
    r = subprocess.run([M.BIN, fa] + flags + ["--output", str(tmp_path / "a1k.clstr"), "--quiet", "--save-model", str(model),
                                              "--save-centres", str(cen)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    recs = read_fasta(fa)
    f_recs = [(h, s.translate(_RC)[::-1] if i % 2 else s) for i, (h, s) in enumerate(recs)]
    ffa, rfa = tmp_path / "F.fa", tmp_path / "R.fa"
    write_fasta(ffa, f_recs)
    write_fasta(rfa, [(h, s.translate(_RC)[::-1]) for h, s in f_recs])
    rows = {}
    for name, reads in (("F", ffa), ("R", rfa)):
        r = run_assign(model, cen, reads, tmp_path / (name + ".tsv"))
        assert r.returncode == 0, r.stderr[-3000:]
        rows[name] = [ln.split("\t") for ln in (tmp_path / (name + ".tsv")).read_text().splitlines()]
        assert all(len(x) == 5 for x in rows[name])  # no flag: no strand column
    want = []
    for p, m in zip(rows["F"], rows["R"]):
        assert p[0] == m[0]
        minus = m[2] != "-1" and (p[2] == "-1" or float(m[3]) > float(p[3]))
        w = m if minus else p
        want.append([w[0], w[1], w[2], w[3], str(int(p[4]) + int(m[4])), "*" if w[2] == "-1" else "-" if minus else "+"])
    stats = tmp_path / "both.json"
    r = run_assign(model, cen, ffa, tmp_path / "both.tsv", ["--both-strands", "--stats-json", str(stats)])
    assert r.returncode == 0, r.stderr[-3000:]
    got = [ln.split("\t") for ln in (tmp_path / "both.tsv").read_text().splitlines()]
    assert got == want
    n_plus_only = sum(x[2] != "-1" for x in rows["F"])
    n_both = sum(x[2] != "-1" for x in got)
    n_minus = sum(x[5] == "-" for x in got)
    assert n_plus_only < n_both and n_minus > 0  # one strand alone loses reads
    import json
    st = json.loads(stats.read_text())
    assert st["strands"] == 3 and st["assigned_minus"] == n_minus and st["assigned"] == n_both and st["path"] == "device"
    # the same job in process (mcl_assign_strands), and without the flag the file of today
    st = M.assign_files(eng, str(model), str(cen), str(ffa), str(tmp_path / "lib.tsv"), threads=2, both_strands=True)
    _state.clear()  # (the context now holds other sequences)
    assert (tmp_path / "lib.tsv").read_bytes() == (tmp_path / "both.tsv").read_bytes()
    assert st["strands"] == 3 and st["assigned_minus"] == n_minus
    st = M.assign_files(eng, str(model), str(cen), str(ffa), str(tmp_path / "lib1.tsv"), threads=2)
    assert (tmp_path / "lib1.tsv").read_bytes() == (tmp_path / "F.tsv").read_bytes()
    assert "strands" not in st and "assigned_minus" not in st
    # where the device kernel does not apply the flag is refused, never scored on one strand
    r = run_assign(model, cen, ffa, tmp_path / "x.tsv", ["--both-strands"], env={"MC_FORCE_WIDTH": "4"})
    assert r.returncode == 2 and "--both-strands" in r.stderr and not (tmp_path / "x.tsv").exists()
