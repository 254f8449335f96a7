"""mc_nw_msa_crossover / host/chimera.hpp, the parts that need no GPU:
  * the two Python restatements of tests/crossover_cases.py (from the operation words, and from the rows
    msa_cases.block renders) agree on every candidate and strand naming, and the case set holds what it is for;
  * the consequences of the definition: the ids, best >= max(ids), x == y, the exchange of x and y, a read
    of no bases;
  * the planted chimeras, on the restatement alone: every planted cut within [cut_first, cut_last] of the
    winning order, every planted gain 3 or more, every pure read's gain 0;
  * host/chimera.hpp (tests/native/chimera_check.cpp) passes its own check and gives the answers of
    crossover_cases' port on seeded tables, with a census of ties and of gain == N on both sides;
  * the header, the exports, the Engine methods, the usage text and assign_files' parameters."""
import os
import subprocess

import numpy as np
import pytest

import crossover_cases as X
import fixtures
import meshclust_amd as M
import nw_trace_cases as T

ROOT = fixtures.HERE.rsplit(os.sep, 1)[0]
HOST_SRC = os.path.join(ROOT, "meshclust_amd", "csrc", "host")


@pytest.mark.parametrize("name", X.NAMES)
def test_the_two_restatements_agree(name):
    q = X.cross()
    want, rows = X.expected(name), X.expected(name, "rows")
    assert want.shape == (len(q.x), X.RES) and want.dtype == np.int32
    assert np.array_equal(want, rows), np.nonzero((want != rows).any(axis=1))[0]
    for k, (ew, er) in enumerate(zip(X.bitmaps(name), X.bitmaps(name, "rows"))):
        assert np.array_equal(ew, er), (name, k)


def test_the_case_set_holds_what_it_is_for():
    q = X.cross()
    plus = X.aligned()[0]
    m = len(q.a)
    assert all(q.a[int(x)] == q.a[int(y)] for x, y in zip(q.x, q.y)) and q.x.max() < m and q.y.max() < m
    assert sorted(set(int(j) for j in q.b)) == sorted(int(j) for j in q.targets)
    per_read = {}
    for k in range(m):
        per_read.setdefault(int(q.a[k]), []).append(int(q.b[k]))
    assert {len(set(v)) for v in per_read.values()} == {1, 2, 3}  # two and three targets (one: the chunk-edge reads)
    lens = {q.la(int(x)) for x in q.x}
    assert set(X.SMALL) | {0, 2047, 2048, 2049} <= lens
    assert sum(max(q.la(k), len(q.codes[q.b[k]])) > 600 for k in range(m)) == 4
    nwords = lambda k: len(plus[k][0])
    assert 64 < nwords(q.mid[0]) <= 128 and all(nwords(k) > 128 for k in q.long2048)
    assert all(max(q.la(k), len(q.codes[q.b[k]])) <= 600 for k in q.mid)
    # '=' runs inside one bitmap word, across two words, and over more than 64 words
    inside = two = 0
    for k in range(m):
        i = 0
        for wd in plus[k][0]:
            n, op = int(wd) >> 4, int(wd) & 15
            if op == T.OP_EQ:
                span = (i + n - 1) // 32 - i // 32
                inside += span == 0
                two += span == 1
            if op != T.OP_D:
                i += n
    words, = [plus[k][0] for k in q.long2049]
    assert inside and two and int(words[0]) == (2049 << 4 | T.OP_EQ) and (2049 - 1) // 32 - 0 == 64  # words 0 .. 64
    # strands: a candidate whose two pairs differ under the mixed naming; x == y
    am = q.strands("mixed")
    assert any(am[int(x)] != am[int(y)] for x, y in zip(q.x, q.y)) and any(am[int(x)] == am[int(y)] == v for v in (0, 1) for x, y in zip(q.x, q.y))
    assert sum(int(x) == int(y) for x, y in zip(q.x, q.y)) == 6
    # the planted reads: A[:cut] + B[cut':], cuts in [30, 90)
    pa, pb = (q.codes[j] for j in q.parents)
    assert len(pa) == 120 and len(q.planted) == 6 and len(q.pure) == 6
    for c, cut in q.planted:
        r = q.codes[q.a[int(q.x[c])]]
        assert 30 <= cut < 90 and np.array_equal(r[:cut], pa[:cut]) and np.array_equal(r[cut:], pb[len(pb) - (len(r) - cut):])
        assert [int(q.b[int(q.x[c])]), int(q.b[int(q.y[c])])] == q.parents


@pytest.mark.parametrize("name", X.NAMES)
def test_consequences_of_the_definition(name):
    q = X.cross()
    want = X.expected(name)
    e = X.bitmaps(name)
    al = X.aligned()
    am = q.strands(name)
    ids = np.array([al[am[k]][k][3] for k in range(len(q.a))])  # the '=' counts of the alignments
    assert np.array_equal(want[:, 0], ids[q.x.astype(np.int64)]) and np.array_equal(want[:, 1], ids[q.y.astype(np.int64)])
    assert all(int(e[k].sum()) == ids[k] for k in range(len(q.a)))
    single = np.maximum(want[:, 0], want[:, 1])
    assert (want[:, 2] >= single).all() and (want[:, 5] >= single).all()
    la = np.array([q.la(int(x)) for x in q.x])
    assert (want[:, 3] <= want[:, 4]).all() and (want[:, 6] <= want[:, 7]).all() and (want[:, [3, 4, 6, 7]] >= 0).all()
    assert (want[:, [4, 7]] <= la[:, None]).all()
    same = q.x == q.y
    assert same.any() and all(v.tolist() == [i, i, i, 0, n, i, 0, n] for v, i, n in zip(want[same], want[same, 0], la[same]))
    for c in range(len(q.x)):  # the exchange of x and y
        assert np.array_equal(X.crossover(e[int(q.y[c])], e[int(q.x[c])]), X.exchanged(want[c])), c
    none = [c for c in range(len(q.x)) if q.la(int(q.x[c])) == 0]  # the read of no bases: eight zeros
    assert len(none) == 2 and not want[none].any() and X.crossover(np.zeros(0, np.uint8), np.zeros(0, np.uint8)).tolist() == [0] * 8


def test_small_cases_by_hand():
    bits = lambda s: np.array([int(ch) for ch in s], np.uint8)
    # x matches the left half, y the right half: the best cut is between them, both ways of naming
    v = X.crossover(bits("11110000"), bits("00001111"))
    assert v.tolist() == [4, 4, 8, 4, 4, 4, 0, 8]
    assert X.exchanged(v).tolist() == X.crossover(bits("00001111"), bits("11110000")).tolist() == [4, 4, 4, 0, 8, 8, 4, 4]
    # a stretch where both agree leaves the cut free: first and last differ
    assert X.crossover(bits("1011100"), bits("0011111")).tolist() == [4, 5, 6, 1, 5, 5, 7, 7]
    assert X.chimera_order([4, 5, 6, 1, 5, 6, 0, 0]) == (True, 6, 1, 1, 5, 4, 5)  # a tie goes to xy
    assert X.chimera_order([4, 5, 5, 0, 0, 7, 2, 3]) == (False, 7, 2, 2, 3, 5, 4)
    assert X.chimera_candidates([7, 7, 3, 7, 2]) == [2, 4] and X.chimera_candidates([7]) == [] and X.chimera_candidates([]) == []
    res = [[90, 80, 93, 1, 2, 90, 0, 0], [90, 85, 93, 5, 6, 91, 0, 0], [90, 70, 92, 0, 0, 90, 0, 0]]
    assert X.chimera_pick([1, 2, 4], res, 3) == (1, True, 93, 3, 1, 2, 90, 80, True)  # equal gains: the lowest hit
    assert X.chimera_pick([1, 2, 4], res, 4)[-1] is False and X.chimera_pick([], [], 1) is None


def test_planted_chimeras_on_the_restatement():
    q = X.cross()
    want = X.expected("plus")  # the reads are planted as written
    for c, cut in q.planted:
        xy, best, gain, first, last, left, right = X.chimera_order(want[c])
        assert xy and first <= cut <= last and gain >= 3, (q.label[c], cut, first, last, gain)
        assert best > max(left, right)
    for c in q.pure:
        assert X.chimera_order(want[c])[2] == 0, q.label[c]


# ---------------------------------------------------------------- host/chimera.hpp
def test_chimera_native(tmp_path):
    exe = str(tmp_path / "chimera_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-I", HOST_SRC, os.path.join(fixtures.HERE, "native", "chimera_check.cpp"), "-o", exe],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)  # its own seeded check and census
    assert r.returncode == 0 and r.stdout.startswith("OK\n"), r.stdout[-2000:] + r.stderr
    rng = np.random.default_rng(78)
    cases, text = [], []
    want = X.expected("mixed")
    for c in range(len(want)):  # the case set's own values: a read of two hits
        cases.append((3, [0, 1], [want[c].tolist()]))
    for _ in range(1500):  # seeded tables of close values: ties are common
        n = int(rng.integers(0, 6))
        centres = rng.integers(0, 4, n).tolist()
        vals = []
        for _ in range(max(n - 1, 0)):
            ix, iy = (int(v) for v in rng.integers(90, 101, 2))
            s = max(ix, iy)
            vals.append([ix, iy, s + int(rng.integers(0, 5)), int(rng.integers(0, 50)), int(rng.integers(50, 101)),
                         s + int(rng.integers(0, 5)), int(rng.integers(0, 50)), int(rng.integers(50, 101))])
        cases.append((int(rng.integers(1, 5)), centres, vals))
    for g, centres, vals in cases:
        text.append(" ".join(str(v) for v in [len(centres), g] + centres + [x for v in vals for x in v]))
    fix = tmp_path / "cases.txt"
    fix.write_text("\n".join(text) + "\n")
    r = subprocess.run([exe, str(fix)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("OK\n"), r.stdout[-2000:] + r.stderr
    lines = r.stdout.splitlines()
    assert int(lines[1]) == len(cases) and len(lines) == 3 + len(cases)
    census = dict(none=0, same_centre=0, tie_order=0, tie_gain=0, at_gain=0, below_gain=0)
    for (g, centres, vals), ln in zip(cases, lines[3:]):
        cand = X.chimera_candidates(centres)
        census["same_centre"] += max(len(centres) - 1, 0) - len(cand)
        census["tie_order"] += sum(vals[j - 1][2] == vals[j - 1][5] for j in cand)
        pick = X.chimera_pick(cand, [vals[j - 1] for j in cand], g)
        if pick is None:
            census["none"] += 1
            assert ln == "-1"
            continue
        gains = sorted((X.chimera_order(vals[j - 1])[2] for j in cand), reverse=True)
        census["tie_gain"] += len(gains) > 1 and gains[0] == gains[1]
        census["at_gain"] += gains[0] == g
        census["below_gain"] += gains[0] + 1 == g
        assert pick[3] == gains[0] and [int(v) for v in ln.split(" ")] == [int(v) for v in pick], (ln, pick)
    assert [int(v) for v in lines[2].split(" ")] == list(census.values())
    assert all(v > 20 for v in census.values()), census


# ---------------------------------------------------------------- what is declared, exported and documented
@pytest.fixture(scope="module")
def host_built(built):
    M.build()


def test_new_entries_are_declared(built):
    header = open(M.HEADER).read()
    for text in ("#define MC_CROSS_RES 8", "#define MC_CROSS_MAX_READ (1u << 18)", "MC_CROSS_BATCH_CANDS",
                 "int mc_nw_msa_crossover(mc_ctx *ctx, const uint64_t *x, const uint64_t *y, uint64_t nc, int32_t *out",
                 "int mc_nw_msa_crossover_profile(mc_ctx *ctx, double *out"):
        assert text in header, text
    assert hasattr(M.Engine, "nw_msa_crossover") and hasattr(M.Engine, "nw_msa_crossover_profile") and M.CROSS_RES == X.RES == 8
    assert os.path.exists(os.path.join(HOST_SRC, "chimera.hpp"))
    assert os.path.exists(os.path.join(ROOT, "meshclust_amd", "csrc", "gpu", "crossover.hip"))


def test_new_entries_are_exported(host_built):
    lib = M.gpu_lib()
    assert hasattr(lib, "mc_nw_msa_crossover") and hasattr(lib, "mc_nw_msa_crossover_profile") and hasattr(M.host_lib(), "mcl_assign_chimeras")
    assign = os.path.join(os.path.dirname(M.BIN), "meshclust-assign")
    sym = subprocess.run(["nm", "-D", "--undefined-only", assign], capture_output=True, text=True, check=True).stdout
    assert " mc_nw_msa_crossover" in sym
    r = subprocess.run([assign], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and all(x in r.stderr for x in ("--chimeras FILE", "--min-chimera-gain N", "not tuned", "Real data was not measured"))
    import inspect
    par = inspect.signature(M.assign_files).parameters
    assert "chimeras" in par and par["chimeras"].default is None and par["min_chimera_gain"].default == 3


def test_usage_errors_name_both_options(host_built, tmp_path):
    assign = os.path.join(os.path.dirname(M.BIN), "meshclust-assign")
    f = tmp_path / "x.fa"
    f.write_text(">a\nACGT\n")
    base = [assign, "--model", str(f), "--centres", str(f), str(f), "--output", str(tmp_path / "o.tsv"), "--chimeras", str(tmp_path / "c.tsv")]
    for extra in ([], ["--top", "1", "--hits", str(tmp_path / "h.tsv")]):
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and "--chimeras FILE needs --top K with K >= 2" in r.stderr, r.stderr[:300]
    for bad in ("0", "-2", "x", "1.5"):
        r = subprocess.run(base + ["--top", "2", "--hits", str(tmp_path / "h.tsv"), "--min-chimera-gain", bad], capture_output=True, text=True,
                           timeout=120)
        assert r.returncode == 1 and "--min-chimera-gain must be 1 or more" in r.stderr, (bad, r.stderr[:300])
    assert not (tmp_path / "c.tsv").exists()
