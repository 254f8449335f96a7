"""mc_derep / host/derep.hpp / meshclust-derep, the parts that need no GPU:
  * the case set of tests/derep_cases.py holds what it is for: a census of every length, both orientations,
    every near-miss kind and every start offset mod 16 and mod 4 among the duplicates;
  * consequences of the definition on the Python restatement: rep[rep] == rep, rep <= position, the plus-only
    classes refine the both-strand classes, a permuted id list gives the permuted classes;
  * tests/native/derep_check.cpp: derep_host against an O(m^2) brute force on seeded sets, the planner with keys
    cut to 0, 1 and 4 bits ending in the same classes, derep_classes' order with ties;
  * libmeshclust's derep_host equals the restatement on the case set;
  * the header declares mc_derep and mc_derep_profile and libmcgpu.so exports them; Engine.derep, derep_files and
    the tool's usage text exist."""
import inspect
import os
import subprocess

import numpy as np
import pytest

import derep_cases as D
import fixtures
import meshclust_amd as M

ROOT = fixtures.HERE.rsplit(os.sep, 1)[0]
HOST_SRC = os.path.join(ROOT, "meshclust_amd", "csrc", "host")


def test_rc_is_rc_byte():
    want = list(range(256))
    want[0:4] = [3, 2, 1, 0]
    for a, b in ("AT", "TA", "CG", "GC"):
        want[ord(a)] = ord(b)
    assert D.rc(np.arange(256, dtype=np.uint8)).tolist() == want[::-1]
    s = np.array([0, 1, 78, 3, 65, 255], np.uint8)
    assert D.rc(D.rc(s)).tolist() == s.tolist() and D.rc(s).tolist() == [255, 84, 0, 78, 2, 3]


def test_the_case_set_holds_what_it_is_for():
    c = D.cases()
    ids = np.arange(c.n)
    rep, minus = c.expected(ids, 3)
    rep1, minus1 = c.expected(ids, 1)
    assert not minus1.any()
    by = {}
    for i in range(c.n):
        by.setdefault(c.group[i], {}).setdefault(c.kind[i], []).append(i)
    for L in D.LENGTHS:
        g = by[("len", L)]
        base, = g["base"]
        copy, = g["copy"]
        mcopy, = g["minus"]
        assert len(c.points[base]) == L and rep[copy] == rep1[copy] == base and minus[copy] == 0
        assert rep[mcopy] == base and np.array_equal(c.points[mcopy], D.rc(c.points[base]))
        assert minus[mcopy] == (0 if np.array_equal(c.points[mcopy], c.points[base]) else 1)
        if L >= 15:  # (a random string of 15 bases or more is not its own minus strand, nor one byte from it)
            assert minus[mcopy] == 1 and rep1[mcopy] == mcopy
        kinds = ("first", "middle", "last", "shorter") if L >= 1 else ()
        assert set(g) == {"filler", "base", "copy", "minus", "longer", *kinds}
        for kind in kinds + ("longer",):
            i, = g[kind]
            assert len(c.points[i]) == L + (kind == "longer") - (kind == "shorter")
            if kind in ("first", "middle", "last"):
                diff = np.nonzero(c.points[i] != c.points[base])[0].tolist()
                assert diff == [{"first": 0, "middle": L // 2, "last": L - 1}[kind]]
            if L >= 15:
                assert rep[i] == i, (L, kind)  # a near miss is no duplicate
    for L in (2, 64, 1000):  # their own minus strand: equality as written wins
        base, = by[("self", L)]["base"]
        copy, = by[("self", L)]["copy"]
        # (the one of 2 bases may itself repeat an earlier point of 2 bases)
        assert np.array_equal(D.rc(c.points[base]), c.points[base]) and rep[copy] == rep[base] and minus[copy] == minus[base] == 0
        assert L == 2 or rep[base] == base
    g = by[("N", 90)]
    base, = g["base"]
    assert (c.points[base] == D.N).sum() == 12 and [int(rep[i]) for i in g["copy"] + g["minus"]] == [base, base]
    assert minus[g["minus"][0]] == 1 and rep[g["n_replaced"][0]] == g["n_replaced"][0]
    g = by[("letters", 50)]
    base, = g["base"]
    assert set(c.points[base].tolist()) <= set(b"ACGT") and rep[g["minus"][0]] == base and minus[g["minus"][0]] == 1
    assert rep[g["copy"][0]] == base and rep[g["digits"][0]] == g["digits"][0]  # the bytes decide, not the letters
    four = sorted(i for v in by[("four", 100)].values() for i in v)
    assert [int(rep[i]) for i in four] == [four[0]] * 4 and [int(minus[i]) for i in four] == [0, 1, 1, 0]
    assert [int(rep1[i]) for i in four] == [four[0], four[1], four[1], four[0]]
    # the duplicates' start offsets: every residue mod 16 (so mod 4), in both orientations
    dup = [i for i in range(c.n) if rep[i] != i and len(c.points[i]) >= 16]
    for sign in (0, 1):
        assert {int(c.seq_off[i]) % 16 for i in dup if minus[i] == sign} == set(range(16)), sign
    assert {int(c.seq_off[int(rep[i])]) % 4 for i in dup} == set(range(4))
    assert c.seq_off[-1] < 1 << 20 and c.n < 300


@pytest.mark.parametrize("strands", [1, 3])
def test_consequences_of_the_definition(strands):
    c = D.cases()
    rng = np.random.default_rng(5)
    ids = np.concatenate([np.arange(c.n), rng.integers(0, c.n, 40)])  # (ids listed twice)
    rep, minus = c.expected(ids, strands)
    pos = np.arange(len(ids))
    assert np.array_equal(rep[rep], rep) and (rep <= pos).all() and not minus[rep == pos].any()
    assert all(rep[i] == rep[j] for i in range(c.n, len(ids)) for j in [int(np.nonzero(ids[:c.n] == ids[i])[0][0])])
    if strands == 1:
        assert not minus.any()
        rep3 = c.expected(ids, 3)[0]
        assert np.array_equal(rep3[rep], rep3)  # the plus-only classes refine the both-strand classes
        assert len(set(rep3.tolist())) < len(set(rep.tolist()))
    # a permuted list gives the permuted classes
    perm = rng.permutation(len(ids))
    prep, pminus = c.expected(ids[perm], strands)
    inv = np.argsort(perm)
    same = lambda r: {frozenset(np.nonzero(r == v)[0].tolist()) for v in set(r.tolist())}
    assert {frozenset(int(inv[i]) for i in cl) for cl in same(rep)} == same(prep)
    for cl in same(prep):  # the smallest position represents, and minus is relative to it
        j = min(cl)
        assert all(prep[i] == j for i in cl)
        assert all(pminus[i] == (0 if np.array_equal(c.points[ids[perm[i]]], c.points[ids[perm[j]]]) else 1) for i in cl)


def test_classes_order():
    assert D.classes([0, 1, 0, 3, 1, 5, 3, 7, 3, 1]) == [(1, 3), (3, 3), (0, 2), (5, 1), (7, 1)]
    assert D.classes([]) == []


def test_derep_native(tmp_path):
    exe = str(tmp_path / "derep_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-I", HOST_SRC, os.path.join(fixtures.HERE, "native", "derep_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("OK\n"), r.stdout[-2000:] + r.stderr
    dup, minus, own, rounds, coll, repeat = (int(v) for v in r.stdout.splitlines()[1].split())
    assert min(dup, minus, own, rounds, coll, repeat) > 50, r.stdout


# ---------------------------------------------------------------- what is built, declared and exported
@pytest.fixture(scope="module")
def host_built(built):
    M.build()


@pytest.mark.parametrize("strands", [1, 3])
def test_host_route_equals_the_restatement(host_built, strands):
    c = D.cases()
    rng = np.random.default_rng(9)
    for ids in (np.arange(c.n), rng.permutation(c.n)[: c.n // 2], np.zeros(0, np.int64), np.array([7]), np.array([3, 3, 3])):
        rep, minus = M.derep_host(c.codes, c.seq_off, ids, strands)
        want = c.expected(ids, strands)
        assert rep.dtype == np.uint32 and minus.dtype == np.uint8
        assert np.array_equal(rep, want[0]) and np.array_equal(minus, want[1])


def test_new_entries_are_declared(built):
    header = open(M.HEADER).read()
    for text in ("int mc_derep(mc_ctx *ctx, const uint32_t *ids, uint64_t m, int strands", "uint32_t *rep /* m */, uint8_t *minus",
                 "int mc_derep_profile(mc_ctx *ctx, double *out /* 5 */, int reset);", "#define MC_DEREP_BATCH_PAIRS (1ull << 22)",
                 "MC_DEREP_HASH_BITS", "MC_DEREP_BATCH=", "#define MC_ABI_VERSION 1"):
        assert text in header, text
    assert hasattr(M.Engine, "derep") and hasattr(M.Engine, "derep_profile")
    assert inspect.signature(M.Engine.derep).parameters["strands"].default == M.MC_STRAND_PLUS
    par = inspect.signature(M.derep_files).parameters
    assert list(par) == ["engine", "reads", "out", "table", "both_strands", "min_size", "threads"]
    assert par["table"].default is None and par["both_strands"].default is False and par["min_size"].default == 1
    for name in ("gpu/derep.hip", "host/derep.hpp", "host/derep_main.cpp", "host/capi_derep.cpp"):
        assert os.path.exists(os.path.join(ROOT, "meshclust_amd", "csrc", name)), name


def test_new_entries_are_exported(host_built):
    sym = subprocess.run(["nm", "-D", "--defined-only", M.GPU_LIB], capture_output=True, text=True, check=True).stdout
    assert " T mc_derep\n" in sym and " T mc_derep_profile\n" in sym
    assert hasattr(M.host_lib(), "mcl_derep")
    tool = os.path.join(os.path.dirname(M.BIN), "meshclust-derep")
    und = subprocess.run(["nm", "-D", "--undefined-only", tool], capture_output=True, text=True, check=True).stdout
    assert " mc_derep\n" in und
    r = subprocess.run([tool], capture_output=True, text=True, timeout=120)  # no reads: the usage text, exit code 1
    assert r.returncode == 1 and r.stderr.count("Usage: meshclust-derep") == 1
    assert all(x in r.stderr for x in ("--output", "--table FILE", "--both-strands", "--min-size N", "--device N", "--threads N", "--stats-json FILE",
                                       "--quiet", ";size=N"))
    for bad in (["--min-size", "0", "x.fa"], ["--min-size", "x", "x.fa"], ["--nonsense", "x.fa"]):
        r = subprocess.run([tool] + bad, capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and "Usage: meshclust-derep" in r.stderr, (bad, r.stderr[:200])
