"""mc_nw_pileup_strands / meshclust-assign --consensus --pileup, the parts that need no GPU:
  * the Python restatement of the table and of the consensus (tests/pileup_cases.py), the
    definition test_gpu_pileup.py compares the device with: its invariants per target, its '='
    counts tied to the CPU oracle (mco_nw) and the planted-truth family's consensus;
  * host/consensus.hpp and the options (tests/native/consensus_check.cpp), which must agree with
    the restatement on the same tables."""
import json
import os
import subprocess

import numpy as np
import pytest

import fixtures
import meshclust_amd as M
import nw_trace_cases as T
import oracle_lib as O
import pileup_cases as P

ROOT = fixtures.HERE.rsplit(os.sep, 1)[0]
HOST_SRC = os.path.join(ROOT, "meshclust_amd", "csrc", "host")


@pytest.fixture(scope="module")
def host_built(built):
    M.build()


def target_view(am):
    """-> per target (id, rows [L + 1, 8], pair indices)."""
    p = P.pile()
    tab = P.expected_table(am)
    out = []
    for t, j in enumerate(p.targets):
        ks = [k for k in range(len(p.a)) if p.b[k] == j]
        out.append((int(j), tab[int(p.row_off[t]):int(p.row_off[t + 1])], ks))
    return out


def test_the_list_holds_the_new_cases(built):
    p = P.pile()
    plus, minus = P.expected()
    assert len(p.a) == p.nbase + 150 + 1 + 30 + 1 and list(p.a[:p.nbase]) == list(p.base.a)
    assert p.names[-1] == "x70" and T.cigar_string(plus[-1][0]) == "95=70X95="
    assert sum(1 for j in p.b if j == p.contended) == 150 and sum(1 for j in p.b if j == p.planted) == 30
    assert p.lonely in p.targets and p.lonely not in p.b and len(set(p.targets.tolist())) == len(p.targets)
    wide = p.base.pairs["b1100x1100"][1]
    assert len(p.codes[wide]) == 1100 and sum(1 for j in p.b if j == wide) == 3  # three reads on one 1,100-base centre
    k = p.names.index("runs")
    assert len(plus[k][0]) > 64 and len(minus[k][0]) > 64  # the prefix carry crosses a chunk of 64 words
    assert int(p.row_off[-1]) == sum(len(p.codes[j]) + 1 for j in p.targets)
    # the new pairs' integers are the CPU oracle's (the base list: test_nw_trace_host.py)
    for s, res in enumerate((plus, minus)):
        for k in range(p.nbase, len(p.a)):
            _, o_len, o_ids, o_score = O.nw(p.read(k, bool(s)).tobytes(), p.codes[p.b[k]].tobytes())
            assert res[k][1:] == (o_score, o_len, o_ids), (p.names[k], s)


def test_every_class_of_runs_the_kernels_branch_on(built):
    """The pile-up kernels (gpu/pileup.hip) treat a run by its operation and its length: at most
    SPREAD = 8 columns by its own lane, more by the whole wave 64 columns at a time, so a run of
    more than 64 takes a second turn of that loop.  The runs of the list per class, <= 8 / 9 .. 64 /
    > 64, with the strands test_gpu_pileup.py and test_gpu_qpileup.py use:

               X                  I                 D                 =
      plus     7882 /  1 / 1      959 / 40 /  4     1165 / 45 / 2     8138 / 1619 / 66
      minus   17738 /  9 / 1     2644 / 90 / 18     2827 / 58 / 1    20943 /    6 /  0
      mixed   14273 /  5 / 1     2043 / 74 / 13     2258 / 51 / 1    16440 /  572 / 18

    Without the pair "x70" no strand has an 'X' run of more than 64.  Every class of X, I and D is
    asserted for every strand choice; '=' (which only the weighted and the naive kernel walk by
    column) for the plus and the mixed one: the list has no read that is related to its centre on
    the minus strand."""
    p = P.pile()
    exp = P.expected()
    for name, am in (("plus", np.zeros(len(p.a), np.uint8)), ("minus", np.ones(len(p.a), np.uint8)), ("mixed", P.mixed_strands())):
        cnt = {}
        for k in range(len(p.a)):
            for w in exp[am[k]][k][0]:
                n, op = int(w) >> 4, int(w) & 15
                key = (T.OPCH[op], 0 if n <= 8 else 1 if n <= 64 else 2)
                cnt[key] = cnt.get(key, 0) + 1
        for op in "XID" + ("=" if name != "minus" else ""):
            assert all(cnt.get((op, c), 0) > 0 for c in range(3)), (name, op, cnt)


@pytest.mark.parametrize("strands", ["plus", "minus", "mixed"])
def test_table_invariants(built, strands):
    p = P.pile()
    am = {"plus": np.zeros(len(p.a), np.uint8), "minus": np.ones(len(p.a), np.uint8), "mixed": P.mixed_strands()}[strands]
    exp = P.expected()
    kinds = set()
    for j, rows, ks in target_view(am):
        L, depth = len(p.codes[j]), len(ks)
        assert rows.shape == (L + 1, 8)
        assert (rows[:L, :6].sum(axis=1) == depth).all(), j  # a global alignment covers every column
        assert (rows[L, :6] == 0).all(), j
        ids = sum(exp[am[k]][k][3] for k in ks)
        cen = p.codes[j]
        own = np.where(cen <= 3, cen, 4)
        # '=' columns carry the centre's own byte; an 'X' column over two bytes of class 4 (N
        # against a raw letter) lands in the same channel, so the sum may only exceed there
        eq_cells = int(rows[np.arange(L), own].sum())
        if (cen <= 3).all():
            assert eq_cells == ids, j
        else:
            assert eq_cells >= ids, j
        assert ids == sum(int(w) >> 4 for k in ks for w in exp[am[k]][k][0] if int(w) & 15 == T.OP_EQ)
        la = sum(len(p.codes[p.a[k]]) for k in ks)
        assert int(rows[:L, :5].sum()) + int(rows[:, 7].sum()) == la, j  # every read base is in a column or inserted
        assert (rows[:, 6] <= depth).all() and (rows[:, 7] >= rows[:, 6]).all()
        kinds.update(np.nonzero(rows.sum(axis=0))[0].tolist())
        if j == p.lonely:
            assert depth == 0 and not rows.any()
    assert kinds == set(range(8))
    # rows 0 and L: the leading / trailing runs of 1 x 300 and 300 x 1
    view = {j: rows for j, rows, _ in target_view(am)}
    one, three = p.base.pairs["one_x300"], p.base.pairs["300x_one"]
    assert view[one[1]][:, 5].sum() == 299 and view[three[1]][:, 7].sum() == 299
    assert view[three[1]][0, 6] + view[three[1]][1, 6] >= 1


def test_planted_truth(built):
    p = P.pile()
    want = "".join(P.LETTERS[x] for x in p.truth)
    for am in (np.zeros(len(p.a), np.uint8),):
        for j, rows, ks in target_view(am):
            if j != p.planted:
                continue
            exp = P.expected()[0]
            runs = [r for k in ks for r in P.insertion_runs(exp[k][0], p.read(k, False))]
            seq, sub, dele, ins = P.consensus(p.codes[j], rows, len(ks), runs)
            assert seq == want and (sub, dele, ins) == (6, 2, 1)
            assert "".join(P.base_char(x) for x in p.codes[j]) != want


def test_consensus_native(host_built, tmp_path):
    p = P.pile()
    exe = str(tmp_path / "consensus_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-I", HOST_SRC, os.path.join(fixtures.HERE, "native", "consensus_check.cpp"),
                    "-L", M.LIB_DIR, "-lmeshclust", "-lmcgpu", "-Wl,-rpath," + M.LIB_DIR, "-Wl,-rpath-link," + M.LIB_DIR,
                    "-o", exe], check=True)
    want, text = [], []
    for s, am in enumerate((P.mixed_strands(), np.zeros(len(p.a), np.uint8))):
        exp = P.expected()
        for j, rows, ks in target_view(am):
            cen = p.codes[j]
            runs = [r for k in ks for r in P.insertion_runs(exp[am[k]][k][0], p.read(k, bool(am[k])))]
            for depth in {len(ks), max(0, len(ks) - 1) * 2}:  # (a second depth moves the majority line)
                seq, sub, dele, ins = P.consensus(cen, rows, depth, runs)
                want.append("%d %d %d [%s]" % (sub, dele, ins, seq))
                text.append("centre %d %d %d" % (len(cen), depth, len(runs)))
                text.append(" ".join(str(int(x)) for x in cen))
                text.append(" ".join(str(int(x)) for x in rows.reshape(-1)))
                text += ["run %d %d %s" % (row, len(b), " ".join(str(x) for x in b)) for row, b in runs]
    fix = tmp_path / "tables.txt"
    fix.write_text("\n".join(text) + "\n")
    r = subprocess.run([exe, str(fix), os.path.abspath(__file__)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("OK\n"), r.stdout[-2000:] + r.stderr
    lines = r.stdout.splitlines()[1:]
    assert lines[:len(want)] == want
    assert any(ln.split(" ", 3)[2] != "0" for ln in want) and any(ln.split(" ", 3)[1] != "0" for ln in want)
    plain, cons = (json.loads(ln) for ln in lines[len(want):len(want) + 2])
    new = ["consensus_pairs", "consensus_centres", "consensus_passes", "realigned_centres", "insertion_sites"]
    assert not any(k in plain for k in new)
    keys = list(cons)
    at = keys.index("rejected")
    assert keys[at + 1:at + 6] == new and [cons[k] for k in new] == [7, 3, 1, 1, 2]
    assert {k: v for k, v in cons.items() if k in plain} == plain


def test_new_entries_are_exported(host_built):
    lib = M.gpu_lib()
    assert hasattr(lib, "mc_nw_pileup_strands") and hasattr(M.host_lib(), "mcl_assign_consensus")
    assert M.PILEUP_CH == 8 and hasattr(M.Engine, "nw_pileup_strands")
    header = open(M.HEADER).read()
    for text in ("#define MC_PILEUP_CH 8", "mc_nw_pileup_strands(", "#define MC_ABI_VERSION 1"):
        assert text in header, text
    assign = os.path.join(os.path.dirname(M.BIN), "meshclust-assign")
    sym = subprocess.run(["nm", "-D", "--undefined-only", assign], capture_output=True, text=True, check=True).stdout
    assert " mc_nw_pileup_strands" in sym
    r = subprocess.run([assign], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--consensus FILE" in r.stderr and "--pileup FILE" in r.stderr
