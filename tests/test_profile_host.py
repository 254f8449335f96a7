"""mc_nw_msa_counts / host/profile.hpp, the parts that need no GPU:
  * the two Python restatements of tests/profile_cases.py (from the operation words, and as the
    column histogram of msa_cases.block's rows) agree, and keep the invariants the header states,
    against the pile-up tables of pileup_cases / qpileup_cases (themselves tied to the CPU oracle);
  * host/profile.hpp's consensus equals host/consensus.hpp's (tests/native/profile_check.cpp) on the
    planted families and on seeded random alignments that hold every tie, and profile_cases' port of
    it gives the same answers."""
import os
import subprocess

import numpy as np
import pytest

import fixtures
import meshclust_amd as M
import msa_cases as A
import nw_trace_cases as T
import pileup_cases as P
import profile_cases as F
import qpileup_cases as Q

ROOT = fixtures.HERE.rsplit(os.sep, 1)[0]
HOST_SRC = os.path.join(ROOT, "meshclust_amd", "csrc", "host")
NAMES = ["plus", "minus", "mixed"]


@pytest.mark.parametrize("name", NAMES)
def test_the_two_restatements_agree(built, name):
    q = A.msa()
    pr = F.profiles(name)
    bl = A.named_blocks(name)
    assert len(pr) == len(bl) == len(q.targets)
    same = 0
    for t, ((w, col, W, counts, _), (bw, bW, rows, ks)) in enumerate(zip(pr, bl)):
        L = len(q.codes[q.targets[t]])
        assert W == bW and np.array_equal(w, bw) and counts.shape == (W, F.CH)
        if F.renders_its_classes([q.codes[q.a[k]] for k in ks]):
            assert np.array_equal(counts, F.from_rows(L, bw, bW, rows)), (name, t)
            same += 1
    assert same >= len(q.targets) - 2  # (nw_trace_cases' raw-letter reads: class 4, shown as letters)


@pytest.mark.parametrize("name", NAMES)
def test_invariants_against_the_pileup(built, name):
    q = A.msa()
    p = P.pile()
    am = q.strands(name)
    exp = A.expected()
    ql = F.qualities()
    assert len(ql) == len(q.codes) and all(len(x) == len(c) for x, c in zip(ql, q.codes))
    old, wold = P.expected_table(am[:q.nold]), Q.expected_wtable(am[:q.nold])
    seen_n = seen_two = seen_slot = 0
    for t, (w, col, W, counts, wcounts) in enumerate(F.profiles(name)):
        j = int(q.targets[t])
        cen = q.codes[j]
        L = len(cen)
        ks = [k for k in range(len(q.a)) if q.b[k] == j]
        depth = len(ks)
        if t < len(p.targets):
            sl = slice(int(q.row_off[t]), int(q.row_off[t + 1]))
            tab, wtab = old[sl], wold[sl]
        else:
            tab, wtab = np.zeros((L + 1, 8), np.uint32), np.zeros((L + 1, 8), np.uint32)
            for k in ks:
                x = ql[q.a[k]]
                P.table_from_words(exp[am[k]][k][0], q.read(k, bool(am[k])), cen, tab)
                Q.wtable_from_words(exp[am[k]][k][0], q.read(k, bool(am[k])), x[::-1] if am[k] else x, cen, wtab)
        c = col[:L].astype(np.int64)
        assert np.array_equal(counts[c, :6], tab[:L, :6]) and np.array_equal(wcounts[c, :6], wtab[:L, :6])
        assert np.array_equal(counts[c, 6], np.arange(L)) and not counts[c, 7].any()
        assert (counts[:, :6].sum(axis=1) == depth).all()
        assert not wcounts[:, 6:].any()
        for r in range(L + 1):
            s0, wr = int(col[r]) - int(w[r]), int(w[r])
            if not wr:
                assert tab[r, 6] == 0
                continue
            seen_slot += 1
            assert counts[s0, 5] == depth - tab[r, 6] and counts[s0:s0 + wr, :5].sum() == tab[r, 7]
            assert np.array_equal(counts[s0:s0 + wr, 6], np.full(wr, r)) and np.array_equal(counts[s0:s0 + wr, 7], np.arange(1, wr + 1))
            assert not wcounts[s0:s0 + wr, 5].any()
            gaps = counts[s0:s0 + wr, 5]
            assert (np.diff(gaps.astype(np.int64)) >= 0).all()  # left-justified: later slots hold no fewer gaps
            seen_two += int(len(set(gaps.tolist())) > 1)
        seen_n += int(counts[:, 4].any())
        if not ks:
            assert W == L and not counts[:, :6].any() and not counts[:, 7].any() and not wcounts.any()
    assert seen_slot and seen_two and seen_n  # inserted columns, two run lengths at one site, class 4
    assert any(not len([k for k in range(len(q.a)) if q.b[k] == j]) for j in q.targets)


# ---------------------------------------------------------------- host/profile.hpp
def sub_only_words(r, t):
    w, i = [], 0
    while i < len(t):
        j = i
        while j < len(t) and (r[j] == t[j]) == (r[i] == t[i]):
            j += 1
        w.append((j - i) << 4 | (T.OP_EQ if r[i] == t[i] else T.OP_X))
        i = j
    return w


def random_case(rng):
    """A centre of 1 .. 10 bytes and 0 .. 7 alignments made of random operations over a small
    alphabet (ties are common): at most one 'I' run per row, rows 0 and L included."""
    L = int(rng.integers(1, 11))
    cen = rng.integers(0, 3, L).astype(np.uint8)
    pairs = []
    for _ in range(int(rng.integers(0, 8))):
        ops, read = [], []
        for r in range(L + 1):
            if rng.random() < (0.5 if r in (0, L, L // 2) else 0.1):
                n = int(rng.integers(1, 4))
                ops += [T.OP_I] * n
                read += [int(x) for x in rng.choice([0, 1, 78], n)]
            if r == L:
                break
            u = rng.random()
            if u < 0.6:
                ops.append(T.OP_EQ)
                read.append(int(cen[r]))
            elif u < 0.85:
                ops.append(T.OP_X)
                read.append(int((cen[r] + 1 + rng.integers(0, 2)) % 3) if rng.random() < 0.9 else 78)
            else:
                ops.append(T.OP_D)
        words, k = [], 0
        while k < len(ops):
            e = k
            while e < len(ops) and ops[e] == ops[k]:
                e += 1
            words.append((e - k) << 4 | ops[k])
            k = e
        qs = rng.choice([0, 7, 7, 20, 93], len(read)).astype(np.uint8)
        pairs.append((words, np.array(read, np.uint8), qs))
    return cen, pairs


def native_cases():
    p = P.pile()
    out = []
    exp = P.expected()[0]
    q = Q.qualities()
    ks = [k for k in range(len(p.a)) if p.b[k] == p.planted]
    out.append((p.codes[p.planted], [(exp[k][0], p.read(k, False), q[p.a[k]]) for k in ks]))
    t, reads, quals = Q.planted_q()
    out.append((t, [(sub_only_words(r, t), r, x) for r, x in zip(reads, quals)]))
    rng = np.random.default_rng(312)
    out += [random_case(rng) for _ in range(400)]
    return out


def census(cases):
    """What the random cases hold: applied sites with tied run lengths, tied pluralities inside an
    applied insertion, depth 0, applied sites at row 0 and at row L."""
    tied_len = tied_base = zero = first = last = 0
    for cen, pairs in cases:
        L, depth = len(cen), len(pairs)
        zero += depth == 0
        if not depth:
            continue
        w, col, W, counts, _ = F.from_words(cen, pairs)
        for r in range(L + 1):
            wr, s0 = int(w[r]), int(col[r]) - int(w[r])
            if not wr or 2 * (depth - int(counts[s0, 5])) <= depth:
                continue
            first += r == 0
            last += r == L
            ng = [int(counts[s0 + t, :5].sum()) for t in range(wr)] + [0]
            exact = [ng[t] - ng[t + 1] for t in range(wr)]
            tied_len += exact.count(max(exact)) > 1
            length = exact.index(max(exact)) + 1
            for t in range(length):
                n = [int(v) for v in counts[s0 + t, :5]]
                tied_base += n.count(max(n)) > 1
    return tied_len, tied_base, zero, first, last


def test_profile_native(built, tmp_path):
    cases = native_cases()
    assert all(x > 0 for x in census(cases[2:])), census(cases[2:])
    exe = str(tmp_path / "profile_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-I", HOST_SRC, os.path.join(fixtures.HERE, "native", "profile_check.cpp"), "-o", exe],
                   check=True)
    text = []
    for cen, pairs in cases:
        text.append("C %d %s" % (len(cen), " ".join(str(int(x)) for x in cen)))
        for words, read, qs in pairs:
            text.append("P %d %s %d %s %s" % (len(words), " ".join(str(int(x)) for x in words), len(read),
                                              " ".join(str(int(x)) for x in read), " ".join(str(int(x)) for x in qs)))
        text.append("E")
    fix = tmp_path / "cases.txt"
    fix.write_text("\n".join(text) + "\n")
    r = subprocess.run([exe, str(fix)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("OK\n"), r.stdout[-2000:] + r.stderr
    lines = r.stdout.splitlines()
    assert int(lines[1]) == len(cases) and len(lines) == 2 + len(cases)
    blank = lambda s: "" if s == "." else s
    for (cen, pairs), ln in zip(cases, lines[2:]):
        f = ln.split(" ")
        got = (blank(f[0]), int(f[1]), int(f[2]), int(f[3])), (blank(f[4]), blank(f[5]), int(f[6]), int(f[7]), int(f[8]))
        depth = len(pairs)
        _, _, _, counts, wcounts = F.from_words(cen, pairs)
        # the Python port of profile.hpp, and the restated consensus of pileup_cases / qpileup_cases
        assert F.consensus_from_profile(cen, counts) == got[0] and F.consensus_from_profile(cen, counts, wcounts) == got[1]
        rows = wrows = None
        runs, qruns = [], []
        for words, read, qs in pairs:
            rows = P.table_from_words(words, read, cen, rows)
            wrows = Q.wtable_from_words(words, read, qs, cen, wrows)
            runs += P.insertion_runs(words, read)
            qruns += Q.insertion_runs(words, read, qs)
        if depth:
            assert P.consensus(cen, rows, depth, runs) == got[0] and Q.consensus(cen, rows, wrows, depth, qruns) == got[1]
    # the planted truths come back from the profile alone
    want = "".join(P.LETTERS[x] for x in P.pile().truth)
    assert lines[2].split(" ")[0] == want
    t = Q.planted_q()[0]
    assert lines[3].split(" ")[4] == "".join(P.LETTERS[x] for x in t) and lines[3].split(" ")[0] != lines[3].split(" ")[4]


@pytest.fixture(scope="module")
def host_built(built):
    M.build()


def test_new_entries_are_exported(host_built):
    lib = M.gpu_lib()
    assert hasattr(lib, "mc_nw_msa_counts") and hasattr(lib, "mc_nw_msa_counts_profile") and hasattr(M.host_lib(), "mcl_assign_profile")
    assign = os.path.join(os.path.dirname(M.BIN), "meshclust-assign")
    sym = subprocess.run(["nm", "-D", "--undefined-only", assign], capture_output=True, text=True, check=True).stdout
    assert " mc_nw_msa_counts" in sym
    r = subprocess.run([assign], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--profile FILE" in r.stderr and "--msa FILE" in r.stderr
    import inspect
    assert "profile" in inspect.signature(M.assign_files).parameters


def test_new_entries_are_declared(built):
    header = open(M.HEADER).read()
    for text in ("#define MC_MSA_CH 8", "mc_nw_msa_counts(", "mc_nw_msa_counts_profile("):
        assert text in header, text
    assert M.MSA_CH == 8 and hasattr(M.Engine, "nw_msa_counts") and hasattr(M.Engine, "nw_msa_counts_profile")
    assert os.path.exists(os.path.join(HOST_SRC, "profile.hpp"))
