"""mc_nw_align_strands / meshclust-assign --paf, the parts that need no GPU:
  * host/cigar.hpp and the --paf option (tests/native/cigar_check.cpp);
  * the numpy restatement of GlobAlignE's recurrences with recorded choices and a traceback
    (tests/nw_trace_cases.py) -- the definition the device kernels are compared with in
    test_gpu_nw_align.py.  Here it is shown, for the restatement alone and on every pair of the
    shared list, that the path the choices describe is the path the reference's payload
    describes: score / columns / '=' equal mco_nw of the CPU oracle, and the CIGAR replays
    truthfully over the two strings, consumes both, has that many columns and '=', and replays
    to the DP score under 1 / -1 / 2 / 1.

Score replay: GlobAlignE's "-infinity" is finite, so a boundary state that is not a real alignment
prefix can still be chosen; its path length is still the bases left (which is why columns always
agree), but its score is not the score of that gap.  SCORE_EXEMPT lists the pairs where the
optimum runs through such a state (none here); the issue allows at most 1 % of the list."""
import json
import os
import subprocess

import numpy as np
import pytest

import fixtures
import meshclust_amd as M
import nw_trace_cases as T
import oracle_lib as O

ROOT = fixtures.HERE.rsplit(os.sep, 1)[0]
HOST_SRC = os.path.join(ROOT, "meshclust_amd", "csrc", "host")
SCORE_EXEMPT = frozenset()  # (name, strand) whose replayed score is not the DP score


@pytest.fixture(scope="module")
def host_built(built):
    M.build()


def test_cigar_native(host_built, tmp_path):
    exe = str(tmp_path / "cigar_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-I", HOST_SRC, os.path.join(fixtures.HERE, "native", "cigar_check.cpp"),
                    "-L", M.LIB_DIR, "-lmeshclust", "-lmcgpu", "-Wl,-rpath," + M.LIB_DIR, "-Wl,-rpath-link," + M.LIB_DIR,
                    "-o", exe], check=True)
    r = subprocess.run([exe, os.path.abspath(__file__)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.startswith("OK\n"), r.stdout + r.stderr
    ident, paf = (json.loads(ln) for ln in r.stdout.splitlines()[1:3])
    assert "paf_pairs" not in ident and "cigar_ops" not in ident  # no new key without --paf
    keys = list(paf)
    at = keys.index("rejected")
    assert keys[at + 1:at + 3] == ["paf_pairs", "cigar_ops"] and paf["paf_pairs"] == 21 and paf["cigar_ops"] == 88
    assert {k: v for k, v in paf.items() if k in ident} == ident


def test_new_entries_are_exported(host_built):
    lib = M.gpu_lib()
    assert hasattr(lib, "mc_nw_align_strands") and hasattr(M.host_lib(), "mcl_assign_paf")
    assert (M.CIGAR_I, M.CIGAR_D, M.CIGAR_EQ, M.CIGAR_X) == (1, 2, 7, 8) and hasattr(M.Engine, "nw_align_strands")
    header = open(M.HEADER).read()
    for text in ("#define MC_CIGAR_I 1u", "#define MC_CIGAR_D 2u", "#define MC_CIGAR_EQ 7u", "#define MC_CIGAR_X 8u",
                 "#define MC_ALIGN_BATCH_PAIRS (1ull << 16)", "#define MC_ALIGN_SCRATCH_BYTES (1ull << 30)", "mc_nw_align_strands("):
        assert text in header, text
    assign = os.path.join(os.path.dirname(M.BIN), "meshclust-assign")
    sym = subprocess.run(["nm", "-D", "--undefined-only", assign], capture_output=True, text=True, check=True).stdout
    assert " mc_nw_align_strands" in sym
    r = subprocess.run([assign], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--paf FILE" in r.stderr


def test_the_list_holds_the_cases():
    c = T.cases()
    la = np.array([len(c.codes[i]) for i in c.a])
    lb = np.array([len(c.codes[i]) for i in c.b])
    for x in T.SMALL:
        for y in T.SMALL:
            assert ((la == x) & (lb == y)).any(), (x, y)
    for rows in (255, 256, 257, 511, 512, 513, 1024, 1025, 1100):
        assert (la == rows).any(), rows
    assert {T.rows_per_lane(int(x)) for x in la} == {4, 8, 16}
    for rows in (1024, 1025, 1100):
        assert ((la == rows) & (lb == 1100)).any() and ((la == rows) & (lb == 90)).any()
    assert ((la == 1) & (lb == 300)).any() and ((la == 300) & (lb == 1)).any()
    assert sum(1 for n in c.names if n.startswith("f")) == 200
    assert T.choice_bytes(1000, 1000) == 1063 * 512 and T.choice_bytes(1100, 1100) == 2 * 1163 * 512
    assert T.choice_bytes(256, 10) == 73 * 128 and T.choice_bytes(257, 10) == 73 * 256
    # the minus-strand half: an involution, and the parser's reverse complement for digits
    for i in (0, c.pairs["n_run"][0], c.pairs["raw_letters"][0]):
        assert np.array_equal(T.np_minus(c.codes[c.NP + i]), c.codes[i])
    assert bytes(c.codes[c.NP + c.pairs["raw_letters"][0]]) == b"AGCCTTGCAACGTNATGCTAACCGGTNNACGT"


@pytest.mark.parametrize("strand", ["plus", "minus"])
def test_restatement_is_the_reference_path(built, strand):
    c = T.cases()
    res = T.expected()[strand == "minus"]
    exempt = 0
    shapes = set()
    for k, name in enumerate(c.names):
        a = c.codes[(c.NP if strand == "minus" else 0) + c.a[k]]
        b = c.codes[c.b[k]]
        words, score, cols, ids = res[k]
        _, o_len, o_ids, o_score = O.nw(a.tobytes(), b.tobytes())
        assert (score, cols, ids) == (o_score, o_len, o_ids), (name, strand)
        r_cols, r_eq, r_score, ua, ub, true = T.replay(words, a, b)
        assert true and (ua, ub) == (len(a), len(b)) and (r_cols, r_eq) == (cols, ids), (name, strand)
        if (name, strand) in SCORE_EXEMPT:
            exempt += 1
            assert r_score != score, (name, strand)  # (the exemption is needed)
        else:
            assert r_score == score, (name, strand, r_score, score)
        runs = [int(w) >> 4 for w in words]
        ops = [int(w) & 15 for w in words]
        assert all(n > 0 for n in runs) and all(x != y for x, y in zip(ops, ops[1:]))  # run-length encoded
        shapes.update(ops)
    assert exempt * 100 <= len(c.names)
    assert shapes == {T.OP_I, T.OP_D, T.OP_EQ, T.OP_X}


def test_restatement_edge_shapes(built):
    c = T.cases()
    res = dict(zip(c.names, T.expected()[0]))
    words, score, cols, ids = res["self"]
    assert T.cigar_string(words) == "180=" and (score, cols, ids) == (180, 180, 180)
    words, _, cols, ids = res["zeros_ones"]
    assert ids == 0 and T.OP_EQ not in {int(w) & 15 for w in words}
    words, _, cols, ids = res["homopolymers"]  # every cell ties: the fixed rules pick one path
    assert ids == 40 and cols == 57 and sum(int(w) >> 4 for w in words if int(w) & 15 == T.OP_D) == 17
    for name, op in (("g16_del", T.OP_D), ("g16_ins", T.OP_I), ("g1024_del", T.OP_D), ("g1024_ins", T.OP_I)):
        assert any(int(w) & 15 == op and int(w) >> 4 >= 30 for w in res[name][0]), name  # the long gap is found
    plus, minus = T.expected()
    assert any(not np.array_equal(p[0], m[0]) for p, m in zip(plus, minus))  # the strand changes the alignment
