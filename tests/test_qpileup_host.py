"""mc_nw_qpileup_strands / meshclust-assign --quality, the parts that need no GPU:
  * the Python restatement of the weight table and of the weighted consensus
    (tests/qpileup_cases.py), the definition test_gpu_qpileup.py compares the device with: its
    invariants and a planted truth that the plurality vote gets wrong;
  * host/consensus.hpp's weighted consensus and the option (tests/native/qconsensus_check.cpp),
    which must agree with the restatement on the same tables;
  * bin/meshclust's host objects on the CPU engine, reading an e2e golden's input as FASTQ."""
import gzip
import json
import os
import subprocess

import numpy as np
import pytest

import fixtures
import meshclust_amd as M
import nw_trace_cases as T
import pileup_cases as P
import qpileup_cases as Q

ROOT = fixtures.HERE.rsplit(os.sep, 1)[0]
HOST_SRC = os.path.join(ROOT, "meshclust_amd", "csrc", "host")


@pytest.fixture(scope="module")
def host_built(built):
    M.build()


def test_the_qualities_hold_the_special_reads(built):
    p = P.pile()
    q = Q.qualities()
    assert len(q) == len(p.codes) and all(len(x) == len(c) and x.dtype == np.uint8 for x, c in zip(q, p.codes))
    zero, full, ramp = Q.special_reads()
    assert not q[zero].any() and (q[full] == Q.QMAX).all() and list(q[ramp][:5]) == [0, 1, 2, 3, 4]
    wide = p.base.pairs["b1100x1100"][0]
    assert len(q[wide]) == 1100 and q[wide][94] == 0 and q[wide][93] == 93
    assert max(int(x.max()) for x in q) == Q.QMAX and min(int(x.min()) for x in q) == 0
    exp = P.expected()[0]
    k = p.names.index("zeros_ones")
    assert any(int(w) >> 4 == 47 and int(w) & 15 == T.OP_X for w in exp[k][0])  # the 47-column 'X' run
    assert len(Q.flat(q)) == sum(len(c) for c in p.codes)


def test_all_ones_give_the_counts(built):
    """With every quality 1 the weight of channels 0..6 is the count (no read here is empty)."""
    p = P.pile()
    assert min(len(p.codes[i]) for i in p.a) >= 1
    tabs = P.pair_tables()
    exp = P.expected()
    for s in (0, 1):
        for k in range(len(p.a)):
            read = p.read(k, bool(s))
            w = Q.wtable_from_words(exp[s][k][0], read, np.ones(len(read), np.uint8), p.codes[p.b[k]])
            assert np.array_equal(w[:, :7], tabs[s][k][:, :7]) and not w[:, 7].any(), (p.names[k], s)


@pytest.mark.parametrize("strand", [0, 1])
def test_a_pairs_weight_is_its_reads_quality(built, strand):
    """Channels 0..4 of a pair's table hold every read base that is in a column: the read's
    qualities less those of its inserted bases.  Channel 5 / 6 hold a minimum per row / run."""
    p = P.pile()
    q = Q.qualities()
    exp = P.expected()[strand]
    tabs = Q.pair_wtables()[strand]
    seen = set()
    for k in range(len(p.a)):
        qs = Q.aligned_quality(q, k, strand).astype(np.int64)
        ins = sum(sum(v) for _, _, v in Q.insertion_runs(exp[k][0], p.read(k, bool(strand)), qs))
        assert int(tabs[k][:, :5].sum()) == int(qs.sum()) - ins, p.names[k]
        assert not tabs[k][:, 7].any() and not tabs[k][-1, :6].any()
        assert (tabs[k][:, 5:7] <= Q.QMAX).all()
        seen.update(np.nonzero(tabs[k].sum(axis=0))[0].tolist())
    assert seen == set(range(7))
    zero, full, _ = Q.special_reads()
    kz, kf = list(p.a).index(zero), list(p.a).index(full)
    assert not tabs[kz].any()
    assert set(np.unique(tabs[kf][:, :7]).tolist()) <= {0, Q.QMAX}


def test_minus_of_a_palindromic_quality_is_plus_of_the_reverse_complement(built):
    """Pair k on minus aligns the minus-strand string of its read; with qualities that read the
    same backwards its weights are those of that string, as a read of its own, on plus."""
    p = P.pile()
    exp = P.expected()[1]
    rng = np.random.default_rng(3)
    for k in list(range(0, p.nbase, 23)) + [p.names.index("runs"), p.names.index("p00")]:
        n = len(p.codes[p.a[k]])
        half = rng.integers(0, Q.QMAX + 1, (n + 1) // 2).astype(np.uint8)
        pal = np.concatenate([half, half[:n // 2][::-1]])
        assert len(pal) == n and np.array_equal(pal, pal[::-1])
        q = list(Q.qualities())
        q[p.a[k]] = pal
        minus = Q.pair_wtable(q, k, 1)
        plus_of_rc = Q.wtable_from_words(exp[k][0], T.np_minus(p.codes[p.a[k]]), pal, p.codes[p.b[k]])
        assert np.array_equal(minus, plus_of_rc) and minus.any()
    # ... and a ramp is no palindrome: the reversed index shows
    k = list(p.a).index(Q.special_reads()[2])
    ramp = Q.qualities()[p.a[k]]
    a = Q.wtable_from_words(exp[k][0], p.read(k, True), ramp[::-1], p.codes[p.b[k]])
    b = Q.wtable_from_words(exp[k][0], p.read(k, True), ramp, p.codes[p.b[k]])
    assert not np.array_equal(a, b)


def target_view(am):
    """-> per target (id, count rows, weight rows, pair indices)."""
    p = P.pile()
    tab, wtab = P.expected_table(am), Q.expected_wtable(am)
    out = []
    for t, j in enumerate(p.targets):
        ks = [k for k in range(len(p.a)) if p.b[k] == j]
        sl = slice(int(p.row_off[t]), int(p.row_off[t + 1]))
        out.append((int(j), tab[sl], wtab[sl], ks))
    return out


def planted_tables():
    t, reads, quals = Q.planted_q()
    rows, wrows = None, None
    for r, q in zip(reads, quals):
        w = []  # the alignment of a read with substitutions only: runs of '=' and 'X'
        i = 0
        while i < 300:
            j = i
            while j < 300 and (r[j] == t[j]) == (r[i] == t[i]):
                j += 1
            w.append((j - i) << 4 | (T.OP_EQ if r[i] == t[i] else T.OP_X))
            i = j
        rows = P.table_from_words(w, r, t, rows)
        wrows = Q.wtable_from_words(w, r, q, t, wrows)
    return t, rows, wrows


def test_planted_truth(built):
    """Two Q2 reads with a wrong base outvote one Q40 read in the plurality consensus; the weighted
    consensus returns the template, with quality 36 = 40 - 2 - 2 at those columns."""
    t, rows, wrows = planted_tables()
    want = "".join(P.LETTERS[x] for x in t)
    plain, sub, _, _ = P.consensus(t, rows, 3, [])
    assert plain != want and sub == 3
    assert [c for c in range(300) if plain[c] != want[c]] == [31, 150, 268]
    seq, qual, sub, dele, ins = Q.consensus(t, rows, wrows, 3, [])
    assert seq == want and (sub, dele, ins) == (0, 0, 0)
    assert [ord(qual[c]) - 33 for c in (31, 150, 268)] == [36, 36, 36]
    assert all(ord(qual[c]) - 33 == Q.QMAX for c in range(300) if c not in (31, 150, 268))  # 120, clamped


def test_qconsensus_native(host_built, tmp_path):
    p = P.pile()
    exe = str(tmp_path / "qconsensus_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-I", HOST_SRC, os.path.join(fixtures.HERE, "native", "qconsensus_check.cpp"),
                    "-L", M.LIB_DIR, "-lmeshclust", "-lmcgpu", "-Wl,-rpath," + M.LIB_DIR, "-Wl,-rpath-link," + M.LIB_DIR,
                    "-o", exe], check=True)
    q = Q.qualities()
    want, text = [], []

    def add(cen, rows, wrows, depth, runs):
        seq, qual, sub, dele, ins = Q.consensus(cen, rows, wrows, depth, runs)
        want.append("%d %d %d [%s] [%s]" % (sub, dele, ins, seq, qual))
        text.append("centre %d %d %d" % (len(cen), depth, len(runs)))
        text.append(" ".join(str(int(x)) for x in cen))
        text.append(" ".join(str(int(x)) for x in rows.reshape(-1)))
        text.append(" ".join(str(int(x)) for x in wrows.reshape(-1)))
        text.extend("run %d %d %s %s" % (row, len(b), " ".join(str(x) for x in b), " ".join(str(x) for x in v)) for row, b, v in runs)

    exp = P.expected()
    for am in (P.mixed_strands(), np.zeros(len(p.a), np.uint8)):
        for j, rows, wrows, ks in target_view(am):
            runs = [r for k in ks for r in Q.insertion_runs(exp[am[k]][k][0], p.read(k, bool(am[k])), Q.aligned_quality(q, k, am[k]))]
            for depth in {len(ks), max(0, len(ks) - 1) * 2}:  # (a second depth moves the majority line)
                add(p.codes[j], rows, wrows, depth, runs)
    t, rows, wrows = planted_tables()
    add(t, rows, wrows, 3, [])
    fix = tmp_path / "tables.txt"
    fix.write_text("\n".join(text) + "\n")
    r = subprocess.run([exe, str(fix), os.path.abspath(__file__)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("OK\n"), r.stdout[-2000:] + r.stderr
    lines = r.stdout.splitlines()[1:]
    assert lines[:len(want)] == want
    assert any(ln.split(" ", 3)[2] != "0" for ln in want) and any(ln.split(" ", 3)[1] != "0" for ln in want)
    # the weights decide somewhere: some weighted consensus differs from the plurality one
    differs = 0
    for j, rows, wrows, ks in target_view(np.zeros(len(p.a), np.uint8)):
        runs = [r for k in ks for r in Q.insertion_runs(exp[0][k][0], p.read(k, False), q[p.a[k]])]
        differs += Q.consensus(p.codes[j], rows, wrows, len(ks), runs)[0] != P.consensus(p.codes[j], rows, len(ks), [(a, b) for a, b, _ in runs])[0]
    assert differs > 0
    plain, withq = (json.loads(ln) for ln in lines[len(want):len(want) + 2])
    assert "quality" not in plain and withq["quality"] == 1
    keys = list(withq)
    assert keys[keys.index("insertion_sites") + 1] == "quality"
    assert {k: v for k, v in withq.items() if k != "quality"} == plain


def test_new_entries_are_exported(host_built):
    lib, host = M.gpu_lib(), M.host_lib()
    assert hasattr(lib, "mc_load_qualities") and hasattr(lib, "mc_nw_qpileup_strands")
    assert all(hasattr(host, n) for n in ("mcl_parse_q", "mcl_qualities", "mcl_assign_qconsensus"))
    assert M.QUAL_MAX == 93 and all(hasattr(M.Engine, n) for n in ("load_qualities", "nw_qpileup_strands"))
    assert hasattr(M.Dataset, "qualities")
    header = open(M.HEADER).read()
    for text in ("#define MC_QUAL_MAX 93", "mc_load_qualities(", "mc_nw_qpileup_strands(", "#define MC_ABI_VERSION 1"):
        assert text in header, text
    assign = os.path.join(os.path.dirname(M.BIN), "meshclust-assign")
    sym = subprocess.run(["nm", "-D", "--undefined-only", assign], capture_output=True, text=True, check=True).stdout
    assert " mc_nw_qpileup_strands" in sym and " mc_load_qualities" in sym and " mc_nw_pileup_strands" in sym
    r = subprocess.run([assign], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--quality" in r.stderr


def test_meshclust_reads_fastq_on_the_cpu_engine(built, tmp_path):
    """bin/meshclust's host objects on the CPU oracle engine (as test_host_harness.py): the smallest
    e2e golden's input rewritten as FASTQ gives the golden .clstr byte for byte."""
    harness = os.path.join(ROOT, "oracle", "_build", "meshclust_cpu")
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "harness"], check=True)
    name = "al300"  # (300 reads of 500 bases: the smallest input among the e2e goldens)
    fa, flags = fixtures.e2e_input(name, tmp_path)
    rng = np.random.default_rng(1)
    fq = str(tmp_path / (name + ".fastq"))
    recs, cur = [], None
    for ln in open(fa, "rb").read().splitlines():
        if ln.startswith(b">"):
            cur = [ln, b""]
            recs.append(cur)
        else:
            cur[1] += ln
    with open(fq, "wb") as f:
        for i, (h, s) in enumerate(recs):
            ql = bytes(bytearray(int(v) + 33 for v in rng.integers(0, 94, len(s))))
            if i % 3 == 0:
                ql = b"@" + ql[1:]
            f.write(b"@" + h[1:] + b"\n" + s + b"\n+\n" + ql + b"\n")
    out = tmp_path / (name + ".clstr")
    r = subprocess.run([harness, fq] + flags + ["--output", str(out), "--quiet"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    with gzip.open(fixtures.golden("e2e_%s.clstr.gz" % name), "rb") as f:
        assert out.read_bytes() == f.read()
