"""mc_derep / meshclust-derep on the GPU.  Every comparison is ==.

The expectations are the Python restatement of tests/derep_cases.py (a dict keyed by min(s, rc(s))) over its
own seeded points, held to the definition by test_derep_host.py; for the tool, the same rule on the letters of
its reads.  One set of points, loaded once."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import derep_cases as D
import meshclust_amd as M

pytestmark = pytest.mark.gpu

BOTH = M.MC_STRAND_PLUS | M.MC_STRAND_MINUS
ENV_VARS = ("MC_DEREP_BATCH", "MC_DEREP_HASH_BITS", "MC_IDENT_BATCH", "MC_IDENT_BYTES")


def clean_env(monkeypatch, **kw):
    for var in ENV_VARS:
        monkeypatch.delenv(var, raising=False)
    for k, v in kw.items():
        monkeypatch.setenv(k, str(v))


@pytest.fixture(scope="module")
def eng(built):
    e = M.Engine(0)
    e.load_sequences(*D.cases().load_args())
    yield e
    e.close()


def id_lists():
    c = D.cases()
    rng = np.random.default_rng(41)
    sub = rng.permutation(c.n)[: 2 * c.n // 3]
    sub = np.insert(sub, 50, sub[3])  # one id listed twice
    return {"all": np.arange(c.n), "subset": sub, "none": np.zeros(0, np.int64), "one": np.array([int(np.argmax(c.lens))])}


def same(got, want, what):
    for g, w, name in zip(got, want, ("rep", "minus")):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name)
        bad = np.nonzero(g != w)[0]
        assert not len(bad), (what, name, len(bad), bad[:8].tolist(), g[bad[:8]].tolist(), w[bad[:8]].tolist())
    return True


@pytest.mark.parametrize("strands", [M.MC_STRAND_PLUS, BOTH])
@pytest.mark.parametrize("which", ["all", "subset", "none", "one"])
def test_derep_equals_the_restatement(eng, which, strands, monkeypatch):
    clean_env(monkeypatch)
    ids = id_lists()[which]
    eng.derep_profile(reset=True)
    same(eng.derep(ids, strands), D.cases().expected(ids, strands), (which, strands))
    prof = eng.derep_profile()
    assert prof["collisions"] == 0  # at the default 128 bits no key of this set collides
    assert prof["rounds"] == (1 if len(ids) > 1 else 0) and (prof["pairs"] > 0) == (len(ids) > 1)


@pytest.mark.parametrize("strands", [M.MC_STRAND_PLUS, BOTH])
def test_hash_bits_and_batches_change_nothing(eng, strands, monkeypatch):
    c = D.cases()
    for which in ("all", "subset"):
        ids = id_lists()[which]
        want = c.expected(ids, strands)
        nclass = len(set(want[0].tolist()))
        for env in (dict(MC_DEREP_HASH_BITS=0), dict(MC_DEREP_HASH_BITS=1), dict(MC_DEREP_HASH_BITS=4), dict(MC_DEREP_BATCH=7),
                    dict(MC_DEREP_HASH_BITS=0, MC_DEREP_BATCH=7)):
            clean_env(monkeypatch, **env)
            eng.derep_profile(reset=True)
            same(eng.derep(ids, strands), want, (which, strands, env))
            prof = eng.derep_profile()
            if env.get("MC_DEREP_HASH_BITS") == 0:  # the collision rounds run
                assert prof["rounds"] > 1 and prof["collisions"] > 0
            else:
                assert prof["rounds"] >= 1
            assert prof["pairs"] >= len(ids) - nclass  # every member that is no representative was compared at least once
            assert eng.derep_profile(reset=True) == prof and eng.derep_profile()["pairs"] == 0
    clean_env(monkeypatch)


def test_other_entries_change_nothing_and_are_not_changed(eng, monkeypatch):
    clean_env(monkeypatch)
    c = D.cases()
    ids = id_lists()["subset"]
    a = np.array([i for i in range(c.n) if 1 <= c.lens[i] <= 300][:40], np.uint32)
    b = a[::-1].copy()
    am = (np.arange(len(a)) % 2).astype(np.uint8)
    ident0 = eng.nw_identity_strands(a, b, am)
    rc0 = eng.revcomp_sequences(a)
    assert all(np.array_equal(rc0[0][int(rc0[1][k]):int(rc0[1][k + 1])], D.rc(c.points[int(a[k])])) for k in range(len(a)))
    timers0 = eng.timers(reset=True)
    del timers0
    want = c.expected(ids, BOTH)
    same(eng.derep(ids, BOTH), want, "between")
    t = eng.timers()
    assert all(t[f] == (0.0, 0) for f in M.FAMILIES), t  # mc_derep's kernels are counted in no family of mc_timers
    ident1 = eng.nw_identity_strands(a, b, am)
    rc1 = eng.revcomp_sequences(a)
    assert all(np.array_equal(x, y) for x, y in zip(ident0, ident1)) and all(np.array_equal(x, y) for x, y in zip(rc0, rc1))
    same(eng.derep(ids, BOTH), want, "after")


def test_errors_leave_rep_untouched(eng, monkeypatch):
    clean_env(monkeypatch)
    c = D.cases()
    lib = eng.lib
    ids = np.arange(8, dtype=np.uint32)
    rep = np.full(8, 0xABCD, np.uint32)
    minus = np.full(8, 0xEE, np.uint8)

    def call(ctx, ids_, m, strands, rep_, minus_):
        return lib.mc_derep(ctx, M._p(ids_), C.c_uint64(m), strands, M._p(rep_), M._p(minus_))

    bad = ids.copy()
    bad[5] = c.n
    assert call(eng.ctx, bad, 8, BOTH, rep, minus) == M.ERR_ARG
    assert call(eng.ctx, None, 8, BOTH, rep, minus) == M.ERR_ARG
    assert call(eng.ctx, ids, 8, BOTH, None, minus) == M.ERR_ARG
    assert call(eng.ctx, ids, 8, BOTH, rep, None) == M.ERR_ARG  # minus is required with both strands
    for strands in (0, 2, 4, -1):
        assert call(eng.ctx, ids, 8, strands, rep, minus) == M.ERR_ARG
    assert (rep == 0xABCD).all() and (minus == 0xEE).all()
    assert call(eng.ctx, None, 0, BOTH, None, None) == 0  # m = 0
    fresh = M.Engine(0)
    try:
        assert call(fresh.ctx, ids, 8, BOTH, rep, minus) == M.ERR_STATE  # no sequences
        with pytest.raises(M.MCError) as ei:
            fresh.derep(ids)
        assert ei.value.code == M.ERR_STATE
    finally:
        fresh.close()
    assert (rep == 0xABCD).all() and (minus == 0xEE).all()
    # plus only: minus may be NULL; given, it is all zeros
    assert call(eng.ctx, ids, 8, M.MC_STRAND_PLUS, rep, None) == 0
    assert np.array_equal(rep, c.expected(ids, 1)[0]) and (minus == 0xEE).all()
    assert call(eng.ctx, ids, 8, M.MC_STRAND_PLUS, rep, minus) == 0 and not minus.any()
    assert lib.mc_derep_profile(eng.ctx, None, 0) == M.ERR_ARG


# ---------------------------------------------------------------- the tool and derep_files
@pytest.fixture(scope="module")
def tool_input(tmp_path_factory):
    d = tmp_path_factory.mktemp("derep_tool")
    reads = D.tool_reads()
    cut = len(reads) // 2
    paths = {}
    for ext, text in (("fa", D.fasta_text), ("fq", D.fastq_text)):
        paths[ext] = [str(d / ("a." + ext)), str(d / ("b." + ext))]  # the reads split over two files
        open(paths[ext][0], "w").write(text(reads[:cut]))
        open(paths[ext][1], "w").write(text(reads[cut:]))
    assert any(s != s.upper() for _, s in reads) and any("N" in s for _, s in reads) and len(reads) > 100
    return d, reads, paths


TOOL = os.path.join(os.path.dirname(M.BIN), "meshclust-derep")
STAT_KEYS = ["reads", "uniques", "written", "largest", "minus", "strands", "compare_pairs", "rounds", "collisions", "phases_ms"]


def check_stats(st, want):
    assert list(st) == STAT_KEYS and list(st["phases_ms"]) == ["parse", "upload", "derep", "write"]
    assert {k: st[k] for k in want} == want
    assert st["collisions"] == 0 and st["rounds"] == 1 and st["compare_pairs"] >= st["reads"] - st["uniques"] > 0


@pytest.mark.parametrize("both", [False, True])
def test_tool_files_are_the_expected_bytes(built, tool_input, both, monkeypatch):
    clean_env(monkeypatch)
    d, reads, paths = tool_input
    fa, tab, stats = D.tool_expected(reads, both)
    assert stats["uniques"] < stats["reads"] and (stats["minus"] > 0) == both
    outs = {}
    for ext in ("fa", "fq"):  # the FASTQ twin gives the same two files
        out, table, js = (str(d / ("%s_%d.%s" % (ext, both, x))) for x in ("out.fa", "tsv", "json"))
        cmd = [TOOL, "--output", out, "--table", table, "--stats-json", js, "--quiet"] + (["--both-strands"] if both else []) + paths[ext]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stdout == "", r.stderr[-500:]
        outs[ext] = (open(out, "rb").read(), open(table, "rb").read())
        assert outs[ext][0] == fa and outs[ext][1] == tab, ext
        check_stats(json.load(open(js)), stats)
    # --min-size 2 drops exactly the singletons from --output and leaves --table alone
    fa2, tab2, stats2 = D.tool_expected(reads, both, min_size=2)
    assert tab2 == tab and 0 < stats2["written"] < stats["written"] and fa.startswith(fa2) and b";size=1\n" in fa and b";size=1\n" not in fa2
    out, table, js = (str(d / ("min2_%d.%s" % (both, x))) for x in ("out.fa", "tsv", "json"))
    cmd = [TOOL, "-o", out, "--table", table, "--stats-json", js, "--min-size", "2"] + (["--both-strands"] if both else []) + paths["fa"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("%d reads: %d unique (%d written)" % (stats2["reads"], stats2["uniques"], stats2["written"])), r.stderr
    assert open(out, "rb").read() == fa2 and open(table, "rb").read() == tab
    check_stats(json.load(open(js)), stats2)


def test_derep_files_and_exit_codes(eng, tool_input, monkeypatch):
    clean_env(monkeypatch)
    d, reads, paths = tool_input
    other = M.Engine(0)  # (derep_files loads its reads: not into the engine the other tests share)
    try:
        for both in (False, True):
            fa, tab, stats = D.tool_expected(reads, both, min_size=2)
            out, table = str(d / ("py_%d.fa" % both)), str(d / ("py_%d.tsv" % both))
            st = M.derep_files(other, paths["fq"], out, table=table, both_strands=both, min_size=2, threads=2)
            assert open(out, "rb").read() == fa and open(table, "rb").read() == tab
            check_stats(st, stats)
        st = M.derep_files(other, paths["fa"][0], str(d / "py_one.fa"))
        assert st["reads"] == len(reads) // 2 and not os.path.exists(str(d / "derep.fa"))
        with pytest.raises(M.MCError) as ei:
            M.derep_files(other, str(d / "missing.fa"), str(d / "x.fa"))
        assert ei.value.code == 2
    finally:
        other.close()
    # a run without reads: the usage text, exit code 1; an unreadable file or a file without reads: 2
    r = subprocess.run([TOOL, "--both-strands"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "Usage: meshclust-derep" in r.stderr
    r = subprocess.run([TOOL, "-o", str(d / "x.fa"), str(d / "missing.fa")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "Usage" not in r.stderr and not os.path.exists(str(d / "x.fa"))
    empty = d / "empty.fa"
    empty.write_text("")
    r = subprocess.run([TOOL, "-o", str(d / "x.fa"), str(empty)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and not os.path.exists(str(d / "x.fa")), r.stderr
    same(eng.derep(np.arange(D.cases().n), BOTH), D.cases().expected(np.arange(D.cases().n), BOTH), "the shared engine, after the tool")
