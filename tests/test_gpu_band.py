"""The certified band on the GPU: mc_set_align_band, mc_nw_band_plan, mc_nw_band_profile and
meshclust-assign --band.  Every comparison is ==.

The expectations: the same engine with the band off (kernels this feature does not touch), the numpy
restatement of tests/nw_trace_cases.py for words and scores, and the formulas of tests/band_cases.py
(which test_band_host.py holds against host/band.hpp) for widths and bytes.  One set of points --
nw_trace_cases' and the pairs below -- loaded once."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import band_cases as Bc
import meshclust_amd as M
import msa_cases as A
import nw_trace_cases as T
import pileup_cases as P
import qpileup_cases as Q
import test_gpu_nw_align as G

pytestmark = pytest.mark.gpu

ASSIGN_BIN = G.ASSIGN_BIN
ENV_VARS = ("MC_ALIGN_BATCH", "MC_ALIGN_SCRATCH", "MC_IDENT_BATCH", "MC_IDENT_BYTES", "MC_BAND_W0", "MC_MSA_BYTES", "MC_PILEUP_NAIVE")
ROWS = Bc.BAND_ROWS
e2e = G.e2e  # the a1k fixture: 260 reads, every second one flipped


def clean_env(monkeypatch, **kw):
    for var in ENV_VARS:
        monkeypatch.delenv(var, raising=False)
    for k, v in kw.items():
        monkeypatch.setenv(k, str(v))


class Points:
    """nw_trace_cases' points (both halves) and, behind them, the points of the pairs this file adds;
    names / a / b: every pair, nw_trace_cases' first."""

    def __init__(self):
        c = T.cases()
        rng = np.random.default_rng(4242)
        self.codes, self.segs = list(c.codes), list(c.segs)
        self.names, a, b = list(c.names), list(c.a), list(c.b)

        def point(x):
            x = np.asarray(x, np.uint8)
            self.codes.append(x)
            self.segs.append([[0, len(x) - 1]] if len(x) else [])
            return len(self.codes) - 1

        def rnd(n):
            return rng.integers(0, 4, n).astype(np.uint8)

        def pair(name, x, y):
            self.names.append(name)
            a.append(point(x))
            b.append(point(y))

        for la in (ROWS - 1, ROWS, ROWS + 1, 2 * ROWS + 1):  # around the band's own row blocks, 3 % mutation
            x = rnd(la)
            pair("rows%d" % la, x, T.mutate(rng, x, 0.03))
        for la in (2 * ROWS + 1, 3 * ROWS + 40):  # the read written on the other strand: banded as a minus pair only
            x = rnd(la)
            pair("rc%d" % la, T.np_minus(T.mutate(rng, x, 0.03)), x)
        x = rnd(300)  # the shorter is the longer with one 100-base deletion
        pair("300x200", x, np.concatenate([x[:120], x[220:]]))
        pair("200x300", np.concatenate([x[:120], x[220:]]), x)
        cen = rnd(600)  # a 40-base gap at row ROWS: the path runs along a window's edge at the block edge
        pair("edge_del", np.concatenate([cen[:ROWS], cen[ROWS + 40:]]), cen)
        pair("edge_ins", np.concatenate([cen[:ROWS - 20], rnd(40), cen[ROWS - 20:]]), cen)
        x = rnd(65)  # the window clipped at column 1 and at lb within one block
        pair("17x65", T.fit(rng, T.mutate(rng, x[:17], 0.05), 17), x)
        pair("65x17", x, T.fit(rng, T.mutate(rng, x[:17], 0.05), 17))
        x = rnd(300)
        s = point(x)
        self.names.append("self300")  # w* = 0
        a.append(s)
        b.append(s)
        pair("unrelated300", rnd(300), rnd(300))  # ends full
        pair("1x300", rnd(1), rnd(300))
        pair("300x1", rnd(300), rnd(1))
        pair("empty_x300", np.zeros(0, np.uint8), rnd(300))
        # 1,100 x 1,100 at 47 % substitutions: still above (A), and its band is wider than half the matrix
        x = rnd(1100)
        y = x.copy()
        hit = rng.random(1100) < 0.47
        y[hit] = (y[hit] + rng.integers(1, 4, int(hit.sum()))) % 4
        pair("far1100", x, y)
        self.a, self.b = np.array(a, np.uint32), np.array(b, np.uint32)
        self.n_trace = len(c.names)

    def load_args(self):
        lens = [len(x) for x in self.codes]
        seq_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        seg = np.array([v for s in self.segs for pr in s for v in pr], np.int32)
        seg_off = np.concatenate([[0], np.cumsum([len(s) for s in self.segs])]).astype(np.uint64)
        return np.concatenate(self.codes), seq_off, seg, seg_off

    def lens(self, k):
        return len(self.codes[self.a[k]]), len(self.codes[self.b[k]])


_cache = {}


def points():
    if "p" not in _cache:
        _cache["p"] = Points()
    return _cache["p"]


def expected():
    """Computed once: (plus, minus) results of the restatement for every pair of points()."""
    if "e" not in _cache:
        p = points()
        plus, minus = T.expected()
        extra = range(p.n_trace, len(p.a))
        more = T.align_all([(p.codes[p.a[k]], p.codes[p.b[k]]) for k in extra] +
                           [(T.np_minus(p.codes[p.a[k]]), p.codes[p.b[k]]) for k in extra])
        _cache["e"] = (list(plus) + more[:len(extra)], list(minus) + more[len(extra):])
    return _cache["e"]


def strands(name):
    n = len(points().a)
    return {"plus": np.zeros(n, np.uint8), "minus": np.ones(n, np.uint8)}[name]


def planned(name):
    """The restatement's plan: width (-1 full) and choice bytes of every pair."""
    p = points()
    exp = expected()[name == "minus"]
    ws = [Bc.plan(*p.lens(k), exp[k][1]) for k in range(len(p.a))]
    nbytes = [Bc.band_choice_bytes(*p.lens(k), w) if w >= 0 else T.choice_bytes(*p.lens(k)) for k, w in enumerate(ws)]
    return np.array(ws, np.int32), nbytes


@pytest.fixture(scope="module")
def eng(built):
    e = M.Engine(0)
    e.load_sequences(*points().load_args())
    yield e
    e.close()


class banded:
    """with banded(eng): the band is on inside, off after."""

    def __init__(self, eng):
        self.eng = eng

    def __enter__(self):
        self.eng.set_align_band(1)

    def __exit__(self, *exc):
        self.eng.set_align_band(0)


def same(xs, ys):
    return len(xs) == len(ys) and all(x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(xs, ys))


@pytest.fixture(scope="module")
def off_results(eng):
    """The band-off answers with the default caps, computed once: plus, minus."""
    for var in ENV_VARS:
        assert var not in os.environ
    p = points()
    eng.set_align_band(0)
    return {s: eng.nw_align_strands(p.a, p.b, strands(s)) for s in ("plus", "minus")}


# ---------------------------------------------------------------- 1, 2. every pair, both strands
@pytest.mark.parametrize("strand", ["plus", "minus"])
def test_band_on_equals_band_off_and_the_restatement(eng, off_results, strand, monkeypatch):
    clean_env(monkeypatch)
    p = points()
    with banded(eng):
        eng.nw_band_profile(reset=True)
        on = eng.nw_align_strands(p.a, p.b, strands(strand))
        n_band, n_full, launches, ms, w_sum = eng.nw_band_profile()
    assert same(on, off_results[strand])
    words, off, score, ln, ids = on
    exp = expected()[strand == "minus"]
    for k, name in enumerate(p.names):
        w, s, cols, eq = exp[k]
        assert np.array_equal(words[int(off[k]):int(off[k + 1])], w), name
        assert (score[k], ln[k], ids[k]) == (s, cols, eq), name
    ws, _ = planned(strand)
    assert (n_band, n_full, w_sum) == (int((ws >= 0).sum()), int((ws < 0).sum()), int(ws[ws >= 0].sum()))
    assert launches >= 2 and ms > 0  # (a second round of the search)
    for name in ("unrelated300", "zeros_ones", "1x300", "300x1", "empty_x300"):
        assert ws[p.names.index(name)] == -1, name
    # what ends banded (pairs of at most ROWS rows never do: one block's window is every column)
    if strand == "plus":
        assert n_band >= 15 and ws[p.names.index("self300")] == 0
        some = ("rows%d" % (2 * ROWS + 1), "edge_del", "edge_ins", "far1100", "b1100x1100", "b1024x1100", "g1024_del", "g1024_ins")
    else:
        some = ("rc%d" % (2 * ROWS + 1), "rc%d" % (3 * ROWS + 40))
    for name in some:
        assert ws[p.names.index(name)] >= 0, name


# ---------------------------------------------------------------- 3. the plan
@pytest.mark.parametrize("strand", ["plus", "minus"])
def test_plan_is_the_needed_width_of_the_exact_score(eng, strand, monkeypatch):
    clean_env(monkeypatch)
    p = points()
    minus = strand == "minus"
    w, score = eng.nw_band_plan(p.a, p.b, strands(strand))
    seqa = [T.np_minus(p.codes[i]) if minus else p.codes[i] for i in p.a]
    seqb = [p.codes[i] for i in p.b]
    a_off = np.concatenate([[0], np.cumsum([len(x) for x in seqa])]).astype(np.uint64)
    b_off = np.concatenate([[0], np.cumsum([len(x) for x in seqb])]).astype(np.uint64)
    _, _, _, r_score = eng.nw_identity_raw(np.concatenate(seqa), a_off, np.concatenate(seqb), b_off)
    assert score.dtype == r_score.dtype and np.array_equal(score, r_score)
    assert np.array_equal(score, np.array([e[1] for e in expected()[minus]], np.int32))
    assert w.dtype == np.int32 and np.array_equal(w, planned(strand)[0])
    w0, s0 = eng.nw_band_plan([], [], [])
    assert len(w0) == 0 and len(s0) == 0
    with pytest.raises(M.MCError) as e:
        eng.nw_band_plan([len(p.codes)], [0], [0])
    assert e.value.code == M.ERR_ARG


# ---------------------------------------------------------------- 4. schedule independence
def test_the_schedule_changes_nothing(eng, off_results, monkeypatch):
    p = points()
    am = (np.arange(len(p.a)) % 3 != 2).astype(np.uint8)
    clean_env(monkeypatch)
    base_plan = eng.nw_band_plan(p.a, p.b, am)
    with banded(eng):
        base = eng.nw_align_strands(p.a, p.b, am)
    for k in range(len(p.a)):  # the mixed list is the two one-strand lists, pair by pair
        ref = off_results["minus" if am[k] else "plus"]
        assert np.array_equal(base[0][int(base[1][k]):int(base[1][k + 1])], ref[0][int(ref[1][k]):int(ref[1][k + 1])])
    nbytes = T.ident_bytes([len(x) for x in p.codes], p.a[am != 0])
    launches = {}
    for env in ({"MC_BAND_W0": 1}, {"MC_BAND_W0": 4096}, {"MC_ALIGN_BATCH": 7}, {"MC_IDENT_BYTES": nbytes}, {"MC_IDENT_BATCH": 5},
                {"MC_BAND_W0": 3, "MC_ALIGN_BATCH": 7, "MC_IDENT_BYTES": nbytes, "MC_IDENT_BATCH": 11}):
        clean_env(monkeypatch, **env)
        eng.nw_band_profile(reset=True)
        assert same(eng.nw_band_plan(p.a, p.b, am), base_plan), env
        launches[tuple(env)] = eng.nw_band_profile()[2]
        with banded(eng):
            assert same(eng.nw_align_strands(p.a, p.b, am), base), env
    clean_env(monkeypatch)
    assert launches[("MC_BAND_W0",)] >= 1  # (the last one written: w0 = 4096 holds every matrix here, one round)
    assert launches[("MC_IDENT_BATCH",)] > launches[("MC_ALIGN_BATCH",)]  # (the search is cut by the identity's pair cap)


# ---------------------------------------------------------------- 5. choice bytes
def test_choice_bytes_are_the_plans(eng, monkeypatch):
    clean_env(monkeypatch)
    p = points()
    ws, nbytes = planned("plus")
    eng.set_align_band(0)
    eng.nw_align_profile(reset=True)
    eng.nw_align_strands(p.a, p.b, None, cigar=False)
    off_bytes = eng.nw_align_profile(reset=True)[2]
    assert off_bytes == sum(T.choice_bytes(*p.lens(k)) for k in range(len(p.a)))
    with banded(eng):
        eng.nw_align_strands(p.a, p.b, None, cigar=False)
        assert eng.nw_align_profile(reset=True)[2] == sum(nbytes)
        ks = [p.names.index(n) for n in ("b1024x1100", "b1025x1100", "b1100x1100")]
        eng.nw_align_strands(p.a[ks], p.b[ks], None, cigar=False)
        on3 = eng.nw_align_profile(reset=True)[2]
    assert on3 == sum(nbytes[k] for k in ks) and all(ws[k] >= 0 for k in ks)
    eng.nw_align_strands(p.a[ks], p.b[ks], None, cigar=False)
    assert on3 < eng.nw_align_profile(reset=True)[2] == sum(T.choice_bytes(*p.lens(k)) for k in ks)


# ---------------------------------------------------------------- 6. the scratch cap
def test_scratch_cap_is_decided_on_the_planned_bytes(eng, off_results, monkeypatch):
    p = points()
    lib, ptr = eng.lib, M._p
    ws, nbytes = planned("plus")
    k, far = p.names.index("b1100x1100"), p.names.index("far1100")
    assert p.lens(k) == (1100, 1100) and T.choice_bytes(1100, 1100) == 1190912 and nbytes[k] < 600000
    assert ws[far] >= 0 and 600000 < nbytes[far] < 1190912  # a banded pair that still does not fit
    ref = off_results["plus"]
    want = ref[0][int(ref[1][k]):int(ref[1][k + 1])]
    SENT = 0xDEADBEEF

    def call(ids):
        a, b = np.ascontiguousarray(p.a[ids]), np.ascontiguousarray(p.b[ids])
        buf, o, s = np.full(4096, SENT, np.uint32), np.full(len(ids) + 1, 77, np.uint64), np.full(len(ids), -7, np.int32)
        rc = lib.mc_nw_align_strands(eng.ctx, ptr(a), ptr(b), None, C.c_uint64(len(ids)), ptr(buf), C.c_uint64(len(buf)), ptr(o),
                                     ptr(s), None, None)
        return rc, buf, o, s

    clean_env(monkeypatch, MC_ALIGN_SCRATCH=600000)
    eng.set_align_band(0)
    rc, buf, o, s = call([k])
    assert rc == M.ERR_UNSUPPORTED and (buf == SENT).all() and (o == 77).all() and (s == -7).all()
    with banded(eng):
        rc, buf, o, s = call([k])
        assert rc == 0 and list(o) == [0, len(want)] and np.array_equal(buf[:len(want)], want) and s[0] == ref[2][k]
        rc, buf, o, s = call([k, far])
        assert rc == M.ERR_UNSUPPORTED and (buf == SENT).all() and (o == 77).all() and (s == -7).all()
    clean_env(monkeypatch)


# ---------------------------------------------------------------- 7. the other entries
def test_pileups_do_not_change(built, monkeypatch):
    clean_env(monkeypatch)
    p = P.pile()
    am = P.mixed_strands()
    e = M.Engine(0)
    try:
        e.load_sequences(*p.load_args())
        e.load_qualities(Q.flat(Q.qualities()))
        off = (e.nw_pileup_strands(p.a, p.b, am, p.targets), e.nw_qpileup_strands(p.a, p.b, am, p.targets))
        with banded(e):
            e.nw_band_profile(reset=True)
            on = (e.nw_pileup_strands(p.a, p.b, am, p.targets), e.nw_qpileup_strands(p.a, p.b, am, p.targets))
            assert e.nw_band_profile()[2] >= 2
        assert same(on[0], off[0]) and same(on[1], off[1])
        assert np.array_equal(off[0][0], P.expected_table(am))
    finally:
        e.close()


def test_msa_does_not_change(built, monkeypatch):
    clean_env(monkeypatch)
    q = A.msa()
    am = q.strands("mixed")
    n = len(q.targets) + len(q.a)
    e = M.Engine(0)
    try:
        e.load_sequences(*q.load_args())

        def run():
            res = e.nw_msa_begin(q.a, q.b, am, q.targets)
            buf, off = e.nw_msa_rows(0, n)
            return tuple(res) + (buf, off) + tuple(e.nw_msa_counts(0, len(q.targets)))

        off = run()
        with banded(e):
            e.nw_band_profile(reset=True)
            on = run()
            assert e.nw_band_profile()[2] >= 1
        assert same(on, off)
    finally:
        e.close()


# ---------------------------------------------------------------- 8. the tool
def test_cli_band_changes_no_file(e2e):
    tmp = e2e.reads.parent
    outs = {}
    for name, more in (("plain", []), ("band", ["--band"])):
        cons, msa = tmp / (name + ".cons.fa"), tmp / (name + ".msa.fa")
        tsv, hits, paf, st = e2e("b_" + name, ["--paf", "@PAF", "--consensus", str(cons), "--msa", str(msa)] + more)
        outs[name] = ([f.read_bytes() for f in (tsv, hits, paf, cons, msa)], st)
    assert outs["band"][0] == outs["plain"][0] and all(len(x) > 0 for x in outs["plain"][0])
    st, st0 = outs["band"][1], outs["plain"][1]
    keys = list(st)
    assert keys[:len(st0)] == list(st0) and keys[len(st0):] == ["band_pairs", "band_full", "band_launches", "band_w_sum"]
    assert {k: v for k, v in st.items() if k in st0 and k != "phases_ms" and k != "device_us"} == \
        {k: v for k, v in st0.items() if k != "phases_ms" and k != "device_us"}
    assert st["band_pairs"] + st["band_full"] >= st["paf_pairs"] and st["band_pairs"] > 0 and st["band_launches"] >= 1
    r = subprocess.run([ASSIGN_BIN, "--model", "x", "--centres", str(e2e.cen), str(e2e.reads), "--band"], capture_output=True, text=True)
    assert r.returncode == 1 and "--band needs" in r.stderr and "Usage" in r.stderr


def test_assign_files_band(e2e, tmp_path):
    model = str(e2e.cen).replace(".centres.fa", ".model")
    e = M.Engine(0)
    try:
        outs = {}
        for name, band in (("plain", False), ("band", True)):
            paf = tmp_path / (name + ".paf")
            st = M.assign_files(e, model, str(e2e.cen), str(e2e.reads), str(tmp_path / (name + ".tsv")), both_strands=True, paf=str(paf),
                                band=band)
            outs[name] = (paf.read_bytes(), (tmp_path / (name + ".tsv")).read_bytes(), st)
        assert outs["band"][:2] == outs["plain"][:2]
        assert "band_pairs" in outs["band"][2] and "band_pairs" not in outs["plain"][2]
        with pytest.raises(Exception):
            M.assign_files(e, model, str(e2e.cen), str(e2e.reads), str(tmp_path / "x.tsv"), band=True)  # band alone
    finally:
        e.close()


# ---------------------------------------------------------------- 9. modes
def test_modes(eng, monkeypatch):
    clean_env(monkeypatch)
    p = points()
    ks = [p.names.index(n) for n in ("b1100x1100", "rows%d" % (2 * ROWS + 1))]
    full = sum(T.choice_bytes(*p.lens(k)) for k in ks)
    assert eng.lib.mc_set_align_band(eng.ctx, 2) == M.ERR_ARG and eng.lib.mc_set_align_band(eng.ctx, -1) == M.ERR_ARG
    eng.nw_align_profile(reset=True)
    eng.nw_align_strands(p.a[ks], p.b[ks], None, cigar=False)  # (a refused mode changes nothing: still off)
    assert eng.nw_align_profile(reset=True)[2] == full
    eng.set_align_band(1)
    eng.nw_align_strands(p.a[ks], p.b[ks], None, cigar=False)
    assert eng.nw_align_profile(reset=True)[2] < full
    eng.set_align_band(0)
    eng.nw_align_strands(p.a[ks], p.b[ks], None, cigar=False)
    assert eng.nw_align_profile(reset=True)[2] == full
