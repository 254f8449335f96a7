"""mc_nw_align_strands / meshclust-assign --paf on the GPU.  Every comparison is ==.

The expectations: mc_nw_identity_raw / mc_nw_identity / mc_nw_identity_strands (kernels this
feature does not touch) for score, columns and '=' count; the numpy restatement of
tests/nw_trace_cases.py, which test_nw_trace_host.py ties to the CPU oracle, for the operation
words; for the minus strand the read's minus-strand string loaded as a point of its own.  One set
of points, loaded once."""
import json
import os
import subprocess

import numpy as np
import pytest

import fixtures
import meshclust_amd as M
import nw_trace_cases as T

pytestmark = pytest.mark.gpu

ASSIGN_BIN = os.path.join(os.path.dirname(M.BIN), "meshclust-assign")


@pytest.fixture(scope="module")
def eng(built):
    e = M.Engine(0)
    e.load_sequences(*T.cases().load_args())
    yield e
    e.close()


@pytest.fixture(scope="module")
def mixed():
    """The whole list with strands mixed (two minus pairs, then a plus pair, ...) and what the
    restatement gives for it."""
    c = T.cases()
    am = (np.arange(len(c.a)) % 3 != 2).astype(np.uint8)
    plus, minus = T.expected()
    return am, [minus[k] if am[k] else plus[k] for k in range(len(am))]


def clean_env(monkeypatch, **kw):
    for var in ("MC_ALIGN_BATCH", "MC_ALIGN_SCRATCH", "MC_IDENT_BATCH", "MC_IDENT_BYTES"):
        monkeypatch.delenv(var, raising=False)
    for k, v in kw.items():
        monkeypatch.setenv(k, str(v))


@pytest.fixture(scope="module")
def got(eng):
    """The device's answers with the default caps, computed once: plus, minus."""
    for var in ("MC_ALIGN_BATCH", "MC_ALIGN_SCRATCH", "MC_IDENT_BATCH", "MC_IDENT_BYTES"):
        assert var not in os.environ
    c = T.cases()
    return (eng.nw_align_strands(c.a, c.b, None), eng.nw_align_strands(c.a, c.b, np.ones(len(c.a), np.uint8)))


# ---------------------------------------------------------------- 1. score, columns, '='
@pytest.mark.parametrize("strand", ["plus", "minus"])
def test_integers_equal_the_identity_kernels(eng, got, strand, monkeypatch):
    clean_env(monkeypatch)
    c = T.cases()
    minus = strand == "minus"
    _, _, score, ln, ids = got[minus]
    a1 = (c.a + (c.NP if minus else 0)).astype(np.uint32)  # seq1 as a point of its own
    seqa = [c.codes[i] for i in a1]
    seqb = [c.codes[i] for i in c.b]
    a_off = np.concatenate([[0], np.cumsum([len(x) for x in seqa])]).astype(np.uint64)
    b_off = np.concatenate([[0], np.cumsum([len(x) for x in seqb])]).astype(np.uint64)
    r_ident, r_len, r_ids, r_score = eng.nw_identity_raw(np.concatenate(seqa), a_off, np.concatenate(seqb), b_off)
    assert score.dtype == r_score.dtype and np.array_equal(score, r_score)
    assert np.array_equal(ln, r_len) and np.array_equal(ids, r_ids)
    p_ident, p_len, p_ids = eng.nw_identity(a1, c.b)
    assert np.array_equal(ln, p_len) and np.array_equal(ids, p_ids)
    s_ident, s_len, s_ids = eng.nw_identity_strands(c.a, c.b, np.full(len(c.a), 1 if minus else 0, np.uint8))
    mine = ids.astype(np.float64) / ln.astype(np.float64)
    assert np.array_equal(mine, s_ident) and np.array_equal(ln, s_len) and np.array_equal(ids, s_ids)
    assert len(set(mine.tolist())) > 50  # (identities, not a constant)


# ---------------------------------------------------------------- 2. the operations
@pytest.mark.parametrize("strand", ["plus", "minus"])
def test_operations_equal_the_restatement(eng, got, strand):
    c = T.cases()
    minus = strand == "minus"
    words, off, score, ln, ids = got[minus]
    want = T.expected()[minus]
    assert off.dtype == np.uint64 and words.dtype == np.uint32
    assert np.array_equal(off, np.concatenate([[0], np.cumsum([len(w[0]) for w in want])]).astype(np.uint64))
    assert len(words) == int(off[-1])
    for k, name in enumerate(c.names):
        w = words[int(off[k]):int(off[k + 1])]
        assert np.array_equal(w, want[k][0]), (name, strand, T.cigar_string(w), T.cigar_string(want[k][0]))
        assert (int(score[k]), int(ln[k]), int(ids[k])) == want[k][1:], (name, strand)
    if minus:  # the same as the minus-strand strings aligned as points of their own
        w2 = eng.nw_align_strands((c.a + c.NP).astype(np.uint32), c.b, None)
        assert all(np.array_equal(x, y) for x, y in zip(w2, got[1]))


# ---------------------------------------------------------------- 3. batching changes nothing
def test_batches_give_the_same_bytes(eng, mixed, monkeypatch):
    c = T.cases()
    am, want = mixed
    clean_env(monkeypatch)
    base = eng.nw_align_strands(c.a, c.b, am)
    for k in range(len(am)):
        assert np.array_equal(base[0][int(base[1][k]):int(base[1][k + 1])], want[k][0]), c.names[k]
    big = T.choice_bytes(1100, 1100)
    n_big = sum(1 for i in c.a if len(c.codes[i]) > 1024)
    assert n_big >= 6 and big == max(T.choice_bytes(len(c.codes[i]), len(c.codes[j])) for i, j in zip(c.a, c.b))
    # MC_IDENT_BYTES: batch ends by the cap on the minus-strand strings (host/pairbatch.hpp's rule restated)
    lens = [len(x) for x in c.codes]
    nbytes = T.ident_bytes(lens, c.a[am != 0])
    by = [i1 for i1, why in T.batch_ends(lens, c.a, c.b, am, 1 << 16, nbytes, 1 << 30) if why == "bytes"]
    assert len(by) >= 2, (nbytes, by)
    for env in ({"MC_ALIGN_BATCH": 7}, {"MC_ALIGN_SCRATCH": 3 * big + 64}, {"MC_ALIGN_BATCH": 7, "MC_ALIGN_SCRATCH": 3 * big + 64},
                {"MC_ALIGN_BATCH": 1}, {"MC_IDENT_BYTES": nbytes}, {"MC_ALIGN_BATCH": 7, "MC_IDENT_BYTES": nbytes}):
        clean_env(monkeypatch, **env)
        res = eng.nw_align_strands(c.a, c.b, am)
        assert all(x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(res, base)), env
    assert 0 < am.sum() < len(am) and len(set(am[:7].tolist())) == 2  # mixed strands inside a batch of 7


# ---------------------------------------------------------------- 4. the call's contract
def test_offsets_only_capacity_and_errors(eng, mixed, monkeypatch):
    import ctypes as C
    c = T.cases()
    am, _ = mixed
    clean_env(monkeypatch)
    words, off, score, ln, ids = eng.nw_align_strands(c.a, c.b, am)
    none, off0, score0, ln0, ids0 = eng.nw_align_strands(c.a, c.b, am, cigar=False)  # cigar = NULL
    assert none is None and np.array_equal(off0, off)
    assert np.array_equal(score0, score) and np.array_equal(ln0, ln) and np.array_equal(ids0, ids)
    lib, p = eng.lib, M._p
    m, total = len(c.a), int(off[-1])
    a, b = np.ascontiguousarray(c.a), np.ascontiguousarray(c.b)

    def call(n, buf, cap, o, s=None):
        return lib.mc_nw_align_strands(eng.ctx, p(a[:n]), p(b[:n]), p(am[:n]), C.c_uint64(n), p(buf), C.c_uint64(cap), p(o),
                                       p(s), None, None)

    SENT = 0xDEADBEEF
    buf = np.full(total + 8, SENT, np.uint32)
    o = np.full(m + 1, 77, np.uint64)
    assert call(m, buf, total - 1, o) == M.ERR_ARG  # one word short
    assert np.array_equal(o, off) and (buf == SENT).all()
    assert call(m, buf, total, o) == 0  # exactly enough; score / len / ids NULL
    assert np.array_equal(buf[:total], words) and (buf[total:] == SENT).all()
    # a cap below one pair's need: refused before anything is written
    need = [T.choice_bytes(len(c.codes[i]), len(c.codes[j])) for i, j in zip(c.a, c.b)]
    k = need.index(max(need))  # the first pair that does not fit
    assert k > 64 and max(need) == T.choice_bytes(1100, 1100)
    clean_env(monkeypatch, MC_ALIGN_SCRATCH=T.choice_bytes(1100, 1100) - 1)
    buf[:] = SENT
    o[:] = 77
    s = np.full(m, -7, np.int32)
    assert call(m, buf, total, o, s) == M.ERR_UNSUPPORTED
    assert (buf == SENT).all() and (o == 77).all() and (s == -7).all()
    assert call(k, buf, total, o, s) == 0 and np.array_equal(o[:k + 1], off[:k + 1])  # the pairs before it fit
    clean_env(monkeypatch)
    for x, y in (([len(c.codes)], [0]), ([0], [len(c.codes)])):
        with pytest.raises(M.MCError) as e:
            eng.nw_align_strands(x, y, [1])
        assert e.value.code == M.ERR_ARG
    o[:] = 77
    assert call(0, buf, 0, o) == 0 and o[0] == 0 and o[1] == 77  # m = 0
    w0, off00, _, _, _ = eng.nw_align_strands([], [], [])
    assert len(w0) == 0 and list(off00) == [0]
    fresh = M.Engine(0)  # no sequences loaded
    try:
        with pytest.raises(M.MCError) as e:
            fresh.nw_align_strands([0], [0], [1])
        assert e.value.code == 3  # MC_ERR_STATE
    finally:
        fresh.close()
    eng.timers(reset=True)
    eng.nw_align_strands(c.a[:5], c.b[:5], [1, 0, 0, 0, 0])
    t = eng.timers()
    assert t["layout"][1] == 1 and t["nw"][1] >= 2  # the reverse complement as layout; forward and traceback as nw
    assert all(t[f][1] == 0 for f in t if f not in ("layout", "nw"))


# ---------------------------------------------------------------- 5. end to end
_RC = bytes.maketrans(b"ACGT", b"TGCA")


def read_fasta(path):
    recs = []
    with open(path, "rb") as f:
        for ln in f.read().splitlines():
            if ln.startswith(b">"):
                recs.append([ln, b""])
            else:
                recs[-1][1] += ln
    return recs


def rows(path):
    return [ln.split("\t") for ln in open(path).read().splitlines()]


def parse_cigar(text):
    out, n = [], 0
    for ch in text:
        if ch.isdigit():
            n = 10 * n + int(ch)
        else:
            out.append(n << 4 | {"I": T.OP_I, "D": T.OP_D, "=": T.OP_EQ, "X": T.OP_X}[ch])
            n = 0
    return out


@pytest.fixture(scope="module")
def e2e(built, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("paf")
    fa, flags = fixtures.e2e_input("a1k", tmp)
    model, cen = tmp / "a1k.model", tmp / "a1k.centres.fa"
    r = subprocess.run([M.BIN, fa] + flags + ["--output", str(tmp / "a1k.clstr"), "--quiet", "--save-model", str(model),
                                              "--save-centres", str(cen)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    recs = read_fasta(fa)[:260]  # 260 reads, every second one reverse-complemented
    reads = tmp / "F.fa"
    with open(reads, "wb") as f:
        for i, (h, s) in enumerate(recs):
            f.write(h + b"\n" + (s.upper().translate(_RC)[::-1] if i % 2 else s) + b"\n")
    env = {k: v for k, v in os.environ.items() if k not in ("MC_ASSIGN_FORM", "MC_ASSIGN_TILE", "MC_ASSIGN_PAIRS", "MC_IDENT_BATCH",
                                                             "MC_IDENT_BYTES", "MC_ALIGN_BATCH", "MC_ALIGN_SCRATCH")}
    done = {}

    def run(name, extra):
        if name not in done:
            tsv, hits, paf, stats = (tmp / (name + ext) for ext in (".tsv", ".hits", ".paf", ".json"))
            args = [a.replace("@PAF", str(paf)) for a in extra]
            r = subprocess.run([ASSIGN_BIN, "--model", str(model), "--centres", str(cen), str(reads), "--output", str(tsv), "--quiet",
                                "--both-strands", "--top", "3", "--hits", str(hits), "--stats-json", str(stats)] + args,
                               capture_output=True, text=True, timeout=300, env=env)
            assert r.returncode == 0, r.stderr[-3000:]
            done[name] = (tsv, hits, paf, json.loads(stats.read_text()))
        return done[name]

    run.reads, run.cen = reads, cen
    return run


def test_cli_paf(e2e):
    i_tsv, i_hits, i_paf, i_st = e2e("ident", ["--identity"])
    p_tsv, p_hits, p_paf, p_st = e2e("paf", ["--paf", "@PAF"])  # --paf implies --identity
    assert p_tsv.read_bytes() == i_tsv.read_bytes() and p_hits.read_bytes() == i_hits.read_bytes()
    assert not i_paf.exists() and "paf_pairs" not in i_st and "cigar_ops" not in i_st
    hits, paf = rows(p_hits), rows(p_paf)
    assert len(paf) == len(hits) > 260 and p_st["paf_pairs"] == len(paf) == p_st["identity_pairs"]
    assert {k: v for k, v in p_st.items() if k not in ("paf_pairs", "cigar_ops", "phases_ms", "device_us")} == \
        {k: v for k, v in i_st.items() if k not in ("phases_ms", "device_us")}
    reads = {h[1:].decode(): s.upper() for h, s in read_fasta(e2e.reads)}
    cents = {h[1:].decode(): s.upper() for h, s in read_fasta(e2e.cen)}
    nops, strands, kinds = 0, set(), set()
    for h, x in zip(hits, paf):
        assert len(x) == 15 and len(h) == 7
        q, t = reads[x[0]], cents[x[5]]
        assert (x[0], x[5], x[4]) == (h[0], h[2], h[5])  # the same order, centre and strand
        assert x[1:4] == [str(len(q)), "0", str(len(q))] and x[6:9] == [str(len(t)), "0", str(len(t))] and x[11] == "255"
        ids, ln = int(x[9]), int(x[10])
        assert "%.17g" % (ids / ln) == h[6]
        assert x[13] == "rk:i:" + h[1] and x[12].startswith("AS:i:") and x[14].startswith("cg:Z:")
        words = parse_cigar(x[14][5:])
        if x[4] == "-":
            q = q.translate(_RC)[::-1]
        cols, eq, score, ua, ub, true = T.replay(words, np.frombuffer(q, np.uint8), np.frombuffer(t, np.uint8))
        assert true and (ua, ub) == (len(q), len(t)) and (cols, eq) == (ln, ids), x[:6]
        assert score == int(x[12][5:]), x[:6]
        nops += len(words)
        strands.add(x[4])
        kinds.update(w & 15 for w in words)
    assert p_st["cigar_ops"] == nops and strands == {"+", "-"} and kinds == {T.OP_I, T.OP_D, T.OP_EQ, T.OP_X}
    # --min-identity selects as without --paf; the PAF lists every aligned pair
    ident = sorted(float(h[6]) for h in hits if h[1] == "1")
    mid = repr(ident[len(ident) // 2])
    m_tsv, m_hits, _, m_st = e2e("mid", ["--min-identity", mid])
    mp_tsv, mp_hits, mp_paf, mp_st = e2e("mid_paf", ["--min-identity", mid, "--paf", "@PAF"])
    assert mp_paf.read_bytes() == p_paf.read_bytes()
    assert mp_tsv.read_bytes() == m_tsv.read_bytes() and mp_hits.read_bytes() == m_hits.read_bytes()
    assert mp_tsv.read_bytes() != p_tsv.read_bytes() and mp_st["rejected"] == m_st["rejected"] > 0


def test_assign_files_paf(e2e, tmp_path):
    """The same job in process (mcl_assign_paf), on a context of its own sequences."""
    _, p_hits, p_paf, _ = e2e("paf", ["--paf", "@PAF"])
    e = M.Engine(0)
    try:
        model = str(e2e.cen).replace(".centres.fa", ".model")
        st = M.assign_files(e, model, str(e2e.cen), str(e2e.reads), str(tmp_path / "l.tsv"), threads=2, both_strands=True, top=3,
                            hits=str(tmp_path / "l.hits"), paf=str(tmp_path / "l.paf"))
    finally:
        e.close()
    assert (tmp_path / "l.paf").read_bytes() == p_paf.read_bytes() and (tmp_path / "l.hits").read_bytes() == p_hits.read_bytes()
    assert st["paf_pairs"] == len(rows(p_paf))
