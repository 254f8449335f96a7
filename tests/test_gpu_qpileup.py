"""mc_load_qualities / mc_nw_qpileup_strands / meshclust-assign --quality on the GPU.  Every
comparison is ==.

The expectations: the Python restatements of tests/pileup_cases.py (counts) and
tests/qpileup_cases.py (weights, weighted consensus) over the words of tests/nw_trace_cases.py, and
mc_nw_pileup_strands itself for the count table and the integers.  One set of points and
qualities, loaded once."""
import ctypes as C
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

pytestmark = pytest.mark.gpu

ASSIGN_BIN = os.path.join(os.path.dirname(M.BIN), "meshclust-assign")
ENV_VARS = ("MC_ALIGN_BATCH", "MC_ALIGN_SCRATCH", "MC_IDENT_BATCH", "MC_IDENT_BYTES", "MC_PILEUP_NAIVE")


@pytest.fixture(scope="module")
def eng(built):
    e = M.Engine(0)
    e.load_sequences(*P.pile().load_args())
    e.load_qualities(Q.flat(Q.qualities()))
    yield e
    e.close()


def clean_env(monkeypatch, **kw):
    for var in ENV_VARS:
        monkeypatch.delenv(var, raising=False)
    for k, v in kw.items():
        monkeypatch.setenv(k, str(v))


def same(xs, ys):
    return len(xs) == len(ys) and all(x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(xs, ys))


# ---------------------------------------------------------------- 1. both tables
@pytest.mark.parametrize("name", ["plus", "minus", "mixed"])
def test_tables_equal_the_restatement(eng, name, monkeypatch):
    clean_env(monkeypatch)
    p = P.pile()
    n = len(p.a)
    am = {"plus": None, "minus": np.ones(n, np.uint8), "mixed": P.mixed_strands()}[name]
    flags = np.zeros(n, np.uint8) if am is None else am
    tab, wtab, off, score, ln, ids = eng.nw_qpileup_strands(p.a, p.b, am, p.targets)
    # the count table, the offsets and the integers are mc_nw_pileup_strands' (which is unchanged)
    ref = eng.nw_pileup_strands(p.a, p.b, am, p.targets)
    assert same((tab, off, score, ln, ids), ref)
    assert np.array_equal(ref[0], P.expected_table(flags))
    assert wtab.dtype == np.uint32 and wtab.shape == tab.shape
    want = Q.expected_wtable(flags)
    bad = np.nonzero((wtab != want).any(axis=1))[0]
    assert len(bad) == 0, (name, bad[:8], wtab[bad[:4]], want[bad[:4]])
    assert not wtab[:, 7].any()
    t = p.tindex[p.lonely]
    assert not wtab[int(off[t]):int(off[t + 1])].any()  # a target with no pair


# ---------------------------------------------------------------- 2. batching, a repeated call
def test_batches_give_the_same_bytes(eng, monkeypatch):
    p = P.pile()
    am = P.mixed_strands()
    clean_env(monkeypatch)
    base = eng.nw_qpileup_strands(p.a, p.b, am, p.targets)
    assert np.array_equal(base[1], Q.expected_wtable(am))
    big = T.choice_bytes(1100, 1100)
    # MC_IDENT_BYTES: as test_gpu_pileup.py, batch ends by the byte cap, one of them inside the contended centre's reads
    lens = [len(x) for x in p.codes]
    nbytes = T.ident_bytes(lens, p.a[am != 0])
    by = [i1 for i1, why in T.batch_ends(lens, p.a, p.b, am, 1 << 16, nbytes, 1 << 30) if why == "bytes"]
    assert len(by) >= 2 and any(p.b[i1 - 1] == p.contended == p.b[i1] for i1 in by), (nbytes, by)
    for env in ({"MC_ALIGN_BATCH": 7}, {"MC_ALIGN_BATCH": 1}, {"MC_ALIGN_SCRATCH": 3 * big + 64}, {"MC_IDENT_BYTES": nbytes}):
        clean_env(monkeypatch, **env)
        assert same(eng.nw_qpileup_strands(p.a, p.b, am, p.targets), base), env
    # a second call overwrites: fewer pairs give smaller tables
    clean_env(monkeypatch)
    half = np.arange(0, len(p.a), 2)
    tab, wtab, _, _, _, _ = eng.nw_qpileup_strands(p.a[half], p.b[half], am[half], p.targets)
    assert np.array_equal(tab, P.expected_table(am, half)) and np.array_equal(wtab, Q.expected_wtable(am, half))


# ---------------------------------------------------------------- 3. the calls' contract
def test_contract(eng, monkeypatch):
    p = P.pile()
    am = P.mixed_strands()
    clean_env(monkeypatch)
    tab, wtab, off, score, ln, ids = eng.nw_qpileup_strands(p.a, p.b, am, p.targets)
    lib, ptr = eng.lib, M._p
    m, nt, rows = len(p.a), len(p.targets), int(off[-1])
    a, b, tg = np.ascontiguousarray(p.a), np.ascontiguousarray(p.b), np.ascontiguousarray(p.targets)
    SENT = 0xDEADBEEF
    buf = np.full((rows + 2) * 8, SENT, np.uint32)
    wbuf = np.full((rows + 2) * 8, SENT, np.uint32)
    o = np.full(nt + 1, 77, np.uint64)
    s = np.full(m, -7, np.int32)

    def call(ctx, n, t, w, cap):
        return lib.mc_nw_qpileup_strands(ctx, ptr(a[:n]), ptr(b[:n]), ptr(am[:n]), C.c_uint64(n), ptr(tg), C.c_uint32(nt), ptr(o),
                                         ptr(t), ptr(w), C.c_uint64(cap), ptr(s), ptr(s), ptr(s))

    def untouched(offsets=True):
        return (buf == SENT).all() and (wbuf == SENT).all() and (s == -7).all() and (not offsets or (o == 77).all())

    # exactly one table NULL: refused, nothing written; both NULL: the offsets only
    assert call(eng.ctx, m, buf, None, rows) == M.ERR_ARG and untouched()
    assert call(eng.ctx, m, None, wbuf, rows) == M.ERR_ARG and untouched()
    assert call(eng.ctx, m, None, None, 0) == 0 and np.array_equal(o, off) and untouched(offsets=False)
    # one row short: the offsets are valid, the tables untouched (as mc_nw_pileup_strands)
    o[:] = 77
    assert call(eng.ctx, m, buf, wbuf, rows - 1) == M.ERR_ARG and np.array_equal(o, off) and untouched(offsets=False)
    # exactly enough
    assert call(eng.ctx, m, buf, wbuf, rows) == 0
    assert np.array_equal(buf[:rows * 8].reshape(rows, 8), tab) and (buf[rows * 8:] == SENT).all()
    assert np.array_equal(wbuf[:rows * 8].reshape(rows, 8), wtab) and (wbuf[rows * 8:] == SENT).all()
    assert np.array_equal(s, ids)
    # m = 0: two zeroed tables
    buf[:], wbuf[:], o[:], s[:] = SENT, SENT, 77, -7
    assert call(eng.ctx, 0, buf, wbuf, rows) == 0 and np.array_equal(o, off)
    for x in (buf, wbuf):
        assert (x[:rows * 8] == 0).all() and (x[rows * 8:] == SENT).all()
    # a scratch cap below one pair's need: refused before anything is written
    buf[:], wbuf[:], o[:] = SENT, SENT, 77
    clean_env(monkeypatch, MC_ALIGN_SCRATCH=T.choice_bytes(1100, 1100) - 1)
    assert call(eng.ctx, m, buf, wbuf, rows) == M.ERR_UNSUPPORTED and untouched()
    clean_env(monkeypatch)
    # a context of its own: no sequences, no qualities, bad qualities, a reload of the sequences
    q = Q.flat(Q.qualities())
    fresh = M.Engine(0)
    try:
        assert lib.mc_load_qualities(fresh.ctx, ptr(q), C.c_uint64(len(q))) == M.ERR_STATE  # no sequences
        assert call(fresh.ctx, m, buf, wbuf, rows) == M.ERR_STATE and untouched()
        fresh.load_sequences(*p.load_args())
        assert call(fresh.ctx, m, buf, wbuf, rows) == M.ERR_STATE and untouched()  # no qualities
        assert call(fresh.ctx, m, None, None, 0) == M.ERR_STATE and untouched()
        bad = q.copy()
        bad[len(bad) // 2] = 94
        assert lib.mc_load_qualities(fresh.ctx, ptr(bad), C.c_uint64(len(bad))) == M.ERR_ARG  # above MC_QUAL_MAX
        assert lib.mc_load_qualities(fresh.ctx, ptr(q), C.c_uint64(len(q) - 1)) == M.ERR_ARG  # a wrong size
        assert lib.mc_load_qualities(fresh.ctx, ptr(np.concatenate([q, q[:1]])), C.c_uint64(len(q) + 1)) == M.ERR_ARG
        assert call(fresh.ctx, m, buf, wbuf, rows) == M.ERR_STATE and untouched()  # (a refused load loads nothing)
        fresh.load_qualities(q)
        assert call(fresh.ctx, m, buf, wbuf, rows) == 0
        assert np.array_equal(wbuf[:rows * 8].reshape(rows, 8), wtab) and np.array_equal(buf[:rows * 8].reshape(rows, 8), tab)
        fresh.load_sequences(*p.load_args())  # drops the qualities
        buf[:], wbuf[:], o[:], s[:] = SENT, SENT, 77, -7
        assert call(fresh.ctx, m, buf, wbuf, rows) == M.ERR_STATE and untouched()
        with pytest.raises(M.MCError) as e:
            fresh.nw_qpileup_strands(p.a, p.b, am, p.targets)
        assert e.value.code == M.ERR_STATE
        # the count-only entry needs no qualities and returns what it did
        assert np.array_equal(fresh.nw_pileup_strands(p.a, p.b, am, p.targets)[0], P.expected_table(am))
    finally:
        fresh.close()
    eng.timers(reset=True)
    eng.nw_pileup_profile(reset=True)
    eng.nw_qpileup_strands(p.a[:5], p.b[:5], [1, 0, 0, 0, 0], p.targets)
    t = eng.timers()
    assert t["layout"][1] == 1 and t["nw"][1] >= 4  # forward, traceback, pile-up and finish as nw
    assert all(t[f][1] == 0 for f in t if f not in ("layout", "nw"))
    assert all(x > 0 for x in eng.nw_pileup_profile())


# ---------------------------------------------------------------- 4. end to end
_RC = bytes.maketrans(b"ACGT", b"TGCA")
_LUT = np.full(256, 255, np.uint8)
for _i, _c in enumerate(b"ACGT"):
    _LUT[_c] = _i


def read_fasta(path):
    recs = []
    with open(path, "rb") as f:
        for ln in f.read().splitlines():
            if ln.startswith(b">"):
                recs.append([ln, b""])
            else:
                recs[-1][1] += ln
    return recs


def read_fastq(path):
    ls = open(path, "rb").read().splitlines()
    assert len(ls) % 4 == 0 and all(x.startswith(b"@") for x in ls[0::4]) and all(x.startswith(b"+") for x in ls[2::4])
    return [(ls[i][1:].decode(), ls[i + 1], ls[i + 3]) for i in range(0, len(ls), 4)]


def rows_of(path):
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


def codes_of(seq):
    c = _LUT[np.frombuffer(seq, np.uint8)]
    assert (c <= 3).all()
    return c


def outputs_from_paf(paf, reads_fq, centres_fa):
    """-> (consensus FASTQ text, widened pile-up TSV text) from a PAF's CIGARs, the FASTQ reads and
    the centres alone."""
    reads = {name: (s.upper(), np.frombuffer(q, np.uint8) - 33) for name, s, q in read_fastq(reads_fq)}
    cents = [(h[1:].decode(), codes_of(s.upper())) for h, s in read_fasta(centres_fa)]
    cen = dict(cents)
    tabs = {name: np.zeros((len(c) + 1, 8), np.uint32) for name, c in cents}
    wtabs = {name: np.zeros((len(c) + 1, 8), np.uint32) for name, c in cents}
    runs = {name: [] for name, _ in cents}
    depth = {name: 0 for name, _ in cents}
    for x in rows_of(paf):
        s, q = reads[x[0]]
        if x[4] == "-":
            s, q = s.translate(_RC)[::-1], q[::-1]
        s = codes_of(s)
        words = parse_cigar(x[14][5:])
        P.table_from_words(words, s, cen[x[5]], tabs[x[5]])
        Q.wtable_from_words(words, s, q, cen[x[5]], wtabs[x[5]])
        runs[x[5]] += Q.insertion_runs(words, s, q)
        depth[x[5]] += 1
    fq, tsv = [], []
    for name, c in cents:
        seq, qual, sub, dele, ins = Q.consensus(c, tabs[name], wtabs[name], depth[name], runs[name])
        fq.append("@%s depth=%d sub=%d del=%d ins=%d\n%s\n+\n%s\n" % (name, depth[name], sub, dele, ins, seq, qual))
        if depth[name]:
            for r in range(len(c) + 1):
                tsv.append("\t".join([name, str(r + 1), P.base_char(c[r]) if r < len(c) else "*", str(depth[name])] +
                                     [str(int(v)) for v in tabs[name][r]] + [str(int(v)) for v in wtabs[name][r][:6]]) + "\n")
    return "".join(fq), "".join(tsv)


@pytest.fixture(scope="module")
def family(built, tmp_path_factory):
    """A saved clustering whose first centre is the planted centre of pileup_cases, its 30 reads as
    FASTQ (seeded qualities 0 .. 5, every second read reverse-complemented) and as the FASTA twin."""
    tmp = tmp_path_factory.mktemp("qpileup")
    fa, flags = fixtures.e2e_input("a1k", tmp)
    model, cen = tmp / "a1k.model", tmp / "a1k.centres.fa"
    r = subprocess.run([M.BIN, fa] + flags + ["--output", str(tmp / "a1k.clstr"), "--quiet", "--save-model", str(model),
                                              "--save-centres", str(cen)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    p = P.pile()
    letters = lambda c: "".join(P.LETTERS[x] for x in c).encode()
    cens = read_fasta(cen)
    cens[0][1] = letters(p.codes[p.planted])
    cfile, fq, twin = tmp / "planted.centres.fa", tmp / "planted.fastq", tmp / "planted.fa"
    cfile.write_bytes(b"".join(h + b"\n" + s + b"\n" for h, s in cens))
    rng = np.random.default_rng(7)
    ks = [k for k in range(len(p.a)) if p.b[k] == p.planted]
    with open(fq, "wb") as f, open(twin, "wb") as g:
        for i, k in enumerate(ks):
            s = letters(p.codes[p.a[k]])
            if i % 2:
                s = s.translate(_RC)[::-1]
            # (low qualities: 30 reads of them leave most columns of the consensus below the clamp at 93)
            q = bytes(bytearray(int(v) + 33 for v in rng.integers(0, 6, len(s))))
            f.write(b"@p%d\n" % i + s + b"\n+\n" + q + b"\n")
            g.write(b">p%d\n" % i + s + b"\n")
    env = {k: v for k, v in os.environ.items() if k not in ("MC_ASSIGN_FORM", "MC_ASSIGN_TILE", "MC_ASSIGN_PAIRS") + ENV_VARS}

    def run(name, extra, reads, code=0):
        out = {k: tmp / (name + ext) for k, ext in (("tsv", ".tsv"), ("paf", ".paf"), ("cons", ".cons"), ("pile", ".pile.tsv"),
                                                    ("stats", ".json"))}
        args = [str(out[a[1:]]) if a.startswith("@") else a for a in extra]
        r = subprocess.run([ASSIGN_BIN, "--model", str(model), "--centres", str(cfile), str(reads), "--output", str(out["tsv"]),
                            "--quiet", "--stats-json", str(out["stats"])] + args, capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode == code, r.stderr[-3000:]
        out["stderr"] = r.stderr
        if code == 0:
            out["st"] = json.loads(out["stats"].read_text())
        return out

    run.model, run.cen, run.fq, run.twin, run.tmp, run.ncen = model, cfile, fq, twin, tmp, len(cens)
    return run


ALL = ["--both-strands", "--paf", "@paf", "--consensus", "@cons", "--pileup", "@pile"]


def test_cli_quality_end_to_end(family):
    full = family("q", ALL + ["--quality"], family.fq)
    st = full["st"]
    assert st["quality"] == 1 and st["assigned"] == 30 and st["assigned_minus"] == 15 and st["consensus_centres"] == 1
    paf = rows_of(full["paf"])
    assert len(paf) == 30 and {x[4] for x in paf} == {"+", "-"}
    fq, tsv = outputs_from_paf(full["paf"], family.fq, family.cen)
    assert full["cons"].read_text() == fq
    assert full["pile"].read_text() == tsv
    recs = read_fastq(full["cons"])
    assert len(recs) == family.ncen and " depth=30 sub=" in recs[0][0]
    assert all(len(s) == len(q) for _, s, q in recs)
    assert all(q == b"!" * len(s) and name.endswith(" depth=0 sub=0 del=0 ins=0") for name, s, q in recs[1:])
    assert len(set(recs[0][2])) > 1 and all(len(x) == 18 for x in rows_of(full["pile"]))
    # the same job in process
    e = M.Engine(0)
    try:
        lst = M.assign_files(e, str(family.model), str(family.cen), str(family.fq), str(family.tmp / "l.tsv"), threads=2,
                             both_strands=True, consensus=str(family.tmp / "l.fq"), pileup=str(family.tmp / "l.pile"), quality=True)
    finally:
        e.close()
    assert lst["quality"] == 1
    assert (family.tmp / "l.fq").read_bytes() == full["cons"].read_bytes()
    assert (family.tmp / "l.pile").read_bytes() == full["pile"].read_bytes()


def test_cli_without_quality_fastq_is_its_fasta_twin(family):
    q = family("noq", ALL, family.fq)
    a = family("twin", ALL, family.twin)
    for k in ("tsv", "paf", "cons", "pile"):
        assert q[k].read_bytes() == a[k].read_bytes(), k
    assert "quality" not in q["st"] and q["cons"].read_bytes().startswith(b">")
    drop = ("phases_ms", "device_us")
    assert {k: v for k, v in q["st"].items() if k not in drop} == {k: v for k, v in a["st"].items() if k not in drop}
    # the counts of the weighted run are this run's
    full = family("q2", ALL + ["--quality"], family.fq)
    assert [x[:12] for x in rows_of(full["pile"])] == rows_of(q["pile"])
    assert full["tsv"].read_bytes() == q["tsv"].read_bytes() and full["paf"].read_bytes() == q["paf"].read_bytes()
    # --quality refuses FASTA reads (code 2, naming the file) and needs --consensus or --pileup
    r = family("fa", ALL + ["--quality"], family.twin, code=2)
    assert str(family.twin) in r["stderr"] and "FASTQ" in r["stderr"]
    r = family("alone", ["--quality"], family.fq, code=1)
    assert "--quality needs --consensus FILE and/or --pileup FILE" in r["stderr"]
