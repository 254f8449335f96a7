"""mc_nw_msa_crossover / meshclust-assign --chimeras on the GPU.  Every comparison is ==.

The expectations: the Python restatement of tests/crossover_cases.py over its own seeded points (held
equal to a second restatement from rendered rows by test_crossover_host.py, the alignments tied to the
CPU oracle by test_nw_trace_host.py), begin's own ids, and for the tool the CIGARs of the same run's
--paf file.  One set of points, loaded once."""
import ctypes as C

import numpy as np
import pytest

import crossover_cases as X
import meshclust_amd as M
import test_gpu_pileup as G

pytestmark = pytest.mark.gpu

e2e = G.e2e  # the a1k model and centres; this file's reads and three planted centres go through it
ENV_VARS = G.ENV_VARS + ("MC_MSA_BYTES", "MC_CROSS_BATCH", "MC_CROSS_MAX")


def clean_env(monkeypatch, **kw):
    for var in ENV_VARS:
        monkeypatch.delenv(var, raising=False)
    for k, v in kw.items():
        monkeypatch.setenv(k, str(v))


@pytest.fixture(scope="module")
def eng(built):
    e = M.Engine(0)
    e.load_sequences(*X.cross().load_args())
    yield e
    e.close()


def begin(eng, name):
    q = X.cross()
    return eng.nw_msa_begin(q.a, q.b, None if name == "plus" else q.strands(name), q.targets)


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert not len(bad), (what, len(bad), bad[:6], got[bad[:6]].tolist(), want[bad[:6]].tolist(), [X.cross().label[c] for c in bad[:6]])
    return True


# ---------------------------------------------------------------- 1. the values
@pytest.mark.parametrize("name", X.NAMES)
def test_crossover_equals_the_restatement(eng, name, monkeypatch):
    clean_env(monkeypatch)
    q = X.cross()
    ids = begin(eng, name)[5]
    got = eng.nw_msa_crossover(q.x, q.y)
    same(got, X.expected(name), name)
    # slots 0 and 1 are begin's ids; the exchange of x and y
    assert np.array_equal(got[:, 0], ids[q.x.astype(np.int64)]) and np.array_equal(got[:, 1], ids[q.y.astype(np.int64)])
    same(eng.nw_msa_crossover(q.y, q.x), X.exchanged(X.expected(name)), (name, "exchanged"))


# ---------------------------------------------------------------- 2. batches, ranges, other entries, the band
def test_batches_ranges_and_other_entries_change_nothing(eng, monkeypatch):
    q = X.cross()
    am = q.strands("mixed")
    nt, m, nc = len(q.targets), len(q.a), len(q.x)
    want = X.expected("mixed")
    clean_env(monkeypatch)
    begin(eng, "mixed")
    # unbatched: one launch per length bucket in use (at most 1024 bases; 2047 and 2048; 2049)
    eng.timers(reset=True)
    same(eng.nw_msa_crossover(q.x, q.y), want, "one batch")
    assert eng.timers()["nw"][1] == 3
    for per in (1, 7):
        clean_env(monkeypatch, MC_CROSS_BATCH=per)
        eng.timers(reset=True)
        same(eng.nw_msa_crossover(q.x, q.y), want, ("MC_CROSS_BATCH", per))
        assert eng.timers()["nw"][1] >= (nc + per - 1) // per
    clean_env(monkeypatch)
    for step in (1, 5):  # ranges of candidates over calls, and the list backwards
        got = [eng.nw_msa_crossover(q.x[k:k + step], q.y[k:k + step]) for k in range(0, nc, step)]
        same(np.concatenate(got), want, ("ranges", step))
    same(eng.nw_msa_crossover(q.x[::-1], q.y[::-1]), want[::-1], "backwards")
    # rows, counts, sites, a pile-up and an identity call in between: they share the scratch, not the plan
    base_rows = eng.nw_msa_rows(0, nt + m)[0].tobytes()
    base_counts = eng.nw_msa_counts(0, nt)
    bw = eng.nw_msa_rows(0, nt, rows=False)[1]
    so = np.concatenate([[0], np.cumsum([1 if bw[t + 1] > bw[t] else 0 for t in range(nt)])]).astype(np.uint64)
    st = np.zeros(int(so[-1]), np.uint32)
    base_sites = eng.nw_msa_sites(so, st, 0, m)[1].tobytes()
    same(eng.nw_msa_crossover(q.x, q.y), want, "after rows, counts and sites")
    tab = eng.nw_pileup_strands(q.a, q.b, am, q.targets)[0]
    eng.nw_identity_strands(q.a[:9], q.b[:9], np.ones(9, np.uint8))
    eng.nw_align_profile(reset=True)
    assert tab[:, :4].any()
    same(eng.nw_msa_crossover(q.x, q.y), want, "after the pile-up")
    assert eng.nw_msa_rows(0, nt + m)[0].tobytes() == base_rows and eng.nw_msa_sites(so, st, 0, m)[1].tobytes() == base_sites
    assert all(np.array_equal(a, b) for a, b in zip(eng.nw_msa_counts(0, nt), base_counts))
    same(eng.nw_msa_crossover(q.x, q.y), want, "after rows, counts and sites again")
    assert eng.nw_align_profile()[2] == 0  # no choice bytes since the reset: nothing was aligned again
    # the kernel is "nw" and nothing else; a measurement entry of its own
    eng.timers(reset=True)
    eng.nw_msa_profile(reset=True)
    eng.nw_msa_counts_profile(reset=True)
    eng.nw_msa_sites_profile(reset=True)
    assert eng.nw_msa_crossover_profile(reset=True) > 0 and eng.nw_msa_crossover_profile() == 0
    eng.nw_msa_crossover(q.x, q.y)
    t = eng.timers()
    assert t["nw"][1] == 3 and all(t[f][1] == 0 for f in t if f != "nw")
    assert eng.nw_msa_crossover_profile() > 0
    assert eng.nw_msa_profile() == (0.0, 0.0, 0.0, 0.0) and eng.nw_msa_counts_profile() == 0 and eng.nw_msa_sites_profile() == 0


def test_the_band_changes_nothing(eng, monkeypatch):
    clean_env(monkeypatch)
    q = X.cross()
    eng.set_align_band(1)
    try:
        begin(eng, "mixed")
        same(eng.nw_msa_crossover(q.x, q.y), X.expected("mixed"), "band")
    finally:
        eng.set_align_band(0)


# ---------------------------------------------------------------- 3. the contract
def test_errors_and_state(eng, monkeypatch):
    q = X.cross()
    m, nc = len(q.a), len(q.x)
    clean_env(monkeypatch)
    begin(eng, "mixed")
    want = X.expected("mixed")
    lib, ptr = eng.lib, M._p
    SENT = -0x5A5A5A5B

    def call(x, y, n, out, e=None):
        return lib.mc_nw_msa_crossover((e or eng).ctx, ptr(x), ptr(y), C.c_uint64(n), ptr(out))

    fresh = lambda: np.full((nc + 1) * X.RES, SENT, np.int32)
    untouched = lambda a: bool((a == SENT).all())
    u64 = lambda v: np.array(v, np.uint64)
    out = fresh()
    assert call(q.x, q.y, nc, out) == 0 and np.array_equal(out[:nc * X.RES].reshape(nc, X.RES), want) and untouched(out[nc * X.RES:])
    # nc = 0: MC_OK whatever the pointers; NULL with nc > 0
    out = fresh()
    eng.timers(reset=True)
    assert call(None, None, 0, None) == 0 and call(q.x, q.y, 0, out) == 0 and untouched(out)
    assert call(None, q.y, nc, out) == M.ERR_ARG and call(q.x, None, nc, out) == M.ERR_ARG and call(q.x, q.y, nc, None) == M.ERR_ARG
    assert untouched(out)
    # an index >= m, as the first candidate and as the last; two pairs of different reads
    for bad in (m, m + 1, 1 << 40, (1 << 64) - 1):
        for where in (0, nc - 1):
            x2, y2 = q.x.copy(), q.y.copy()
            x2[where] = bad
            assert call(x2, q.y, nc, out) == M.ERR_ARG and untouched(out), (bad, where)
            y2[where] = bad
            assert call(q.x, y2, nc, out) == M.ERR_ARG and untouched(out), (bad, where)
    other = next(k for k in range(m) if q.a[k] != q.a[int(q.x[nc - 1])])
    y2 = q.y.copy()
    y2[nc - 1] = other
    assert call(q.x, y2, nc, out) == M.ERR_ARG and untouched(out)
    with pytest.raises(M.MCError) as err:
        eng.nw_msa_crossover(u64([0]), u64([m]))
    assert err.value.code == M.ERR_ARG
    # MC_CROSS_MAX below one read's length: refused before any launch, nothing written; at its length: accepted
    longest = max(q.la(int(x)) for x in q.x)
    assert longest == 2049
    clean_env(monkeypatch, MC_CROSS_MAX=100)
    c120 = next(c for c in range(nc) if q.la(int(q.x[c])) == 120)
    assert call(q.x[c120:c120 + 1], q.y[c120:c120 + 1], 1, out) == M.ERR_UNSUPPORTED and untouched(out)
    clean_env(monkeypatch, MC_CROSS_MAX=longest - 1)
    assert call(q.x, q.y, nc, out) == M.ERR_UNSUPPORTED and untouched(out)
    assert all(v[1] == 0 for v in eng.timers().values())  # every error so far was found before any launch
    short = np.array([q.la(int(x)) < longest for x in q.x])
    assert call(q.x[short], q.y[short], int(short.sum()), out) == 0
    assert np.array_equal(out[:int(short.sum()) * X.RES].reshape(-1, X.RES), want[short])
    out = fresh()
    clean_env(monkeypatch, MC_CROSS_MAX=longest)
    assert call(q.x, q.y, nc, out) == 0 and np.array_equal(out[:nc * X.RES].reshape(nc, X.RES), want)
    clean_env(monkeypatch)

    # no plan: after end, before any begin, after a load of sequences
    def no_plan(e=None):
        return call(u64([0]), u64([0]), 1, fresh(), e) == M.ERR_STATE and call(None, None, 0, None, e) == M.ERR_STATE

    assert not no_plan()
    eng.nw_msa_end()
    out = fresh()
    assert no_plan() and call(q.x, q.y, nc, out) == M.ERR_STATE and untouched(out)
    begin(eng, "mixed")
    same(eng.nw_msa_crossover(q.x, q.y), want, "after end and a new begin")  # (end freed the buffers: they come back)
    other = M.Engine(0)
    try:
        assert no_plan(other)  # no sequences
        other.load_sequences(*q.load_args())
        assert no_plan(other)  # sequences, but no begin yet
        other.nw_msa_begin(q.a[:4], q.b[:4], None, sorted(set(int(j) for j in q.b[:4])))
        assert call(u64([0, 2]), u64([1, 3]), 2, out, other) == 0
        other.load_sequences(*q.load_args())
        assert no_plan(other)
    finally:
        other.close()


# ---------------------------------------------------------------- 4. end to end
CHIMERA_KEYS = ("chimera_candidates", "chimeras")
DROP = CHIMERA_KEYS + ("phases_ms", "device_us")
CUTS = (120, 200, 250, 310, 390)


@pytest.fixture(scope="module")
def planted(e2e):
    """Three centres of the a1k file replaced: P (its first centre), Q (P with a substitution every 16 bases) and
    R (P with two substitutions); the reads: error-free chimeras of P and Q cut at CUTS, both ways round, reads of
    P, Q and R with private substitutions, and 40 of the a1k reads; every second read reverse-complemented.
    -> (centres file, reads file, the planted chimeras' names)."""
    rng = np.random.default_rng(3)
    cens = G.read_fasta(e2e.cen)
    P = bytearray(cens[0][1].upper())
    assert len(P) >= 450 and set(P) <= set(b"ACGT")

    def subst(s, at):
        s = bytearray(s)
        for i in at:
            s[i] = b"ACGT"[(b"ACGT".index(s[i]) + 1 + i % 3) % 4]
        return bytes(s)

    Q, R = subst(P, range(5, len(P), 16)), subst(P, (100, 400))
    cens[0][1], cens[1][1], cens[2][1] = bytes(P), Q, R
    cfile, rfile = e2e.tmp / "chim.centres.fa", e2e.tmp / "chim.reads.fa"
    cfile.write_bytes(b"".join(h + b"\n" + s + b"\n" for h, s in cens))
    recs, names = [], []
    for cut in CUTS:
        recs += [(b">pq%d" % cut, bytes(P[:cut]) + Q[cut:]), (b">qp%d" % cut, Q[:cut] + bytes(P[cut:]))]
        names += ["pq%d" % cut, "qp%d" % cut]
    for n, s in enumerate((bytes(P), Q, R, bytes(P), Q)):
        recs.append((b">pure%d" % n, subst(s, sorted(int(v) for v in rng.choice(len(s), 4, replace=False)))))
    recs += [(h, s.upper()) for h, s in G.read_fasta(e2e.reads)[:40]]
    rfile.write_bytes(b"".join(h + b"\n" + (s.translate(G._RC)[::-1] if i % 2 else s) + b"\n" for i, (h, s) in enumerate(recs)))
    return cfile, rfile, names


def chimeras_from_paf(paf, min_gain):
    """The --chimeras text from the --paf file of the same run (one line per hit, ranks ascending) by
    crossover_cases' restatement and its port of chimera.hpp -> (text, lines, flagged)."""
    reads, order = {}, []
    for x in G.rows_of(paf):
        if x[0] not in reads:
            reads[x[0]] = []
            order.append(x[0])
        rank = int(next(t for t in x[12:] if t.startswith("rk:i:"))[5:])
        assert rank == len(reads[x[0]]) + 1
        reads[x[0]].append((x[5], x[4], G.parse_cigar(x[14][5:]), int(x[1])))
    text, lines, flagged = [], 0, 0
    for name in order:
        hits = reads[name]
        cand = X.chimera_candidates([h[0] for h in hits])
        if not cand:
            continue
        e = [X.e_from_words(words, la, sd == "-") for _, sd, words, la in hits]
        pick = X.chimera_pick(cand, [X.crossover(e[0], e[j]) for j in cand], min_gain)
        j, xy, best, gain, first, last, left, right, flag = pick
        lt, rt = (hits[0], hits[j]) if xy else (hits[j], hits[0])
        text.append("%s\t%s\t%s\t%s\t%s\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%s\n" % (name, lt[0], rt[0], lt[1], rt[1], first, last, left, right, best, gain,
                                                                             hits[0][3], "Y" if flag else "N"))
        lines += 1
        flagged += flag
    return "".join(text), lines, flagged


def test_cli_chimeras(e2e, planted):
    cfile, rfile, names = planted
    path = lambda name, ext: str(e2e.tmp / (name + ext))
    base = lambda name: ["--both-strands", "--top", "3", "--hits", path(name, ".hits.tsv"), "--paf", "@paf"]
    full = e2e("c_full", base("c_full") + ["--chimeras", path("c_full", ".chim.tsv")], reads_fa=rfile, centres=cfile)
    plain = e2e("c_plain", base("c_plain"), reads_fa=rfile, centres=cfile)
    got = open(path("c_full", ".chim.tsv")).read()
    want, lines, flagged = chimeras_from_paf(full["paf"], 3)
    assert got == want
    # not vacuous: a planted chimera flagged Y with its cut inside the reported range, a candidate flagged N, both strands
    rows = [ln.split("\t") for ln in got.splitlines()]
    hit = [x for x in rows if x[0] in names and x[12] == "Y"]
    planted_cut = lambda x: int(x[11]) - int(x[0][2:]) if x[0].startswith("qp") else int(x[0][2:])  # (the qp reads are written flipped)
    assert hit and all(int(x[5]) <= planted_cut(x) <= int(x[6]) and int(x[10]) >= 3 for x in hit), [x for x in hit if x[0] in names]
    assert any(x[12] == "N" for x in rows) and {x[3] for x in rows} == {"+", "-"} and all(len(x) == 13 for x in rows)
    # every other output and the remaining stats are those of the run without the new option
    assert full["tsv"].read_bytes() == plain["tsv"].read_bytes() and full["paf"].read_bytes() == plain["paf"].read_bytes()
    assert open(path("c_full", ".hits.tsv"), "rb").read() == open(path("c_plain", ".hits.tsv"), "rb").read()
    st, pst = full["st"], plain["st"]
    assert not any(k in pst for k in CHIMERA_KEYS) and "chimeras" not in pst["phases_ms"]
    assert {k: v for k, v in st.items() if k not in DROP} == {k: v for k, v in pst.items() if k not in DROP}
    assert list(st)[:-2] == list(pst) and list(st)[-2:] == list(CHIMERA_KEYS) and [st[k] for k in CHIMERA_KEYS] == [lines, flagged]
    assert list(st["phases_ms"])[:-1] == list(pst["phases_ms"]) and list(st["phases_ms"])[-1] == "chimeras" and st["phases_ms"]["chimeras"] > 0
    # another threshold flags by the same rule; --band and the other plan users beside it change nothing
    high = e2e("c_high", base("c_high") + ["--chimeras", path("c_high", ".chim.tsv"), "--min-chimera-gain", "1000"], reads_fa=rfile, centres=cfile)
    assert open(path("c_high", ".chim.tsv")).read() == chimeras_from_paf(high["paf"], 1000)[0] == want.replace("\tY\n", "\tN\n")
    assert [high["st"][k] for k in CHIMERA_KEYS] == [lines, 0]
    band = e2e("c_band", base("c_band") + ["--band", "--msa", path("c_band", ".msa.fa"), "--alleles", path("c_band", ".al.tsv"), "--chimeras",
                                           path("c_band", ".chim.tsv")], reads_fa=rfile, centres=cfile)
    nochim = e2e("c_nochim", base("c_nochim") + ["--msa", path("c_nochim", ".msa.fa"), "--alleles", path("c_nochim", ".al.tsv")],
                 reads_fa=rfile, centres=cfile)
    assert open(path("c_band", ".chim.tsv")).read() == want
    assert open(path("c_band", ".msa.fa"), "rb").read() == open(path("c_nochim", ".msa.fa"), "rb").read()
    assert open(path("c_band", ".al.tsv"), "rb").read() == open(path("c_nochim", ".al.tsv"), "rb").read()
    assert list(band["st"])[-2:] == list(CHIMERA_KEYS) and band["st"]["band_pairs"] > 0


def test_assign_files_chimeras(e2e, planted, tmp_path):
    """The same job in process (mcl_assign_chimeras), on a context of its own sequences."""
    cfile, rfile, _ = planted
    path = lambda name, ext: str(e2e.tmp / (name + ext))
    full = e2e("c_full", ["--both-strands", "--top", "3", "--hits", path("c_full", ".hits.tsv"), "--paf", "@paf", "--chimeras",
                          path("c_full", ".chim.tsv")], reads_fa=rfile, centres=cfile)
    e = M.Engine(0)
    try:
        model = str(e2e.cen).replace(".centres.fa", ".model")
        st = M.assign_files(e, model, str(cfile), str(rfile), str(tmp_path / "l.tsv"), threads=2, both_strands=True, top=3,
                            hits=str(tmp_path / "l.hits"), chimeras=str(tmp_path / "l.chim"))
        st2 = M.assign_files(e, model, str(cfile), str(rfile), str(tmp_path / "l2.tsv"), threads=2, both_strands=True, top=3,
                             hits=str(tmp_path / "l2.hits"), chimeras=str(tmp_path / "l2.chim"), min_chimera_gain=1000)
        for kw in (dict(top=1, hits=str(tmp_path / "l3.hits")), dict(), dict(top=3, hits=str(tmp_path / "l3.hits"), min_chimera_gain=0)):
            with pytest.raises(Exception):
                M.assign_files(e, model, str(cfile), str(rfile), str(tmp_path / "l3.tsv"), chimeras=str(tmp_path / "l3.chim"), **kw)
    finally:
        e.close()
    want = open(path("c_full", ".chim.tsv"), "rb").read()
    assert (tmp_path / "l.chim").read_bytes() == want and (tmp_path / "l2.chim").read_bytes() == want.replace(b"\tY\n", b"\tN\n")
    assert (tmp_path / "l.tsv").read_bytes() == full["tsv"].read_bytes()
    assert [st[k] for k in CHIMERA_KEYS] == [full["st"][k] for k in CHIMERA_KEYS] and list(st)[-2:] == list(CHIMERA_KEYS)
    assert st2["chimeras"] == 0 and st2["chimera_candidates"] == st["chimera_candidates"]
