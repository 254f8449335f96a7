"""mc_nw_msa_counts / meshclust-assign --profile on the GPU.  Every comparison is ==.

The expectations: the Python restatement of tests/profile_cases.py over msa_cases.msa()'s points
(tied to the CPU oracle by test_nw_trace_host.py, test_pileup_host.py, test_msa_host.py and
test_profile_host.py), the rows mc_nw_msa_rows returns in the same test, and the tables of
mc_nw_pileup_strands / mc_nw_qpileup_strands.  One set of points, loaded once, with one set of
qualities."""
import ctypes as C

import numpy as np
import pytest

import meshclust_amd as M
import msa_cases as A
import nw_trace_cases as T
import pileup_cases as P
import profile_cases as F
import qpileup_cases as Q
import test_gpu_msa as GM
import test_gpu_pileup as G

pytestmark = pytest.mark.gpu

e2e = G.e2e  # the a1k fixture: 260 reads, every second one flipped
clean_env = GM.clean_env


@pytest.fixture(scope="module")
def eng(built):
    e = M.Engine(0)
    e.load_sequences(*A.msa().load_args())
    e.load_qualities(Q.flat(F.qualities()))
    yield e
    e.close()


def begin(eng, am):
    q = A.msa()
    return eng.nw_msa_begin(q.a, q.b, am, q.targets)


def histogram(rows_of_target, W):
    """The per-class histogram of a target's rendered pair rows -> [W, 6]."""
    out = np.zeros((W, 6), np.uint32)
    for row in rows_of_target:
        out[np.arange(W), F._CLASS[np.frombuffer(row, np.uint8)]] += 1
    return out


# ---------------------------------------------------------------- 1. the counts and the weights
@pytest.mark.parametrize("name", ["plus", "minus", "mixed"])
def test_counts_equal_the_restatement(eng, name, monkeypatch):
    clean_env(monkeypatch)
    q = A.msa()
    flags = q.strands(name)
    am = None if name == "plus" else flags
    nt, m = len(q.targets), len(q.a)
    want_off, want, wwant = F.tables(name)
    row_off, width, bw, _, _, _ = begin(eng, am)
    off, counts, wcounts = eng.nw_msa_counts(0, nt, weights=True)
    assert off.dtype == np.uint64 and np.array_equal(off, want_off) and np.array_equal(np.diff(off.astype(np.int64)), bw.astype(np.int64))
    assert counts.dtype == np.uint32 and counts.shape == want.shape and wcounts.shape == want.shape
    bad = np.nonzero((counts != want).any(axis=1))[0]
    assert not len(bad), (name, bad[:8], counts[bad[:4]], want[bad[:4]])
    bad = np.nonzero((wcounts != wwant).any(axis=1))[0]
    assert not len(bad), (name, bad[:8], wcounts[bad[:4]], wwant[bad[:4]])
    off2, counts2 = eng.nw_msa_counts(0, nt)  # without the weights: the same counts from the other kernel
    assert np.array_equal(off2, off) and np.array_equal(counts2, counts)
    # the histogram of the rows rendered from the same plan
    buf, roff = eng.nw_msa_rows(nt, m)
    rows = GM.split(buf, roff)
    same = 0
    for t, j in enumerate(q.targets):
        ks = [k for k in range(m) if q.b[k] == j]
        if F.renders_its_classes([q.codes[q.a[k]] for k in ks]):
            sl = slice(int(off[t]), int(off[t + 1]))
            assert np.array_equal(counts[sl, :6], histogram([rows[k] for k in ks], int(bw[t]))), (name, t)
            same += 1
    assert same >= nt - 2
    # the centre's columns are the pile-up's rows, counts and weights
    tab, wtab = eng.nw_qpileup_strands(q.a, q.b, am, q.targets)[:2]
    assert np.array_equal(tab, eng.nw_pileup_strands(q.a, q.b, am, q.targets)[0])
    width = width.astype(np.int64)
    col = np.concatenate([np.arange(int(row_off[t + 1] - row_off[t]), dtype=np.int64) + np.cumsum(width[int(row_off[t]):int(row_off[t + 1])])
                          + int(off[t]) for t in range(nt)])  # col[r] of every row, in the whole table
    base = np.ones(len(col), bool)
    base[row_off[1:].astype(np.int64) - 1] = False  # (row L of every target: no column of its own)
    assert np.array_equal(counts[col[base], :6], tab[base, :6]) and np.array_equal(wcounts[col[base], :6], wtab[base, :6])
    assert np.array_equal(counts[col[base], 6], np.concatenate([np.arange(int(row_off[t + 1] - row_off[t]) - 1) for t in range(nt)]))
    slot0 = np.nonzero(width)[0]  # slot 0 of every site that has one: its gap count
    depth = np.concatenate([np.full(int(row_off[t + 1] - row_off[t]), int((q.b == q.targets[t]).sum())) for t in range(nt)])
    assert np.array_equal(counts[col[slot0] - width[slot0], 5], depth[slot0] - tab[slot0, 6])
    t = q.tindex[P.pile().lonely]  # a target with no pair
    sl = slice(int(off[t]), int(off[t + 1]))
    assert not counts[sl, :6].any() and np.array_equal(counts[sl, 6], np.arange(33)) and not counts[sl, 7].any() and not wcounts[sl].any()


# ---------------------------------------------------------------- 2. batching, ranges and other entries change nothing
def test_batches_and_ranges_give_the_same_values(eng, monkeypatch):
    q = A.msa()
    am = q.strands("mixed")
    nt, m = len(q.targets), len(q.a)
    want_off, want, wwant = F.tables("mixed")
    lens = [len(x) for x in q.codes]
    nbytes = T.ident_bytes(lens, q.a[am != 0])
    clean_env(monkeypatch)
    begin(eng, am)
    eng.nw_align_profile(reset=True)
    for env in ({"MC_IDENT_BYTES": nbytes}, {"MC_MSA_BYTES": 4096}, {"MC_MSA_BYTES": 1000}):
        clean_env(monkeypatch, **env)
        eng.timers(reset=True)
        off, counts, wcounts = eng.nw_msa_counts(0, nt, weights=True)
        assert np.array_equal(off, want_off) and np.array_equal(counts, want) and np.array_equal(wcounts, wwant), env
        if env.get("MC_MSA_BYTES") == 1000:  # 64 bytes per column: a target of more than 15 columns is a batch of its own
            alone = int((np.diff(want_off.astype(np.int64)) > 15).sum())
            assert alone > nt // 2 and eng.timers()["nw"][1] >= alone, env  # (a finish kernel per batch at least)
        assert np.array_equal(eng.nw_msa_counts(0, nt)[1], want), env
    clean_env(monkeypatch)
    # one target per call, ranges of 3
    for step in (1, 3):
        got, wgot = [], []
        for k in range(0, nt, step):
            off, c, w = eng.nw_msa_counts(k, min(step, nt - k), weights=True)
            assert np.array_equal(off, want_off[k:k + step + 1] - want_off[k])
            got.append(c)
            wgot.append(w)
        assert np.array_equal(np.concatenate(got), want) and np.array_equal(np.concatenate(wgot), wwant), step
    # rows and other alignment entries in between: they share the scratch, not the plan
    base_rows = eng.nw_msa_rows(0, nt + m)[0].tobytes()
    tab = eng.nw_pileup_strands(q.a, q.b, am, q.targets)[0]
    eng.nw_identity_strands(q.a[:9], q.b[:9], np.ones(9, np.uint8))
    eng.nw_align_profile(reset=True)
    assert tab[:, 6].any()
    off, counts, wcounts = eng.nw_msa_counts(0, nt, weights=True)
    assert np.array_equal(counts, want) and np.array_equal(wcounts, wwant)
    assert eng.nw_msa_rows(0, nt + m)[0].tobytes() == base_rows
    assert np.array_equal(eng.nw_msa_counts(0, nt)[1], want)
    assert eng.nw_align_profile()[2] == 0  # no choice bytes since the reset: nothing was aligned again
    # the counts kernels are "nw", the reverse complement "layout"; a measurement entry of their own
    eng.timers(reset=True)
    before = eng.nw_msa_profile(reset=True)
    assert eng.nw_msa_counts_profile(reset=True) > 0 and eng.nw_msa_counts_profile() == 0
    eng.nw_msa_counts(0, nt)
    t = eng.timers()
    assert t["layout"][1] >= 1 and t["nw"][1] >= 2 and all(t[f][1] == 0 for f in t if f not in ("layout", "nw"))
    assert eng.nw_msa_counts_profile() > 0 and len(before) == 4 and eng.nw_msa_profile() == (0.0, 0.0, 0.0, 0.0)


# ---------------------------------------------------------------- 3. the contract
def test_offsets_capacity_errors_and_state(eng, monkeypatch):
    q = A.msa()
    am = q.strands("mixed")
    nt = len(q.targets)
    want_off, want, wwant = F.tables("mixed")
    cols = int(want_off[-1])
    clean_env(monkeypatch)
    begin(eng, am)
    lib, ptr = eng.lib, M._p
    SENT = 0xDEADBEEF

    def call(first, count, off, counts, wcounts, cap, e=None):
        return lib.mc_nw_msa_counts((e or eng).ctx, C.c_uint32(first), C.c_uint32(count), ptr(off), ptr(counts), ptr(wcounts), C.c_uint64(cap))

    def fresh():
        return np.full(nt + 2, 77, np.uint64), np.full((cols + 4, 8), SENT, np.uint32), np.full((cols + 4, 8), SENT, np.uint32)

    untouched = lambda *arrs: all((a == SENT).all() for a in arrs)
    # both NULL: the offsets only, no device work
    off, c, w = fresh()
    eng.timers(reset=True)
    assert call(0, nt, off, None, None, 0) == 0 and np.array_equal(off[:nt + 1], want_off) and off[nt + 1] == 77
    assert all(v[1] == 0 for v in eng.timers().values())
    assert eng.nw_msa_counts(0, nt, counts=False)[0].tolist() == want_off.tolist()
    # wcounts alone
    off, c, w = fresh()
    assert call(0, nt, off, None, w, cols) == M.ERR_ARG and untouched(w)
    # one column short: col_off valid, nothing written
    off, c, w = fresh()
    assert call(0, nt, off, c, w, cols - 1) == M.ERR_ARG and np.array_equal(off[:nt + 1], want_off) and untouched(c, w)
    off, c, w = fresh()
    assert call(0, nt, off, c, None, cols - 1) == M.ERR_ARG and np.array_equal(off[:nt + 1], want_off) and untouched(c)
    # exactly enough
    assert call(0, nt, off, c, w, cols) == 0
    assert np.array_equal(c[:cols], want) and np.array_equal(w[:cols], wwant) and untouched(c[cols:], w[cols:])
    # a range past the plan's nt
    off, c, w = fresh()
    for first, count in ((nt, 1), (nt + 1, 0), (5, nt - 4), (0, nt + 1), (0xFFFFFFFF, 2)):
        assert call(first, count, off, c, w, cols) == M.ERR_ARG and (off == 77).all() and untouched(c, w), (first, count)
    # ntargets = 0; col_off is required
    assert call(nt, 0, off, c, w, cols) == 0 and off[0] == 0 and off[1] == 77 and untouched(c, w)
    assert call(3, 0, off, c, w, 0) == 0 and untouched(c, w)
    assert call(0, nt, None, c, w, cols) == M.ERR_ARG and untouched(c, w)
    # overwritten, not added to: a second call over the same tables
    off, c, w = fresh()
    assert call(2, 5, off, c, w, cols) == 0 and call(2, 5, off, c, w, cols) == 0
    lo, hi = int(want_off[2]), int(want_off[7])
    assert np.array_equal(c[:hi - lo], want[lo:hi]) and np.array_equal(w[:hi - lo], wwant[lo:hi]) and untouched(c[hi - lo:], w[hi - lo:])
    with pytest.raises(M.MCError) as e:
        eng.nw_msa_counts(nt, 1)
    assert e.value.code == M.ERR_ARG

    # a begin with m = 0: every block is its centre alone
    eng.nw_msa_begin([], [], None, q.targets)
    off0, c0, w0 = eng.nw_msa_counts(0, nt, weights=True)
    lens = [len(q.codes[j]) for j in q.targets]
    assert np.array_equal(np.diff(off0.astype(np.int64)), lens)
    assert not c0[:, :6].any() and not c0[:, 7].any() and not w0.any() and np.array_equal(c0[:, 6], np.concatenate([np.arange(n) for n in lens]))

    # no plan: after end, after a failed begin, before any begin, after a load of sequences
    def no_plan(e=None):
        o = np.zeros(2, np.uint64)
        return call(0, 0, o, None, None, 0, e) == M.ERR_STATE

    assert not no_plan()
    eng.nw_msa_end()
    assert no_plan()
    off, c, w = fresh()
    assert call(0, nt, off, c, w, cols) == M.ERR_STATE and (off == 77).all() and untouched(c, w)
    with pytest.raises(M.MCError) as e:
        eng.nw_msa_counts(0, 1)
    assert e.value.code == M.ERR_STATE
    begin(eng, am)
    assert np.array_equal(eng.nw_msa_counts(0, nt)[1], want)  # (end freed the scratch: it comes back)

    # no qualities loaded: the weights are a state error, the counts are not
    other = M.Engine(0)
    try:
        assert no_plan(other)  # no sequences
        small = P.pile()
        other.load_sequences(*small.load_args())
        assert no_plan(other)  # sequences, but no begin yet
        ks = np.arange(small.nbase, small.nbase + 12)
        tg = sorted(set(int(j) for j in small.b[ks]))
        bw = other.nw_msa_begin(small.a[ks], small.b[ks], None, tg)[2]
        n = int(bw.sum())
        off, c, w = np.full(len(tg) + 1, 77, np.uint64), np.full((n, 8), SENT, np.uint32), np.full((n, 8), SENT, np.uint32)
        assert call(0, len(tg), off, c, w, n, other) == M.ERR_STATE and untouched(c, w)
        assert call(0, len(tg), off, c, None, n, other) == 0 and (c[:, :6].sum(axis=1) == 12).all()
        other.load_qualities(Q.flat(Q.qualities()))
        assert call(0, len(tg), off, c, w, n, other) == 0 and w[:, :5].any()
        other.load_sequences(*small.load_args())
        assert no_plan(other)
    finally:
        other.close()


# ---------------------------------------------------------------- 4. end to end
import test_gpu_qpileup as GQ  # noqa: E402

family = GQ.family  # the planted centre and its 30 reads as FASTQ, every second one flipped
PROFILE_KEYS = ("profile_centres", "profile_columns")
DROP = PROFILE_KEYS + ("phases_ms", "device_us")


def profile_from_paf(paf, reads, centres_fa):
    """reads: name -> (letters, qualities or None).  -> (the --profile file's text, [centres,
    columns]) from a PAF's CIGARs, the reads and the centres alone (the PAF of a run without --top
    lists the assigned reads' pairs, in input order)."""
    cents = [(h[1:].decode(), G.codes_of(s.upper())) for h, s in G.read_fasta(centres_fa)]
    pairs = {name: [] for name, _ in cents}
    weighted = False
    for x in G.rows_of(paf):
        s, q = reads[x[0]]
        if x[4] == "-":
            s, q = s.translate(G._RC)[::-1], None if q is None else q[::-1]
        weighted |= q is not None
        pairs[x[5]].append((G.parse_cigar(x[14][5:]), G.codes_of(s), q))
    out, stats = [], [0, 0]
    for name, c in cents:
        if not pairs[name]:
            continue
        _, _, W, counts, wcounts = F.from_words(c, pairs[name])
        for k in range(W):
            x = counts[k]
            f = [name, str(k + 1), str(int(x[6]) + 1), str(int(x[7])), P.base_char(c[x[6]]) if x[7] == 0 else "-", str(len(pairs[name]))]
            f += [str(int(v)) for v in x[:6]] + ([str(int(v)) for v in wcounts[k][:6]] if weighted else [])
            out.append("\t".join(f) + "\n")
        stats = [stats[0] + 1, stats[1] + W]
    return "".join(out), stats


def tables_of_profile(path):
    """The --profile file alone -> {centre: (its bytes, counts[W, 8], wcounts[W, 8] or None)}."""
    out = {}
    for x in G.rows_of(path):
        out.setdefault(x[0], []).append(x)
    res = {}
    for name, rows in out.items():
        assert [int(x[1]) for x in rows] == list(range(1, len(rows) + 1))
        counts = np.array([[int(v) for v in x[6:12]] + [int(x[2]) - 1, int(x[3])] for x in rows], np.uint32)
        wcounts = np.array([[int(v) for v in x[12:18]] + [0, 0] for x in rows], np.uint32) if len(rows[0]) == 18 else None
        assert all((x[4] == "-") == (x[3] != "0") for x in rows) and len({x[5] for x in rows}) == 1
        cen = G.codes_of("".join(x[4] for x in rows if x[3] == "0").encode())
        res[name] = (cen, counts, wcounts)
    return res


def fasta_reads(path):
    return {h[1:].decode(): (s.upper(), None) for h, s in G.read_fasta(path)}


def test_cli_profile(e2e):
    path = lambda name, ext: str(e2e.tmp / (name + ext))
    others = ["--both-strands", "--paf", "@paf", "--consensus", "@cons", "--pileup", "@pile"]
    full = e2e("p_full", others + ["--msa", path("p_full", ".msa.fa"), "--profile", path("p_full", ".profile.tsv")])
    plain = e2e("p_plain", others + ["--msa", path("p_plain", ".msa.fa")])
    text, stats = profile_from_paf(full["paf"], fasta_reads(e2e.reads), e2e.cen)
    assert open(path("p_full", ".profile.tsv")).read() == text
    # every other output and the remaining stats are those of the run without --profile
    for k in ("tsv", "paf", "cons", "pile"):
        assert full[k].read_bytes() == plain[k].read_bytes(), k
    assert open(path("p_full", ".msa.fa"), "rb").read() == open(path("p_plain", ".msa.fa"), "rb").read()
    st, pst = full["st"], plain["st"]
    assert not any(k in pst for k in PROFILE_KEYS) and "profile" not in pst["phases_ms"]
    assert {k: v for k, v in st.items() if k not in DROP} == {k: v for k, v in pst.items() if k not in DROP}
    assert list(st)[:-2] == list(pst) and list(st)[-2:] == list(PROFILE_KEYS) and list(st)[-6:-2] == list(GM.MSA_KEYS)
    assert list(st["phases_ms"])[:-1] == list(pst["phases_ms"]) and list(st["phases_ms"])[-2:] == ["msa", "profile"]
    assert [st[k] for k in PROFILE_KEYS] == stats == [st["msa_centres"], st["msa_columns"]] and st["phases_ms"]["profile"] > 0
    assert any(x[3] != "0" for x in G.rows_of(path("p_full", ".profile.tsv")))  # (some block has an inserted column)
    # the --consensus file of the same run from the --profile file alone
    tabs = tables_of_profile(path("p_full", ".profile.tsv"))
    fa = []
    for h, s in G.read_fasta(e2e.cen):
        name = h[1:].decode()
        if name in tabs:
            cen, counts, _ = tabs[name]
            assert np.array_equal(cen, G.codes_of(s.upper()))
            seq, sub, dele, ins = F.consensus_from_profile(cen, counts)
            depth = int(counts[0][:6].sum())
        else:
            seq, sub, dele, ins, depth = s.upper().decode(), 0, 0, 0, 0
        fa.append(">%s depth=%d sub=%d del=%d ins=%d\n%s\n" % (name, depth, sub, dele, ins, seq))
    assert full["cons"].read_text() == "".join(fa)
    assert any(" ins=0" not in ln for ln in fa) or st["insertion_sites"] == 0
    # --profile alone: the same file, the TSV of --identity, and no msa keys
    alone = e2e("p_alone", ["--both-strands", "--profile", path("p_alone", ".profile.tsv")])
    ident = e2e("p_ident", ["--both-strands", "--identity"])
    assert open(path("p_alone", ".profile.tsv")).read() == text and alone["tsv"].read_bytes() == ident["tsv"].read_bytes()
    ast = alone["st"]
    assert list(ast)[-2:] == list(PROFILE_KEYS) and not any(k in ast for k in GM.MSA_KEYS) and list(ast["phases_ms"])[-1] == "profile"
    assert {k: v for k, v in ast.items() if k not in DROP} == {k: v for k, v in ident["st"].items() if k not in DROP}


def test_cli_profile_with_quality(family):
    pf = lambda name: str(family.tmp / (name + ".profile.tsv"))
    full = family("pq", ["--both-strands", "--paf", "@paf", "--pileup", "@pile", "--quality", "--profile", pf("pq")], family.fq)
    reads = {name: (s.upper(), np.frombuffer(q, np.uint8) - 33) for name, s, q in GQ.read_fastq(family.fq)}
    text, stats = profile_from_paf(full["paf"], reads, family.cen)
    assert open(pf("pq")).read() == text and stats[0] == 1 and full["st"]["profile_columns"] == stats[1]
    rows, pile = G.rows_of(pf("pq")), G.rows_of(full["pile"])
    assert all(len(x) == 18 for x in rows) and any(int(v) for x in rows for v in x[12:17] if x[3] != "0")
    # line by line: a centre column's six counts and six weights are the pile-up row's
    base = [x for x in rows if x[3] == "0"]
    assert len(base) == len(pile) - 1 and all(x[2] == y[1] and x[4] == y[2] and x[5] == y[3] for x, y in zip(base, pile))
    assert all(x[6:12] == y[4:10] and x[12:18] == y[12:18] for x, y in zip(base, pile))
    # ... and over a site's slots the counts add up to its inserted bases, the first slot's gaps to the reads without one
    for y in pile:
        slots = [x for x in rows if x[2] == y[1] and x[3] != "0"]
        assert sum(int(v) for x in slots for v in x[6:11]) == int(y[11]) and (not slots or int(slots[0][11]) == int(y[3]) - int(y[10]))
    # --quality beside --profile alone is accepted and writes the same file; without --quality no weights
    alone = family("pq_alone", ["--both-strands", "--quality", "--profile", pf("pq_alone")], family.fq)
    assert open(pf("pq_alone")).read() == text and "quality" not in alone["st"]
    noq = family("pq_noq", ["--both-strands", "--profile", pf("pq_noq")], family.fq)
    assert [x[:12] for x in rows] == G.rows_of(pf("pq_noq"))


def test_assign_files_profile(e2e, tmp_path):
    """The same job in process (mcl_assign_profile), on a context of its own sequences."""
    pfile = str(e2e.tmp / "p_alone.profile.tsv")
    alone = e2e("p_alone", ["--both-strands", "--profile", pfile])
    e = M.Engine(0)
    try:
        model = str(e2e.cen).replace(".centres.fa", ".model")
        st = M.assign_files(e, model, str(e2e.cen), str(e2e.reads), str(tmp_path / "l.tsv"), threads=2, both_strands=True,
                            profile=str(tmp_path / "l.profile.tsv"))
        st2 = M.assign_files(e, model, str(e2e.cen), str(e2e.reads), str(tmp_path / "l2.tsv"), threads=2, both_strands=True,
                             msa=str(tmp_path / "l2.msa.fa"), profile=str(tmp_path / "l2.profile.tsv"))
    finally:
        e.close()
    assert (tmp_path / "l.profile.tsv").read_bytes() == open(pfile, "rb").read() == (tmp_path / "l2.profile.tsv").read_bytes()
    assert (tmp_path / "l.tsv").read_bytes() == alone["tsv"].read_bytes()
    assert [st[k] for k in PROFILE_KEYS] == [alone["st"][k] for k in PROFILE_KEYS] == [st2[k] for k in PROFILE_KEYS]
    assert list(st2)[-6:] == list(GM.MSA_KEYS + PROFILE_KEYS)
