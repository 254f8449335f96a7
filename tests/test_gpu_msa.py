"""mc_nw_msa_begin / mc_nw_msa_rows / meshclust-assign --msa on the GPU.  Every comparison is ==.

The expectations: the Python restatement of tests/msa_cases.py over the words of
tests/nw_trace_cases.py (tied to the CPU oracle by test_nw_trace_host.py, test_pileup_host.py and
test_msa_host.py), mc_nw_align_strands for score / columns / '=' and mc_nw_pileup_strands for the
rows that have a slot.  One set of points, loaded once."""
import ctypes as C
import os

import numpy as np
import pytest

import meshclust_amd as M
import msa_cases as A
import nw_trace_cases as T
import pileup_cases as P
import test_gpu_pileup as G

pytestmark = pytest.mark.gpu

ENV_VARS = G.ENV_VARS + ("MC_MSA_BYTES",)
e2e = G.e2e  # the a1k fixture: 260 reads, every second one flipped


@pytest.fixture(scope="module")
def eng(built):
    e = M.Engine(0)
    e.load_sequences(*A.msa().load_args())
    yield e
    e.close()


def clean_env(monkeypatch, **kw):
    for var in ENV_VARS:
        monkeypatch.delenv(var, raising=False)
    for k, v in kw.items():
        monkeypatch.setenv(k, str(v))


def split(buf, off):
    return [buf[int(off[k]):int(off[k + 1])].tobytes() for k in range(len(off) - 1)]


def whole(eng, am):
    """begin over the whole list and every row in one call -> (begin's results, the rows)."""
    q = A.msa()
    res = eng.nw_msa_begin(q.a, q.b, am, q.targets)
    buf, off = eng.nw_msa_rows(0, len(q.targets) + len(q.a))
    return res, split(buf, off)


# ---------------------------------------------------------------- 1. the rows and the integers
@pytest.mark.parametrize("name", ["plus", "minus", "mixed"])
def test_rows_equal_the_restatement(eng, name, monkeypatch):
    clean_env(monkeypatch)
    q = A.msa()
    flags = q.strands(name)
    am = None if name == "plus" else flags
    want_rows, want_w, want_bw = A.all_rows(A.named_blocks(name), len(q.a))
    (off, width, bw, score, ln, ids), rows = whole(eng, am)
    assert off.dtype == np.uint64 and np.array_equal(off, q.row_off)
    assert width.dtype == np.uint32 and np.array_equal(width, want_w)
    assert bw.dtype == np.uint64 and np.array_equal(bw, want_bw)
    assert len(rows) == len(want_rows)
    bad = [k for k in range(len(rows)) if rows[k] != want_rows[k]]
    assert not bad, (name, bad[:8], rows[bad[0]], want_rows[bad[0]])
    _, _, a_score, a_ln, a_ids = eng.nw_align_strands(q.a, q.b, am, cigar=False)
    for x, y in ((score, a_score), (ln, a_ln), (ids, a_ids)):
        assert x.dtype == y.dtype and np.array_equal(x, y)
    tab = eng.nw_pileup_strands(q.a, q.b, am, q.targets)[0]
    assert np.array_equal(width > 0, tab[:, 6] > 0) and (width <= tab[:, 7]).all()
    t = q.tindex[q.slots]
    if name == "plus":
        assert int(bw[t]) == 145 and int(bw[q.tindex[q.long_target]]) == 170
    t = q.tindex[P.pile().lonely]  # a target with no pair: its centre alone
    assert int(bw[t]) == len(q.codes[P.pile().lonely]) and not width[int(off[t]):int(off[t + 1])].any()


# ---------------------------------------------------------------- 2. batching and ranges change nothing
def test_batches_and_ranges_give_the_same_bytes(eng, monkeypatch):
    q = A.msa()
    am = q.strands("mixed")
    n = len(q.targets) + len(q.a)
    clean_env(monkeypatch)
    eng.nw_align_profile(reset=True)
    base_res, base = whole(eng, am)
    after_begin = eng.nw_align_profile()[2]
    assert base == A.all_rows(A.named_blocks("mixed"), len(q.a))[0]
    big = T.choice_bytes(1100, 1100)
    assert big == max(T.choice_bytes(len(q.codes[i]), len(q.codes[j])) for i, j in zip(q.a, q.b))
    lens = [len(x) for x in q.codes]
    nbytes = T.ident_bytes(lens, q.a[am != 0])
    assert nbytes == T.ident_bytes([len(x) for x in P.pile().codes], P.pile().a[P.mixed_strands() != 0])  # pileup's value
    widest, total = max(len(r) for r in base), sum(len(r) for r in base)
    assert widest == 2561 > 1000
    for env in ({"MC_ALIGN_BATCH": 7}, {"MC_ALIGN_BATCH": 1}, {"MC_ALIGN_SCRATCH": 3 * big + 64}, {"MC_IDENT_BYTES": nbytes},
                {"MC_MSA_BYTES": 4096}, {"MC_MSA_BYTES": 1000}):
        clean_env(monkeypatch, **env)
        res = eng.nw_msa_begin(q.a, q.b, am, q.targets)
        assert all(x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(res, base_res)), env
        eng.timers(reset=True)
        buf, off = eng.nw_msa_rows(0, n)
        assert split(buf, off) == base, env
        if "MC_MSA_BYTES" in env:  # many render batches: a launch each
            assert eng.timers()["nw"][1] >= total // env["MC_MSA_BYTES"], env
    clean_env(monkeypatch)
    # the choices were written once: begin's are those of one alignment pass, rows adds none
    assert eng.nw_align_profile(reset=True)[2] > 0
    eng.nw_msa_begin(q.a, q.b, am, q.targets)
    assert eng.nw_align_profile()[2] == after_begin
    eng.nw_msa_rows(0, n)
    assert eng.nw_align_profile(reset=True)[2] == after_begin
    eng.nw_align_strands(q.a, q.b, am, cigar=False)
    assert eng.nw_align_profile(reset=True)[2] == after_begin
    # other alignment entries between begin and rows share the scratch, not the plan
    tab = eng.nw_pileup_strands(q.a, q.b, am, q.targets)[0]
    eng.nw_identity_strands(q.a[:9], q.b[:9], np.ones(9, np.uint8))
    assert tab[:, 6].any()
    buf, off = eng.nw_msa_rows(0, n)
    assert split(buf, off) == base
    # one row per call, ranges of 7
    assert [eng.nw_msa_rows(k, 1)[0].tobytes() for k in range(n)] == base
    got = []
    for k in range(0, n, 7):
        buf, off = eng.nw_msa_rows(k, min(7, n - k))
        got += split(buf, off)
    assert got == base
    # a range that starts among the centre rows and ends among the pair rows, under a small cap
    clean_env(monkeypatch, MC_MSA_BYTES=4096, MC_IDENT_BYTES=nbytes)
    nt = len(q.targets)
    buf, off = eng.nw_msa_rows(nt - 3, 40)
    assert split(buf, off) == base[nt - 3:nt + 37]


# ---------------------------------------------------------------- 3. the contract
def test_offsets_capacity_errors_and_state(eng, monkeypatch):
    q = A.msa()
    am = q.strands("mixed")
    clean_env(monkeypatch)
    (off, width, bw, score, ln, ids), base = whole(eng, am)
    m, nt = len(q.a), len(q.targets)
    n, total = nt + m, sum(len(r) for r in base)
    none, roff = eng.nw_msa_rows(0, n, rows=False)  # out = NULL
    assert none is None and roff.dtype == np.uint64 and np.array_equal(np.diff(roff.astype(np.int64)), [len(r) for r in base])
    lib, ptr = eng.lib, M._p
    SENT = 0xEE

    def rows(first, count, buf, cap, o):
        return lib.mc_nw_msa_rows(eng.ctx, C.c_uint64(first), C.c_uint64(count), ptr(buf), C.c_uint64(cap), ptr(o))

    buf = np.full(total + 16, SENT, np.uint8)
    o = np.full(n + 1, 77, np.uint64)
    assert rows(0, n, buf, total - 1, o) == M.ERR_ARG  # one byte short
    assert np.array_equal(o, roff) and (buf == SENT).all()
    assert rows(0, n, buf, total, o) == 0  # exactly enough
    assert buf[:total].tobytes() == b"".join(base) and (buf[total:] == SENT).all()
    buf[:] = SENT
    o[:] = 77
    assert rows(n, 1, buf, total, o) == M.ERR_ARG and rows(n + 1, 0, buf, total, o) == M.ERR_ARG  # past nt + m
    assert rows(5, n - 4, buf, total, o) == M.ERR_ARG and (buf == SENT).all() and (o == 77).all()
    assert rows(n, 0, buf, total, o) == 0 and o[0] == 0 and (buf == SENT).all()  # count = 0
    assert rows(0, n, buf, total, None) == M.ERR_ARG  # off is required

    # begin's argument errors: nothing written, and the plan before them is gone
    a, b, tg = np.ascontiguousarray(q.a), np.ascontiguousarray(q.b), np.ascontiguousarray(q.targets)
    nrow = int(off[-1])

    def begin(targets=tg, bb=b, aa=a):
        ro = np.full(len(targets) + 2, 77, np.uint64)
        w = np.full(nrow + 4000, 0xDEADBEEF, np.uint32)
        wb = np.full(len(targets) + 2, 77, np.uint64)
        s = np.full(m, -7, np.int32)
        rc = lib.mc_nw_msa_begin(eng.ctx, ptr(aa), ptr(bb), ptr(am), C.c_uint64(m), ptr(targets), C.c_uint32(len(targets)), ptr(ro),
                                 ptr(w), ptr(wb), ptr(s), ptr(s), ptr(s))
        return rc, (ro == 77).all() and (w == 0xDEADBEEF).all() and (wb == 77).all() and (s == -7).all()

    def no_plan():
        o2 = np.zeros(2, np.uint64)
        return lib.mc_nw_msa_rows(eng.ctx, C.c_uint64(0), C.c_uint64(1), None, C.c_uint64(0), ptr(o2)) == M.ERR_STATE

    far = tg.copy()
    far[3] = len(q.codes)
    bad_b = b.copy()
    bad_b[5] = len(q.codes)
    bad_a = a.copy()
    bad_a[0] = len(q.codes)
    assert q.b[-1] in tg[-2:]
    for kw in (dict(targets=np.concatenate([tg, tg[:1]])), dict(targets=np.ascontiguousarray(tg[:-2])), dict(targets=far),
               dict(bb=bad_b), dict(aa=bad_a)):
        assert begin() == (0, False) and not no_plan()
        assert begin(**kw) == (M.ERR_ARG, True), list(kw)
        assert no_plan(), list(kw)
    assert begin() == (0, False)
    clean_env(monkeypatch, MC_ALIGN_SCRATCH=T.choice_bytes(1100, 1100) - 1)  # a cap below one pair's need
    assert begin() == (M.ERR_UNSUPPORTED, True) and no_plan()
    clean_env(monkeypatch)
    with pytest.raises(M.MCError) as e:
        eng.nw_msa_rows(0, 1)
    assert e.value.code == M.ERR_STATE

    # a second begin replaces the first; end drops the plan
    half = np.arange(0, m, 2)
    eng.nw_msa_begin(q.a, q.b, am, q.targets)
    res = eng.nw_msa_begin(q.a[half], q.b[half], am[half], q.targets)
    bl = A.blocks(am, pairs=half)
    assert np.array_equal(res[2], [W for _, W, _, _ in bl]) and np.array_equal(res[1], np.concatenate([w for w, _, _, _ in bl]))
    want = [rows_[0] for _, _, rows_, _ in bl] + [None] * len(half)
    place = {int(k): i for i, k in enumerate(half)}
    for _, _, rows_, ks in bl:
        for i, k in enumerate(ks):
            want[nt + place[k]] = rows_[1 + i]
    buf2, off2 = eng.nw_msa_rows(0, nt + len(half))
    assert split(buf2, off2) == want
    with pytest.raises(M.MCError) as e:
        eng.nw_msa_rows(nt + len(half), 1)
    assert e.value.code == M.ERR_ARG
    eng.nw_msa_end()
    assert no_plan()
    eng.nw_msa_end()  # (nothing to drop: MC_OK)

    # m = 0: every block is its centre alone
    res = eng.nw_msa_begin([], [], None, q.targets)
    assert np.array_equal(res[0], q.row_off) and not res[1].any() and np.array_equal(res[2], [len(q.codes[j]) for j in q.targets])
    buf2, off2 = eng.nw_msa_rows(0, nt)
    assert split(buf2, off2) == [bytes(A.char(x) for x in q.codes[j]) for j in q.targets]

    # timers: the new kernels are "nw", the reverse complement "layout"
    eng.timers(reset=True)
    eng.nw_msa_profile(reset=True)
    eng.nw_msa_begin(q.a[:5], q.b[:5], [1, 0, 0, 0, 0], q.targets)
    t = eng.timers()
    assert t["layout"][1] == 1 and t["nw"][1] >= 5  # forward, traceback, pack, width, column
    eng.nw_msa_rows(0, nt + 5)
    t = eng.timers()
    assert t["layout"][1] == 2 and t["nw"][1] >= 7  # + a render per segment
    assert all(t[f][1] == 0 for f in t if f not in ("layout", "nw"))
    assert all(x > 0 for x in eng.nw_msa_profile()) and len(eng.nw_msa_profile()) == 4

    # no sequences / a load of sequences: no plan
    fresh = M.Engine(0)
    try:
        with pytest.raises(M.MCError) as e:
            fresh.nw_msa_rows(0, 1)
        assert e.value.code == M.ERR_STATE
        o2 = np.zeros(3, np.uint64)
        assert fresh.lib.mc_nw_msa_begin(fresh.ctx, ptr(a[:1]), ptr(b[:1]), None, C.c_uint64(1), ptr(b[:1]), C.c_uint32(1), ptr(o2), None,
                                         ptr(o2), None, None, None) == M.ERR_STATE
        small = P.pile().base
        fresh.load_sequences(*P.pile().load_args())
        with pytest.raises(M.MCError) as e:  # sequences, but no begin yet
            fresh.nw_msa_rows(0, 1)
        assert e.value.code == M.ERR_STATE
        fresh.nw_msa_begin(small.a[:3], small.b[:3], None, sorted(set(int(j) for j in small.b[:3])))
        assert fresh.nw_msa_rows(0, 2)[0] is not None
        fresh.load_sequences(*P.pile().load_args())
        with pytest.raises(M.MCError) as e:
            fresh.nw_msa_rows(0, 1)
        assert e.value.code == M.ERR_STATE
    finally:
        fresh.close()


# ---------------------------------------------------------------- 3b. a second plan owes nothing to the first
def two_lists():
    """-> ((a, b, minus, targets), (a, b, None, targets)): about 40 pairs on 6 targets with minus flags,
    then about half of them in another order on 5 of the targets in another order, no flags.  In both,
    one target has a single pair and one has none; four reads are aligned to two centres each (the
    crossover's candidates).  Reads of 50 to 300 bases, all from msa_cases.msa()."""
    q = A.msa()
    p = q.pile
    lens = [len(c) for c in q.codes]
    of = {int(j): [k for k in range(len(q.a)) if q.b[k] == j] for j in q.targets}
    small = [j for j in of if 3 <= len(of[j]) <= 5 and all(50 <= lens[q.a[k]] <= 300 for k in of[j])][:2]
    ks = of[small[0]] + of[small[1]]
    n0 = len(ks)
    ks += of[p.contended][:15] + of[q.slots][:16] + of[q.long_target]
    a = [int(q.a[k]) for k in ks]
    b = [int(q.b[k]) for k in ks]
    c0, s0, m0 = n0, n0 + 15, len(ks)  # the first contended pair, the first slots pair, the first of the four added
    a += [a[0], a[c0], a[c0 + 1], a[s0]]
    b += [q.slots, q.slots, small[0], p.contended]
    assert len(of[q.long_target]) == 1 and not of[p.lonely] and all(50 <= lens[i] <= 300 for i in a) and 40 <= len(a) <= 48
    t1 = [small[0], small[1], p.contended, q.slots, q.long_target, p.lonely]
    minus = (np.arange(len(a)) % 3 != 2).astype(np.uint8)
    pick = [m0 + 3, s0, m0 + 1, c0, m0 - 1] + list(range(s0 + 7, s0, -2)) + list(range(c0 + 12, c0 + 1, -2)) + [0, m0, c0 + 1, m0 + 2]
    assert len(set(pick)) == len(pick) and not any(b[i] == small[1] for i in pick)
    t2 = [q.slots, p.lonely, p.contended, q.long_target, small[0]]
    u32 = lambda v: np.array(v, np.uint32)
    return (u32(a), u32(b), minus, u32(t1)), (u32([a[i] for i in pick]), u32([b[i] for i in pick]), None, u32(t2))


def read_everything(e, a, b, am, targets):
    """begin, then every reader of the plan over all of it -> the arrays they return, in one list."""
    nt, m = len(targets), len(a)
    out = list(e.nw_msa_begin(a, b, am, targets))
    out += e.nw_msa_rows(0, nt + m)
    col_off, tab = e.nw_msa_counts(0, nt)
    out += [col_off, tab]
    cols = [np.arange(0, int(w), 3) for w in np.diff(col_off.astype(np.int64))]  # every third column of every block
    out += e.nw_msa_sites(np.concatenate([[0], np.cumsum([len(x) for x in cols])]), np.concatenate(cols), 0, m)
    same = [(i, j) for i in range(m) for j in range(i + 1, m) if a[i] == a[j]]
    assert len(same) == 4
    out.append(e.nw_msa_crossover([i for i, _ in same], [j for _, j in same]))
    return out


@pytest.fixture(scope="module")
def second_alone(built):
    """What a fresh engine gives for the second list."""
    e = M.Engine(0)
    try:
        e.load_sequences(*A.msa().load_args())
        return read_everything(e, *two_lists()[1])
    finally:
        e.close()


@pytest.mark.parametrize("end_between", [True, False])
def test_second_plan_equals_a_fresh_engine(eng, second_alone, end_between, monkeypatch):
    """A plan with minus flags, read by rows, counts, sites and crossover; then a shorter list without
    flags on the same engine, after mc_nw_msa_end or straight away: every reader returns what a fresh
    engine returns, so nothing of the first plan (its flags, its pairs' targets, its per-target lists)
    is left."""
    clean_env(monkeypatch)
    first, second = two_lists()
    got1 = read_everything(eng, *first)
    assert len(got1[7]) == len(first[3]) + len(first[0]) + 1  # rows' offsets: every row of the first plan was read
    if end_between:
        eng.nw_msa_end()
    got = read_everything(eng, *second)
    assert len(got) == len(second_alone) == 13
    for k, (x, y) in enumerate(zip(got, second_alone)):
        assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y), k
    assert not np.array_equal(got1[6][:64], got[6][:64])  # (the two plans' rows do differ)


# ---------------------------------------------------------------- 4. end to end
def msa_from_paf(paf, reads_fa, centres_fa):
    """-> the --msa file's text from a PAF's CIGARs and the two FASTA files alone (the PAF of a run
    without --top lists the assigned reads' pairs, in input order)."""
    reads = {h[1:].decode(): s.upper() for h, s in G.read_fasta(reads_fa)}
    cents = [(h[1:].decode(), G.codes_of(s.upper())) for h, s in G.read_fasta(centres_fa)]
    pairs = {name: [] for name, _ in cents}
    for x in G.rows_of(paf):
        s = reads[x[0]]
        if x[4] == "-":
            s = s.translate(G._RC)[::-1]
        pairs[x[5]].append((x[0], x[4], G.parse_cigar(x[14][5:]), G.codes_of(s)))
    out, stats = [], [0, 0, 0, 0]
    for name, c in cents:
        if not pairs[name]:
            continue
        _, W, rows = A.block(c, [(words, s) for _, _, words, s in pairs[name]])
        out.append(">%s depth=%d width=%d\n%s\n" % (name, len(pairs[name]), W, rows[0].decode()))
        for (read, strand, _, _), row in zip(pairs[name], rows[1:]):
            out.append(">%s strand=%s\n%s\n" % (read, strand, row.decode()))
        stats = [stats[0] + len(pairs[name]), stats[1] + 1, stats[2] + W, stats[3] + len(rows) * W]
    return "".join(out), stats


MSA_KEYS = ("msa_pairs", "msa_centres", "msa_columns", "msa_bytes")


def strip_stats(st):
    out = {k: v for k, v in st.items() if k not in MSA_KEYS + ("phases_ms", "device_us")}
    return out


def test_cli_msa(e2e):
    mfile = lambda name: str(e2e.tmp / (name + ".msa.fa"))
    full = e2e("m_full", ["--both-strands", "--paf", "@paf", "--msa", mfile("m_full")])
    plain = e2e("m_plain", ["--both-strands", "--paf", "@paf"])
    text, stats = msa_from_paf(full["paf"], e2e.reads, e2e.cen)
    assert open(mfile("m_full")).read() == text
    assert full["tsv"].read_bytes() == plain["tsv"].read_bytes() and full["paf"].read_bytes() == plain["paf"].read_bytes()
    assert not any(k in plain["st"] for k in MSA_KEYS) and "msa" not in plain["st"]["phases_ms"]
    assert strip_stats(full["st"]) == strip_stats(plain["st"])
    st = full["st"]
    assert [st[k] for k in MSA_KEYS] == stats and st["msa_pairs"] == st["assigned"] > 200 and st["phases_ms"]["msa"] > 0
    assert list(st)[-4:] == list(MSA_KEYS) and list(st["phases_ms"])[-1] == "msa"
    assert {ln.rsplit(" strand=", 1)[1] for ln in text.splitlines() if " strand=" in ln} == {"+", "-"}
    assert any("-" in ln for ln in text.splitlines() if not ln.startswith(">"))  # (some block has a slot or a deletion)
    # --msa alone: the same file, and the identity column --paf gives
    alone = e2e("m_alone", ["--both-strands", "--msa", mfile("m_alone")])
    assert open(mfile("m_alone")).read() == text and alone["tsv"].read_bytes() == full["tsv"].read_bytes()
    # beside --consensus --pileup: their files are those of the run without --msa
    both = e2e("m_both", ["--both-strands", "--consensus", "@cons", "--pileup", "@pile", "--msa", mfile("m_both")])
    cons = e2e("m_cons", ["--both-strands", "--consensus", "@cons", "--pileup", "@pile"])
    assert both["cons"].read_bytes() == cons["cons"].read_bytes() and both["pile"].read_bytes() == cons["pile"].read_bytes()
    assert both["tsv"].read_bytes() == cons["tsv"].read_bytes() and open(mfile("m_both")).read() == text
    assert strip_stats(both["st"]) == strip_stats(cons["st"]) and both["st"]["consensus_passes"] == 1


def test_cli_planted_family(e2e):
    """test_gpu_pileup.py's planted family: one block of the centre and its 30 reads."""
    p = P.pile()
    cens = G.read_fasta(e2e.cen)
    letters = lambda c: "".join(P.LETTERS[x] for x in c).encode()
    cens[0][1] = letters(p.codes[p.planted])
    cfile, rfile = e2e.tmp / "planted.centres.fa", e2e.tmp / "planted.reads.fa"
    cfile.write_bytes(b"".join(h + b"\n" + s + b"\n" for h, s in cens))
    ks = [k for k in range(len(p.a)) if p.b[k] == p.planted]
    rfile.write_bytes(b"".join(b">p%d\n" % i + letters(p.codes[p.a[k]]) + b"\n" for i, k in enumerate(ks)))
    mfile = str(e2e.tmp / "planted.msa.fa")
    out = e2e("m_planted", ["--msa", mfile], reads_fa=rfile, centres=cfile)
    assert out["st"]["assigned"] == 30 and out["st"]["msa_centres"] == 1 and out["st"]["msa_pairs"] == 30
    lines = open(mfile).read().splitlines()
    exp = P.expected()[0]
    _, W, rows = A.block(p.codes[p.planted], [(exp[k][0], p.read(k, False)) for k in ks])
    assert lines[0] == cens[0][0].decode() + " depth=30 width=%d" % W and len(lines) == 2 * 31
    assert lines[1::2] == [r.decode() for r in rows]
    assert lines[2::2] == [">p%d strand=+" % i for i in range(30)]
    assert out["st"]["msa_columns"] == W and out["st"]["msa_bytes"] == 31 * W


def test_assign_files_msa(e2e, tmp_path):
    """The same job in process (mcl_assign_msa), on a context of its own sequences."""
    mfile = str(e2e.tmp / "m_full.msa.fa")
    full = e2e("m_full", ["--both-strands", "--paf", "@paf", "--msa", mfile])
    e = M.Engine(0)
    try:
        model = str(e2e.cen).replace(".centres.fa", ".model")
        st = M.assign_files(e, model, str(e2e.cen), str(e2e.reads), str(tmp_path / "l.tsv"), threads=2, both_strands=True,
                            msa=str(tmp_path / "l.msa.fa"))
    finally:
        e.close()
    assert (tmp_path / "l.msa.fa").read_bytes() == open(mfile, "rb").read()
    assert (tmp_path / "l.tsv").read_bytes() == full["tsv"].read_bytes()
    assert [st[k] for k in MSA_KEYS] == [full["st"][k] for k in MSA_KEYS]
