"""mc_nw_msa_sites / meshclust-assign --variants --alleles --haplotypes on the GPU.  Every comparison is ==.

The expectations: the Python restatement of tests/sites_cases.py over msa_cases.msa()'s points (tied
to the CPU oracle by test_nw_trace_host.py, test_msa_host.py, test_profile_host.py and
test_sites_host.py), and the rows and counts mc_nw_msa_rows / mc_nw_msa_counts return from the same
plan.  One set of points, loaded once, with one set of qualities."""
import ctypes as C

import numpy as np
import pytest

import meshclust_amd as M
import msa_cases as A
import nw_trace_cases as T
import pileup_cases as P
import profile_cases as F
import qpileup_cases as Q
import sites_cases as S
import test_gpu_msa as GM
import test_gpu_pileup as G
import test_gpu_qpileup as GQ

pytestmark = pytest.mark.gpu

e2e = G.e2e  # the a1k fixture: 260 reads, every second one flipped
family = GQ.family  # the planted centre and its 30 reads as FASTQ, every second one flipped
clean_env = GM.clean_env
NAMES = ["plus", "minus", "mixed"]


@pytest.fixture(scope="module")
def eng(built):
    e = M.Engine(0)
    e.load_sequences(*A.msa().load_args())
    e.load_qualities(Q.flat(F.qualities()))
    yield e
    e.close()


def begin(eng, name):
    q = A.msa()
    return eng.nw_msa_begin(q.a, q.b, None if name == "plus" else q.strands(name), q.targets)


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    bad = np.nonzero(got != want)[0]
    assert not len(bad), (what, len(bad), bad[:8], got[bad[:8]], want[bad[:8]])
    return True


# ---------------------------------------------------------------- 1. the alleles and the weights
@pytest.mark.parametrize("name", NAMES)
def test_sites_equal_the_restatement(eng, name, monkeypatch):
    clean_env(monkeypatch)
    m = len(A.msa().a)
    begin(eng, name)
    for which in S.LISTS:
        so, st, want_off, want_al, want_ql = S.expected(which, name)
        off, al, ql = eng.nw_msa_sites(so, st, 0, m, quals=True)
        same(off, want_off, (name, which, "off"))
        same(al, want_al, (name, which, "alleles"))
        same(ql, want_ql, (name, which, "quals"))
        off2, al2 = eng.nw_msa_sites(so, st, 0, m)  # without the weights: the same bytes from the other kernel
        same(off2, want_off, (name, which)) and same(al2, want_al, (name, which))


# ---------------------------------------------------------------- 2. every column: the render again
@pytest.mark.parametrize("name", NAMES)
def test_all_columns_are_the_rendered_rows(eng, name, monkeypatch):
    clean_env(monkeypatch)
    q = A.msa()
    nt, m = len(q.targets), len(q.a)
    begin(eng, name)
    so, st = S.flat(S.site_lists("all", name))
    off, al = eng.nw_msa_sites(so, st, 0, m)
    buf, roff = eng.nw_msa_rows(nt, m)
    same(off, roff, name)
    same(al, buf, name)
    assert (al == A.GAP).any() and len(al) == int(roff[-1]) > 50000


# ---------------------------------------------------------------- 3. the weights and alleles per column
@pytest.mark.parametrize("name", NAMES)
def test_sums_per_column_are_the_profile(eng, name, monkeypatch):
    clean_env(monkeypatch)
    q = A.msa()
    nt, m = len(q.targets), len(q.a)
    begin(eng, name)
    col_off, counts, wcounts = eng.nw_msa_counts(0, nt, weights=True)
    checked = rendering = 0
    for which in ("all", "default", "edges"):
        lists = S.site_lists(which, name)
        so, st = S.flat(lists)
        off, al, ql = eng.nw_msa_sites(so, st, 0, m, quals=True)
        got = np.zeros((len(st), 6), np.uint32)
        wgot = np.zeros((len(st), 6), np.uint32)
        for k in range(m):
            t = q.tindex[int(q.b[k])]
            sl = slice(int(off[k]), int(off[k + 1]))
            at = np.arange(int(so[t]), int(so[t + 1]))
            cls = F._CLASS[al[sl]]
            got[at, cls] += 1
            wgot[at, cls] += ql[sl]
        for t, j in enumerate(q.targets):
            sl = slice(int(so[t]), int(so[t + 1]))
            cols = lists[t].astype(np.int64) + int(col_off[t])
            ks = [k for k in range(m) if q.b[k] == j]
            if F.renders_its_classes([q.codes[q.a[k]] for k in ks]):
                assert np.array_equal(wgot[sl], wcounts[cols, :6]) and np.array_equal(got[sl], counts[cols, :6]), (name, which, t)
                checked += len(cols)
                rendering += which == "all"
            else:  # (a raw letter byte: class 4 in the profile, that letter in the row)
                assert np.array_equal(wgot[sl].sum(axis=1), wcounts[cols, :6].sum(axis=1)), (name, which, t)
    assert rendering >= nt - 2 and checked > int(col_off[-1]) // 2


# ---------------------------------------------------------------- 4. batching, ranges and other entries change nothing
def test_batches_and_ranges_give_the_same_bytes(eng, monkeypatch):
    q = A.msa()
    am = q.strands("mixed")
    nt, m = len(q.targets), len(q.a)
    lens = [len(x) for x in q.codes]
    nbytes = T.ident_bytes(lens, q.a[am != 0])
    clean_env(monkeypatch)
    begin(eng, "mixed")
    eng.nw_align_profile(reset=True)
    want = {which: S.expected(which, "mixed") for which in ("all", "default", "edges")}
    for env in ({"MC_MSA_BYTES": 4096}, {"MC_MSA_BYTES": 64}, {"MC_IDENT_BYTES": nbytes}):
        for which, (so, st, woff, wal, wql) in want.items():
            clean_env(monkeypatch, **env)
            eng.timers(reset=True)
            off, al, ql = eng.nw_msa_sites(so, st, 0, m, quals=True)
            same(off, woff, env) and same(al, wal, env) and same(ql, wql, env)
            if which == "all" and "MC_MSA_BYTES" in env:  # a pair of more than the cap (two bytes per site with the weights) is a batch of its own
                alone = int((2 * np.diff(woff.astype(np.int64)) > env["MC_MSA_BYTES"]).sum())
                assert eng.timers()["nw"][1] >= alone and (alone > m // 2 or env["MC_MSA_BYTES"] > 64), env
            same(eng.nw_msa_sites(so, st, 0, m)[1], wal, env)
    clean_env(monkeypatch)
    # one pair per call, ranges of 7
    for which, step in (("default", 1), ("all", 7), ("edges", 7)):
        so, st, woff, wal, wql = want[which]
        got, qgot = [], []
        for k in range(0, m, step):
            off, al, ql = eng.nw_msa_sites(so, st, k, min(step, m - k), quals=True)
            same(off, woff[k:k + step + 1] - woff[k], (which, k))
            got.append(al)
            qgot.append(ql)
        same(np.concatenate(got), wal, which) and same(np.concatenate(qgot), wql, which)
    # rows, counts and other alignment entries in between: they share the scratch, not the plan
    so, st, woff, wal, wql = want["default"]
    base_rows = eng.nw_msa_rows(0, nt + m)[0].tobytes()
    base_counts = eng.nw_msa_counts(0, nt, weights=True)
    same(eng.nw_msa_sites(so, st, 0, m)[1], wal, "after rows and counts")
    tab = eng.nw_pileup_strands(q.a, q.b, am, q.targets)[0]
    eng.nw_identity_strands(q.a[:9], q.b[:9], np.ones(9, np.uint8))
    eng.nw_align_profile(reset=True)
    assert tab[:, 6].any()
    off, al, ql = eng.nw_msa_sites(so, st, 0, m, quals=True)
    same(al, wal, "after the pile-up") and same(ql, wql, "after the pile-up")
    assert eng.nw_msa_rows(0, nt + m)[0].tobytes() == base_rows
    assert all(np.array_equal(x, y) for x, y in zip(eng.nw_msa_counts(0, nt, weights=True), base_counts))
    same(eng.nw_msa_sites(so, st, 0, m)[1], wal, "after rows and counts again")
    assert eng.nw_align_profile()[2] == 0  # no choice bytes since the reset: nothing was aligned again
    # the kernels are "nw", the reverse complement "layout"; a measurement entry of their own
    eng.timers(reset=True)
    eng.nw_msa_profile(reset=True)
    eng.nw_msa_counts_profile(reset=True)
    assert eng.nw_msa_sites_profile(reset=True) > 0 and eng.nw_msa_sites_profile() == 0
    eng.nw_msa_sites(so, st, 0, m, quals=True)
    t = eng.timers()
    assert t["layout"][1] >= 1 and t["nw"][1] >= 2 and all(t[f][1] == 0 for f in t if f not in ("layout", "nw"))
    assert eng.nw_msa_sites_profile() > 0 and eng.nw_msa_profile() == (0.0, 0.0, 0.0, 0.0) and eng.nw_msa_counts_profile() == 0


# ---------------------------------------------------------------- 5. the certified band changes nothing
def test_the_band_changes_nothing(eng, monkeypatch):
    clean_env(monkeypatch)
    m = len(A.msa().a)
    eng.set_align_band(1)
    try:
        begin(eng, "mixed")
        for which in ("default", "edges", "long"):
            so, st, woff, wal, wql = S.expected(which, "mixed")
            off, al, ql = eng.nw_msa_sites(so, st, 0, m, quals=True)
            same(off, woff, which) and same(al, wal, which) and same(ql, wql, which)
    finally:
        eng.set_align_band(0)


# ---------------------------------------------------------------- 6. the contract
def test_offsets_capacity_errors_and_state(eng, monkeypatch):
    q = A.msa()
    nt, m = len(q.targets), len(q.a)
    clean_env(monkeypatch)
    bw = begin(eng, "mixed")[2]
    so, st, woff, wal, wql = (np.array(x) for x in S.expected("default", "mixed"))
    n = int(woff[-1])
    lib, ptr = eng.lib, M._p
    SENT = 0xA5

    def call(so, st, first, count, al, ql, cap, off, e=None):
        return lib.mc_nw_msa_sites((e or eng).ctx, ptr(so), ptr(st), C.c_uint64(first), C.c_uint64(count), ptr(al), ptr(ql), C.c_uint64(cap),
                                   ptr(off))

    def fresh():
        return np.full(n + 8, SENT, np.uint8), np.full(n + 8, SENT, np.uint8), np.full(m + 2, 77, np.uint64)

    untouched = lambda *arrs: all((a == SENT).all() for a in arrs)
    # alleles NULL: the offsets only, no device work
    al, ql, off = fresh()
    eng.timers(reset=True)
    assert call(so, st, 0, m, None, None, 0, off) == 0 and np.array_equal(off[:m + 1], woff) and off[m + 1] == 77
    assert all(v[1] == 0 for v in eng.timers().values())
    assert eng.nw_msa_sites(so, st, 0, m, alleles=False)[0].tolist() == woff.tolist()
    # quals without alleles
    al, ql, off = fresh()
    assert call(so, st, 0, m, None, ql, n, off) == M.ERR_ARG and untouched(ql) and (off == 77).all()
    # one byte short: off valid, nothing written
    assert call(so, st, 0, m, al, ql, n - 1, off) == M.ERR_ARG and np.array_equal(off[:m + 1], woff) and untouched(al, ql)
    al, ql, off = fresh()
    assert call(so, st, 0, m, al, None, n - 1, off) == M.ERR_ARG and np.array_equal(off[:m + 1], woff) and untouched(al)
    # exactly enough
    assert call(so, st, 0, m, al, ql, n, off) == 0
    assert np.array_equal(al[:n], wal) and np.array_equal(ql[:n], wql) and untouched(al[n:], ql[n:])
    # a range past m
    al, ql, off = fresh()
    for first, count in ((m, 1), (m + 1, 0), (5, m - 4), (0, m + 1), (1 << 63, 1 << 63)):
        assert call(so, st, first, count, al, ql, n, off) == M.ERR_ARG and (off == 77).all() and untouched(al, ql), (first, count)
    # count = 0; off and site_off are required
    assert call(so, st, m, 0, al, ql, n, off) == 0 and off[0] == 0 and off[1] == 77 and untouched(al, ql)
    assert call(so, st, 3, 0, al, ql, 0, off) == 0 and untouched(al, ql)
    assert call(so, st, 0, m, al, ql, n, None) == M.ERR_ARG and call(None, st, 0, m, al, ql, n, off) == M.ERR_ARG and untouched(al, ql)
    # the site lists: not strictly ascending, a site at W, offsets that do not start at 0 or decrease
    t = next(t for t in range(nt) if so[t + 1] - so[t] >= 3)
    lo = int(so[t])
    off[:] = 77
    for change in ("equal", "descending", "at W", "not from 0", "decreasing"):
        so2, st2 = so.copy(), st.copy()
        if change == "equal":
            st2[lo + 1] = st2[lo]
        elif change == "descending":
            st2[lo + 1], st2[lo + 2] = st[lo + 2], st[lo + 1]
        elif change == "at W":
            st2[int(so[t + 1]) - 1] = bw[t]
        elif change == "not from 0":
            so2[0] = 1
        else:
            so2[t + 1], so2[t + 2] = so[t + 1] + 1, so[t + 1]
        assert call(so2, st2, 0, m, al, ql, n, off) == M.ERR_ARG and (off == 77).all() and untouched(al, ql), change
        assert call(so2, st2, 0, m, None, None, 0, off) == M.ERR_ARG and (off == 77).all(), change
    with pytest.raises(M.MCError) as e:
        eng.nw_msa_sites(so, st, m, 1)
    assert e.value.code == M.ERR_ARG
    # an ascending list may run up to W - 1 and start anew in the next target
    lists = [np.array([w - 1], np.uint32) if w else np.zeros(0, np.uint32) for w in bw.astype(np.int64)]
    so3, st3 = S.flat(lists)
    off3, al3 = eng.nw_msa_sites(so3, st3, 0, m)
    rows = GM.split(*eng.nw_msa_rows(nt, m))
    assert al3.tobytes() == b"".join(r[-1:] for r in rows)
    # the target with no pairs: sites of its own change nothing; a target without sites between two with sites
    lone = q.tindex[P.pile().lonely]
    assert not (q.b == P.pile().lonely).any() and bw[lone] == 33
    lists = [np.zeros(0, np.uint32)] * nt
    lists[lone] = np.arange(33, dtype=np.uint32)
    off4, al4 = eng.nw_msa_sites(*S.flat(lists), 0, m)
    assert not off4.any() and len(al4) == 0
    has = [bool((q.b == j).any()) for j in q.targets]
    three = next([t - 1, t, t + 1] for t in range(1, nt - 1) if has[t - 1] and has[t] and has[t + 1] and bw[t + 1] >= 6)
    lists = [np.zeros(0, np.uint32)] * nt
    lists[three[0]], lists[three[2]] = np.arange(int(bw[three[0]]), dtype=np.uint32), np.array([0, 5], np.uint32)
    off5, al5 = eng.nw_msa_sites(*S.flat(lists), 0, m)
    ks = {t: [k for k in range(m) if q.tindex[int(q.b[k])] == t] for t in three}
    assert all(len(ks[t]) for t in three)
    assert all(off5[k + 1] - off5[k] == (len(lists[q.tindex[int(q.b[k])]])) for k in range(m))
    assert all(al5[int(off5[k]):int(off5[k + 1])].tobytes() == rows[k] for k in ks[three[0]])
    assert all(al5[int(off5[k]):int(off5[k + 1])].tobytes() == rows[k][0:1] + rows[k][5:6] for k in ks[three[2]])

    # no plan: after end, before any begin, after a load of sequences
    def no_plan(e=None):
        o = np.zeros(2, np.uint64)
        return call(np.zeros(nt + 1, np.uint64), None, 0, 0, None, None, 0, o, e) == M.ERR_STATE

    assert not no_plan()
    eng.nw_msa_end()
    assert no_plan()
    al, ql, off = fresh()
    assert call(so, st, 0, m, al, ql, n, off) == M.ERR_STATE and (off == 77).all() and untouched(al, ql)
    begin(eng, "mixed")
    same(eng.nw_msa_sites(so, st, 0, m)[1], wal, "after end and a new begin")  # (end freed the scratch: it comes back)

    # no qualities loaded: the weights are a state error, the alleles are not
    other = M.Engine(0)
    try:
        assert no_plan(other)  # no sequences
        small = P.pile()
        other.load_sequences(*small.load_args())
        assert no_plan(other)  # sequences, but no begin yet
        ks = np.arange(small.nbase, small.nbase + 12)
        tg = sorted(set(int(j) for j in small.b[ks]))
        bw2 = other.nw_msa_begin(small.a[ks], small.b[ks], None, tg)[2]
        so6, st6 = S.flat([np.arange(int(w), dtype=np.uint32) for w in bw2])
        want6 = other.nw_msa_rows(len(tg), 12)[0]
        al, ql, off = np.full(len(want6), SENT, np.uint8), np.full(len(want6), SENT, np.uint8), np.full(13, 77, np.uint64)
        assert call(so6, st6, 0, 12, al, ql, len(al), off, other) == M.ERR_STATE and untouched(al, ql) and (off == 77).all()
        assert call(so6, st6, 0, 12, al, None, len(al), off, other) == 0 and np.array_equal(al, want6)
        other.load_qualities(Q.flat(Q.qualities()))
        assert call(so6, st6, 0, 12, al, ql, len(al), off, other) == 0 and np.array_equal(al, want6) and ql.any()
        other.load_sequences(*small.load_args())
        assert no_plan(other)
    finally:
        other.close()


# ---------------------------------------------------------------- 7. a planted cluster
def planted_cluster():
    """-> (codes, segs, a, b): a centre of 60 seeded bases, 6 exact copies, 6 copies of haplotype B
    (one substitution, one 2-base insertion, one 1-base deletion) and one read with a private
    substitution."""
    rng = np.random.default_rng(5)
    while True:  # a centre in which no edit can slide: no two equal neighbours around the edits
        cen = rng.integers(0, 4, 60).astype(np.uint8)
        if all(cen[k] != cen[k + 1] for k in range(59)):
            break
    hb = cen.copy()
    hb[12] = (hb[12] + 2) % 4
    ins = np.array([x for x in range(4) if x not in (cen[29], cen[30])], np.uint8)  # the two letters of neither neighbour
    hb = np.concatenate([hb[:30], ins, hb[30:45], hb[46:]])
    priv = cen.copy()
    priv[50] = (priv[50] + 1) % 4
    codes = [cen] + [cen.copy() for _ in range(6)] + [hb.copy() for _ in range(6)] + [priv]
    segs = [[[0, len(c) - 1]] for c in codes]
    return codes, segs, np.arange(1, 14, dtype=np.uint32), np.zeros(13, np.uint32)


def test_planted_cluster(built, monkeypatch):
    clean_env(monkeypatch)
    codes, segs, a, b = planted_cluster()
    lens = [len(c) for c in codes]
    seq_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    seg = np.array([v for s in segs for pair in s for v in pair], np.int32)
    seg_off = np.concatenate([[0], np.cumsum([len(s) for s in segs])]).astype(np.uint64)
    e = M.Engine(0)
    try:
        e.load_sequences(np.concatenate(codes), seq_off, seg, seg_off)
        bw = e.nw_msa_begin(a, b, None, [0])[2]
        col_off, counts = e.nw_msa_counts(0, 1)
        rows = GM.split(*e.nw_msa_rows(1, 13))
        sites = S.variant_sites(counts, 0.2, 2)
        off, al = e.nw_msa_sites(*S.flat([sites]), 0, 13)
    finally:
        e.close()
    assert int(bw[0]) == 62
    # the restatement's sites, from the rows alone
    hist = np.zeros((62, 8), np.uint32)
    for r in rows:
        hist[np.arange(62), F._CLASS[np.frombuffer(r, np.uint8)]] += 1
    assert np.array_equal(hist[:, :6], counts[:, :6]) and np.array_equal(sites, S.variant_sites(hist, 0.2, 2))
    assert len(sites) >= 4 and (counts[sites.astype(np.int64), 7] != 0).sum() == 2  # the two slot columns
    assert any(counts[c, 7] == 0 and counts[c, 5] == 6 for c in sites)  # the deleted centre column
    priv_col = next(c for c in range(62) if counts[c, 6] == 50 and counts[c, 7] == 0)
    assert priv_col not in sites.tolist() and sorted(counts[priv_col, :4].tolist())[-2:] == [1, 12]
    S_ = len(sites)
    assert np.array_equal(off, np.arange(14, dtype=np.uint64) * S_)
    strings = [al[k * S_:(k + 1) * S_].tobytes() for k in range(13)]
    assert strings == [bytes(np.frombuffer(r, np.uint8)[sites.astype(np.int64)]) for r in rows]
    hap = S.haplotypes(strings, 2)
    assert [n for _, n in hap] == [7, 6] and len(S.haplotypes(strings, 1)) == 2
    assert hap[0][0] == strings[0] == strings[12] and hap[1][0] == strings[6] and hap[1][0].count(b"-") == 1 and hap[0][0].count(b"-") == 2


# ---------------------------------------------------------------- 8. end to end
VARIANT_KEYS = ("variant_centres", "variant_sites", "allele_bytes")
DROP = VARIANT_KEYS + ("phases_ms", "device_us")
LOW = ["--min-allele-count", "1", "--min-allele-frac", "0.05"]


def profile_blocks(path):
    """The --profile (or --variants) file -> [(centre, its lines with their newline, counts[n, 8])] in file order."""
    out = []
    for ln in open(path).read().splitlines(True):
        x = ln.rstrip("\n").split("\t")
        if not out or out[-1][0] != x[0]:
            out.append((x[0], [], []))
        out[-1][1].append(ln)
        out[-1][2].append([int(v) for v in x[6:12]] + [int(x[2]) - 1, int(x[3])])
    return [(name, lines, np.array(c, np.uint32)) for name, lines, c in out]


def msa_blocks(path):
    """The --msa file -> [(centre, [(read, strand, row)])] in file order."""
    recs = G.read_fasta(path)
    out = []
    for h, row in recs:
        h = h[1:].decode()
        if h.rsplit(" ", 1)[1].startswith("width="):
            out.append((h.rsplit(" ", 2)[0], []))
        else:
            name, sd = h.rsplit(" ", 1)
            assert sd in ("strand=+", "strand=-")
            out[-1][1].append((name, sd[-1], row))
    return out


def expected_files(profile, msa, frac, count):
    """-> (the --variants text, the --alleles text, the --haplotypes text, [centres with a site, sites, allele
    bytes], the sites per centre) from the --profile and --msa files alone, by sites_cases' port of variants.hpp."""
    var, al, hap, stats, sites_of = [], [], [], [0, 0, 0], {}
    blocks = msa_blocks(msa)
    prof = profile_blocks(profile)
    assert [b[0] for b in blocks] == [p[0] for p in prof]
    for (name, lines, counts), (_, reads) in zip(prof, blocks):
        sites = S.variant_sites(counts, frac, count).astype(np.int64)
        sites_of[name] = (sites, counts)
        var += [lines[c] for c in sites]
        strings = [bytes(np.frombuffer(row, np.uint8)[sites]) for _, _, row in reads]
        al += ["%s\t%s\t%s\t%s\n" % (r, name, sd, x.decode() if len(sites) else ".") for (r, sd, _), x in zip(reads, strings)]
        if len(sites):
            hap += ["%s\t%d\t%d\t%d\t%s\n" % (name, k + 1, n, len(reads), x.decode()) for k, (x, n) in enumerate(S.haplotypes(strings, count))]
            stats = [stats[0] + 1, stats[1] + len(sites), stats[2] + len(sites) * len(reads)]
    return "".join(var), "".join(al), "".join(hap), stats, sites_of


def test_cli_variants(e2e):
    path = lambda name, ext: str(e2e.tmp / (name + ext))
    new = lambda name: ["--variants", path(name, ".var.tsv"), "--alleles", path(name, ".al.tsv"), "--haplotypes", path(name, ".hap.tsv")]
    both = lambda name: ["--both-strands", "--msa", path(name, ".msa.fa"), "--profile", path(name, ".profile.tsv")]
    full = e2e("v_full", both("v_full") + new("v_full") + LOW)
    plain = e2e("v_plain", both("v_plain"))
    read = lambda name, ext: open(path(name, ext)).read()
    var, al, hap, stats, sites_of = expected_files(path("v_full", ".profile.tsv"), path("v_full", ".msa.fa"), 0.05, 1)
    assert read("v_full", ".var.tsv") == var
    assert read("v_full", ".al.tsv") == al
    assert read("v_full", ".hap.tsv") == hap
    # not vacuous: three centres with two sites or more, a site that is a slot column, two strings somewhere
    assert sum(len(s) >= 2 for s, _ in sites_of.values()) >= 3
    assert any((c[s, 7] != 0).any() for s, c in sites_of.values() if len(s))
    assert any(x.split("\t")[1] == "2" for x in hap.splitlines()) and "\t-\t" in al and "\t+\t" in al
    # every other output and the remaining stats are those of the run without the new options
    assert full["tsv"].read_bytes() == plain["tsv"].read_bytes()
    assert read("v_full", ".msa.fa") == read("v_plain", ".msa.fa") and read("v_full", ".profile.tsv") == read("v_plain", ".profile.tsv")
    st, pst = full["st"], plain["st"]
    assert not any(k in pst for k in VARIANT_KEYS) and "variants" not in pst["phases_ms"]
    assert {k: v for k, v in st.items() if k not in DROP} == {k: v for k, v in pst.items() if k not in DROP}
    assert list(st)[:-3] == list(pst) and list(st)[-3:] == list(VARIANT_KEYS)
    assert list(st["phases_ms"])[:-1] == list(pst["phases_ms"]) and list(st["phases_ms"])[-1] == "variants" and st["phases_ms"]["variants"] > 0
    assert [st[k] for k in VARIANT_KEYS] == stats
    # the defaults: fewer sites, the same rule
    dflt = e2e("v_default", both("v_default") + new("v_default"))
    var2, al2, hap2, stats2, _ = expected_files(path("v_default", ".profile.tsv"), path("v_default", ".msa.fa"), 0.2, 2)
    assert (read("v_default", ".var.tsv"), read("v_default", ".al.tsv"), read("v_default", ".hap.tsv")) == (var2, al2, hap2)
    assert [dflt["st"][k] for k in VARIANT_KEYS] == stats2 and stats2[1] < stats[1]
    # --alleles alone computes the sites; --band beside it changes nothing; --haplotypes alone reads the alleles too
    alone = e2e("v_alone", ["--both-strands", "--alleles", path("v_alone", ".al.tsv")] + LOW)
    band = e2e("v_band", ["--both-strands", "--band", "--alleles", path("v_band", ".al.tsv"), "--haplotypes", path("v_band", ".hap.tsv")] + LOW)
    only = e2e("v_only", ["--both-strands", "--haplotypes", path("v_only", ".hap.tsv")] + LOW)
    ident = e2e("v_ident", ["--both-strands", "--identity"])
    assert read("v_alone", ".al.tsv") == al == read("v_band", ".al.tsv") and read("v_band", ".hap.tsv") == hap == read("v_only", ".hap.tsv")
    assert alone["tsv"].read_bytes() == ident["tsv"].read_bytes() == band["tsv"].read_bytes()
    ast = alone["st"]
    assert list(ast)[-3:] == list(VARIANT_KEYS) and [ast[k] for k in VARIANT_KEYS] == stats and list(ast["phases_ms"])[-1] == "variants"
    assert not any(k in ast for k in GM.MSA_KEYS + ("profile_centres", "profile_columns"))
    assert {k: v for k, v in ast.items() if k not in DROP} == {k: v for k, v in ident["st"].items() if k not in DROP}
    assert list(band["st"])[-3:] == list(VARIANT_KEYS) and band["st"]["band_pairs"] > 0
    # --variants alone reads no alleles
    vonly = e2e("v_vonly", ["--both-strands", "--variants", path("v_vonly", ".var.tsv")] + LOW)
    assert read("v_vonly", ".var.tsv") == var and [vonly["st"][k] for k in VARIANT_KEYS] == stats[:2] + [0]


def test_cli_variants_with_quality(family):
    pf = lambda name, ext: str(family.tmp / (name + ext))
    args = lambda name: ["--both-strands", "--paf", "@paf", "--quality", "--profile", pf(name, ".profile.tsv"), "--variants", pf(name, ".var.tsv"),
                         "--alleles", pf(name, ".al.tsv"), "--haplotypes", pf(name, ".hap.tsv"), "--min-allele-count", "2",
                         "--min-allele-frac", "0.1"]
    full = family("vq", args("vq"), family.fq)
    reads = {name: (s.upper(), np.frombuffer(q, np.uint8) - 33) for name, s, q in GQ.read_fastq(family.fq)}
    cents = {h[1:].decode(): G.codes_of(s.upper()) for h, s in G.read_fasta(family.cen)}
    pairs, who = {}, {}
    for x in G.rows_of(full["paf"]):
        s, q = reads[x[0]]
        if x[4] == "-":
            s, q = s.translate(G._RC)[::-1], q[::-1]
        pairs.setdefault(x[5], []).append((G.parse_cigar(x[14][5:]), G.codes_of(s), q))
        who.setdefault(x[5], []).append((x[0], x[4]))
    assert len(pairs) == 1
    (name, ps), = pairs.items()
    w, col, W, counts, wcounts = F.from_words(cents[name], ps)
    sites = S.variant_sites(counts, 0.1, 2)
    assert len(sites) >= 2
    prof = profile_blocks(pf("vq", ".profile.tsv"))
    assert len(prof) == 1 and np.array_equal(prof[0][2], counts)
    assert open(pf("vq", ".var.tsv")).read() == "".join(prof[0][1][c] for c in sites) and all(len(ln.split("\t")) == 18 for ln in prof[0][1])
    want, strings = [], []
    for (rname, sd), (words, read, qs) in zip(who[name], ps):
        al, ql = S.from_words(w, col, words, read, qs, sites)
        strings.append(al.tobytes())
        want.append("%s\t%s\t%s\t%s\t%s\n" % (rname, name, sd, al.tobytes().decode(), (ql + 33).tobytes().decode()))
    assert open(pf("vq", ".al.tsv")).read() == "".join(want)
    assert any(x.split("\t")[4].strip("!") for x in want) and {x.split("\t")[2] for x in want} == {"+", "-"}
    hap = ["%s\t%d\t%d\t%d\t%s\n" % (name, k + 1, n, len(ps), x.decode()) for k, (x, n) in enumerate(S.haplotypes(strings, 2))]
    assert open(pf("vq", ".hap.tsv")).read() == "".join(hap) and len(hap) >= 1
    assert full["st"]["allele_bytes"] == 2 * len(sites) * len(ps)
    # without --quality: four columns, the same alleles
    noq = family("vq_noq", ["--both-strands", "--alleles", pf("vq_noq", ".al.tsv"), "--min-allele-count", "2", "--min-allele-frac", "0.1"], family.fq)
    assert open(pf("vq_noq", ".al.tsv")).read() == "".join(x.rsplit("\t", 1)[0] + "\n" for x in want)
    assert noq["st"]["allele_bytes"] == len(sites) * len(ps)


def test_assign_files_variants(e2e, tmp_path):
    """The same job in process (mcl_assign_variants), on a context of its own sequences."""
    path = lambda name, ext: str(e2e.tmp / (name + ext))
    new = lambda name: ["--variants", path(name, ".var.tsv"), "--alleles", path(name, ".al.tsv"), "--haplotypes", path(name, ".hap.tsv")]
    full = e2e("v_full", ["--both-strands", "--msa", path("v_full", ".msa.fa"), "--profile", path("v_full", ".profile.tsv")] + new("v_full") + LOW)
    e = M.Engine(0)
    try:
        model = str(e2e.cen).replace(".centres.fa", ".model")
        st = M.assign_files(e, model, str(e2e.cen), str(e2e.reads), str(tmp_path / "l.tsv"), threads=2, both_strands=True,
                            variants=str(tmp_path / "l.var"), alleles=str(tmp_path / "l.al"), haplotypes=str(tmp_path / "l.hap"),
                            min_allele_frac=0.05, min_allele_count=1)
        st2 = M.assign_files(e, model, str(e2e.cen), str(e2e.reads), str(tmp_path / "l2.tsv"), threads=2, both_strands=True, band=True,
                             msa=str(tmp_path / "l2.msa.fa"), profile=str(tmp_path / "l2.profile.tsv"), alleles=str(tmp_path / "l2.al"),
                             min_allele_frac=0.05, min_allele_count=1)
        with pytest.raises(Exception):
            M.assign_files(e, model, str(e2e.cen), str(e2e.reads), str(tmp_path / "l3.tsv"), alleles=str(tmp_path / "l3.al"), min_allele_frac=0.0)
    finally:
        e.close()
    for ext, mine in ((".var.tsv", "l.var"), (".al.tsv", "l.al"), (".hap.tsv", "l.hap")):
        assert (tmp_path / mine).read_bytes() == open(path("v_full", ext), "rb").read(), ext
    assert (tmp_path / "l2.al").read_bytes() == (tmp_path / "l.al").read_bytes()
    assert (tmp_path / "l2.msa.fa").read_bytes() == open(path("v_full", ".msa.fa"), "rb").read()
    assert (tmp_path / "l.tsv").read_bytes() == full["tsv"].read_bytes()
    assert [st[k] for k in VARIANT_KEYS] == [full["st"][k] for k in VARIANT_KEYS] and list(st)[-3:] == list(VARIANT_KEYS)
    assert list(st2)[-3:] == list(VARIANT_KEYS) and st2["variant_sites"] == st["variant_sites"] and st2["band_pairs"] > 0
