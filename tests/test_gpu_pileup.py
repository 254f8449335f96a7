"""mc_nw_pileup_strands / meshclust-assign --consensus --pileup on the GPU.  Every comparison is ==.

The expectations: the Python restatement of tests/pileup_cases.py over the words of
tests/nw_trace_cases.py (tied to the CPU oracle by test_nw_trace_host.py and test_pileup_host.py),
and mc_nw_align_strands for score / columns / '='.  One set of points, loaded once."""
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

pytestmark = pytest.mark.gpu

ASSIGN_BIN = os.path.join(os.path.dirname(M.BIN), "meshclust-assign")
ENV_VARS = ("MC_ALIGN_BATCH", "MC_ALIGN_SCRATCH", "MC_IDENT_BATCH", "MC_IDENT_BYTES", "MC_PILEUP_NAIVE")


@pytest.fixture(scope="module")
def eng(built):
    e = M.Engine(0)
    e.load_sequences(*P.pile().load_args())
    yield e
    e.close()


def clean_env(monkeypatch, **kw):
    for var in ENV_VARS:
        monkeypatch.delenv(var, raising=False)
    for k, v in kw.items():
        monkeypatch.setenv(k, str(v))


def strands(name):
    n = len(P.pile().a)
    return {"plus": None, "minus": np.ones(n, np.uint8), "mixed": P.mixed_strands()}[name]


# ---------------------------------------------------------------- 1. the table and the integers
@pytest.mark.parametrize("name", ["plus", "minus", "mixed"])
def test_table_equals_the_restatement(eng, name, monkeypatch):
    clean_env(monkeypatch)
    p = P.pile()
    am = strands(name)
    flags = np.zeros(len(p.a), np.uint8) if am is None else am
    tab, off, score, ln, ids = eng.nw_pileup_strands(p.a, p.b, am, p.targets)
    assert off.dtype == np.uint64 and np.array_equal(off, p.row_off)
    assert tab.dtype == np.uint32 and tab.shape == (int(p.row_off[-1]), 8)
    want = P.expected_table(flags)
    bad = np.nonzero((tab != want).any(axis=1))[0]
    assert len(bad) == 0, (name, bad[:8], tab[bad[:4]], want[bad[:4]])
    _, _, a_score, a_ln, a_ids = eng.nw_align_strands(p.a, p.b, am, cigar=False)
    for x, y in ((score, a_score), (ln, a_ln), (ids, a_ids)):
        assert x.dtype == y.dtype and np.array_equal(x, y)
    exp = P.expected()
    assert [(int(s), int(c), int(i)) for s, c, i in zip(score, ln, ids)] == [exp[flags[k]][k][1:] for k in range(len(p.a))]
    t = p.tindex[p.lonely]
    assert not tab[int(off[t]):int(off[t + 1])].any()  # a target with no pair
    t = p.tindex[p.contended]
    assert (tab[int(off[t]):int(off[t + 1]) - 1, :6].sum(axis=1) == 150).all()


# ---------------------------------------------------------------- 2. batching changes nothing
def test_batches_give_the_same_bytes(eng, monkeypatch):
    p = P.pile()
    am = P.mixed_strands()
    clean_env(monkeypatch)
    base = eng.nw_pileup_strands(p.a, p.b, am, p.targets)
    assert np.array_equal(base[0], P.expected_table(am))
    big = T.choice_bytes(1100, 1100)
    assert big == max(T.choice_bytes(len(p.codes[i]), len(p.codes[j])) for i, j in zip(p.a, p.b))
    # MC_IDENT_BYTES: the batch end no other cap reaches, several times in the list and inside the
    # contended centre's reads (host/pairbatch.hpp's rule restated: nw_trace_cases.batch_ends)
    lens = [len(x) for x in p.codes]
    nbytes = T.ident_bytes(lens, p.a[am != 0])
    by = [i1 for i1, why in T.batch_ends(lens, p.a, p.b, am, 1 << 16, nbytes, 1 << 30) if why == "bytes"]
    assert len(by) >= 2 and any(p.b[i1 - 1] == p.contended == p.b[i1] for i1 in by), (nbytes, by)
    for env in ({"MC_ALIGN_BATCH": 7}, {"MC_ALIGN_BATCH": 1}, {"MC_ALIGN_SCRATCH": 3 * big + 64}, {"MC_PILEUP_NAIVE": 1},
                {"MC_PILEUP_NAIVE": 1, "MC_ALIGN_BATCH": 7}, {"MC_IDENT_BYTES": nbytes}):
        clean_env(monkeypatch, **env)
        res = eng.nw_pileup_strands(p.a, p.b, am, p.targets)
        assert all(x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(res, base)), env
    assert sum(1 for j in p.b if j == p.contended) > 7 * 20  # the contended centre is split over many batches
    # a second call overwrites: the same pairs give the same table, fewer pairs a smaller one
    clean_env(monkeypatch)
    half = np.arange(0, len(p.a), 2)
    tab, _, _, _, _ = eng.nw_pileup_strands(p.a[half], p.b[half], am[half], p.targets)
    assert np.array_equal(tab, P.expected_table(am, half))


# ---------------------------------------------------------------- 3. the call's contract
def test_offsets_only_capacity_and_errors(eng, monkeypatch):
    p = P.pile()
    am = P.mixed_strands()
    clean_env(monkeypatch)
    tab, off, score, ln, ids = eng.nw_pileup_strands(p.a, p.b, am, p.targets)
    none, off0, _, _, _ = eng.nw_pileup_strands(p.a, p.b, am, p.targets, table=False)  # table = NULL
    assert none is None and np.array_equal(off0, off)
    lib, ptr = eng.lib, M._p
    m, nt, rows = len(p.a), len(p.targets), int(off[-1])
    a, b, tg = np.ascontiguousarray(p.a), np.ascontiguousarray(p.b), np.ascontiguousarray(p.targets)

    def call(n, buf, cap, o, s=None, targets=tg, bb=b):
        return lib.mc_nw_pileup_strands(eng.ctx, ptr(a[:n]), ptr(bb[:n]), ptr(am[:n]), C.c_uint64(n), ptr(targets),
                                        C.c_uint32(len(targets)), ptr(o), ptr(buf), C.c_uint64(cap), ptr(s), None, None)

    SENT = 0xDEADBEEF
    buf = np.full((rows + 2) * 8, SENT, np.uint32)
    o = np.full(nt + 1, 77, np.uint64)
    assert call(m, buf, rows - 1, o) == M.ERR_ARG  # one row short
    assert np.array_equal(o, off) and (buf == SENT).all()
    assert call(m, buf, rows, o) == 0  # exactly enough; score / len / ids NULL
    assert np.array_equal(buf[:rows * 8].reshape(rows, 8), tab) and (buf[rows * 8:] == SENT).all()
    buf[:] = SENT
    o[:] = 77
    assert call(0, buf, rows, o) == 0 and np.array_equal(o, off)  # m = 0: a zeroed table
    assert (buf[:rows * 8] == 0).all() and (buf[rows * 8:] == SENT).all()
    # a duplicate target, a b that is no target, an id >= n: MC_ERR_ARG, nothing written
    buf[:] = SENT
    o[:] = 77
    s = np.full(m, -7, np.int32)
    dup = np.concatenate([tg, tg[:1]])
    o2 = np.full(nt + 2, 77, np.uint64)
    assert call(m, buf, rows + 4000, o2, s, targets=dup) == M.ERR_ARG and (o2 == 77).all()
    assert call(m, buf, rows, o[:nt], s, targets=np.ascontiguousarray(tg[:-2])) == M.ERR_ARG  # (the last pairs' centre is gone)
    assert p.b[-1] in tg[-2:]
    far = tg.copy()
    far[3] = len(p.codes)
    assert call(m, buf, rows, o, s, targets=far) == M.ERR_ARG
    bad_b = b.copy()
    bad_b[5] = len(p.codes)
    assert call(m, buf, rows, o, s, bb=bad_b) == M.ERR_ARG
    with pytest.raises(M.MCError) as e:
        eng.nw_pileup_strands([len(p.codes)], [p.targets[0]], [0], p.targets)
    assert e.value.code == M.ERR_ARG
    assert (buf == SENT).all() and (o == 77).all() and (s == -7).all()
    # a cap below one pair's need: refused before anything is written
    clean_env(monkeypatch, MC_ALIGN_SCRATCH=T.choice_bytes(1100, 1100) - 1)
    assert call(m, buf, rows, o, s) == M.ERR_UNSUPPORTED
    assert (buf == SENT).all() and (o == 77).all() and (s == -7).all()
    clean_env(monkeypatch)
    fresh = M.Engine(0)  # no sequences loaded
    try:
        with pytest.raises(M.MCError) as e:
            fresh.nw_pileup_strands([0], [0], [1], [0])
        assert e.value.code == M.ERR_STATE
    finally:
        fresh.close()
    eng.timers(reset=True)
    eng.nw_pileup_profile(reset=True)
    eng.nw_pileup_strands(p.a[:5], p.b[:5], [1, 0, 0, 0, 0], p.targets)
    t = eng.timers()
    assert t["layout"][1] == 1 and t["nw"][1] >= 4  # forward, traceback, pile-up and finish as nw
    assert all(t[f][1] == 0 for f in t if f not in ("layout", "nw"))
    fwd, tb, pu = eng.nw_pileup_profile()
    assert fwd > 0 and tb > 0 and pu > 0


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
    assert (c <= 3).all()  # (pure ACGT: the parser's digits are the letters' ranks)
    return c


def outputs_from_paf(paf, reads_fa, centres_fa):
    """-> (consensus FASTA text, pile-up TSV text, centres with an insertion site) from a PAF's
    CIGARs and the two FASTA files alone."""
    reads = {h[1:].decode(): s.upper() for h, s in read_fasta(reads_fa)}
    cents = [(h[1:].decode(), codes_of(s.upper())) for h, s in read_fasta(centres_fa)]
    tabs = {name: np.zeros((len(c) + 1, 8), np.uint32) for name, c in cents}
    runs = {name: [] for name, _ in cents}
    depth = {name: 0 for name, _ in cents}
    cen = dict(cents)
    for x in rows_of(paf):
        q = reads[x[0]]
        if x[4] == "-":
            q = q.translate(_RC)[::-1]
        q = codes_of(q)
        words = parse_cigar(x[14][5:])
        P.table_from_words(words, q, cen[x[5]], tabs[x[5]])
        runs[x[5]] += P.insertion_runs(words, q)
        depth[x[5]] += 1
    fa, tsv, sited = [], [], 0
    for name, c in cents:
        seq, sub, dele, ins = P.consensus(c, tabs[name], depth[name], runs[name])
        sited += any(2 * int(v) > depth[name] for v in tabs[name][:, 6]) if depth[name] else 0
        fa.append(">%s depth=%d sub=%d del=%d ins=%d\n%s\n" % (name, depth[name], sub, dele, ins, seq))
        if depth[name]:
            for r, row in enumerate(tabs[name]):
                tsv.append("\t".join([name, str(r + 1), P.base_char(c[r]) if r < len(c) else "*", str(depth[name])] +
                                     [str(int(v)) for v in row]) + "\n")
    return "".join(fa), "".join(tsv), sited


@pytest.fixture(scope="module")
def e2e(built, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("pileup")
    fa, flags = fixtures.e2e_input("a1k", tmp)
    model, cen = tmp / "a1k.model", tmp / "a1k.centres.fa"
    r = subprocess.run([M.BIN, fa] + flags + ["--output", str(tmp / "a1k.clstr"), "--quiet", "--save-model", str(model),
                                              "--save-centres", str(cen)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    recs = read_fasta(fa)[:260]  # 260 reads, every second one reverse-complemented (the PAF test's families)
    reads = tmp / "F.fa"
    with open(reads, "wb") as f:
        for i, (h, s) in enumerate(recs):
            f.write(h + b"\n" + (s.upper().translate(_RC)[::-1] if i % 2 else s) + b"\n")
    env = {k: v for k, v in os.environ.items() if k not in ("MC_ASSIGN_FORM", "MC_ASSIGN_TILE", "MC_ASSIGN_PAIRS") + ENV_VARS}
    done = {}

    def run(name, extra, reads_fa=reads, centres=cen):
        if name not in done:
            out = {k: tmp / (name + ext) for k, ext in (("tsv", ".tsv"), ("paf", ".paf"), ("cons", ".cons.fa"), ("pile", ".pile.tsv"),
                                                        ("stats", ".json"))}
            args = [str(out[a[1:]]) if a.startswith("@") else a for a in extra]
            r = subprocess.run([ASSIGN_BIN, "--model", str(model), "--centres", str(centres), str(reads_fa), "--output", str(out["tsv"]),
                                "--quiet", "--stats-json", str(out["stats"])] + args, capture_output=True, text=True, timeout=300, env=env)
            assert r.returncode == 0, r.stderr[-3000:]
            out["st"] = json.loads(out["stats"].read_text())
            done[name] = out
        return done[name]

    run.reads, run.cen, run.tmp = reads, cen, tmp
    return run


NEW_KEYS = ("consensus_pairs", "consensus_centres", "consensus_passes", "realigned_centres", "insertion_sites")


def test_cli_consensus_and_pileup(e2e):
    full = e2e("full", ["--both-strands", "--paf", "@paf", "--consensus", "@cons", "--pileup", "@pile"])
    plain = e2e("plain", ["--both-strands", "--paf", "@paf"])
    # the TSV, its identity column and the PAF are those of the run without the new options
    assert full["tsv"].read_bytes() == plain["tsv"].read_bytes() and full["paf"].read_bytes() == plain["paf"].read_bytes()
    assert not plain["cons"].exists() and not plain["pile"].exists() and not any(k in plain["st"] for k in NEW_KEYS)
    assert {k: v for k, v in full["st"].items() if k not in NEW_KEYS + ("phases_ms", "device_us")} == \
        {k: v for k, v in plain["st"].items() if k not in ("phases_ms", "device_us")}
    # both files again from the PAF's CIGARs and the FASTA files
    fa, tsv, sited = outputs_from_paf(full["paf"], e2e.reads, e2e.cen)
    assert full["cons"].read_text() == fa
    assert full["pile"].read_text() == tsv
    st = full["st"]
    paf = rows_of(full["paf"])
    assert st["consensus_pairs"] == len(paf) == st["assigned"] > 200 and st["consensus_passes"] == 2
    assert st["consensus_centres"] == len({x[5] for x in paf}) and st["realigned_centres"] == sited
    assert {x[4] for x in paf} == {"+", "-"}
    heads = [ln for ln in fa.splitlines() if ln.startswith(">")]
    cens = read_fasta(e2e.cen)
    assert len(heads) == len(cens) >= st["consensus_centres"]  # every centre, in the file's order
    assert any(" sub=0 " not in h for h in heads)  # (some consensus differs from its centre)
    # a few reads only: the centres without a read are written too, as their own sequence
    few_fa = e2e.tmp / "few.fa"
    few_fa.write_bytes(b"".join(h + b"\n" + s + b"\n" for h, s in read_fasta(e2e.reads)[:4]))
    few = e2e("few", ["--both-strands", "--consensus", "@cons", "--pileup", "@pile"], reads_fa=few_fa)
    recs = read_fasta(few["cons"])
    assert [h.split(b" depth=")[0] for h, _ in recs] == [h for h, _ in cens]
    bare = [k for k, (h, _) in enumerate(recs) if h.endswith(b" depth=0 sub=0 del=0 ins=0")]
    assert len(bare) == len(cens) - few["st"]["consensus_centres"] >= len(cens) - 4
    assert all(recs[k][1] == cens[k][1].upper() for k in bare)
    assert {x[0] for x in rows_of(few["pile"])} == {cens[k][0][1:].decode() for k in range(len(cens)) if k not in bare}
    # --consensus alone: the pile-up is the only alignment pass, the identities are its own
    ident = e2e("ident", ["--both-strands", "--identity"])
    alone = e2e("alone", ["--both-strands", "--consensus", "@cons"])
    assert alone["cons"].read_text() == fa and not alone["pile"].exists()
    assert alone["st"]["consensus_passes"] == 1 and alone["st"]["consensus_pairs"] == st["consensus_pairs"]
    assert alone["tsv"].read_bytes() == ident["tsv"].read_bytes() == full["tsv"].read_bytes()
    # --pileup alone
    only = e2e("only", ["--both-strands", "--pileup", "@pile"])
    assert only["pile"].read_text() == tsv and not only["cons"].exists() and only["st"]["consensus_passes"] == 1


def test_cli_planted_truth(e2e):
    """The planted family through the tool: its centre takes the place of the first centre of the
    file, its 30 reads are assigned to it, and the consensus is the template."""
    p = P.pile()
    cens = read_fasta(e2e.cen)
    letters = lambda c: "".join(P.LETTERS[x] for x in c).encode()
    cens[0][1] = letters(p.codes[p.planted])
    cfile, rfile = e2e.tmp / "planted.centres.fa", e2e.tmp / "planted.reads.fa"
    cfile.write_bytes(b"".join(h + b"\n" + s + b"\n" for h, s in cens))
    ks = [k for k in range(len(p.a)) if p.b[k] == p.planted]
    rfile.write_bytes(b"".join(b">p%d\n" % i + letters(p.codes[p.a[k]]) + b"\n" for i, k in enumerate(ks)))
    out = e2e("planted", ["--consensus", "@cons", "--pileup", "@pile"], reads_fa=rfile, centres=cfile)
    assert out["st"]["assigned"] == 30 and out["st"]["consensus_centres"] == 1
    assert out["st"]["realigned_centres"] == 1 and out["st"]["insertion_sites"] == 1
    head, seq = out["cons"].read_text().splitlines()[:2]
    assert head == cens[0][0].decode() + " depth=30 sub=6 del=2 ins=1"
    assert seq == letters(p.truth).decode()
    tab = np.array([[int(v) for v in x[4:]] for x in rows_of(out["pile"])], np.uint32)
    t = p.tindex[p.planted]
    assert np.array_equal(tab, P.expected_table(np.zeros(len(p.a), np.uint8), ks)[int(p.row_off[t]):int(p.row_off[t + 1])])


def test_assign_files_consensus(e2e, tmp_path):
    """The same job in process (mcl_assign_consensus), on a context of its own sequences."""
    full = e2e("full", ["--both-strands", "--paf", "@paf", "--consensus", "@cons", "--pileup", "@pile"])
    e = M.Engine(0)
    try:
        model = str(e2e.cen).replace(".centres.fa", ".model")
        st = M.assign_files(e, model, str(e2e.cen), str(e2e.reads), str(tmp_path / "l.tsv"), threads=2, both_strands=True,
                            consensus=str(tmp_path / "l.fa"), pileup=str(tmp_path / "l.pile"))
    finally:
        e.close()
    assert (tmp_path / "l.fa").read_bytes() == full["cons"].read_bytes()
    assert (tmp_path / "l.pile").read_bytes() == full["pile"].read_bytes()
    assert st["consensus_passes"] == 1 and st["consensus_pairs"] == full["st"]["consensus_pairs"]
