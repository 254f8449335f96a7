"""mc_revcomp_sequences / mc_nw_identity_strands / meshclust-assign --identity, --min-identity.

Every value is compared with ==, and every expectation comes from code that existed before this
feature: numpy on the loaded bytes (the minus-strand string is the bytes reversed and mapped),
mc_nw_identity on reverse-complemented records loaded as points of their own, and the
command-line tool's files without the new options.

Points (one load, in this order):
  LAY    16 passes over records of 1, 15, 16, 17, 31, 33, 63, 64, 65 and 1,000 digits; a pass is
         1,305 bytes = 9 mod 16, so every one of the ten lengths starts at every byte alignment
  G      two segments around an N run;  E  a record without segments (raw letters and N);
  P      a reverse palindrome s + rc(s)
  READS  260 reads of 100 .. 300 bases in 13 families (identities from ~0.5 to 1.0)
  RC     the reverse complements of READS, as points of their own
  BIG    two related records of 1,100 bases (more than one block of 1,024 rows), and BIGRC
"""
import json
import os
import subprocess

import numpy as np
import pytest

import fixtures
import meshclust_amd as M
import nw_trace_cases as T

pytestmark = pytest.mark.gpu

LENS = (1, 15, 16, 17, 31, 33, 63, 64, 65, 1000)
N_LAY = 16 * len(LENS)
G, E, P = N_LAY, N_LAY + 1, N_LAY + 2
R0, N_READS = N_LAY + 3, 260
RC0 = R0 + N_READS
BIG0 = RC0 + N_READS  # BIG0, BIG0 + 1; their reverse complements BIG0 + 2, BIG0 + 3
N_POINTS = BIG0 + 4
ASSIGN_BIN = os.path.join(os.path.dirname(M.BIN), "meshclust-assign")
_LETTER = {ord("A"): ord("T"), ord("T"): ord("A"), ord("C"): ord("G"), ord("G"): ord("C")}


def np_minus(x):
    """The minus-strand string in numpy: reversed; d <= 3 -> 3 - d, A <-> T, C <-> G, the rest stays."""
    x = np.asarray(x, np.uint8)[::-1]
    out = x.copy()
    out[x <= 3] = 3 - x[x <= 3]
    for a, b in _LETTER.items():
        out[x == a] = b
    return out


def mutate(rng, s, rate):
    s = s.copy()
    hit = rng.random(len(s)) < rate
    s[hit] = (s[hit] + rng.integers(1, 4, int(hit.sum()))) % 4
    drop = rng.random(len(s)) < rate / 4  # a few deletions, so that gaps open
    return s[~drop].astype(np.uint8)


@pytest.fixture(scope="module")
def points():
    rng = np.random.default_rng(11)
    codes, segs = [], []
    for _ in range(16):
        for n in LENS:
            codes.append(rng.integers(0, 4, n).astype(np.uint8))
            segs.append([[0, n - 1]])
    a, b = rng.integers(0, 4, 70).astype(np.uint8), rng.integers(0, 4, 45).astype(np.uint8)
    codes.append(np.concatenate([a, np.full(6, ord("N"), np.uint8), b]))  # G
    segs.append([[0, 69], [76, 120]])
    codes.append(np.frombuffer(b"ACGTNNACCGGTTAGCATNACGTTGCAAGGCT", np.uint8).copy())  # E: raw letters
    segs.append([])
    s = rng.integers(0, 4, 150).astype(np.uint8)
    codes.append(np.concatenate([s, 3 - s[::-1]]).astype(np.uint8))  # P
    segs.append([[0, 299]])
    reads = []
    for fam in range(13):
        t = rng.integers(0, 4, int(rng.integers(140, 290))).astype(np.uint8)
        for i in range(20):
            r = mutate(rng, t, 0.01 + 0.012 * i)
            r = r[:max(100, min(300, len(r)))]
            reads.append(r)
    assert len(reads) == N_READS and all(100 <= len(r) <= 300 for r in reads)
    for r in reads:
        codes.append(r)
        segs.append([[0, len(r) - 1]])
    for r in reads:
        codes.append((3 - r[::-1]).astype(np.uint8))
        segs.append([[0, len(r) - 1]])
    big = rng.integers(0, 4, 1100).astype(np.uint8)
    big2 = mutate(rng, np.concatenate([big, rng.integers(0, 4, 40).astype(np.uint8)]), 0.05)[:1100]
    assert len(big2) == 1100
    for x in (big, big2, 3 - big[::-1], 3 - big2[::-1]):
        codes.append(np.asarray(x, np.uint8))
        segs.append([[0, 1099]])
    assert len(codes) == N_POINTS
    return codes, segs


@pytest.fixture(scope="module")
def eng(built):
    e = M.Engine(0)
    yield e
    e.close()


_state = {}


def load(eng, points):
    if _state.get("loaded") is not eng:
        codes, segs = points
        lens = [len(c) for c in codes]
        seq_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        seg = np.array([v for s in segs for pair in s for v in pair], np.int32)
        seg_off = np.concatenate([[0], np.cumsum([len(s) for s in segs])]).astype(np.uint64)
        eng.load_sequences(np.concatenate(codes), seq_off, seg, seg_off)
        _state.clear()
        _state["loaded"] = eng
        _state["seq_off"] = seq_off
    return _state["seq_off"]


def rcpoint(ids):
    """The point that holds the reverse complement of each point (READS, RC, BIG only)."""
    ids = np.asarray(ids, np.int64)
    out = np.full(len(ids), -1, np.int64)
    for lo, n, to in ((R0, N_READS, RC0), (RC0, N_READS, R0), (BIG0, 2, BIG0 + 2), (BIG0 + 2, 2, BIG0)):
        m = (ids >= lo) & (ids < lo + n)
        out[m] = ids[m] - lo + to
    assert (out >= 0).all()
    return out.astype(np.uint32)


# ---------------------------------------------------------------- 1. the strings
def test_revcomp_sequences_equal_numpy(eng, points, monkeypatch):
    monkeypatch.delenv("MC_IDENT_BYTES", raising=False)
    codes, _ = points
    seq_off = load(eng, points)
    for j, n in enumerate(LENS):  # every length at every alignment of its source bytes
        starts = {int(seq_off[p * len(LENS) + j]) % 16 for p in range(16)}
        assert starts == set(range(16)), (n, starts)
    ids = np.concatenate([np.arange(N_LAY), [G, E, P], [R0, RC0, BIG0], [5, G, 5, E]]).astype(np.uint32)
    got, off = eng.revcomp_sequences(ids)
    want_off = np.concatenate([[0], np.cumsum([len(codes[i]) for i in ids])]).astype(np.uint64)
    assert off.dtype == np.uint64 and np.array_equal(off, want_off)  # no padding at the ABI
    assert got.dtype == np.uint8 and len(got) == int(want_off[-1])
    for r, i in enumerate(ids):
        assert np.array_equal(got[int(off[r]):int(off[r + 1])], np_minus(codes[i])), (r, int(i), len(codes[i]))
    piece = {r: got[int(off[r]):int(off[r + 1])] for r in range(len(ids))}
    n = len(ids)
    assert np.array_equal(piece[n - 4], piece[n - 2]) and np.array_equal(piece[n - 4], piece[5])  # an id given twice
    assert np.array_equal(piece[N_LAY + 2], codes[P])  # the palindrome is its own minus strand
    assert np.array_equal(piece[N_LAY + 3], codes[RC0]) and np.array_equal(piece[N_LAY + 4], codes[R0])
    e = piece[N_LAY + 1]
    assert bytes(e) == b"AGCCTTGCAACGTNATGCTAACCGGTNNACGT"  # raw letters: complemented, N kept
    g = piece[N_LAY]
    assert (g[45:51] == ord("N")).all() and (g[:45] <= 3).all() and (g[51:] <= 3).all()
    got0, off0 = eng.revcomp_sequences([])
    assert len(got0) == 0 and list(off0) == [0]
    # batches that end by the cap on the strings' bytes (host/pairbatch.hpp's rule restated): the same bytes
    lens = [len(x) for x in codes]
    nbytes = T.ident_bytes(lens, ids)
    ends = T.batch_ends(lens, ids, None, np.ones(len(ids), np.uint8), 1 << 20, nbytes)
    assert sum(1 for _, why in ends if why == "bytes") >= 2 and ends[-1][0] - ends[-2][0] >= 4  # (the repeated ids in one batch)
    monkeypatch.setenv("MC_IDENT_BYTES", str(nbytes))
    got2, off2 = eng.revcomp_sequences(ids)
    assert np.array_equal(got2, got) and np.array_equal(off2, off)


# ---------------------------------------------------------------- 2. no minus pair
def pair_lists(rng):
    """name -> (a, b, a_minus): point ids of READS / BIG."""
    reads = np.arange(R0, R0 + N_READS)
    out = {}
    out["m1"] = (np.array([R0 + 7]), np.array([R0 + 3]), np.array([1]))
    a = rng.choice(reads, 65)
    out["m65"] = (a, R0 + (a - R0) // 20 * 20 + rng.integers(0, 20, 65), rng.integers(0, 2, 65))  # b: of a's family
    a = rng.choice(reads, 1100)
    b = rng.choice(reads, 1100)
    out["m1100_mixed"] = (a, b, rng.integers(0, 2, 1100))
    out["m1100_minus"] = (a, b, np.ones(1100, np.int64))  # 1,100 minus pairs in one launch: the throughput form
    # a 1,100 x 1,100 pair on either strand inside a small batch: a chained row block
    a = np.concatenate([rng.choice(reads, 5), [BIG0, BIG0], rng.choice(reads, 5)])
    b = np.concatenate([rng.choice(reads, 5), [BIG0 + 1, BIG0 + 1], rng.choice(reads, 5)])
    out["big"] = (a, b, np.array([0, 1, 1, 0, 1, 1, 0, 0, 1, 0, 1, 1]))
    # one query on both strands and in many pairs (20 in a row: several batches of 7 share it)
    q = R0 + 41
    a = np.concatenate([[q] * 20, rng.choice(reads, 6), [q] * 4])
    b = np.concatenate([np.arange(R0 + 40, R0 + 60), rng.choice(reads, 6), [R0 + 44, R0 + 45, R0 + 44, R0 + 45]])
    out["repeat"] = (a, b, np.concatenate([np.arange(20) % 3 != 0, rng.integers(0, 2, 6), [1, 1, 0, 0]]))
    return {k: (np.asarray(x).astype(np.uint32), np.asarray(y).astype(np.uint32), np.asarray(z).astype(np.uint8))
            for k, (x, y, z) in out.items()}


@pytest.fixture(scope="module")
def lists(eng, points):
    """The pair lists and, computed once, what mc_nw_identity gives for them."""
    load(eng, points)
    pl = pair_lists(np.random.default_rng(5))
    ref = {}
    for name, (a, b, am) in pl.items():
        a1 = np.where(am != 0, rcpoint(a), a).astype(np.uint32)
        ref[name] = (eng.nw_identity(a1, b), eng.nw_identity(a, b))
    return pl, ref


def same(x, y):
    return all(u.dtype == v.dtype and np.array_equal(u, v) for u, v in zip(x, y)) and len(x) == len(y) == 3


@pytest.mark.parametrize("batch", [None, "7"], ids=["one_batch", "batch7"])
def test_no_minus_pair_is_nw_identity(eng, points, lists, batch, monkeypatch):
    load(eng, points)
    monkeypatch.delenv("MC_IDENT_BYTES", raising=False)
    if batch:
        monkeypatch.setenv("MC_IDENT_BATCH", batch)
    else:
        monkeypatch.delenv("MC_IDENT_BATCH", raising=False)
    pl, ref = lists
    for name, (a, b, _) in pl.items():
        plus = ref[name][1]
        assert same(eng.nw_identity_strands(a, b, None), plus), name
        assert same(eng.nw_identity_strands(a, b, np.zeros(len(a), np.uint8)), plus), name


# ---------------------------------------------------------------- 3. minus and mixed batches
@pytest.mark.parametrize("batch", [None, "7", "bytes"], ids=["one_batch", "batch7", "bytes"])
def test_minus_pairs_align_the_reverse_complemented_read(eng, points, lists, batch, monkeypatch):
    load(eng, points)
    for var in ("MC_IDENT_BATCH", "MC_IDENT_BYTES"):
        monkeypatch.delenv(var, raising=False)
    pl, ref = lists
    if batch == "bytes":  # batches that end by the cap on the strings' bytes (host/pairbatch.hpp's rule restated)
        lens = [len(x) for x in points[0]]
        nbytes = T.ident_bytes(lens, np.concatenate([a[am != 0] for a, _, am in pl.values()]))
        for name in ("m65", "m1100_mixed", "m1100_minus"):
            a, b, am = pl[name]
            assert sum(1 for _, why in T.batch_ends(lens, a, b, am, 1 << 20, nbytes) if why == "bytes") >= 2, name
        monkeypatch.setenv("MC_IDENT_BYTES", str(nbytes))
    elif batch:
        monkeypatch.setenv("MC_IDENT_BATCH", batch)
    assert set(pl) == {"m1", "m65", "m1100_mixed", "m1100_minus", "big", "repeat"}
    for name, (a, b, am) in pl.items():
        want, plus = ref[name]
        got = eng.nw_identity_strands(a, b, am)
        assert same(got, want), name
        if len(a) > 1:  # (the check can fail: the strand changes the result)
            assert not np.array_equal(want[0], plus[0]), name
    assert (ref["big"][0][1][[5, 6]] >= 1100).all()  # alignment lengths of the 1,100-base pair, either strand
    a, b, am = pl["repeat"]
    assert (a[:20] == a[0]).all() and 0 < am[:20].sum() < 20  # one query, both strands, across batches of 7
    ident = ref["m1100_mixed"][0][0]
    assert ident.min() < 0.7 and ident.max() > 0.8  # unrelated and related pairs


def test_identity_strands_errors(eng, points):
    load(eng, points)
    ident, ln, ids = eng.nw_identity_strands([], [], [])  # m = 0
    assert len(ident) == 0
    for a, b in (([N_POINTS], [0]), ([0], [N_POINTS])):
        with pytest.raises(M.MCError) as e:
            eng.nw_identity_strands(a, b, [1])
        assert e.value.code == M.ERR_ARG
    with pytest.raises(M.MCError) as e:
        eng.revcomp_sequences([N_POINTS])
    assert e.value.code == M.ERR_ARG
    fresh = M.Engine(0)  # no sequences loaded
    try:
        for call in (lambda: fresh.nw_identity_strands([0], [0], [1]), lambda: fresh.revcomp_sequences([0])):
            with pytest.raises(M.MCError) as e:
                call()
            assert e.value.code == 3  # MC_ERR_STATE
    finally:
        fresh.close()
    t0 = eng.timers(reset=True)
    eng.nw_identity_strands([R0], [R0 + 1], [1])
    t = eng.timers()
    assert t["layout"][1] == 1 and t["nw"][1] >= 1 and t0 is not None  # the kernel is timed as layout, NW as nw


# ---------------------------------------------------------------- 4 .. 7. end to end
_RC = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def read_fasta(path):
    recs = []
    with open(path, "rb") as f:
        for ln in f.read().splitlines():
            if ln.startswith(b">"):
                recs.append([ln, b""])
            else:
                recs[-1][1] += ln
    return recs


def write_fasta(path, recs):
    with open(path, "wb") as f:
        for h, s in recs:
            f.write(h + b"\n" + s + b"\n")


def rows(path):
    return [ln.split("\t") for ln in open(path).read().splitlines()]


class E2E:
    """The saved a1k clustering, the read files, and every run of the tool made once."""

    def __init__(self, tmp):
        self.tmp = tmp
        fa, flags = fixtures.e2e_input("a1k", tmp)
        self.model, self.cen = tmp / "a1k.model", tmp / "a1k.centres.fa"
        r = subprocess.run([M.BIN, fa] + flags + ["--output", str(tmp / "a1k.clstr"), "--quiet", "--save-model", str(self.model),
                                                  "--save-centres", str(self.cen)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        self.plain_fa = fa
        recs = read_fasta(fa)
        centres = {h for h, _ in read_fasta(self.cen)}
        # F: every second read reverse-complemented; R: its reverse complement; NC: F without the
        # centres' own reads (a centre aligns to itself at identity 1)
        f_recs = [(h, s.translate(_RC)[::-1] if i % 2 else s) for i, (h, s) in enumerate(recs)]
        self.F, self.R, self.NC = tmp / "F.fa", tmp / "R.fa", tmp / "NC.fa"
        write_fasta(self.F, f_recs)
        write_fasta(self.R, [(h, s.translate(_RC)[::-1]) for h, s in f_recs])
        write_fasta(self.NC, [(h, s) for h, s in f_recs if h not in centres])
        assert 0 < len(centres) < len(recs)
        self.done = {}

    def run(self, name, reads, extra=(), env=None, top=False):
        if name not in self.done:
            tsv, hits, stats, rest = (self.tmp / (name + ext) for ext in (".tsv", ".hits", ".json", ".rest.fa"))
            args = (["--top", "3", "--hits", str(hits)] if top else []) + ["--stats-json", str(stats), "--unassigned", str(rest)]
            e = dict(os.environ, **(env or {}))
            for var in ("MC_ASSIGN_FORM", "MC_ASSIGN_TILE", "MC_ASSIGN_PAIRS", "MC_IDENT_BATCH", "MC_IDENT_BYTES"):
                if not env or var not in env:
                    e.pop(var, None)
            r = subprocess.run([ASSIGN_BIN, "--model", str(self.model), "--centres", str(self.cen), str(reads), "--output",
                                str(tsv), "--quiet"] + args + list(extra), capture_output=True, text=True, timeout=300, env=e)
            assert r.returncode == 0, r.stderr[-3000:]
            self.done[name] = (tsv, hits, json.loads(stats.read_text()), rest)
        return self.done[name]


@pytest.fixture(scope="module")
def e2e(built, tmp_path_factory):
    return E2E(tmp_path_factory.mktemp("ident"))


def test_cli_identity_column(eng, e2e):
    """One strand, on the file with every second read reverse-complemented (those reads are mostly
    unassigned on one strand): the TSV gains a last column and changes in nothing else; the column
    is mc_nw_identity(read, centre) on the parsed records, * for an unassigned read."""
    plain_tsv, _, plain_st, _ = e2e.run("plain", str(e2e.F))
    tsv, _, st, _ = e2e.run("ident", str(e2e.F), ["--identity"])
    got = rows(tsv)
    assert all(len(x) == 6 for x in got)
    assert "".join("\t".join(x[:5]) + "\n" for x in got).encode() == plain_tsv.read_bytes()
    cents = M.Dataset([str(e2e.cen)], threads=2).records()
    reads = M.Dataset([str(e2e.F)], threads=2).records()
    allp = cents + reads
    lens = [len(c) for _, c, _ in allp]
    seq_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    seg = np.array([v for _, _, s in allp for pair in s for v in pair], np.int32)
    seg_off = np.concatenate([[0], np.cumsum([len(s) for _, _, s in allp])]).astype(np.uint64)
    eng.load_sequences(np.concatenate([c for _, c, _ in allp]), seq_off, seg, seg_off)
    _state.clear()  # (the context now holds other sequences)
    C = len(cents)
    q = np.array([i for i, x in enumerate(got) if x[2] != "-1"], np.uint32)
    assert 0 < len(q) and any(x[2] == "-1" for x in got)  # assigned and unassigned reads
    j = np.array([int(got[i][2]) for i in q], np.uint32)
    ident, _, _ = eng.nw_identity(q + C, j)
    cells = 0
    for n, i in enumerate(q):
        assert got[i][5] == "%.17g" % ident[n], (int(i), got[i])
        cells += lens[C + i] * lens[j[n]]
    assert all(x[5] == "*" for x in got if x[2] == "-1")
    assert len({x[5] for x in got}) > 10  # (identities, not a constant)
    # the stats: the new keys only with the option, the rest unchanged
    new = {"identity_pairs", "identity_cells", "rejected"}
    assert not (new & set(plain_st)) and "identity" not in plain_st["phases_ms"]
    assert st["identity_pairs"] == len(q) and st["identity_cells"] == cells and st["rejected"] == 0
    assert "identity" in st["phases_ms"] and {k: v for k, v in st.items() if k not in new and k not in ("phases_ms", "device_us")} == \
        {k: v for k, v in plain_st.items() if k not in ("phases_ms", "device_us")}
    # the same job in process (mcl_assign_identity)
    lib_tsv = e2e.tmp / "lib.tsv"
    st2 = M.assign_files(eng, str(e2e.model), str(e2e.cen), str(e2e.F), str(lib_tsv), threads=2, identity=True)
    assert lib_tsv.read_bytes() == tsv.read_bytes() and st2["identity_pairs"] == len(q)


def test_cli_pair_list_path_reports_the_same_identities(e2e):
    tsv, _, st, _ = e2e.run("ident", str(e2e.F), ["--identity"])
    p_tsv, _, p_st, _ = e2e.run("ident_pairs", str(e2e.F), ["--identity"], env={"MC_ASSIGN_PAIRS": "1"})
    assert st["path"] == "device" and p_st["path"] == "pairs"
    assert p_tsv.read_bytes() == tsv.read_bytes()
    assert p_st["identity_pairs"] == st["identity_pairs"] and p_st["identity_cells"] == st["identity_cells"]


def both_run(e2e, reads=None, name="both"):
    return e2e.run(name, reads or e2e.F, ["--both-strands", "--identity"], top=True)


def test_cli_both_strands_top_identity_is_the_merge_of_the_strands(e2e):
    """The file and its reverse complement, each on one strand with --identity, merged by the
    documented rules (the TSV: minus wins only with a strictly larger combo 0; the hits: combo 0
    descending, plus before minus, index ascending), identities included."""
    f_tsv, f_hits, _, _ = e2e.run("F1", e2e.F, ["--identity"], top=True)
    r_tsv, r_hits, _, _ = e2e.run("R1", e2e.R, ["--identity"], top=True)
    b_tsv, b_hits, b_st, _ = both_run(e2e)
    want = []
    for p, m in zip(rows(f_tsv), rows(r_tsv)):
        assert p[0] == m[0] and len(p) == 6
        minus = m[2] != "-1" and (p[2] == "-1" or float(m[3]) > float(p[3]))
        w = m if minus else p
        want.append([w[0], w[1], w[2], w[3], str(int(p[4]) + int(m[4])), "*" if w[2] == "-1" else "-" if minus else "+", w[5]])
    got = rows(b_tsv)
    assert got == want
    assert any(x[5] == "-" for x in got) and any(x[5] == "+" for x in got)
    merged = {}
    for sign, path in (("+", f_hits), ("-", r_hits)):
        for x in rows(path):
            assert len(x) == 6
            merged.setdefault(x[0], []).append((-float(x[4]), sign != "+", int(x[3]), x, sign))
    want = []
    for x in got:  # reads in input order
        for rank, (_, _, _, h, sign) in enumerate(sorted(merged.get(x[0], []), key=lambda t: t[:3])[:3]):
            want.append([x[0], str(rank + 1), h[2], h[3], h[4], sign, h[5]])
    hits = rows(b_hits)
    assert hits == want
    # rank 1 is the TSV's row, identity included; one alignment per listed hit
    first = {h[0]: h for h in hits if h[1] == "1"}
    for x in got:
        if x[2] != "-1":
            assert first[x[0]][2:] == [x[1], x[2], x[3], x[5], x[6]]
    assert b_st["identity_pairs"] == len(hits) == b_st["hits"] and b_st["rejected"] == 0


def test_cli_min_identity(e2e):
    base_tsv, base_hits, base_st, _ = both_run(e2e, e2e.NC, "nc")
    base, hits = rows(base_tsv), rows(base_hits)
    by_read = {}
    for h in hits:
        by_read.setdefault(h[0], []).append(h)
    ids = [float(h[6]) for h in hits]
    assert max(ids) < 1.0  # no read is a centre's own
    opts = ["--both-strands", "--identity"]
    # X = 0: the rows of --identity
    z_tsv, z_hits, z_st, _ = e2e.run("nc_x0", e2e.NC, opts + ["--min-identity", "0"], top=True)
    assert z_tsv.read_bytes() == base_tsv.read_bytes() and z_hits.read_bytes() == base_hits.read_bytes()
    assert z_st["rejected"] == 0 and z_st["assigned"] == base_st["assigned"]
    # X above every identity: nothing is confirmed
    hi = (max(ids) + 1.0) / 2
    h_tsv, h_hits, h_st, h_rest = e2e.run("nc_hi", e2e.NC, opts + ["--min-identity", repr(hi)], top=True)
    assert [x[:4] + x[5:] for x in rows(h_tsv)] == [[x[0], "*", "-1", "-1", "*", "*"] for x in base]
    assert [x[4] for x in rows(h_tsv)] == [x[4] for x in base]  # n_similar is the classifier's
    assert h_st["assigned"] == 0 and h_st["rejected"] == base_st["assigned"] > 0 and h_st["assigned_minus"] == 0
    assert h_rest.read_bytes() == e2e.NC.read_bytes() and h_hits.read_bytes() == base_hits.read_bytes()
    # a middle X: each row from the hits of the --identity run, the first hit at or above X
    rank1 = sorted(float(h[6]) for h in hits if h[1] == "1")
    mid = rank1[len(rank1) // 2]
    m_tsv, m_hits, m_st, m_rest = e2e.run("nc_mid", e2e.NC, opts + ["--min-identity", repr(mid)], top=True)
    want, rest, kinds = [], [], set()
    for x in base:
        pick = next((h for h in by_read.get(x[0], []) if float(h[6]) >= mid), None)
        if pick is None:
            want.append([x[0], "*", "-1", "-1", x[4], "*", "*"])
            rest.append(x[0])
            kinds.add("rejected" if x[0] in by_read else "unassigned")
        else:
            want.append([x[0], pick[2], pick[3], pick[4], x[4], pick[5], pick[6]])
            kinds.add("rank" + pick[1])
    assert rows(m_tsv) == want
    assert {"rejected", "rank1"} <= kinds, kinds  # both outcomes occur
    assert m_hits.read_bytes() == base_hits.read_bytes()
    assert [h[1:].decode() for h, _ in read_fasta(m_rest)] == rest
    n_rej = sum(1 for x in base if x[0] in by_read and x[0] in set(rest))
    assert m_st["rejected"] == n_rej and m_st["assigned"] == len(base) - len(rest)
    assert m_st["assigned_minus"] == sum(1 for x in want if x[5] == "-")
    print("min-identity outcomes:", sorted(kinds), "rejected", n_rej, "of", len(base))
