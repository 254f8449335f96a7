"""mc_assign / meshclust-assign: placing reads into an existing clustering on the GPU.

Every output is compared with ==.  The expectation of the ABI tests is mc_classify_pairs over
every (query, centre) pair with the argmax and the count done in numpy (largest combo 0 among
the similar centres, lowest index on ties); one case is also checked against the CPU oracle,
the independent checker.  End to end, bin/meshclust saves its model and centres,
bin/meshclust-assign assigns the same reads, and the TSV is recomputed from the saved files
with the CPU oracle alone.
"""
import gzip
import os
import subprocess

import numpy as np
import pytest

import fixtures
import meshclust_amd as M
import oracle_lib as O

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
QUERIES = np.arange(100, 361, dtype=np.uint32)  # 261 reads: 4 full waves + 5, one more than a block
SET_A = np.arange(23, dtype=np.uint32)
SET_B = np.array([0, 1, 2, 3, 4, 5, 6, 3], np.uint32)  # id 3 twice: exact ties
ASSIGN_BIN = os.path.join(os.path.dirname(M.BIN), "meshclust-assign")


@pytest.fixture(scope="module")
def eng(built):
    e = M.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def a1k_data():
    g = np.load(fixtures.golden("train_a1k.npz"))
    recs = fixtures.synth_records(*fixtures.manifest()["e2e"]["a1k"]["generator"])
    lens = np.array([L for _, _, L in recs], np.uint64)
    return g, recs, lens


_state = {}


def setup(eng, a1k_data, k, width, cls=None, label="custom"):
    """The a1k reads with k-mer histograms of the given k / width and a classifier (default: the
    golden one).  Sequences are uploaded once; histograms rebuilt only when (k, width) changes."""
    g, recs, lens = a1k_data
    if _state.get("eng") is not eng:
        _state.clear()
        _state["eng"] = eng
        codes = np.concatenate([c for _, c, _ in recs]).astype(np.uint8)
        seq_off = np.cumsum([0] + [int(L) for _, _, L in recs]).astype(np.uint64)
        seg = np.array([[0, L - 1] for _, _, L in recs], np.int32).reshape(-1)
        eng.load_sequences(codes, seq_off, seg, np.arange(len(recs) + 1, dtype=np.uint64))
    if _state.get("kw") != (k, width):
        eng.kmer_max(k)
        eng.kmer_build(k, width)
        _state["kw"] = (k, width)
        _state["exp"] = {}
    eng.set_classifier(cls if cls is not None else O.classifier_from_golden(g))
    _state["cls"] = "golden" if cls is None else label  # (keys the cached expectations)
    return g, recs, lens


def gate_mask(lens, centres, queries, sim):
    if sim <= 0:
        return np.ones((len(queries), len(centres)), bool)
    lc = lens[centres].astype(np.float64)
    lo = np.array([int(x * sim) for x in lc], np.uint64)  # (uint64_t)(len * sim), in double
    hi = np.array([int(x / sim) for x in lc], np.uint64)
    lq = lens[queries].astype(np.uint64)
    return (lo[None, :] <= lq[:, None]) & (lq[:, None] <= hi[None, :])


def reduce_pairs(simf, c0, gate):
    """(best, best_val, n_similar) from the per-pair decisions: largest combo 0 among the gated
    similar centres, the lowest index on ties."""
    ok = simf & gate
    nsim = ok.sum(axis=1).astype(np.uint32)
    best = np.where(ok, c0, -np.inf).argmax(axis=1)  # (argmax: the first maximum)
    val = c0[np.arange(len(best)), best]
    none = nsim == 0
    return np.where(none, NONE, best).astype(np.uint32), np.where(none, -1.0, val), nsim


def expect(eng, lens, centres, queries, sim=0.0):
    """Expectation from mc_classify_pairs; cached per histogram configuration (never modified)."""
    key = (_state["cls"], bytes(centres), bytes(queries), sim)
    cache = _state["exp"]
    if key not in cache:
        Cn, Mq = len(centres), len(queries)
        simf, c0, _ = eng.classify_pairs(np.repeat(queries, Cn), np.tile(centres, Mq))
        simf, c0 = simf.reshape(Mq, Cn).astype(bool), c0.reshape(Mq, Cn)
        gate = gate_mask(lens, centres, queries, sim)
        cache[key] = reduce_pairs(simf, c0, gate) + (int(gate.sum()), simf & gate, c0)
    return cache[key]


def check(got, want):
    best, val, nsim, stats = got
    assert np.array_equal(best, want[0])
    assert np.array_equal(val, want[1])
    assert np.array_equal(nsim, want[2])
    assert int(stats[0]) == want[3]


@pytest.mark.parametrize("tile", ["7", None], ids=["tile7", "tile_default"])
def test_assign_equals_classify_pairs(eng, a1k_data, tile, monkeypatch):
    """Both centre sets, several ragged LDS tiles and the default tile; the expectation must hold
    assigned and unassigned queries, several similar centres, and exact ties (to the lowest index)."""
    g, recs, lens = setup(eng, a1k_data, int(a1k_data[0]["k"]), 1)
    if tile:
        monkeypatch.setenv("MC_ASSIGN_TILE", tile)
    else:
        monkeypatch.delenv("MC_ASSIGN_TILE", raising=False)
    seen = dict(assigned=False, unassigned=False, multi=False, tie=False)
    for centres in (SET_A, SET_B):
        want = expect(eng, lens, centres, QUERIES)
        check(eng.assign(centres, QUERIES), want)
        ok, c0 = want[4], want[5]
        top = np.where(ok, c0, -np.inf).max(axis=1)
        ties = ((np.where(ok, c0, -np.inf) == top[:, None]) & ok).sum(axis=1)
        seen["assigned"] |= bool((want[2] > 0).any())
        seen["unassigned"] |= bool((want[2] == 0).any())
        seen["multi"] |= bool((want[2] >= 2).any())
        seen["tie"] |= bool((ties >= 2).any())
    assert all(seen.values()), seen
    best = expect(eng, lens, SET_B, QUERIES)[0]
    assert (best == 3).any() and not (best == 7).any()  # the repeated id resolves to index 3


@pytest.mark.parametrize("m", [1, 63, 64, 65])
def test_assign_query_counts(eng, a1k_data, m):
    g, recs, lens = setup(eng, a1k_data, int(a1k_data[0]["k"]), 1)
    q = QUERIES[:m]
    check(eng.assign(SET_A, q), expect(eng, lens, SET_A, q))
    one = SET_A[3:4]
    check(eng.assign(one, q), expect(eng, lens, one, q))  # C = 1


def test_assign_equals_cpu_oracle(eng, a1k_data):
    """The first case against O.raw + O.classify (no device arithmetic in the expectation)."""
    g, recs, lens = setup(eng, a1k_data, int(a1k_data[0]["k"]), 1)
    cls = O.classifier_from_golden(g)
    h, _ = eng.histograms()
    flags = [int(f) for f in g["lookup"]]
    simf = np.zeros((len(QUERIES), len(SET_A)), bool)
    c0 = np.zeros((len(QUERIES), len(SET_A)))
    for a, q in enumerate(QUERIES):
        for b, c in enumerate(SET_A):
            raw = [O.raw(f, h[q], h[c], int(lens[q]), int(lens[c])) for f in flags]
            d, _, v = O.classify(cls, raw)
            simf[a, b], c0[a, b] = d != 0, v
    want = reduce_pairs(simf, c0, np.ones_like(simf))
    best, val, nsim, stats = eng.assign(SET_A, QUERIES)
    assert np.array_equal(best, want[0]) and np.array_equal(val, want[1]) and np.array_equal(nsim, want[2])
    assert (want[2] > 0).any() and (want[2] >= 2).any()
    assert int(stats[0]) == simf.size


def test_assign_undecided_pairs_fall_back(eng, a1k_data):
    """The intercept moved so that one pair's GLM sum lands on the decision threshold (within
    rounding): classify_small's margin cannot decide it, the kernel scores it with classify_std on
    the spot (stats[1] counts it), and every output still equals mc_classify_pairs."""
    g, recs, lens = setup(eng, a1k_data, int(a1k_data[0]["k"]), 1)
    _, _, sums = eng.classify_pairs(np.repeat(QUERIES, len(SET_A)), np.tile(SET_A, len(QUERIES)))
    cls = O.classifier_from_golden(g)
    cls.weights[0] -= float(sums[len(SET_A) * 17 + 5])  # pair (QUERIES[17], SET_A[5]): new sum ~ 0
    setup(eng, a1k_data, int(g["k"]), 1, cls, label="on_threshold")
    want = expect(eng, lens, SET_A, QUERIES)
    got = eng.assign(SET_A, QUERIES)
    check(got, want)
    assert int(got[3][1]) >= 1  # at least that pair was left to classify_std
    assert (want[2] > 0).any() and (want[2] < len(SET_A)).any()


def two_feature_classifier():
    """MANHATTAN and INTERSECTION, one product combo: not the trainer's layout (classify_raw)."""
    c = O.Classifier()
    c.n_single = 2
    c.lookup[0], c.lookup[1] = M.FEAT_MANHATTAN, M.FEAT_INTERSECTION
    c.is_sim[0], c.is_sim[1] = 0, 1
    c.mins[0], c.maxs[0] = 0.0, 400.0
    c.mins[1], c.maxs[1] = 0.5, 1.0
    c.n_combo = 1
    c.combo_kind[0] = M.COMBO_SELF
    c.combo_len[0] = 2
    c.combo_idx[0][0], c.combo_idx[0][1] = 0, 1
    c.weights[0], c.weights[1] = -2.0, 5.0
    return c


@pytest.mark.parametrize("case", ["general_k3", "k6_u8", "k4_u16", "k2", "two_feature"])
def test_assign_forms(eng, a1k_data, case, monkeypatch):
    """The 16-lanes-per-query kernel on the short form's input (equal to it), rows wider than 16
    chunks, 16-bit bins, a short row of one chunk, and a classifier outside the trainer's layout."""
    k, width, cls = {"general_k3": (3, 1, None), "k6_u8": (6, 1, None), "k4_u16": (4, 2, None), "k2": (2, 1, None),
                     "two_feature": (3, 1, two_feature_classifier())}[case]
    g, recs, lens = setup(eng, a1k_data, k, width, cls)
    monkeypatch.delenv("MC_ASSIGN_TILE", raising=False)
    monkeypatch.delenv("MC_ASSIGN_FORM", raising=False)
    for centres in (SET_A, SET_B):
        want = expect(eng, lens, centres, QUERIES)
        if case == "general_k3":
            short = eng.assign(centres, QUERIES)
            monkeypatch.setenv("MC_ASSIGN_FORM", "general")
            gen = eng.assign(centres, QUERIES)
            monkeypatch.delenv("MC_ASSIGN_FORM")
            for x, y in zip(short[:3], gen[:3]):
                assert np.array_equal(x, y)
            check(gen, want)
        else:
            check(eng.assign(centres, QUERIES), want)
            monkeypatch.setenv("MC_ASSIGN_TILE", "5")
            check(eng.assign(centres, QUERIES), want)
            monkeypatch.delenv("MC_ASSIGN_TILE")
    if case == "two_feature":
        ok = expect(eng, lens, SET_A, QUERIES)[4]
        assert 0 < ok.sum() < ok.size  # the hand-made weights call some pairs similar and some not


@pytest.mark.parametrize("form", [None, "general"], ids=["short", "general"])
def test_assign_length_gate(eng, a1k_data, form, monkeypatch):
    g, recs, lens = setup(eng, a1k_data, int(a1k_data[0]["k"]), 1)
    if form:
        monkeypatch.setenv("MC_ASSIGN_FORM", form)
    else:
        monkeypatch.delenv("MC_ASSIGN_FORM", raising=False)
    assert lens.min() == 488 and lens.max() == 515
    gated = expect(eng, lens, SET_A, QUERIES, 0.99)
    assert gated[3] < len(QUERIES) * len(SET_A)  # sim = 0.99 excludes some pairs
    assert not np.array_equal(gated[2], expect(eng, lens, SET_A, QUERIES)[2])
    check(eng.assign(SET_A, QUERIES, 0.99), gated)
    check(eng.assign(SET_A, QUERIES, 0.0), expect(eng, lens, SET_A, QUERIES))  # sim = 0: no gate
    monkeypatch.setenv("MC_ASSIGN_TILE", "4")
    check(eng.assign(SET_A, QUERIES, 0.99), gated)


def test_assign_errors(eng, a1k_data):
    g, recs, lens = setup(eng, a1k_data, int(a1k_data[0]["k"]), 1)
    with pytest.raises(M.MCError) as e:
        eng.assign(SET_A, [len(recs)])
    assert e.value.code == M.ERR_ARG
    with pytest.raises(M.MCError) as e:
        eng.assign([len(recs) + 5], QUERIES)
    assert e.value.code == M.ERR_ARG
    with pytest.raises(M.MCError) as e:
        eng.assign([], QUERIES)  # C = 0
    assert e.value.code == M.ERR_ARG
    best, val, nsim, stats = eng.assign(SET_A, [])  # M = 0
    assert len(best) == 0 and int(stats[0]) == 0
    al = O.Classifier()
    al.n_single, al.n_combo = 1, 1
    al.lookup[0], al.is_sim[0], al.mins[0], al.maxs[0] = M.FEAT_ALIGN, 1, 0.0, 1.0
    al.combo_kind[0], al.combo_len[0], al.combo_idx[0][0] = M.COMBO_SELF, 1, 0
    al.weights[0], al.weights[1] = -0.5, 1.0
    eng.set_classifier(al)
    with pytest.raises(M.MCError) as e:
        eng.assign(SET_A, QUERIES)
    assert e.value.code == M.ERR_UNSUPPORTED
    setup(eng, a1k_data, 3, 4)  # 32-bit bins
    with pytest.raises(M.MCError) as e:
        eng.assign(SET_A, QUERIES)
    assert e.value.code == M.ERR_UNSUPPORTED


# ---------------------------------------------------------------- end to end
def read_model(path):
    """The model file: 'meshclust-model 1', then key value... lines (doubles as C99 hex floats)."""
    with open(path) as f:
        lines = f.read().splitlines()
    assert lines[0] == "meshclust-model 1"
    kv = {ln.split()[0]: ln.split()[1:] for ln in lines[1:] if ln.strip()}
    c = O.Classifier()
    c.n_single = int(kv["n_single"][0])
    c.n_combo = int(kv["n_combo"][0])
    for i in range(8):
        c.lookup[i] = int(kv["lookup"][i])
        c.is_sim[i] = int(kv["is_sim"][i])
        c.mins[i] = float.fromhex(kv["mins"][i])
        c.maxs[i] = float.fromhex(kv["maxs"][i])
        c.combo_kind[i] = int(kv["combo_kind"][i])
        c.combo_len[i] = int(kv["combo_len"][i])
        for j in range(4):
            c.combo_idx[i][j] = int(kv["combo_idx"][4 * i + j])
    for i in range(9):
        c.weights[i] = float.fromhex(kv["weights"][i])
    return dict(k=int(kv["k"][0]), id=float.fromhex(kv["id"][0]), align=int(kv["align"][0]),
                centres=int(kv["centres"][0]), cls=c)


def test_cli_end_to_end(eng, tmp_path):
    fa, flags = fixtures.e2e_input("a1k", tmp_path)
    clstr, model, cen = tmp_path / "a1k.clstr", tmp_path / "a1k.model", tmp_path / "a1k.centres.fa"
    r = subprocess.run([M.BIN, fa] + flags + ["--output", str(clstr), "--quiet", "--save-model", str(model),
                                              "--save-centres", str(cen)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    with gzip.open(fixtures.golden("e2e_a1k.clstr.gz"), "rb") as f:
        assert clstr.read_bytes() == f.read()  # saving changes nothing
    outs = {}
    for name, env in (("dev", {}), ("pairs", {"MC_ASSIGN_PAIRS": "1"})):
        tsv, rest = tmp_path / (name + ".tsv"), tmp_path / (name + ".rest.fa")
        e = dict(os.environ, **env)
        e.pop("MC_ASSIGN_FORM", None)
        e.pop("MC_ASSIGN_TILE", None)
        r = subprocess.run([ASSIGN_BIN, "--model", str(model), "--centres", str(cen), fa, "--output", str(tsv),
                            "--unassigned", str(rest), "--quiet"], capture_output=True, text=True, timeout=300, env=e)
        assert r.returncode == 0, r.stderr[-3000:]
        outs[name] = (tsv.read_bytes(), rest.read_bytes())
    assert outs["dev"] == outs["pairs"]  # the device kernel and the pair-list fallback agree byte for byte
    # the same job in process (mcl_assign on an open context)
    tsv, rest = tmp_path / "lib.tsv", tmp_path / "lib.rest.fa"
    st = M.assign_files(eng, str(model), str(cen), fa, str(tsv), str(rest), threads=2)
    _state.clear()  # (the context now holds other sequences)
    assert (tsv.read_bytes(), rest.read_bytes()) == outs["dev"]
    assert st["path"] == "device" and st["reads"] == 1000 and st["assigned"] + st["unassigned"] == 1000
    # the expectation from the saved files alone, on the CPU oracle
    mdl = read_model(model)
    cents = M.Dataset([str(cen)], threads=2).records()
    reads = M.Dataset([fa], threads=2).records()
    assert mdl["align"] == 0 and mdl["centres"] == len(cents)
    k, cls = mdl["k"], mdl["cls"]
    flags_ = [int(cls.lookup[i]) for i in range(cls.n_single)]
    hc = [O.kmer_hist(c, s, k).astype(np.uint8) for _, c, s in cents]
    lines = []
    for hdr, codes, segs in reads:
        hq = O.kmer_hist(codes, segs, k).astype(np.uint8)
        best, val, n = -1, -1.0, 0
        for j, (_, cc, _) in enumerate(cents):
            lc, lq = len(cc), len(codes)
            if not (int(lc * mdl["id"]) <= lq <= int(lc / mdl["id"])):
                continue
            d, _, v = O.classify(cls, [O.raw(f, hq, hc[j], lq, lc) for f in flags_])
            if d:
                n += 1
                if best < 0 or v > val:
                    best, val = j, v
        lines.append("%s\t%s\t%d\t%s\t%d\n" % (hdr[1:], cents[best][0][1:] if best >= 0 else "*", best, "%.17g" % val, n))
    assert outs["dev"][0].decode() == "".join(lines)
    # every centre read is assigned to its own cluster
    by_hdr = {ln.split("\t")[0]: int(ln.split("\t")[2]) for ln in lines}
    for j, (hdr, _, _) in enumerate(cents):
        assert by_hdr[hdr[1:]] == j
