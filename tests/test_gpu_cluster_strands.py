"""Strand-blind clustering on the GPU: mc_kmer_max_strands / mc_kmer_build_strands /
mc_orient_pairs, the trainer's strand-blind labels, and bin/meshclust --both-strands end to end.

Every value is compared with ==.  Expectations come from code that predates the feature: the CPU
oracle's forward histograms folded by the numpy restatement (strand_cluster_cases.py), the
forward histograms (mc_get_histograms after a plain mc_kmer_build) of the doubled records
r || N x 30 || rc(r), mc_nw_identity_strands, and the planted templates of the synthetic reads.

Row points: the first 64 a1k reads, a record with an N gap (G), a record without segments (E), a
reverse palindrome s + rc(s) (P) and A x 150 || T x 150 (POLY); every record is loaded as
written, reverse-complemented and doubled.  The width contract is the caller's: a case at 8 bits
loads only the records whose canonical maximum -- by the restatement, not by the code under
test -- fits 8 bits (POLY never does; at k = 1 ten of the a1k reads, G and E do).
"""
import gzip
import os
import subprocess

import numpy as np
import pytest

import clstr
import fixtures
import meshclust_amd as M
import oracle_lib as O
import strand_cluster_cases as S

pytestmark = pytest.mark.gpu

BOTH = M.MC_STRAND_PLUS | M.MC_STRAND_MINUS
ASSIGN_BIN = os.path.join(os.path.dirname(M.BIN), "meshclust-assign")


@pytest.fixture(scope="module")
def eng(built):
    e = M.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def records():
    """[(codes, segments)]: 64 a1k reads, then G, E, P, POLY."""
    recs = fixtures.synth_records(*fixtures.manifest()["e2e"]["a1k"]["generator"])[:64]
    out = [(c.astype(np.uint8), [[0, len(c) - 1]]) for _, c, _ in recs]
    rng = np.random.default_rng(7)
    a, b = rng.integers(0, 4, 70).astype(np.uint8), rng.integers(0, 4, 45).astype(np.uint8)
    out.append((np.concatenate([a, np.full(6, S.N, np.uint8), b]), [[0, 69], [76, 120]]))  # G
    out.append((np.full(30, S.N, np.uint8), []))  # E
    s = rng.integers(0, 4, 250).astype(np.uint8)
    out.append((np.concatenate([s, 3 - s[::-1]]).astype(np.uint8), [[0, 499]]))  # P
    out.append((np.concatenate([np.zeros(150, np.uint8), np.full(150, 3, np.uint8)]), [[0, 299]]))  # POLY
    return out


G, E, P, POLY = 64, 65, 66, 67
_hist_cache = {}


def oracle_rows(records, k):
    """Forward histograms of the records and of their reverse complements (CPU oracle), int64."""
    if k not in _hist_cache:
        fwd = np.array([O.kmer_hist(c, s, k) for c, s in records]).astype(np.int64)
        rev = np.array([O.kmer_hist(*S.revcomp(c, s), k) for c, s in records]).astype(np.int64)
        _hist_cache[k] = (fwd, rev)
    return _hist_cache[k]


def load(eng, recs):
    lens = np.array([len(c) for c, _ in recs], np.uint64)
    seq_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    seg = np.array([v for _, s in recs for pair in s for v in pair], np.int32)
    seg_off = np.concatenate([[0], np.cumsum([len(s) for _, s in recs])]).astype(np.uint64)
    eng.load_sequences(np.concatenate([c for c, _ in recs]), seq_off, seg, seg_off)


def kept(records, k, width):
    """Indices of the records whose canonical row fits `width` bytes (by the restatement)."""
    fwd, _ = oracle_rows(records, k)
    return [i for i in range(len(records)) if S.canon_rows(fwd[i], k).max() < (1 << (8 * width))]


ROW_CASES = [(1, 1), (3, 1), (4, 1), (5, 1), (6, 1), (3, 2), (4, 2)]


# ---------------------------------------------------------------- 1. the canonical rows
@pytest.mark.parametrize("k,width", ROW_CASES)
def test_canonical_rows(eng, records, k, width):
    keep = kept(records, k, width)
    assert len(keep) >= 10 and E in keep and G in keep and (width == 1 or len(keep) == len(records))
    assert (POLY in keep) == (width == 2)
    recs = [records[i] for i in keep]
    n = len(recs)
    fwd, rev = (h[keep] for h in oracle_rows(records, k))
    want = S.canon_rows(fwd, k)
    assert np.array_equal(want, S.canon_rows(rev, k))  # the restatement itself is strand-blind
    dt = {1: np.uint8, 2: np.uint16}[width]
    # the doubled records' forward rows, by the code that predates the feature
    load(eng, [S.doubled(c, s) for c, s in recs])
    assert eng.kmer_max(k) == want.max()
    eng.kmer_build(k, width)
    hd, md = eng.histograms()
    assert np.array_equal(hd, want.astype(dt))
    # the records and their reverse complements
    load(eng, recs + [S.revcomp(c, s) for c, s in recs])
    assert eng.kmer_max(k) == max(fwd.max(), rev.max())
    assert eng.kmer_max_strands(k, BOTH) == want.max()
    eng.kmer_build_strands(k, width, BOTH)
    h, mag = eng.histograms()
    assert h.dtype == dt and h.shape == (2 * n, 4 ** k)
    assert np.array_equal(h[:n], want.astype(dt)) and np.array_equal(h[n:], h[:n])
    assert np.array_equal(h[:n], hd)
    assert np.array_equal(mag[:n], md) and np.array_equal(mag[n:], md)
    assert np.array_equal(mag[:n].astype(np.int64), want.sum(axis=1))
    assert np.array_equal(mag[:n].astype(np.int64), 2 * fwd.sum(axis=1) - 4 ** k)
    assert not np.array_equal(fwd[0], rev[0])  # (the check can fail)
    # strands == 1 forwards to mc_kmer_max / mc_kmer_build, and a plain build restores forward rows
    assert eng.kmer_max_strands(k, M.MC_STRAND_PLUS) == max(fwd.max(), rev.max())
    eng.kmer_build_strands(k, width, M.MC_STRAND_PLUS)
    h1, m1 = eng.histograms()
    assert np.array_equal(h1, np.concatenate([fwd, rev]).astype(dt))
    assert np.array_equal(m1.astype(np.int64), np.concatenate([fwd, rev]).sum(axis=1))
    with pytest.raises(M.MCError) as e:
        eng.orient_pairs([0], [1])
    assert e.value.code == M.ERR_STATE
    eng.kmer_build_strands(k, width, BOTH)
    assert np.array_equal(eng.histograms()[0][:n], want.astype(dt))
    eng.kmer_max(k)
    eng.kmer_build(k, width)
    h2, m2 = eng.histograms()
    assert np.array_equal(h2, h1) and np.array_equal(m2, m1)


def test_canonical_maximum_needs_the_wider_type(eng, records):
    load(eng, records + [S.revcomp(c, s) for c, s in records])
    assert eng.kmer_max(4) == 148
    assert eng.kmer_max_strands(4, BOTH) == 295
    assert eng.kmer_max_strands(4, M.MC_STRAND_PLUS) == 148


def test_strands_contract(eng, records):
    load(eng, records[:8])
    for bad in (0, 2, 4, -1):
        with pytest.raises(M.MCError) as e:
            eng.kmer_max_strands(4, bad)
        assert e.value.code == M.ERR_ARG
        with pytest.raises(M.MCError) as e:
            eng.kmer_build_strands(4, 1, bad)
        assert e.value.code == M.ERR_ARG
    for call in (lambda: eng.kmer_max_strands(8, BOTH), lambda: eng.kmer_build_strands(8, 1, BOTH),
                 lambda: eng.kmer_build_strands(4, 4, BOTH), lambda: eng.kmer_build_strands(4, 8, BOTH)):
        with pytest.raises(M.MCError) as e:
            call()
        assert e.value.code == M.ERR_UNSUPPORTED
    with pytest.raises(M.MCError) as e:
        eng.kmer_build_strands(4, 3, BOTH)
    assert e.value.code == M.ERR_ARG


# ---------------------------------------------------------------- 2. the orientation of pairs
GROUPS = [1, 2, 3, 17, 70, 40, 33, 30, 65]  # 261 pairs; 70 and 65 exceed one workgroup's run


@pytest.mark.parametrize("k,width", [(3, 1), (4, 1), (5, 1), (6, 1), (4, 2), (3, 2), (1, 1), (1, 2)])
def test_orient_pairs(eng, records, k, width):
    keep = kept(records, k, width)
    recs = [records[i] for i in keep]
    n = len(recs)
    pal = keep.index(P if P in keep else E)  # rows that are their own permutation: every pair with them ties
    fwd, rev = (h[keep] for h in oracle_rows(records, k))
    rows = np.concatenate([fwd, rev])
    load(eng, recs + [S.revcomp(c, s) for c, s in recs])
    assert eng.kmer_max_strands(k, BOTH) < (1 << (8 * width))
    eng.kmer_build_strands(k, width, BOTH)
    rng = np.random.default_rng(100 + k)
    m = sum(GROUPS)
    assert m == 261
    a = rng.integers(0, 2 * n, m).astype(np.uint32)
    centres = rng.choice(2 * n, len(GROUPS), replace=False)
    centres[3] = pal
    ragged = np.repeat(centres, GROUPS).astype(np.uint32)
    a[:6] = [pal, 0, n, 1, n + 1, pal]  # the palindrome as a read; a read and its twin
    a[7] = pal  # ... and against itself (group 3's centre is the palindrome)
    lists = {"ragged": ragged, "one_b_per_pair": ((np.arange(m) * 7) % (2 * n)).astype(np.uint32),
             "one_b": np.full(m, 5, np.uint32)}
    seen_minus = seen_plus = seen_tie = False
    for name, b in lists.items():
        want = S.orient(rows[a], rows[b], k)
        strand, sad = eng.orient_pairs(a, b)
        assert np.array_equal(strand, want[0]), name
        assert np.array_equal(sad[:, 0], want[1]) and np.array_equal(sad[:, 1], want[2]), name
        tie = want[1] == want[2]
        assert (strand[tie] == 0).all()  # a tie is plus
        seen_tie |= bool(tie.any())
        seen_minus |= bool(strand.any())
        seen_plus |= bool((strand == 0).any())
        assert np.array_equal(eng.orient_pairs(a, b, sad=False)[0], strand)  # sad == NULL
        perm = rng.permutation(m)  # the grouping changes no result
        s2, d2 = eng.orient_pairs(a[perm], b[perm])
        assert np.array_equal(s2, strand[perm]) and np.array_equal(d2, sad[perm])
    assert seen_minus and seen_plus and seen_tie
    # a read against its own reverse complement is minus with sad_minus 0 (k = 1: the rows can tie)
    st, sd = eng.orient_pairs([0], [n])
    assert sd[0, 1] == 0 and st[0] == (1 if sd[0, 0] > 0 else 0)
    st, sd = eng.orient_pairs([], [])
    assert len(st) == 0
    for bad in ([2 * n], [0]), ([0], [2 * n]):
        with pytest.raises(M.MCError) as e:
            eng.orient_pairs(*bad)
        assert e.value.code == M.ERR_ARG


# ---------------------------------------------------------------- 3. end to end, planted truth
E2E = {"s1k_k5": ["--id", "0.85", "--kmer", "5"], "b3k30": ["--id", "0.90"]}


def run_cli(args, timeout=300):
    r = subprocess.run([M.BIN] + [str(a) for a in args] + ["--quiet"], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]


def inputs(name, tmp_path):
    fa, flags = fixtures.e2e_input(name, tmp_path)
    assert flags == E2E[name]
    T = fixtures.manifest()["e2e"][name]["generator"][2]
    flipped = str(tmp_path / (name + ".flipped.fa"))
    names = S.flip_fasta(fa, flipped, T)
    return fa, flipped, T, names


def planted(path, T):
    """{frozenset of read indices}: the .clstr's partition, and the planted one."""
    got = frozenset(frozenset(int(h.split()[0][5:]) for h, _ in c["members"]) for c in clstr.parse(open(path).read()))
    n = sum(len(c) for c in got)
    return got, frozenset(frozenset(range(t, n, T)) for t in range(T))


@pytest.mark.parametrize("which", ["as_written", "flipped"])
@pytest.mark.parametrize("name", list(E2E))
def test_both_strands_returns_the_planted_partition(eng, name, which, tmp_path):
    fa, flipped, T, names = inputs(name, tmp_path)
    src = fa if which == "as_written" else flipped
    out, tsv, js = tmp_path / "o.clstr", tmp_path / "o.strands.tsv", tmp_path / "o.json"
    run_cli([src] + E2E[name] + ["--both-strands", "--output", out, "--strands", tsv, "--stats-json", js])
    got, want = planted(out, T)
    misplaced = sum(len(c - max(want, key=lambda w: len(w & c))) for c in got)
    print("%s %s: %d clusters (planted %d), %d misplaced" % (name, which, len(got), T, misplaced))
    assert got == want
    # every member's strand against its centre; the centre's own line is + 0 sad_minus
    flip = (lambda i: S.flipped(i, T)) if which == "flipped" else (lambda i: False)
    lines = [ln.split("\t") for ln in tsv.read_text().splitlines()]
    order = [h for c in clstr.parse(out.read_text()) for h, _ in c["members"]]
    assert [ln[0] for ln in lines] == [h[1:] for h in order] and all(len(ln) == 6 for ln in lines)
    minus = 0
    for rname, cluster, cname, strand, sp, sm in lines:
        i, c = int(rname.split()[0][4:]), int(cname.split()[0][4:])
        assert i % T == c % T
        assert strand == ("-" if flip(i) != flip(c) else "+"), (rname, cname)
        if i == c:
            assert strand == "+" and int(sp) == 0
        assert (int(sm) < int(sp)) == (strand == "-")
        minus += strand == "-"
    import json
    st = json.load(open(js))
    assert st["strands"] == 3 and st["members_minus"] == minus and st["clusters"] == T
    assert (minus > 0) == (which == "flipped")
    seqs = "".join(ln for ln in open(src).read().splitlines() if not ln.startswith(">"))
    assert st["k_auto_length"] == 2 * (len(seqs) // len(names)) and st["k"] == 5


@pytest.mark.parametrize("name", list(E2E))
def test_one_strand_splits_the_flipped_reads_and_keeps_the_golden(eng, name, tmp_path):
    fa, flipped, T, _ = inputs(name, tmp_path)
    out, js = tmp_path / "p.clstr", tmp_path / "p.json"
    run_cli([flipped] + E2E[name] + ["--output", out])
    got, _ = planted(out, T)
    assert len(got) > T  # (2T seen: every template once per strand)
    run_cli([fa] + E2E[name] + ["--output", out, "--stats-json", js])
    with gzip.open(fixtures.golden("e2e_%s.clstr.gz" % name), "rb") as f:
        assert out.read_bytes() == f.read()
    assert "strands" not in open(js).read()


def test_two_ranks_write_the_same_bytes(eng, tmp_path):
    _, flipped, T, _ = inputs("s1k_k5", tmp_path)
    got = {}
    for name, extra in (("one", []), ("two", ["--devices", "0,0"])):
        out, tsv = tmp_path / (name + ".clstr"), tmp_path / (name + ".tsv")
        run_cli([flipped] + E2E["s1k_k5"] + ["--both-strands", "--output", out, "--strands", tsv] + extra)
        got[name] = (out.read_bytes(), tsv.read_bytes())
    assert got["one"] == got["two"] and len(got["one"][1]) > 0


# ---------------------------------------------------------------- 4. the trainer's labels, library mode
def test_training_labels_and_library_mode(eng, tmp_path):
    _, flipped, T, _ = inputs("s1k_k5", tmp_path)
    ds = M.Dataset([flipped], threads=2)
    out = tmp_path / "lib.clstr"
    st = ds.run(eng, ("--id", "0.85", "--kmer", "5", "--both-strands"), clstr=str(out))
    assert st["strands"] == 3 and st["clusters"] == T
    got, want = planted(out, T)
    assert got == want
    # 50 pairs: same template on the same strand, on opposite strands, and different templates
    a = np.arange(50, dtype=np.uint32)
    b = np.where(a % 3 == 0, a + T, np.where(a % 3 == 1, a + 2 * T, a + 1)).astype(np.uint32)
    plus = eng.nw_identity_strands(a, b, np.zeros(50, np.uint8))[0]
    minus = eng.nw_identity_strands(a, b, np.ones(50, np.uint8))[0]
    want_lab = np.where(minus > plus, minus, plus)
    assert np.array_equal(ds.label_identities(eng, a, b, both_strands=True), want_lab)
    assert np.array_equal(ds.label_identities(eng, a, b, both_strands=False), plus)
    assert (minus > plus).any() and (plus > minus).any()
    assert (want_lab[a % 3 != 2] > 0.8).all() and (want_lab[a % 3 == 2] < 0.7).all()  # (which strand matters)
    # errors throw and never exit: the flag with --align, --strands without the flag
    for args in (("--both-strands", "--align"), ("--strands", str(tmp_path / "x.tsv")), ("--both-strands", "--id", "0.5")):
        with pytest.raises(M.MCError):
            ds.run(eng, args)


# ---------------------------------------------------------------- 5. meshclust-assign with a version-2 model
def split_fasta(src, dst, lo, hi):
    recs = open(src).read().split(">")[1:]
    with open(dst, "w") as f:
        f.write("".join(">" + r for r in recs[lo:hi]))
    return dst


def test_assign_with_a_version_2_model(eng, tmp_path):
    fa, flipped, T, _ = inputs("s1k_k5", tmp_path)
    flags = E2E["s1k_k5"]
    idx = lambda name: int(name.split()[0][4:])  # "read17 template_17" -> 17
    # clustered on both strands: reads 0..899 of the flipped file; assigned: reads 900..1199
    base, rest = split_fasta(flipped, str(tmp_path / "base.fa"), 0, 900), split_fasta(flipped, str(tmp_path / "rest.fa"), 900, 1200)
    model, cen = tmp_path / "v2.model", tmp_path / "v2.centres.fa"
    run_cli([base] + flags + ["--both-strands", "--output", tmp_path / "v2.clstr", "--save-model", model, "--save-centres", cen])
    text = model.read_text().splitlines()
    assert text[0] == "meshclust-model 2" and "strands 3" in text and "centres %d" % T in text
    tsv, cons, js = tmp_path / "v2.tsv", tmp_path / "v2.cons.fa", tmp_path / "v2.json"
    outs = {}
    for name, extra, env in (("plain", [], {}), ("flag", ["--both-strands"], {}), ("pairs", [], {"MC_ASSIGN_PAIRS": "1"}),
                             ("consensus", ["--consensus", str(cons), "--stats-json", str(js)], {})):
        r = subprocess.run([ASSIGN_BIN, "--model", str(model), "--centres", str(cen), rest, "--output", str(tsv), "--quiet"] + extra,
                           capture_output=True, text=True, timeout=300, env=dict(os.environ, **env))
        assert r.returncode == 0, (name, r.stderr[-3000:])
        outs[name] = [ln.split("\t") for ln in tsv.read_text().splitlines()]
    assert outs["plain"] == outs["flag"] == outs["pairs"]  # the flag is implied; the pair list runs on the canonical rows
    assert [ln[:6] for ln in outs["consensus"]] == outs["plain"] and all(len(ln) == 7 for ln in outs["consensus"])
    minus = 0
    assert len(outs["plain"]) == 300
    for rname, cname, cluster, val, nsim, strand in outs["plain"]:
        i, c = idx(rname), idx(cname)
        assert i % T == c % T and int(nsim) >= 1, (rname, cname)
        assert strand == ("-" if S.flipped(i, T) != S.flipped(c, T) else "+"), (rname, cname)
        minus += strand == "-"
    assert all(float(ln[6]) > 0.8 for ln in outs["consensus"])  # aligned on the strand the orientation gave
    import json
    st = json.load(open(js))
    assert st["strands"] == 3 and st["assigned_minus"] == minus and 0 < minus < 300 and st["assigned"] == 300
    assert cons.read_text().count(">") == T
    # a version-1 model of the reads as written: what the saved files give on the CPU oracle, one strand
    base1, rest1 = split_fasta(fa, str(tmp_path / "base1.fa"), 0, 900), split_fasta(fa, str(tmp_path / "rest1.fa"), 900, 1200)
    model1, cen1, tsv1 = tmp_path / "v1.model", tmp_path / "v1.centres.fa", tmp_path / "v1.tsv"
    run_cli([base1] + flags + ["--output", tmp_path / "v1.clstr", "--save-model", model1, "--save-centres", cen1])
    kv = {ln.split()[0]: ln.split()[1:] for ln in model1.read_text().splitlines()[1:]}
    assert model1.read_text().startswith("meshclust-model 1\n") and "strands" not in kv
    r = subprocess.run([ASSIGN_BIN, "--model", str(model1), "--centres", str(cen1), rest1, "--output", str(tsv1), "--quiet"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    cls = O.Classifier()
    cls.n_single, cls.n_combo = int(kv["n_single"][0]), int(kv["n_combo"][0])
    for i in range(8):
        cls.lookup[i], cls.is_sim[i] = int(kv["lookup"][i]), int(kv["is_sim"][i])
        cls.mins[i], cls.maxs[i] = float.fromhex(kv["mins"][i]), float.fromhex(kv["maxs"][i])
        cls.combo_kind[i], cls.combo_len[i] = int(kv["combo_kind"][i]), int(kv["combo_len"][i])
        for j in range(4):
            cls.combo_idx[i][j] = int(kv["combo_idx"][4 * i + j])
    for i in range(9):
        cls.weights[i] = float.fromhex(kv["weights"][i])
    k, sim = int(kv["k"][0]), float.fromhex(kv["id"][0])
    feats = [int(cls.lookup[i]) for i in range(cls.n_single)]
    cents = M.Dataset([str(cen1)], threads=2).records()
    hc = [O.kmer_hist(c, s, k).astype(np.uint8) for _, c, s in cents]
    lines = []
    for hdr, codes, segs in M.Dataset([rest1], threads=2).records():
        hq = O.kmer_hist(codes, segs, k).astype(np.uint8)
        best, bval, n = -1, -1.0, 0
        for j, (_, cc, _) in enumerate(cents):
            if not (int(len(cc) * sim) <= len(codes) <= int(len(cc) / sim)):
                continue
            d, _, v = O.classify(cls, [O.raw(f, hq, hc[j], len(codes), len(cc)) for f in feats])
            if d:
                n += 1
                if best < 0 or v > bval:
                    best, bval = j, v
        lines.append("%s\t%s\t%d\t%s\t%d\n" % (hdr[1:], cents[best][0][1:] if best >= 0 else "*", best, "%.17g" % bval, n))
    assert tsv1.read_text() == "".join(lines)
