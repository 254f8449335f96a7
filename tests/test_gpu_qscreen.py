"""The q-gram screen on the GPU: mc_qgram_common against host/qscreen.hpp's count
(mcl_qscreen_common) and a Counter restatement, and bin/meshclust end to end with the screen on
(the device count), off and forced to the host count: the goldens byte for byte."""
import collections
import gzip
import json
import os
import subprocess

import numpy as np
import pytest

import fixtures
import meshclust_amd as M
import strand_cluster_cases as S

pytestmark = pytest.mark.gpu

LENGTHS = (6, 7, 63, 64, 65, 1000, 1023, 1024, 1025, 5000)
NA = M.QGRAM_NA


@pytest.fixture(scope="module")
def eng(built):
    e = M.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def reads(tmp_path_factory):
    """Per length: a random read, its copy, a 5 % substituted copy, an unrelated read and (from 63
    up) the first with a run of N in the middle -> (Dataset, [(codes, segments)], [kind])."""
    rng = np.random.default_rng(77)
    seqs, kinds = [], []
    for L in LENGTHS:
        a = rng.integers(0, 4, L)
        m = a.copy()
        flip = rng.random(L) < 0.05
        m[flip] = (m[flip] + rng.integers(1, 4, int(flip.sum()))) & 3
        group = [("base", a), ("copy", a.copy()), ("near", m), ("far", rng.integers(0, 4, L))]
        for kind, s in group:
            seqs.append("".join("ACGT"[v] for v in s))
            kinds.append(kind)
        if L >= 63:
            s = seqs[-4]
            seqs.append(s[:L // 2 - 5] + "N" * 10 + s[L // 2 + 5:])
            kinds.append("n")
    path = tmp_path_factory.mktemp("qscreen") / "reads.fa"
    path.write_text("".join(">r%d\n%s\n" % (i, s) for i, s in enumerate(seqs)))
    ds = M.Dataset([str(path)])
    recs = [(c, s) for _, c, s in ds.records()]
    assert [len(c) for c, _ in recs] == [len(s) for s in seqs]
    return ds, recs, kinds


def load(eng, recs):
    lens = np.array([len(c) for c, _ in recs], np.uint64)
    seq_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    seg = np.array([v for _, s in recs for pair in s for v in pair], np.int32)
    seg_off = np.concatenate([[0], np.cumsum([len(s) for _, s in recs])]).astype(np.uint64)
    eng.load_sequences(np.concatenate([c for c, _ in recs]), seq_off, seg, seg_off)


def naive(a, b, minus, q):
    if minus:
        a = np.where(a <= 3, 3 - a, a)[::-1]
    if len(a) < q or len(b) < q or a.max() > 3 or b.max() > 3:
        return NA
    ca = collections.Counter(bytes(a[j:j + q]) for j in range(len(a) - q + 1))
    cb = collections.Counter(bytes(b[j:j + q]) for j in range(len(b) - q + 1))
    return sum(min(v, cb[g]) for g, v in ca.items())


def test_kernel_equals_host_count(eng, reads):
    ds, recs, kinds = reads
    load(eng, recs)
    n = len(recs)
    rng = np.random.default_rng(5)
    # every read against itself, its group and a stranger; then random pairs: ~1,000 pairs per q
    a = list(range(n)) + [i for i in range(n) for _ in range(3)]
    b = list(range(n)) + [j for i in range(n) for j in (i - i % 4, (i + 1) % n, (i + 7) % n)]
    extra = 1000 - len(a)
    digits = [i for i in range(n) if recs[i][0].max() <= 3]  # (three quarters of the random pairs have a count)
    pick = lambda: [int(rng.choice(digits)) if t % 4 else int(rng.integers(0, n)) for t in range(extra)]
    a = np.array(a + pick(), np.uint32)
    b = np.array(b + pick(), np.uint32)
    minus = (rng.random(len(a)) < 0.5).astype(np.uint8)
    seen_na = seen_count = checked = 0
    for q in (4, 7):
        got = eng.qgram_common(a, b, q, minus)
        want = ds.qscreen_common(a, b, q, minus)
        assert np.array_equal(got, want), np.flatnonzero(got != want)[:10]
        assert np.array_equal(eng.qgram_common(a, b, q), ds.qscreen_common(a, b, q))  # NULL: all plus
        for i in range(len(a)):
            la, lb = len(recs[a[i]][0]), len(recs[b[i]][0])
            # (the parser leaves a read too short for a segment as raw letters: not available either)
            na = min(la, lb) < q or max(recs[a[i]][0].max(), recs[b[i]][0].max()) > 3
            assert na or "n" not in (kinds[a[i]], kinds[b[i]])
            assert (got[i] == NA) == na, (i, a[i], b[i])
            if na:
                seen_na += 1
                continue
            seen_count += 1
            if a[i] == b[i] and not minus[i]:
                assert got[i] == la - q + 1
            if max(la, lb) <= 1025 and i % 3 == 0:
                assert got[i] == naive(recs[a[i]][0], recs[b[i]][0], minus[i], q), (i, q)
                checked += 1
    assert seen_na >= 100 and seen_count >= 1000 and checked >= 200, (seen_na, seen_count, checked)
    # a pair of identical reads (a read and its copy), plus
    base = kinds.index("base", 4 * 5)  # (the 1,000-base group)
    assert eng.qgram_common([base], [base + 1], 7)[0] == len(recs[base][0]) - 6
    # reads of 6 and 7 digits (loaded directly: the parser keeps none that short as digits)
    rng = np.random.default_rng(9)
    short = [(rng.integers(0, 4, L).astype(np.uint8), [[0, L - 1]]) for L in (6, 7, 7, 6, 8, 63)]
    load(eng, short)
    sa, sb = np.repeat(np.arange(6), 6), np.tile(np.arange(6), 6)
    for q in (4, 7):
        for mi in (0, 1):
            got = eng.qgram_common(sa, sb, q, np.full(36, mi, np.uint8))
            assert list(got) == [naive(short[x][0], short[y][0], mi, q) for x, y in zip(sa, sb)], (q, mi)
    assert eng.qgram_common([0], [1], 7)[0] == NA and eng.qgram_common([1], [1], 7)[0] == 1
    load(eng, recs)
    # m = 0, and the errors of mc_nw_identity
    assert len(eng.qgram_common([], [], 7)) == 0
    for bad in (([n], [0], 7), ([0], [n], 7), ([0], [1], 0), ([0], [1], 8)):
        with pytest.raises(M.MCError) as e:
            eng.qgram_common(*bad)
        assert e.value.code == M.ERR_ARG


def cli(args, env, timeout=600):
    base = {k: v for k, v in os.environ.items() if not k.startswith("MC_NW_")}
    r = subprocess.run([M.BIN] + [str(x) for x in args] + ["--quiet"], capture_output=True, text=True, timeout=timeout,
                       env=dict(base, **env))
    assert r.returncode == 0, r.stderr[-3000:]


SCREEN = {"on": {}, "off": {"MC_NW_SCREEN": "0"}, "host": {"MC_NW_SCREEN": "host"}}


@pytest.mark.parametrize("name", ["a1k", "m2k_id80", "fam2k_id85"])
def test_e2e_cli_screen_byte_identical(eng, name, tmp_path):
    fa, flags = fixtures.e2e_input(name, tmp_path)
    with gzip.open(fixtures.golden("e2e_%s.clstr.gz" % name), "rb") as f:
        want = f.read()
    st = {}
    for mode, env in SCREEN.items():
        out, js = tmp_path / (mode + ".clstr"), tmp_path / (mode + ".json")
        cli([fa] + flags + ["--output", out, "--stats-json", js], env)
        assert out.read_bytes() == want, mode
        st[mode] = json.load(open(js))
    print({m: (s["nw_pairs"], s["nw_screened"]) for m, s in st.items()})
    assert st["off"]["nw_screened"] == 0
    assert (st["on"]["nw_pairs"], st["on"]["nw_screened"]) == (st["host"]["nw_pairs"], st["host"]["nw_screened"])
    if name == "a1k":
        assert st["on"]["nw_screened"] > 0 and st["on"]["nw_pairs"] < st["off"]["nw_pairs"]


def test_e2e_cli_screen_both_strands(eng, tmp_path):
    """--both-strands on a1k with every second template's reads reverse-complemented: a pair is
    screened only if both orientations are; the run with the screen off is the expectation."""
    fa, flags = fixtures.e2e_input("a1k", tmp_path)
    flipped = str(tmp_path / "a1k.flipped.fa")
    S.flip_fasta(fa, flipped, fixtures.manifest()["e2e"]["a1k"]["generator"][2])
    got = {}
    for mode, env in SCREEN.items():
        out, js = tmp_path / (mode + ".clstr"), tmp_path / (mode + ".json")
        cli([flipped] + flags + ["--both-strands", "--output", out, "--stats-json", js], env)
        got[mode] = (out.read_bytes(), json.load(open(js)))
    assert got["on"][0] == got["off"][0] == got["host"][0] and len(got["off"][0]) > 0
    assert got["off"][1]["nw_screened"] == 0 and got["on"][1]["nw_screened"] > 0
    assert got["on"][1]["nw_pairs"] < got["off"][1]["nw_pairs"]
    assert got["on"][1]["nw_screened"] == got["host"][1]["nw_screened"]
