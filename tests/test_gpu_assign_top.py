"""mc_assign_top / meshclust-assign --top K --hits FILE: the K best centres of every read.

Every value is compared with ==, and every expectation comes from code that existed before the
list did: mc_classify_pairs over all (query, centre) pairs gives the plus strand's decisions and
values, the same call on the points that hold the queries' reverse complements gives the minus
strand's, the length gate is applied as in test_gpu_assign.gate_mask, and numpy sorts every
query's similar (value, strand, index) by (-value, strand, index), cuts at K and pads.

Points, queries and configurations are those of test_gpu_assign_strands.py (its helpers are
imported, the file is not changed): every query has a partner point holding its reverse complement.
"""
import json
import subprocess

import numpy as np
import pytest

import fixtures
import meshclust_amd as M
import oracle_lib as O
from test_gpu_assign import gate_mask
from test_gpu_assign_strands import (CONFIGS, N_READS, NONE, P, QUERIES, RC0, _RC, _state, eng, partner,  # noqa: F401
                                     points, read_fasta, run_assign, setup, write_fasta)

pytestmark = pytest.mark.gpu

KS = (1, 2, 3, 5, 8)
KEEP = M.ASSIGN_MAX_TOP + 1  # the expectation keeps one hit more than any K, to see what a cut drops
# T1: reads 100..163 and then their reverse complements: score(q, c) == score(rc q, rc c), so every
#     hit has an exact twin on the other strand at another index (arrival order != sort order)
# T2: 400 reads: several LDS tiles at the default tile, and more than 8 similar centres per query
# T3: query 100's own id nine times (more than K exact ties at combo 0 = 1.0 within a strand), the
#     palindrome twice (ties across the strands for every query it is similar to), reads 0..6
T1 = np.concatenate([np.arange(RC0, RC0 + 64), np.arange(N_READS, N_READS + 64)]).astype(np.uint32)
T2 = np.arange(400).astype(np.uint32)
T3 = np.array([RC0] * 9 + [P, P] + list(range(7)), np.uint32)
SETS = {"T1": T1, "T2": T2, "T3": T3}
SIMS = (0.0, 0.99)

_pairs = {}  # (k, width, set) -> per-pair decisions and values of both strands
_lists = {}  # (k, width, set, strands, sim) -> the sorted lists, KEEP slots


def pair_scores(eng, k, width, name):
    """mc_classify_pairs on every (query, centre) pair and every (partner(query), centre) pair."""
    key = (k, width, name)
    if key not in _pairs:
        cen = SETS[name]
        out = []
        for q in (QUERIES, partner(QUERIES)):
            a = np.repeat(q, len(cen)).astype(np.uint32)
            b = np.tile(cen, len(q)).astype(np.uint32)
            d, c0, _ = eng.classify_pairs(a, b)
            out.append((d.reshape(len(q), len(cen)) != 0, c0.reshape(len(q), len(cen)).copy()))
        _pairs[key] = out
    return _pairs[key]


def expectation(eng, lens, k, width, name, strands, sim):
    """-> (hit, hit_val, hit_strand) with KEEP slots per query, n_similar, pairs after the gate."""
    key = (k, width, name, strands, sim)
    if key not in _lists:
        (dp, vp), (dm, vm) = pair_scores(eng, k, width, name)
        gate = gate_mask(lens, SETS[name], QUERIES, sim)
        m = len(QUERIES)
        hit = np.full((m, KEEP), NONE, np.uint32)
        val = np.full((m, KEEP), -1.0)
        strand = np.zeros((m, KEEP), np.uint8)
        nsim = np.zeros(m, np.uint32)
        for q in range(m):
            vs, ss, js = [], [], []
            for s, (d, v) in enumerate(((dp, vp), (dm, vm))):
                if strands & (1 << s):
                    j = np.flatnonzero(d[q] & gate[q])
                    vs.append(v[q, j])
                    ss.append(np.full(len(j), s))
                    js.append(j)
            vs, ss, js = np.concatenate(vs), np.concatenate(ss), np.concatenate(js)
            order = np.lexsort((js, ss, -vs))[:KEEP]  # by -value, then strand, then index
            n = len(order)
            hit[q, :n], val[q, :n], strand[q, :n], nsim[q] = js[order], vs[order], ss[order], len(vs)
        _lists[key] = (hit, val, strand, nsim, int(gate.sum()))
    return _lists[key]


def flags_of(want, K, n_pairs):
    """Which of the cases this file is there for the expectation (KEEP slots) holds at this K."""
    hit, val, strand, nsim, cand = want
    filled = hit != NONE
    f = {}
    f["truncated"] = bool((nsim > K).any())
    f["padded"] = bool(((nsim > 0) & (nsim < K)).any())
    f["unassigned"] = bool((nsim == 0).any())
    # the last listed hit and the first dropped one: same value, same strand
    f["tie_cut_within_strand"] = bool((filled[:, K] & (val[:, K - 1] == val[:, K]) & (strand[:, K - 1] == strand[:, K])).any())
    # neighbours in the list: a plus hit, then a minus hit of the same value at a lower index (the
    # minus hit arrived first)
    nb = filled[:, 1:K] & (val[:, :K - 1] == val[:, 1:K]) & (strand[:, :K - 1] == 0) & (strand[:, 1:K] == 1)
    f["tie_across_strands_minus_first"] = bool((nb & (hit[:, 1:K] < hit[:, :K - 1])).any())
    f["mixed_strands"] = bool(((filled[:, :K] & (strand[:, :K] == 1)).any(1) & (filled[:, :K] & (strand[:, :K] == 0)).any(1)).any())
    f["gated"] = cand < n_pairs
    return f


@pytest.mark.parametrize("tile", ["7", None], ids=["tile7", "tile_default"])
@pytest.mark.parametrize("config", list(CONFIGS))
def test_assign_top_equals_sorted_pair_list(eng, points, config, tile, monkeypatch):
    k, width, form = CONFIGS[config]
    setup(eng, points, k, width)
    lens = points[2]
    for name, val in (("MC_ASSIGN_TILE", tile), ("MC_ASSIGN_FORM", form)):
        if val:
            monkeypatch.setenv(name, val)
        else:
            monkeypatch.delenv(name, raising=False)
    seen = {}
    for name, centres in SETS.items():
        for sim in SIMS:
            for strands in (1, 2, 3):
                want = expectation(eng, lens, k, width, name, strands, sim)
                for K in KS:
                    hit, val, strand, nsim, stats = eng.assign_top(centres, QUERIES, sim, strands, K)
                    where = (config, tile, name, sim, strands, K)
                    assert hit.shape == (len(QUERIES), K) and hit.dtype == np.uint32 and strand.dtype == np.uint8
                    assert np.array_equal(nsim, want[3]), where
                    assert np.array_equal(hit, want[0][:, :K]), where
                    assert np.array_equal(val, want[1][:, :K]), where
                    assert np.array_equal(strand, want[2][:, :K]), where
                    assert int(stats[0]) == want[4], where
                    for flag, on in flags_of(want, K, len(QUERIES) * len(centres)).items():
                        seen[flag] = seen.get(flag, False) or on
    if config == "short_k4":  # the expectation holds every case this file is there for
        assert all(seen.values()), seen


def test_t1_has_the_twin_hits_and_t2_truncates(eng, points):
    """The data does what the centre sets were chosen for (expectation only, k = 4)."""
    setup(eng, points, 4, 1)
    (dp, vp), (dm, vm) = pair_scores(eng, 4, 1, "T1")
    # score(q, c) == score(rc q, rc c): the plus strand against the forward half is the minus strand
    # against the reverse-complemented half, decision and value, bit for bit
    assert np.array_equal(dp[:, :64], dm[:, 64:]) and np.array_equal(vp[:, :64], vm[:, 64:])
    assert np.array_equal(dp[:, 64:], dm[:, :64]) and np.array_equal(vp[:, 64:], vm[:, :64])
    fwd = QUERIES < N_READS
    n1 = dp[fwd][:, :64].sum(1)
    assert n1.min() > 2 and n1.max() < 8  # K = 2 truncates them all, K = 8 pads them all
    n2 = expectation(eng, points[2], 4, 1, "T2", 1, 0.0)[3][fwd]
    assert n2.min() > M.ASSIGN_MAX_TOP  # K = 8 truncates every forward query
    t3 = expectation(eng, points[2], 4, 1, "T3", 3, 0.0)
    q0 = int(np.flatnonzero(QUERIES == RC0)[0])
    assert (t3[1][q0, :KEEP] == 1.0).all() and (t3[2][q0] == 0).all() and list(t3[0][q0]) == list(range(9))


@pytest.mark.parametrize("form", [None, "general"], ids=["short", "general"])
def test_k1_is_assign_strands(eng, points, form, monkeypatch):
    """K = 1: column 0 and n_similar are mc_assign_strands' result for every strand set.  (On the
    minus strand alone mc_assign_strands reports strand 1 also for an unassigned query; an empty
    slot of the list holds 0, as the header says.)"""
    setup(eng, points, 4, 1)
    monkeypatch.delenv("MC_ASSIGN_TILE", raising=False)
    if form:
        monkeypatch.setenv("MC_ASSIGN_FORM", form)
    else:
        monkeypatch.delenv("MC_ASSIGN_FORM", raising=False)
    for centres in (T1, T3):
        for sim in SIMS:
            for strands in (1, 2, 3):
                best, bval, bstrand, bn, bstats = eng.assign_strands(centres, QUERIES, sim, strands)
                hit, val, strand, nsim, stats = eng.assign_top(centres, QUERIES, sim, strands, 1)
                assert hit.shape == (len(QUERIES), 1)
                assert np.array_equal(hit[:, 0], best) and np.array_equal(val[:, 0], bval) and np.array_equal(nsim, bn)
                assert int(stats[0]) == int(bstats[0]) and int(stats[1]) == int(bstats[1])
                if strands == M.MC_STRAND_MINUS:
                    assert np.array_equal(strand[:, 0], np.where(best == NONE, 0, bstrand))
                else:
                    assert np.array_equal(strand[:, 0], bstrand)
                # and column 0 at a larger K is the same
                hit8, val8, strand8, nsim8, _ = eng.assign_top(centres, QUERIES, sim, strands, 8)
                assert np.array_equal(hit8[:, 0], hit[:, 0]) and np.array_equal(val8[:, 0], val[:, 0])
                assert np.array_equal(strand8[:, 0], strand[:, 0]) and np.array_equal(nsim8, nsim)


def test_assign_top_arguments(eng, points):
    setup(eng, points, 4, 1)
    for K in (0, M.ASSIGN_MAX_TOP + 1):
        with pytest.raises(M.MCError) as e:
            eng.assign_top(T1, QUERIES, 0.0, 3, K)
        assert e.value.code == M.ERR_ARG
    for strands in (0, 4):
        with pytest.raises(M.MCError) as e:
            eng.assign_top(T1, QUERIES, 0.0, strands, 4)
        assert e.value.code == M.ERR_ARG
    hit, val, strand, nsim, stats = eng.assign_top(T1, [], 0.0, 3, 4)  # M = 0
    assert hit.shape == (0, 4) and len(nsim) == 0 and int(stats[0]) == 0
    # NULL outputs: every one may be left out
    cen, q = np.ascontiguousarray(T3), np.ascontiguousarray(QUERIES)
    ref = eng.assign_top(T3, QUERIES, 0.0, 3, 4)
    for K in (1, 4):
        assert eng.lib.mc_assign_top(eng.ctx, M._p(cen), len(cen), M._p(q), len(q), 0.0, 3, K, None, None, None, None, None) == 0
    nsim = np.zeros(len(q), np.uint32)
    assert eng.lib.mc_assign_top(eng.ctx, M._p(cen), len(cen), M._p(q), len(q), 0.0, 3, 4, None, None, None, M._p(nsim), None) == 0
    assert np.array_equal(nsim, ref[3])
    strand = np.full((len(q), 4), 9, np.uint8)
    assert eng.lib.mc_assign_top(eng.ctx, M._p(cen), len(cen), M._p(q), len(q), 0.0, 3, 4, None, None, M._p(strand), None, None) == 0
    assert np.array_equal(strand, ref[2])
    # more slots than hits are possible: one centre, K = 8, one strand
    hit, val, strand, nsim, _ = eng.assign_top([RC0], QUERIES, 0.0, 1, 8)
    q0 = int(np.flatnonzero(QUERIES == RC0)[0])
    assert hit[q0, 0] == 0 and val[q0, 0] == 1.0 and nsim[q0] == 1 and (nsim <= 1).all()
    assert (hit[:, 1:] == NONE).all() and (val[:, 1:] == -1.0).all() and (strand == 0).all()
    assert np.array_equal(hit[:, 0] != NONE, nsim == 1)
    al = O.Classifier()
    al.n_single, al.n_combo = 1, 1
    al.lookup[0], al.is_sim[0], al.mins[0], al.maxs[0] = M.FEAT_ALIGN, 1, 0.0, 1.0
    al.combo_kind[0], al.combo_len[0], al.combo_idx[0][0] = M.COMBO_SELF, 1, 0
    al.weights[0], al.weights[1] = -0.5, 1.0
    setup(eng, points, 4, 1, al)
    for K in (1, 4):
        with pytest.raises(M.MCError) as e:
            eng.assign_top(T1, QUERIES, 0.0, 3, K)
        assert e.value.code == M.ERR_UNSUPPORTED
    setup(eng, points, 3, 4)  # 32-bit bins
    for K in (1, 4):
        with pytest.raises(M.MCError) as e:
            eng.assign_top(T1, QUERIES, 0.0, 1, K)
        assert e.value.code == M.ERR_UNSUPPORTED


# ---------------------------------------------------------------- end to end
def hit_lines(path):
    return [ln.split("\t") for ln in open(path).read().splitlines()]


def test_cli_top_hits(eng, tmp_path):
    fa, flags = fixtures.e2e_input("a1k", tmp_path)
    model, cen = tmp_path / "a1k.model", tmp_path / "a1k.centres.fa"
    r = subprocess.run([M.BIN, fa] + flags + ["--output", str(tmp_path / "a1k.clstr"), "--quiet", "--save-model", str(model),
                                              "--save-centres", str(cen)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    recs = read_fasta(fa)
    f_recs = [(h, s.translate(_RC)[::-1] if i % 2 else s) for i, (h, s) in enumerate(recs)]
    ffa, rfa = tmp_path / "F.fa", tmp_path / "R.fa"
    write_fasta(ffa, f_recs)
    write_fasta(rfa, [(h, s.translate(_RC)[::-1]) for h, s in f_recs])

    def run(name, reads, extra=(), env=None, top=True):
        tsv, hits, stats = (tmp_path / (name + ext) for ext in (".tsv", ".hits", ".json"))
        args = (["--top", "3", "--hits", str(hits)] if top else []) + ["--stats-json", str(stats)] + list(extra)
        r = run_assign(model, cen, reads, tsv, args, env=env)
        assert r.returncode == 0, r.stderr[-3000:]
        return tsv, hits, json.loads(stats.read_text())

    # one strand: the main TSV is the one of a run without the options, the hits file the one the
    # pair list gives
    plain_tsv, _, plain_st = run("plain", ffa, top=False)
    f_tsv, f_hits, f_st = run("F", ffa)
    assert f_tsv.read_bytes() == plain_tsv.read_bytes()
    assert "top" not in plain_st and "hits" not in plain_st
    lines = hit_lines(f_hits)
    assert f_st["path"] == "device" and f_st["top"] == 3 and f_st["hits"] == len(lines) > 0
    assert all(len(x) == 5 for x in lines)  # no strand column
    p_tsv, p_hits, p_st = run("P", ffa, env={"MC_ASSIGN_PAIRS": "1"})
    assert p_st["path"] == "pairs" and p_hits.read_bytes() == f_hits.read_bytes() and p_tsv.read_bytes() == plain_tsv.read_bytes()
    assert p_st["hits"] == len(lines)
    # rank 1 is the main TSV's row, ranks ascend from 1, unassigned reads have no line
    main = {x[0]: x for x in (ln.split("\t") for ln in plain_tsv.read_text().splitlines())}
    ranks = {}
    for x in lines:
        ranks.setdefault(x[0], []).append(x)
    for read, row in main.items():
        got = ranks.get(read, [])
        assert [int(x[1]) for x in got] == list(range(1, min(3, int(row[4])) + 1))
        if got:
            assert got[0][2:5] == row[1:4]
        else:
            assert row[2] == "-1"
    # both strands: the merge, by the stated order, of the one-strand lists of the file and of its
    # reverse complement
    _, r_hits, _ = run("R", rfa)
    merged = {}
    for sign, path in (("+", f_hits), ("-", r_hits)):
        for x in hit_lines(path):
            merged.setdefault(x[0], []).append((-float(x[4]), sign != "+", int(x[3]), x, sign))
    want = []
    for h, _ in f_recs:  # reads in input order
        name = h[1:].decode()
        for rank, (_, _, _, x, sign) in enumerate(sorted(merged.get(name, []), key=lambda t: t[:3])[:3]):
            want.append([name, str(rank + 1), x[2], x[3], x[4], sign])
    both_plain_tsv, _, _ = run("bothplain", ffa, ["--both-strands"], top=False)
    b_tsv, b_hits, b_st = run("both", ffa, ["--both-strands"])
    assert b_tsv.read_bytes() == both_plain_tsv.read_bytes()
    got = hit_lines(b_hits)
    assert got == want
    assert any(x[5] == "-" for x in got) and any(x[5] == "+" for x in got)
    assert b_st["top"] == 3 and b_st["hits"] == len(got) and b_st["strands"] == 3
    # the same job in process (mcl_assign_top)
    st = M.assign_files(eng, str(model), str(cen), str(ffa), str(tmp_path / "lib.tsv"), threads=2, both_strands=True, top=3,
                        hits=str(tmp_path / "lib.hits"))
    _state.clear()  # (the context now holds other sequences)
    assert (tmp_path / "lib.tsv").read_bytes() == b_tsv.read_bytes() and (tmp_path / "lib.hits").read_bytes() == b_hits.read_bytes()
    assert st["top"] == 3 and st["hits"] == len(got)
    with pytest.raises(M.MCError):
        M.assign_files(eng, str(model), str(cen), str(ffa), str(tmp_path / "x.tsv"), threads=2, top=3)
    # the pair list still refuses both strands
    r = run_assign(model, cen, ffa, tmp_path / "y.tsv", ["--both-strands", "--top", "3", "--hits", str(tmp_path / "y.hits")],
                   env={"MC_ASSIGN_PAIRS": "1"})
    assert r.returncode == 2 and not (tmp_path / "y.hits").exists()
