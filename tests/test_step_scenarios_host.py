"""The step scenarios (step_scenarios.py) on the CPU oracle engine alone: the inputs must reach
the cases they were placed for, or the GPU comparison of test_gpu_steps.py proves little.

Checked here, without a GPU: flagged shares that split, first maxima of combo 0 tied across
workgroups and across the waves of one workgroup, get_mean minima tied between members whose
push order disagrees with their position order (with and without the cluster's first member),
the flagged counts at which add_rows and the flag copy-back change path, walks that grow
clusters over several steps, determinism, and the sharded steps' equivalence to whole ones on
the oracle itself.
"""
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import step_scenarios as SS


@pytest.fixture(scope="module")
def harness(built):
    subprocess.run(["make", "-s", "-C", os.path.join(SS.ROOT, "oracle"), "harness"], check=True)


_cache = {}


def scenario(row):
    """(input, histograms, classifier engine, the walk's run) of a row, made once."""
    if row not in _cache:
        inp = SS.make_input(row)
        eng = SS.oracle_engine()
        SS.load(eng, inp)
        eng.set_classifier(SS.make_classifier(inp, eng))
        run = SS.run_walk(eng, inp, sharded=row in SS.FUSED)
        ref = SS.oracle_engine()  # a second context: classify_pairs for the checks
        SS.load(ref, inp)
        ref.set_classifier(SS.make_classifier(inp, ref))
        _cache[row] = (inp, ref.histograms()[0], ref, run)
    return _cache[row]


def first_max_ties(inp, ref, step):
    """Positions (relative to the window start: the scan's workgroups start at S) at which the
    step's maximum of combo 0 is reached."""
    cand = step["cand"]
    if len(cand) < 2 or step["kind"] == "commit":
        return np.zeros(0, np.int64)
    ids = inp.order[cand]
    _, c0, _ = ref.classify_pairs(ids, np.full(len(ids), step["centre"], np.uint32))  # compute(candidate, centre)
    ok = ~np.isnan(c0)
    if not ok.any():
        return np.zeros(0, np.int64)
    return cand[ok & (c0 == c0[ok].max())] - step["S"]


def mean_ties(inp, h, step):
    """Of the step's get_mean: (indices into the member list, push order, that share the minimum
    distance_d; the members' static positions)."""
    mem = step["members"]
    rows = h[mem]
    mean = rows.astype(np.float64).sum(axis=0) / len(mem)
    d = np.array([O.distance_d(np.ascontiguousarray(r), mean) for r in rows])
    return np.nonzero(d == d.min())[0], inp.pos[mem]


def cluster_steps(run):
    out = []
    for tag, _ in run.trace:
        if tag == "cluster_begin":
            out.append(0)
        elif tag in ("scan", "scan_commit"):
            out[-1] += 1
    return out


@pytest.mark.parametrize("row", sorted(SS.ROWS))
def test_walk_conditions(harness, row):
    inp, h, ref, run = scenario(row)
    assert all(d["rc"] == 0 for _, d in run.trace), [t for t in run.trace if t[1]["rc"] != 0][:3]
    shares = [len(s["flagged"]) / len(s["cand"]) for s in run.steps if len(s["cand"])]
    assert any(0.10 <= x <= 0.90 for x in shares), "no step splits its candidates"
    steps = cluster_steps(run)
    assert sum(1 for x in steps if x >= 3) >= 5, steps
    most = max(len(s["flagged"]) for s in run.steps)
    if row == "k3w1":
        assert most >= 300  # add_rows' four-rows-in-flight loop: more than 3 * (256 / nch) rows
    if row == "k2w4":
        assert most > 4096  # the flag list's second copy (kFlagPrefix)
    # every window kind was scanned, the all-dead one included
    assert any(len(s["cand"]) == 0 for s in run.steps), "no window of dead candidates"
    assert any(s["S"] == s["E"] for s in run.steps)
    kills = [i for i, (tag, _) in enumerate(run.trace) if tag == "kill"]
    assert any(all(run.trace[i + j][0] == "kill" for j in range(9)) for i in kills[:-8]), "no nine kills in a row"
    if row in SS.FUSED:
        assert any(tag == "scan_commit" for tag, _ in run.trace)


def test_first_maximum_ties_span_workgroups_and_waves(harness):
    blocks = waves = 0
    for row in SS.FUSED:
        inp, h, ref, run = scenario(row)
        for s in run.steps:
            t = first_max_ties(inp, ref, s)
            if len(t) < 2:
                continue
            blk, wav = t // SS.BLOCK, (t % SS.BLOCK) // 64
            blocks += len(set(blk)) >= 2
            waves += any(len(set(wav[blk == b])) >= 2 for b in set(blk))
    assert blocks >= 1 and waves >= 1, (blocks, waves)


@pytest.mark.parametrize("row", [r for r in sorted(SS.FUSED) if SS.ROWS[r]["n"] >= 1000])
def test_first_maximum_ties_per_row(harness, row):
    """Every fused row of 1,000 reads or more (257 reads leave one position to the second
    workgroup) has a step whose first maximum is tied across workgroups, and so through every
    level of the reduction."""
    inp, h, ref, run = scenario(row)
    n = 0
    for s in run.steps:
        t = first_max_ties(inp, ref, s)
        n += len(t) >= 2 and len(set(t // SS.BLOCK)) >= 2
    assert n >= 1


@pytest.mark.parametrize("row", ["k3w1", "k4w1", "k3w2", "k5w1"])
def test_get_mean_ties_disagree_with_position_order(harness, row):
    """A get_mean whose minimum is shared by members pushed in another order than their static
    positions, the winner (the first pushed) not being the lowest position: once between the
    members of different steps alone, once with the cluster's first member among the tied.
    (These rows cover both forms of mean_closest_fast: a lane per member, with and without the
    nch == 16 loads, and a wave per member.)"""
    inp, h, ref, run = scenario(row)
    by_steps = with_first = 0
    for s in run.steps:
        if s["res"]["is_min"]:
            continue
        tied, pos = mean_ties(inp, h, s)
        if len(tied) < 2 or pos[tied[0]] == pos[tied].min():
            continue
        assert s["res"]["new_centre"] == s["members"][tied[0]]  # the oracle takes the first pushed
        if tied[0] == 0:
            with_first += 1
        else:
            by_steps += 1
    assert by_steps >= 1 and with_first >= 1, (by_steps, with_first)


@pytest.mark.parametrize("row", ["k3w1", "k7w1"])
def test_scripts_are_deterministic(harness, row):
    inp, h, ref, run = scenario(row)
    inp2 = SS.make_input(row)
    assert np.array_equal(inp.order, inp2.order) and np.array_equal(inp.codes, inp2.codes)
    eng = SS.oracle_engine()
    SS.load(eng, inp2)
    eng.set_classifier(SS.make_classifier(inp2, eng))
    assert SS.diff(run.trace, SS.run_walk(eng, inp2).trace) is None
    a = SS.run_sharded(eng, inp2)[0].trace + SS.run_msum(eng, inp2, True).trace + SS.run_mean_shift(eng, inp2)
    b = SS.run_sharded(eng, inp2)[0].trace + SS.run_msum(eng, inp2, True).trace + SS.run_mean_shift(eng, inp2)
    assert SS.diff(a, b) is None


@pytest.mark.parametrize("row", sorted(SS.FUSED))
def test_sharded_steps_equal_whole_steps_on_the_oracle(harness, row):
    inp, h, ref, _ = scenario(row)
    eng = SS.oracle_engine()
    SS.load(eng, inp)
    eng.set_classifier(SS.make_classifier(inp, eng))
    run, cases = SS.run_sharded(eng, inp)
    SS.check_sharded(cases)
    parts = [d for tag, d in run.trace if tag == "scan_part"]
    assert any(d["nparts"] == 7 and not d["has_best"] for d in parts), "no part without a block"
    tail = [d for tag, d in run.trace[-2:]]
    assert tail[0]["is_min"] == 1 and tail[0]["n_members"] == 1 and tail[1]["n_flagged"] > 0  # commit of nothing


@pytest.mark.parametrize("row", ["k3w1", "k5w1", "k7w1", "k6w2"])
def test_msum_sequence_reaches_a_grown_second_step(harness, row):
    """Script (e): the cluster's first step flags nothing, its second does, after another cluster;
    fused and through part / commit the oracle gives the same cluster."""
    inp, h, ref, _ = scenario(row)
    got = []
    for through_parts in (False, True):
        eng = SS.oracle_engine()
        SS.load(eng, inp)
        eng.set_classifier(SS.make_classifier(inp, eng))
        run = SS.run_msum(eng, inp, through_parts)
        quiet = [i for i, s in enumerate(run.steps) if s["S"] == s["E"]]
        assert len(quiet) == 1 and run.steps[quiet[0]]["res"]["is_min"] == 1 and quiet[0] > 0
        nxt = run.steps[quiet[0] + 1]
        assert nxt["res"]["is_min"] == 0 and nxt["res"]["n_flagged"] >= 5
        got.append([(s["res"]["new_centre"], s["res"]["n_members"], tuple(s["flagged"])) for s in run.steps])
    assert got[0] == got[1]


@pytest.mark.parametrize("cutoff", [0.55, 0.9])
def test_alignment_walk_flags_and_splits(harness, cutoff):
    inp = SS.make_input("k6w2")
    eng = SS.oracle_engine()
    SS.load(eng, inp)
    eng.set_classifier(SS.align_classifier(cutoff))
    run = SS.run_align(eng, inp, cutoff)
    assert all(d["rc"] == 0 for _, d in run.trace)
    assert any(tag == "scan_ident" and d["n_flagged"] > 0 for tag, d in run.trace)
    assert any(tag == "scan" and d["n_flagged"] > 0 and d["nw_pairs"] > d["n_flagged"] for tag, d in run.trace)
    parts = [d for tag, d in run.trace if tag == "align_part"]
    assert parts and all(d["pairs"] > 0 and d["cells"] > 0 for d in parts)


def test_mean_shift_cases_and_errors(harness):
    inp, h, ref, _ = scenario("k4w1")
    eng = SS.oracle_engine()
    SS.load(eng, inp)
    eng.set_classifier(SS.make_classifier(inp, eng))
    centres, off, members = SS.mean_shift_cases(inp)
    sizes = np.diff(off.astype(np.int64))
    assert (sizes == 1).any() and len(centres) >= 10
    assert any((h[members[int(off[j]):int(off[j + 1])]][1:] == h[members[int(off[j])]]).all(axis=1).any()
               for j in range(len(centres)) if sizes[j] > 1), "no exact copies in one cluster"
    tr = SS.run_mean_shift(eng, inp)
    assert all(d["rc"] == 0 for _, d in tr)
    moved = [d for t, d in tr if t == "mean_shift" and d["new"] != tuple(int(x) for x in centres)]
    assert moved
    full = {d["delta"]: d["new"] for t, d in tr if t == "mean_shift"}
    for t, d in tr:  # a range is that slice of the whole iteration
        if t == "mean_shift_range":
            assert d["new"] == full[d["delta"]][d["j0"]:d["j1"]]
    errs = dict([d for t, d in SS.run_errors(eng, inp).trace if t == "errors"][0]["rcs"])
    assert all(rc == 1 for rc in errs.values()), errs  # MC_ERR_ARG, every one
