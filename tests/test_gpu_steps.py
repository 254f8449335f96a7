"""The get_close / mean-shift step API of libmcgpu against the CPU oracle engine, call by call.

Every script of step_scenarios.py runs on the GPU engine and on oracle/_build/
libmcoracle_engine.so (each call restated serially in double precision) in one process; the two
traces -- every return code, mc_scan_result field, flagged list, identity, pairs / cells count
and new centre -- must be equal, doubles bit for bit.  One test per table row (histogram shape:
the kernels' branches) and script family, so a failure names the branch.  What makes the inputs
worth comparing (ties of the first maximum across lanes, waves and workgroups, get_mean ties
against the position order, the flagged counts where the kernels change path) is checked
without a GPU in test_step_scenarios_host.py.
"""
import numpy as np
import pytest

import meshclust_amd as M
import step_scenarios as SS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng(built):
    M.build()
    e = M.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module", params=sorted(SS.ROWS))
def pair(eng, request):
    """(input, GPU engine, oracle engine) of one table row, both loaded, the same classifier."""
    inp = SS.make_input(request.param)
    cpu = SS.oracle_engine()
    SS.load(cpu, inp)
    cls = SS.make_classifier(inp, cpu)
    cpu.set_classifier(cls)
    SS.load(eng, inp)
    eng.set_classifier(cls)
    yield inp, eng, cpu
    cpu.close()


def same(gpu_trace, cpu_trace):
    d = SS.diff(gpu_trace, cpu_trace)
    assert d is None, "GPU vs oracle: " + d


def test_histograms(pair):
    inp, eng, cpu = pair
    hg, mg = eng.histograms()
    hc, mc = cpu.histograms()
    assert np.array_equal(hg, hc) and np.array_equal(mg, mc)


def test_walk(pair):
    """(a) clusters grown step by step over windows of every geometry, with deferred kills."""
    inp, eng, cpu = pair
    sharded = inp.row in SS.FUSED
    same(SS.run_walk(eng, inp, sharded=sharded).trace, SS.run_walk(cpu, inp, sharded=sharded).trace)


def test_sharded_steps(pair):
    """(b) mc_scan_part / mc_scan_commit: every part equals the oracle's, and the parts combined by
    the header's rule are mc_scan's step.  32-bit histograms: MC_ERR_UNSUPPORTED."""
    inp, eng, cpu = pair
    if inp.row not in SS.FUSED:
        eng.set_order(inp.order)
        assert eng.scan_part(int(inp.order[0]), 0, inp.n - 1, 0, 2)[0] == M.ERR_UNSUPPORTED
        assert eng.scan_commit(np.array([1], np.uint32))[0] == M.ERR_UNSUPPORTED
        return
    g, cases = SS.run_sharded(eng, inp)
    same(g.trace, SS.run_sharded(cpu, inp)[0].trace)
    SS.check_sharded(cases)


@pytest.mark.parametrize("through_parts", [False, True], ids=["fused", "parts"])
def test_cluster_whose_first_step_flags_nothing(pair, through_parts):
    """(e) mc_cluster_begin, a step that flags nothing, then a step of the same cluster that does:
    the cluster's column sums start from its first member, not from the cluster before."""
    inp, eng, cpu = pair
    if through_parts and inp.row not in SS.FUSED:
        through_parts = False  # (no sharded steps on 32-bit histograms: the whole-step form again)
    same(SS.run_msum(eng, inp, through_parts).trace, SS.run_msum(cpu, inp, through_parts).trace)


def test_mean_shift(pair):
    """(d) mc_mean_shift and mc_mean_shift_range over member lists with exact copies and clusters
    of one point, delta 0, 2 and C, whole, empty and interior ranges."""
    inp, eng, cpu = pair
    same(SS.run_mean_shift(eng, inp), SS.run_mean_shift(cpu, inp))


def test_error_codes(pair):
    """(f) the same code from both engines; the state survives the errors that promise it."""
    inp, eng, cpu = pair
    same(SS.run_errors(eng, inp).trace, SS.run_errors(cpu, inp).trace)


@pytest.mark.parametrize("cutoff", [0.55, 0.9])
def test_alignment_mode(eng, cutoff):
    """(c) mc_scan in alignment mode, and mc_align_part (1, 2, 3 parts) interleaved back into
    mc_scan_ident; a context of its own, so that the rows' loads stay."""
    inp = SS.make_input("k6w2")
    cpu, gpu = SS.oracle_engine(), M.Engine(0)
    try:
        for e in (cpu, gpu):
            SS.load(e, inp)
            e.set_classifier(SS.align_classifier(cutoff))
        same(SS.run_align(gpu, inp, cutoff).trace, SS.run_align(cpu, inp, cutoff).trace)
    finally:
        gpu.close()
        cpu.close()
