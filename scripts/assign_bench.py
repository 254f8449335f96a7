#!/usr/bin/env python3
"""A/B of read assignment: mc_assign against the mc_classify_pairs pair list.

Clusters the seeded synthetic workload of bench.py (config B: 100k x 1 kb, --id 0.90; --workload D:
1M x 1 kb), then assigns the same reads to the final centres two ways, alternating in one process
after a warm-up:

  device  one mc_assign call (stats[2]: kernel time from HIP events; a host clock around the
          synchronised call beside it)
  pairs   what a caller had to do before mc_assign: the candidate pairs of the length gate in
          batches through mc_classify_pairs, the argmax in numpy

Both results are compared for equality first.  Prints one JSON line: both times, their ratio,
candidate pairs per second, bytes and operations per pair from the shape, and the kernel's share
of its bound (which bound is named in the line).

--both-strands also times mc_assign_strands on both strands in every round, right after the
one-strand call, and adds its device time, the spread of both and their ratio to the line.  Its
result is checked first against the header's rule applied in numpy to the one-strand results
of mc_assign_strands (plus alone must equal mc_assign).

--top K also times mc_assign_top in every round, at K = 1, 4, 8 (and K), on plus alone and, with
--both-strands, on both strands, and adds their device times and their ratios to
mc_assign_strands on the same strand set to the line.  Its plus-alone lists are checked first
against a numpy reduction of the pair-list pass (every query's similar centres by combo 0
descending, index ascending, cut at K) on the reads that pass covers; the both-strands lists
against the merge, by the header's order, of the plus-alone and minus-alone lists.

--identity also times the identity phase of meshclust-assign --identity: one mc_nw_identity_strands
call over every (read, its centre) pair, with the reads on one strand (no minus pair) and with every
second read taken on the minus strand (the call reverse-complements those reads on the device: the
work of a file in which every second read is reverse-complemented; NW fills the whole matrix, so
its cost does not depend on what is aligned).  The plus results are checked against mc_nw_identity,
a sample of the minus results against mc_nw_identity_raw on strings reverse-complemented in numpy.
Adds the call's wall time, the NW and reverse-complement kernel times (mc_timers), DP cells per
second, the reverse-complement kernel's bytes per second against the measured HBM copy rate, and
the ratio of the phase to the mc_assign call.

--align also times mc_nw_align_strands (the alignments behind meshclust-assign --paf) over the same
(read, its centre) pairs, every second read on the minus strand, with and without the operation
words, against mc_nw_identity_strands on those pairs (that kernel is the baseline: it does not keep
the path).  Adds the forward and the traceback kernels' device times (mc_nw_align_profile), the
choice bytes the forward pass writes per second, DP cells per second and the ratios; len / ids are
checked against mc_nw_identity_strands first.

--pileup also times mc_nw_pileup_strands (the pile-up behind meshclust-assign --consensus) over the
same (read, its centre) pairs, one pair per read, every second read on the minus strand, beside
mc_nw_align_strands with its operation words on those pairs.  score / len / ids of the two calls
are compared first, and the table's column sums with the sums of the words.  Adds the forward,
traceback and pile-up (+ finish) device times (mc_nw_pileup_profile), the same with an atomic per
column (MC_PILEUP_NAIVE=1; the tables are compared), the bytes each call returns to the host and
the atomics issued per pair against la + lb.

--quality also times mc_nw_qpileup_strands (the pile-up weighed by base quality behind meshclust-assign
--quality) on those pairs with a seeded quality 0 .. 93 on every byte, beside mc_nw_pileup_strands.  The
count table and the integers of the two calls are compared first, and the weights of channels 0..4
with the qualities of the aligned bases.  Adds the two calls' forward, traceback and pile-up
(+ finish) device times, the atomics per pair, and how many columns the lane and the wave run
forms take.

Under rocprofv3 set MC_ACCUM_PLAIN_LAUNCH=1, as scripts/prof_round.sh does: the clustering's
cooperative launch otherwise faults the profiler's exit handler, after the
profile is written.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402  (the workload table and the FASTA cache)
import meshclust_amd as M  # noqa: E402

SIMDS, CLOCK_HZ = 256 * 4, 2.4e9  # MI355X: 256 CUs x 4 SIMDs, ~2.4 GHz
HBM_COPY_BPS = 6.29e12  # MI355X: measured float4 copy rate (8.0 TB/s spec)


def pairs_pass(eng, centres, queries, lens, sim, batch, top=None):
    """The baseline: gate on the host, mc_classify_pairs per batch, argmax on the host.
    Returns (best, val, nsim, candidate pairs, seconds inside mc_classify_pairs).  ``top``: a pair
    of arrays (len(queries), K) that receive every query's K best similar centres and their values
    (combo 0 descending, index ascending; ASSIGN_NONE and -1.0 in the unused slots)."""
    C_ = len(centres)
    lc = lens[centres].astype(np.float64)
    lo = (lc * sim).astype(np.uint64)
    hi = (lc / sim).astype(np.uint64)
    best = np.full(len(queries), M.ASSIGN_NONE, np.uint32)
    val = np.full(len(queries), -1.0)
    nsim = np.zeros(len(queries), np.uint32)
    per = max(1, batch // C_)
    cand, t_call = 0, 0.0
    for q0 in range(0, len(queries), per):
        q = queries[q0:q0 + per]
        lq = lens[q]
        gate = (lo[None, :] <= lq[:, None]) & (lq[:, None] <= hi[None, :])
        qi, cj = np.nonzero(gate)
        t0 = time.perf_counter()
        d, c0, _ = eng.classify_pairs(q[qi], centres[cj])
        t_call += time.perf_counter() - t0
        cand += len(qi)
        m = np.full(gate.shape, -np.inf)
        m[qi[d != 0], cj[d != 0]] = c0[d != 0]
        n = np.zeros(gate.shape, np.uint32)
        n[qi, cj] = d
        ns = n.sum(axis=1)
        b = m.argmax(axis=1)
        has = ns > 0
        best[q0:q0 + len(q)] = np.where(has, b, M.ASSIGN_NONE)
        val[q0:q0 + len(q)] = np.where(has, m[np.arange(len(q)), b], -1.0)
        nsim[q0:q0 + len(q)] = ns
        if top is not None:
            K = top[0].shape[1]
            order = np.argsort(-m, axis=1, kind="stable")[:, :K]  # (a tie keeps the lower index first)
            order = np.pad(order, ((0, 0), (0, K - order.shape[1])))  # (fewer centres than K)
            v = np.take_along_axis(m, order, axis=1)
            used = np.arange(K)[None, :] < np.minimum(ns, min(K, C_))[:, None]
            top[0][q0:q0 + len(q)] = np.where(used, order, M.ASSIGN_NONE)
            top[1][q0:q0 + len(q)] = np.where(used, v, -1.0)
    return best, val, nsim, cand, t_call


def identity_phase(eng, ds, ptr, seq_off, lens, centres, queries, best, a, assign_us):
    """Times mc_nw_identity_strands over every assigned read and its centre -> the keys for the line."""
    has = best != M.ASSIGN_NONE
    qa, cb = queries[has], centres[best[has]]
    cells = int((lens[qa].astype(np.float64) * lens[cb].astype(np.float64)).sum())
    codes = np.ctypeslib.as_array(M.C.cast(ptr[0], M.C.POINTER(M.C.c_uint8)), shape=(int(seq_off[-1]),))
    out = {"identity_pairs": int(len(qa)), "identity_cells": cells}
    plus = eng.nw_identity(qa, cb)
    for name, am in (("one_strand", None), ("alternating", (np.arange(len(qa)) % 2).astype(np.uint8))):
        wall, nw_ms, lay_ms = [], [], []
        for r in range(a.warmup + a.rounds):
            eng.timers(reset=True)
            t0 = time.perf_counter()
            got = eng.nw_identity_strands(qa, cb, am)
            w = time.perf_counter() - t0
            t = eng.timers()
            if r >= a.warmup:
                wall.append(w)
                nw_ms.append(t["nw"][0])
                lay_ms.append(t["layout"][0])
        if am is None:
            assert all(np.array_equal(x, y) for x, y in zip(got, plus)), "no minus pair differs from mc_nw_identity"
        else:
            assert all(np.array_equal(x[am == 0], y[am == 0]) for x, y in zip(got, plus)), "plus pairs differ from mc_nw_identity"
            pick = np.flatnonzero(am)[:256]
            rc = [(3 - codes[int(seq_off[i]):int(seq_off[i + 1])][::-1]).astype(np.uint8) for i in qa[pick]]  # (digits only)
            cs = [codes[int(seq_off[j]):int(seq_off[j + 1])] for j in cb[pick]]
            off = lambda xs: np.concatenate([[0], np.cumsum([len(x) for x in xs])]).astype(np.uint64)  # noqa: E731
            raw = eng.nw_identity_raw(np.concatenate(rc), off(rc), np.concatenate(cs), off(cs))
            assert all(np.array_equal(x[pick], y) for x, y in zip(got, raw[:3])), "minus pairs differ from mc_nw_identity_raw"
        w_s, n_ms, l_ms = float(np.median(wall)), float(np.median(nw_ms)), float(np.median(lay_ms))
        out["identity_%s_call_wall_ms" % name] = round(1e3 * w_s, 3)
        out["identity_%s_call_wall_ms_all" % name] = [round(1e3 * x, 3) for x in wall]
        out["identity_%s_nw_device_ms" % name] = round(n_ms, 3)
        out["identity_%s_cells_per_s" % name] = round(cells / (n_ms * 1e-3), 1)
        out["identity_%s_over_mc_assign" % name] = round(1e3 * w_s / (assign_us * 1e-3), 1)
        if am is not None:
            ids = np.unique(qa[am != 0])
            nbytes = int(lens[ids].sum()) + int(((lens[ids] + 15) // 16 * 16).sum())  # read once, written padded to 16
            out["revseq_reads"] = int(len(ids))
            out["revseq_bytes"] = nbytes
            out["revseq_device_ms"] = round(l_ms, 4)
            out["revseq_device_ms_all"] = [round(x, 4) for x in lay_ms]
            out["revseq_bytes_per_s"] = round(nbytes / (l_ms * 1e-3), 1) if l_ms > 0 else None
            out["revseq_share_of_hbm_copy_rate"] = round(nbytes / (l_ms * 1e-3) / HBM_COPY_BPS, 4) if l_ms > 0 else None
    out["identity_outputs_equal"] = True
    return out


def align_phase(eng, lens, centres, queries, best, a):
    """Times mc_nw_align_strands over every assigned read and its centre (every second read on the
    minus strand) against mc_nw_identity_strands on the same pairs -> the keys for the line."""
    has = best != M.ASSIGN_NONE
    qa, cb = queries[has], centres[best[has]]
    am = (np.arange(len(qa)) % 2).astype(np.uint8)
    cells = int((lens[qa].astype(np.float64) * lens[cb].astype(np.float64)).sum())
    out = {"align_pairs": int(len(qa)), "align_cells": cells}
    res = {}
    for name in ("identity", "align", "align_no_cigar"):
        wall, nw_ms, fwd, tb, chb = [], [], [], [], []
        for r in range(a.warmup + a.rounds):
            eng.timers(reset=True)
            eng.nw_align_profile(reset=True)
            t0 = time.perf_counter()
            if name == "identity":
                got = eng.nw_identity_strands(qa, cb, am)
            else:
                got = eng.nw_align_strands(qa, cb, am, cigar=name == "align")
            w = time.perf_counter() - t0
            t, pr = eng.timers(), eng.nw_align_profile()
            if r >= a.warmup:
                wall.append(w)
                nw_ms.append(t["nw"][0])
                fwd.append(pr[0])
                tb.append(pr[1])
                chb.append(pr[2])
        res[name] = got
        out[name + "_call_wall_ms"] = round(1e3 * float(np.median(wall)), 3)
        out[name + "_call_wall_ms_all"] = [round(1e3 * x, 3) for x in wall]
        out[name + "_nw_device_ms"] = round(float(np.median(nw_ms)), 3)
        if name != "identity":
            f_ms, t_ms = float(np.median(fwd)), float(np.median(tb))
            out[name + "_forward_device_ms"] = round(f_ms, 3)
            out[name + "_forward_device_ms_all"] = [round(x, 3) for x in fwd]
            out[name + "_traceback_device_ms"] = round(t_ms, 3)
            out[name + "_traceback_device_ms_all"] = [round(x, 3) for x in tb]
            out[name + "_choice_bytes"] = int(chb[-1])
            out[name + "_choice_bytes_per_s"] = round(chb[-1] / (f_ms * 1e-3), 1) if f_ms > 0 else None
            out[name + "_forward_cells_per_s"] = round(cells / (f_ms * 1e-3), 1) if f_ms > 0 else None
            out[name + "_device_over_identity"] = round((f_ms + t_ms) / out["identity_nw_device_ms"], 3)
            out[name + "_wall_over_identity"] = round(out[name + "_call_wall_ms"] / out["identity_call_wall_ms"], 3)
    _, ln, ids = res["identity"]
    words, off, _, a_ln, a_ids = res["align"]
    assert np.array_equal(ln, a_ln) and np.array_equal(ids, a_ids), "len / ids differ from mc_nw_identity_strands"
    assert np.array_equal(off, res["align_no_cigar"][1])
    out["align_cigar_ops"] = int(off[-1])
    out["align_outputs_equal"] = True
    return out


def pileup_phase(eng, lens, centres, queries, best, a):
    """Times mc_nw_pileup_strands over every assigned read and its centre (every second read on the
    minus strand) beside mc_nw_align_strands with its words on the same pairs -> the keys for the line."""
    has = best != M.ASSIGN_NONE
    qa, cb = queries[has], centres[best[has]]
    am = (np.arange(len(qa)) % 2).astype(np.uint8)
    targets = np.unique(cb)
    out = {"pileup_pairs": int(len(qa)), "pileup_targets": int(len(targets))}
    res = {}
    for name in ("align", "pileup", "pileup_naive"):
        if name == "pileup_naive":
            os.environ["MC_PILEUP_NAIVE"] = "1"
        wall, fwd, tb, pu = [], [], [], []
        for r in range(a.warmup + a.rounds):
            eng.nw_pileup_profile(reset=True)
            t0 = time.perf_counter()
            got = eng.nw_align_strands(qa, cb, am) if name == "align" else eng.nw_pileup_strands(qa, cb, am, targets)
            w = time.perf_counter() - t0
            pr = eng.nw_pileup_profile()
            if r >= a.warmup:
                wall.append(w)
                fwd.append(pr[0])
                tb.append(pr[1])
                pu.append(pr[2])
        os.environ.pop("MC_PILEUP_NAIVE", None)
        res[name] = got
        out[name + "_call_wall_ms"] = round(1e3 * float(np.median(wall)), 3)
        out[name + "_call_wall_ms_all"] = [round(1e3 * x, 3) for x in wall]
        out[name + "_forward_device_ms"] = round(float(np.median(fwd)), 3)
        out[name + "_traceback_device_ms" + ("_with_pack" if name == "align" else "")] = round(float(np.median(tb)), 3)
        out[name + "_traceback_device_ms_all"] = [round(x, 3) for x in tb]
        if name != "align":
            out[name + "_pileup_finish_device_ms"] = round(float(np.median(pu)), 3)
            out[name + "_pileup_finish_device_ms_all"] = [round(x, 3) for x in pu]
    words, off, sc, ln, ids = res["align"]
    tab, row_off, p_sc, p_ln, p_ids = res["pileup"]
    assert np.array_equal(sc, p_sc) and np.array_equal(ln, p_ln) and np.array_equal(ids, p_ids), "integers differ from mc_nw_align_strands"
    assert all(np.array_equal(x, y) for x, y in zip(res["pileup"], res["pileup_naive"])), "the per-column form gives another table"
    run, op = (words >> 4).astype(np.int64), words & 15
    sums = {k: int(run[op == v].sum()) for k, v in (("eq", M.CIGAR_EQ), ("x", M.CIGAR_X), ("i", M.CIGAR_I), ("d", M.CIGAR_D))}
    n_i = int((op == M.CIGAR_I).sum())
    assert int(tab[:, :5].sum()) == sums["eq"] + sums["x"] and int(tab[:, 5].sum()) == sums["d"], "column sums differ from the words"
    assert int(tab[:, 6].sum()) == n_i and int(tab[:, 7].sum()) == sums["i"], "insertion sums differ from the words"
    assert int(tab[:, :6].sum()) == int(lens[cb].sum()), "a centre column is not covered once per pair"
    m = len(qa)
    atomics = 2 * int((op != M.CIGAR_X).sum()) + sums["x"]
    bases = int(lens[qa].sum()) + int(lens[cb].sum())
    out["pileup_outputs_equal"] = True
    out["align_bytes_to_host"] = int(words.nbytes + off.nbytes + 12 * m)
    out["pileup_bytes_to_host"] = int(tab.nbytes + row_off.nbytes + 12 * m)
    out["pileup_table_rows"] = int(row_off[-1])
    out["pileup_atomics_per_pair"] = round(atomics / m, 2)
    out["pileup_naive_atomics_per_pair"] = round((sums["eq"] + sums["x"] + sums["d"] + 2 * n_i) / m, 2)
    out["pileup_bases_per_pair"] = round(bases / m, 2)
    out["pileup_runs_per_pair"] = round(len(words) / m, 2)
    out["pileup_finish_over_pack_and_download_ms"] = [
        out["pileup_pileup_finish_device_ms"],
        round(out["align_call_wall_ms"] - out["align_forward_device_ms"] - out["pileup_traceback_device_ms"], 3)]
    out["pileup_call_over_align_call"] = round(out["pileup_call_wall_ms"] / out["align_call_wall_ms"], 3)
    return out


def quality_phase(eng, seq_off, centres, queries, best, a):
    """Times mc_nw_qpileup_strands (the pile-up weighed by base quality behind --quality) beside
    mc_nw_pileup_strands on the same pairs: every assigned read and its centre, every second read on
    the minus strand, seeded qualities 0 .. 93 on every byte -> the keys for the line."""
    has = best != M.ASSIGN_NONE
    qa, cb = queries[has], centres[best[has]]
    am = (np.arange(len(qa)) % 2).astype(np.uint8)
    targets = np.unique(cb)
    qual = np.random.default_rng(93).integers(0, M.QUAL_MAX + 1, int(seq_off[-1])).astype(np.uint8)
    eng.load_qualities(qual)
    out = {"quality_pairs": int(len(qa)), "quality_targets": int(len(targets))}
    res = {}
    for name in ("count", "quality"):
        wall, fwd, tb, pu = [], [], [], []
        for r in range(a.warmup + a.rounds):
            eng.nw_pileup_profile(reset=True)
            t0 = time.perf_counter()
            got = eng.nw_pileup_strands(qa, cb, am, targets) if name == "count" else eng.nw_qpileup_strands(qa, cb, am, targets)
            w = time.perf_counter() - t0
            pr = eng.nw_pileup_profile()
            if r >= a.warmup:
                wall.append(w)
                fwd.append(pr[0])
                tb.append(pr[1])
                pu.append(pr[2])
        res[name] = got
        out[name + "_call_wall_ms"] = round(1e3 * float(np.median(wall)), 3)
        out[name + "_call_wall_ms_all"] = [round(1e3 * x, 3) for x in wall]
        out[name + "_forward_device_ms"] = round(float(np.median(fwd)), 3)
        out[name + "_traceback_device_ms"] = round(float(np.median(tb)), 3)
        out[name + "_pileup_finish_device_ms"] = round(float(np.median(pu)), 3)
        out[name + "_pileup_finish_device_ms_all"] = [round(x, 3) for x in pu]
    tab, wtab, row_off, sc, ln, ids = res["quality"]
    assert all(np.array_equal(x, y) for x, y in zip((tab, row_off, sc, ln, ids), res["count"])), "the count table or the integers differ"
    assert not wtab[:, 7].any()
    # with the words: what the weights must add up to, and the atomics the two run forms issue
    words, off, _, _, _ = eng.nw_align_strands(qa, cb, am)
    run, op = (words >> 4).astype(np.int64), words & 15
    pair = np.repeat(np.arange(len(qa)), np.diff(off).astype(np.int64))
    step = np.where(op != M.CIGAR_D, run, 0)
    csum = np.cumsum(step) - step
    start = csum - np.repeat(csum[off[:-1].astype(np.int64)], np.diff(off).astype(np.int64))  # the read bases before a run, in its pair
    ins_q = 0  # the qualities of the inserted bases: they are in no column
    for k in np.nonzero(op == M.CIGAR_I)[0]:
        p, i0, n = int(pair[k]), int(start[k]), int(run[k])
        q = qual[int(seq_off[qa[p]]):int(seq_off[qa[p] + 1])]
        ins_q += int((q[::-1] if am[p] else q)[i0:i0 + n].astype(np.int64).sum())
    read_q = sum(int(qual[int(seq_off[i]):int(seq_off[i + 1])].astype(np.int64).sum()) for i in qa)
    assert int(wtab[:, :5].astype(np.int64).sum()) == read_q - ins_q, "the weights of channels 0..4 are not the aligned bases' qualities"
    col = (op == M.CIGAR_EQ) | (op == M.CIGAR_X) | (op == M.CIGAR_D)
    long_run = run > 8
    m = len(qa)
    out["quality_outputs_equal"] = True
    out["quality_weight_atomics_per_pair"] = round((int(run[col].sum()) + int((op == M.CIGAR_I).sum())) / m, 2)
    out["quality_count_atomics_per_pair"] = round((2 * int((op != M.CIGAR_X).sum()) + int(run[op == M.CIGAR_X].sum())) / m, 2)
    out["quality_columns_by_wave_per_pair"] = round(int(run[col & long_run].sum()) / m, 2)
    out["quality_columns_by_lane_per_pair"] = round(int(run[col & ~long_run].sum()) / m, 2)
    out["quality_long_runs_per_pair"] = round(int((col & long_run).sum()) / m, 2)
    out["quality_runs_per_pair"] = round(len(words) / m, 2)
    out["quality_bytes_to_host"] = int(tab.nbytes + wtab.nbytes + row_off.nbytes + 12 * m)
    out["quality_pileup_over_count_pileup"] = round(out["quality_pileup_finish_device_ms"] / out["count_pileup_finish_device_ms"], 3)
    out["quality_pileup_share_of_kernels"] = round(out["quality_pileup_finish_device_ms"] / (
        out["quality_forward_device_ms"] + out["quality_traceback_device_ms"] + out["quality_pileup_finish_device_ms"]), 4)
    out["quality_call_over_count_call"] = round(out["quality_call_wall_ms"] / out["count_call_wall_ms"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=sorted(bench.WORKLOADS), default="B")
    ap.add_argument("--rounds", type=int, default=3, help="timed device / pairs alternations")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--pairs-rounds", type=int, default=None, help="timed pair-list passes (default: --rounds)")
    ap.add_argument("--pairs-queries", type=int, default=0,
                    help="run the pair list on the first N reads only (0: all); its times are then for those "
                         "reads, and the ratios are per candidate pair (config D: the whole pair list takes minutes)")
    ap.add_argument("--batch", type=int, default=1 << 22, help="pairs per mc_classify_pairs call")
    ap.add_argument("--id", type=float, default=0.90)
    ap.add_argument("--both-strands", action="store_true",
                    help="also time mc_assign_strands on both strands (the centres' permuted rows included)")
    ap.add_argument("--top", type=int, default=0, metavar="K",
                    help="also time mc_assign_top at K = 1, 4, 8 and K (plus alone; with --both-strands both strands too)")
    ap.add_argument("--identity", action="store_true",
                    help="also time the identity phase (mc_nw_identity_strands over every read and its centre), on one "
                         "strand and with every second read on the minus strand")
    ap.add_argument("--align", action="store_true",
                    help="also time mc_nw_align_strands (the alignments behind --paf) over every read and its centre, every "
                         "second read on the minus strand, against mc_nw_identity_strands on the same pairs: forward and "
                         "traceback device time, choice bytes per second, and the ratios")
    ap.add_argument("--pileup", action="store_true",
                    help="also time mc_nw_pileup_strands (the pile-up behind --consensus) over every read and its centre beside "
                         "mc_nw_align_strands on the same pairs: forward, traceback and pile-up device time, bytes returned, "
                         "atomics per pair, and the same with an atomic per column")
    ap.add_argument("--quality", action="store_true",
                    help="also time mc_nw_qpileup_strands (the weighted pile-up behind --quality) beside mc_nw_pileup_strands on "
                         "the same pairs with seeded qualities: pile-up, forward and traceback device time, atomics per pair, and "
                         "the columns the lane and the wave run forms take")
    a = ap.parse_args()
    n, templates, seed = bench.WORKLOADS[a.workload]
    fasta = bench.ensure_fasta(n, 1000, templates, 0.03, seed)
    tmp = tempfile.mkdtemp(prefix="mc_assign_bench")
    model, cen = os.path.join(tmp, "model.txt"), os.path.join(tmp, "centres.fa")
    ds = M.Dataset([fasta], threads=16)
    eng = M.Engine(0)
    st = ds.run(eng, ["--id", str(a.id), "--save-model", model, "--save-centres", cen])
    # the context still holds the reads, their histograms and the trained classifier
    ids = {ds.lib.mcl_header(ds.h, i): i for i in range(ds.n)}
    centres = np.array([ids[ln.rstrip(b"\n")] for ln in open(cen, "rb") if ln.startswith(b">")], np.uint32)
    queries = np.arange(ds.n, dtype=np.uint32)
    npq = a.pairs_queries if 0 < a.pairs_queries < ds.n else ds.n
    seq_off = np.zeros(ds.n + 1, np.uint64)
    ptr = [M.C.c_void_p() for _ in range(4)]
    ds.lib.mcl_view(ds.h, *[M.C.byref(p) for p in ptr])
    seq_off[:] = np.ctypeslib.as_array(M.C.cast(ptr[1], M.C.POINTER(M.C.c_uint64)), shape=(ds.n + 1,))
    lens = np.diff(seq_off).astype(np.uint64)
    k, width = st["k"], st["width"]
    B = 4 ** k
    nch = (B * width + 15) // 16
    dev_us, dev_wall, pair_call, pair_dev_ms, both_us, both_wall = [], [], [], [], [], []
    top_ks = sorted({1, 4, 8, a.top}) if a.top else []
    top_us = {(s, K): [] for K in top_ks for s in ([1, 3] if a.both_strands else [1])}
    plus_us, top_lists = [], {}
    ref = None
    prounds = a.rounds if a.pairs_rounds is None else a.pairs_rounds
    for r in range(a.warmup + a.rounds):
        t0 = time.perf_counter()
        best, val, nsim, stats = eng.assign(centres, queries, a.id)
        wall = time.perf_counter() - t0
        if a.both_strands:
            t0 = time.perf_counter()
            b3 = eng.assign_strands(centres, queries, a.id)
            wall3 = time.perf_counter() - t0
            if r == 0:
                b1 = eng.assign_strands(centres, queries, a.id, M.MC_STRAND_PLUS)
                b2 = eng.assign_strands(centres, queries, a.id, M.MC_STRAND_MINUS)
                assert all(np.array_equal(x, y) for x, y in zip((b1[0], b1[1], b1[3]), (best, val, nsim))), "plus alone differs"
                win = (b2[0] != M.ASSIGN_NONE) & ((b1[0] == M.ASSIGN_NONE) | (b2[1] > b1[1]))
                want = (np.where(win, b2[0], b1[0]), np.where(win, b2[1], b1[1]), win.astype(np.uint8), b1[3] + b2[3])
                assert all(np.array_equal(x, y) for x, y in zip(b3[:4], want)), "both strands differ from the rule"
                assert int(b3[4][0]) == int(stats[0])
                minus_wins, minus_similar = int(win.sum()), int((b2[3] > 0).sum())
            if r >= a.warmup:
                both_us.append(int(b3[4][2]))
                both_wall.append(wall3)
        if a.top:
            p1 = eng.assign_strands(centres, queries, a.id, M.MC_STRAND_PLUS)  # the same entry, the same strand set
            if r >= a.warmup:
                plus_us.append(int(p1[4][2]))
            for (s, K), us in top_us.items():
                t = eng.assign_top(centres, queries, a.id, s, K)
                if r >= a.warmup:
                    us.append(int(t[4][2]))
                if r == 0:
                    top_lists[(s, K)] = t
                    one = p1 if s == 1 else b3
                    assert all(np.array_equal(x[:, 0], y) for x, y in zip(t[:3], one[:3])), "column 0 differs from mc_assign_strands"
                    assert np.array_equal(t[3], one[3]) and int(t[4][0]) == int(one[4][0])
            if r == 0 and a.both_strands:  # both strands: the merge of the one-strand lists, by the header's order
                K8 = M.ASSIGN_MAX_TOP
                tp, tm = top_lists[(1, 8)], eng.assign_top(centres, queries, a.id, M.MC_STRAND_MINUS, K8)
                hj, hv, hs = (np.concatenate([x, y], axis=1) for x, y in zip(tp[:3], tm[:3]))
                empty = hj == M.ASSIGN_NONE
                order = np.lexsort((hj, hs, -hv, empty), axis=-1)  # (empty slots last)
                hj, hv, hs = (np.take_along_axis(x, order, axis=1) for x in (hj, hv, hs))
                for K in top_ks:
                    t = top_lists[(3, K)]
                    assert all(np.array_equal(x, y[:, :K]) for x, y in zip(t[:3], (hj, hv, hs))), "both-strands lists differ from the merge"
                    assert np.array_equal(t[3], tp[3] + tm[3])
        if r == 0 or r - a.warmup < prounds:
            eng.timers(reset=True)
            ptop = (np.zeros((npq, max(top_ks)), np.uint32), np.zeros((npq, max(top_ks)))) if a.top and r == 0 else None
            pb, pv, pn, pcand, t_call = pairs_pass(eng, centres, queries[:npq], lens, a.id, a.batch, ptop)
            if ptop is not None:
                for K in top_ks:
                    t = top_lists[(1, K)]
                    assert np.array_equal(t[0][:npq], ptop[0][:, :K]) and np.array_equal(t[1][:npq], ptop[1][:, :K]), \
                        "mc_assign_top differs from the pair list's reduction"
                    assert not t[2].any() and np.array_equal(t[3][:npq], pn)
                top_truncated = {K: int((pn > K).sum()) for K in top_ks}
            pdev = eng.timers()["pairs"][0]
            assert np.array_equal(best[:npq], pb) and np.array_equal(val[:npq], pv) and np.array_equal(nsim[:npq], pn), \
                "outputs differ"
            assert npq < ds.n or int(stats[0]) == pcand, (int(stats[0]), pcand)
            if r >= a.warmup:
                pair_call.append(t_call)
                pair_dev_ms.append(pdev)
        if ref is None:
            ref = (best.copy(), val.copy(), nsim.copy())
        assert all(np.array_equal(x, y) for x, y in zip(ref, (best, val, nsim))), "mc_assign is not repeatable"
        if r >= a.warmup:
            dev_us.append(int(stats[2]))
            dev_wall.append(wall)
    cand = int(stats[0])
    d_us = float(np.median(dev_us))
    p_dev_ms = float(np.median(pair_dev_ms))
    p_call_s = float(np.median(pair_call))
    short = width == 1 and nch <= 16
    # per pair, from the shape: every chunk is 4 v_sad_u8 + 4 v_dot4_u32_u8 (8-bit rows); the
    # centre's row comes from LDS (nch + 3 broadcast 16-byte reads), the query's row from registers;
    # HBM / L2 traffic per pair: the query's row and results once per query, the centre tile once
    # per workgroup of 256 queries
    int_ops = 8 * nch if width == 1 else 0
    lds_bytes = 16 * (nch + 3)
    mem_bytes = (nch * 16 + 40) / max(1, len(centres)) + (nch + 3) * 16 / 256.0
    floor_pairs_s = SIMDS * 64 * CLOCK_HZ / (2.0 * int_ops) if int_ops else None
    line = {
        "workload": "config %s: %d reads x 1 kb assigned to the %d centres of their own clustering (--id %s, k %d, %d-bit)" % (
            a.workload, ds.n, len(centres), a.id, k, 8 * width),
        "form": "short" if short and not os.environ.get("MC_ASSIGN_FORM") else "general",
        "candidate_pairs": cand,
        "fallback_pairs": int(stats[1]),
        "assigned": int((best != M.ASSIGN_NONE).sum()),
        "mc_assign_device_us": d_us,
        "mc_assign_device_us_all": dev_us,
        "mc_assign_call_wall_ms": round(1e3 * float(np.median(dev_wall)), 3),
        "pairs_kernel_device_ms": round(p_dev_ms, 3),
        "pairs_calls_wall_ms": round(1e3 * p_call_s, 3),
        "pairs_reads": npq,
        "pairs_candidate_pairs": pcand,
        "ratio_device_time": round((p_dev_ms * 1e3 / pcand) / (d_us / cand), 2),
        "ratio_call_time": round((p_call_s / pcand) / (float(np.median(dev_wall)) / cand), 2),
        "mc_assign_pairs_per_s": round(cand / (d_us * 1e-6), 1),
        "per_pair": {"packed_int_valu_ops": int_ops, "lds_bytes": lds_bytes, "hbm_l2_bytes": round(mem_bytes, 3),
                     "pair_list_hbm_l2_bytes": 2 * nch * 16 + 8 + 17},
        "bound": "VALU issue: the %d packed-integer instructions per pair alone, 2 cycles each per wave64 on a 32-wide SIMD, %d SIMDs at %.1f GHz"
                 % (int_ops, SIMDS, CLOCK_HZ / 1e9),
        "bound_pairs_per_s": floor_pairs_s,
        "share_of_bound": round(cand / (d_us * 1e-6) / floor_pairs_s, 4) if floor_pairs_s else None,
        "outputs_equal": True,
    }
    if a.both_strands:
        b_us = float(np.median(both_us))
        line.update({
            "both_strands_device_us": b_us,
            "both_strands_device_us_all": both_us,
            "both_strands_call_wall_ms": round(1e3 * float(np.median(both_wall)), 3),
            "both_over_plus_device_time": round(b_us / d_us, 3),
            "both_strands_fallback_pairs": int(b3[4][1]),
            "both_strands_minus_wins": minus_wins,
            "both_strands_queries_similar_on_minus": minus_similar,
            "both_strands_outputs_equal": True,
        })
    if a.top:
        line["top_plus_alone_assign_strands_device_us"] = float(np.median(plus_us))
        line["top_plus_alone_assign_strands_device_us_all"] = plus_us
        line["top_reads_with_more_than_K_similar"] = {str(K): n for K, n in top_truncated.items()}
        for (s, K), us in top_us.items():
            name = "top_%s_K%d" % ("plus" if s == 1 else "both", K)
            base = float(np.median(plus_us)) if s == 1 else float(np.median(both_us))
            line[name + "_device_us"] = float(np.median(us))
            line[name + "_device_us_all"] = us
            line[name + "_over_assign_strands"] = round(float(np.median(us)) / base, 3)
        line["top_outputs_equal"] = True
    if a.identity:
        line.update(identity_phase(eng, ds, ptr, seq_off, lens, centres, queries, best, a, d_us))
    if a.align:
        line.update(align_phase(eng, lens, centres, queries, best, a))
    if a.pileup:
        line.update(pileup_phase(eng, lens, centres, queries, best, a))
    if a.quality:
        line.update(quality_phase(eng, seq_off, centres, queries, best, a))
    print(json.dumps(line))
    eng.close()


if __name__ == "__main__":
    main()
