#!/usr/bin/env python3
"""Device and wall time of mc_nw_msa_sites beside the only way to the same bytes without it:
mc_nw_msa_rows for every pair row and a numpy take of the site columns on the host.

The workload is scripts/msa_bench.py's and scripts/profile_bench.py's: the seeded synthetic reads of
bench.py (config B: 100k x 1 kb, --id 0.90) clustered, every read assigned to the centres of its own
clustering, the pairs (assigned read, its centre) sorted by centre, every second read on the minus
strand.  One mc_nw_msa_begin leaves the plan and one mc_nw_msa_counts the profile; the sites are
host/variants.hpp's rule on it (--min-frac 0.2, --min-count 2 by default).  Then per round, in this
order: one mc_nw_msa_sites over every pair (device ms of its kernels from mc_nw_msa_sites_profile,
wall time around the call), and one mc_nw_msa_rows over every pair row (render device ms, wall time)
followed by the host's take of the site columns from the returned text (wall time; the index of the
take is built once, outside the timing).  The first round checks that the two are byte-equal.
--plus drops the minus-strand flags: the flagged reads of the default workload are plus-strand reads
aligned reverse-complemented, rows that disagree with their cluster almost everywhere, so it has
many more sites than a cluster of reads that belong together.
Medians over --rounds (default 5) after --warmup; one JSON line with the bytes each way returns."""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import bench  # noqa: E402  (the workload table and the FASTA cache)
import meshclust_amd as M  # noqa: E402


def variant_sites(counts, min_frac, min_count):
    """host/variants.hpp's rule over a whole table at once -> a flag per column."""
    n = np.sort(counts[:, [0, 1, 2, 3, 5]].astype(np.int64), axis=1)
    second, D = n[:, -2], n.sum(axis=1)
    return (second >= min_count) & (second.astype(np.float64) >= min_frac * D.astype(np.float64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=sorted(bench.WORKLOADS), default="B")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--id", type=float, default=0.90)
    ap.add_argument("--min-frac", type=float, default=0.2)
    ap.add_argument("--min-count", type=int, default=2)
    ap.add_argument("--plus", action="store_true", help="every read as written (no minus-strand flags): clusters that agree with themselves")
    a = ap.parse_args()
    n, templates, seed = bench.WORKLOADS[a.workload]
    fasta = bench.ensure_fasta(n, 1000, templates, 0.03, seed)
    tmp = tempfile.mkdtemp(prefix="mc_sites_bench")
    model, cen = os.path.join(tmp, "model.txt"), os.path.join(tmp, "centres.fa")
    ds = M.Dataset([fasta], threads=16)
    eng = M.Engine(0)
    ds.run(eng, ["--id", str(a.id), "--save-model", model, "--save-centres", cen])
    ids = {ds.lib.mcl_header(ds.h, i): i for i in range(ds.n)}
    centres = np.array([ids[ln.rstrip(b"\n")] for ln in open(cen, "rb") if ln.startswith(b">")], np.uint32)
    queries = np.arange(ds.n, dtype=np.uint32)
    best = eng.assign(centres, queries, a.id)[0]
    has = best != M.ASSIGN_NONE
    qa, cb = queries[has], centres[best[has]]
    order = np.argsort(cb, kind="stable")  # sorted by centre, as meshclust-assign sends them
    qa, cb = qa[order], cb[order]
    am = np.zeros(len(qa), np.uint8) if a.plus else (np.arange(len(qa)) % 2).astype(np.uint8)
    targets, depth = np.unique(cb, return_counts=True)
    m, nt = len(qa), len(targets)
    off, width, bw, _, _, _ = eng.nw_msa_begin(qa, cb, am, targets)
    col_off, counts = eng.nw_msa_counts(0, nt)
    flag = variant_sites(counts, a.min_frac, a.min_count)
    cols = np.nonzero(flag)[0]
    tcol = np.searchsorted(col_off, cols, side="right") - 1  # the target of every site
    sites = (cols - col_off[tcol].astype(np.int64)).astype(np.uint32)
    site_off = np.concatenate([[0], np.cumsum(np.bincount(tcol, minlength=nt))]).astype(np.uint64)
    nsites = len(sites)
    slot_sites = int((counts[cols, 7] != 0).sum())
    soff = eng.nw_msa_sites(site_off, sites, 0, m, alleles=False)[0]
    sbytes = int(soff[-1])
    roff = eng.nw_msa_rows(nt, m, rows=False)[1]
    nbytes = int(roff[-1])
    # the take's index: for pair k the site columns of its target, in its row
    tof = np.searchsorted(targets, cb)
    per = np.diff(site_off.astype(np.int64))[tof]
    first = np.repeat(site_off[:-1].astype(np.int64)[tof], per)  # the first site of the pair's target, once per byte
    within = np.arange(int(per.sum())) - np.repeat(np.cumsum(per) - per, per)
    index = np.repeat(roff[:-1].astype(np.int64), per) + sites[first + within].astype(np.int64)
    assert len(index) == sbytes
    keys = ("sites_wall", "sites_kernels", "rows_wall", "rows_render", "host_take_wall")
    t = {k: [] for k in keys}
    for r in range(a.warmup + a.rounds):
        al = np.zeros(sbytes, np.uint8)
        o1 = np.zeros(m + 1, np.uint64)
        eng.nw_msa_sites_profile(reset=True)
        t0 = time.perf_counter()
        rc = eng.lib.mc_nw_msa_sites(eng.ctx, M._p(site_off), M._p(sites), C.c_uint64(0), C.c_uint64(m), M._p(al), None, C.c_uint64(sbytes),
                                     M._p(o1))
        w_sites = time.perf_counter() - t0
        assert rc == 0, rc
        k_sites = eng.nw_msa_sites_profile()
        out = np.zeros(nbytes, np.uint8)
        o2 = np.zeros(m + 1, np.uint64)
        eng.nw_msa_profile(reset=True)
        t0 = time.perf_counter()
        rc = eng.lib.mc_nw_msa_rows(eng.ctx, C.c_uint64(nt), C.c_uint64(m), M._p(out), C.c_uint64(nbytes), M._p(o2))
        w_rows = time.perf_counter() - t0
        assert rc == 0, rc
        render = eng.nw_msa_profile()[3]
        t0 = time.perf_counter()
        taken = out[index]
        w_host = time.perf_counter() - t0
        if r == 0:  # what the tests pin, once more at this size
            assert np.array_equal(o1, soff) and np.array_equal(taken, al)
        if r >= a.warmup:
            for k, v in zip(keys, (1e3 * w_sites, k_sites, 1e3 * w_rows, render, 1e3 * w_host)):
                t[k].append(float(v))
    eng.nw_msa_end()
    med = {k: float(np.median(v)) for k, v in t.items()}
    line = {
        "workload": "config %s: %d assigned reads x 1 kb on %d centres, %s" % (a.workload, m, nt, "every read as written" if a.plus else
                                                                                  "every second read on the minus strand"),
        "rounds": a.rounds, "warmup": a.warmup, "pairs": m, "targets": nt, "columns": int(col_off[-1]), "min_frac": a.min_frac,
        "min_count": a.min_count, "sites": nsites, "slot_sites": slot_sites, "targets_with_sites": int((np.diff(site_off.astype(np.int64)) > 0).sum()),
        "sites_bytes": sbytes, "rows_bytes": nbytes,
        **{k + "_ms": round(v, 3) for k, v in med.items()},
        **{k + "_ms_all": [round(x, 3) for x in v] for k, v in t.items()},
        "rows_and_take_wall_ms": round(med["rows_wall"] + med["host_take_wall"], 3),
        "sites_kernels_over_render": round(med["sites_kernels"] / med["rows_render"], 4),
        "sites_wall_over_rows_and_take_wall": round(med["sites_wall"] / (med["rows_wall"] + med["host_take_wall"]), 4),
        "rows_bytes_over_sites_bytes": round(nbytes / sbytes, 2) if sbytes else None,
    }
    print(json.dumps(line))


if __name__ == "__main__":
    main()
