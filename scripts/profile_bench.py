#!/usr/bin/env python3
"""Device and wall time of mc_nw_msa_counts beside the only way to the same numbers without it:
mc_nw_msa_rows for every pair row and a numpy column count on the host.

The workload is scripts/msa_bench.py's: the seeded synthetic reads of bench.py (config B: 100k x
1 kb, --id 0.90) clustered, every read assigned to the centres of its own clustering, the pairs
(assigned read, its centre) sorted by centre, every second read on the minus strand.  One
mc_nw_msa_begin leaves the plan; then per round, in this order: one mc_nw_msa_counts over every
target (device ms of its kernels from mc_nw_msa_counts_profile, wall time around the call), and one
mc_nw_msa_rows over every pair row (render device ms, wall time) followed by the host's count of the
returned text per column and class (wall time).  The first round checks that the two agree.  Medians
over --rounds (default 5) after --warmup; one JSON line with the bytes each way returns."""
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

CLASS = np.full(256, 4, np.uint8)
for _c, _x in enumerate(b"ACGT"):
    CLASS[_x] = _c
CLASS[M.MSA_GAP] = 5


def host_count(text, off, depth, width):
    """The column histogram of the rendered pair rows: per target its depth rows of width bytes,
    one after the other in text -> counts[sum(width), 6]."""
    out = np.zeros((int(width.sum()), 6), np.uint32)
    at = col = 0
    for d, w in zip(depth, width):
        d, w = int(d), int(w)
        cls = CLASS[text[at:at + d * w]].reshape(d, w)
        for ch in range(6):
            out[col:col + w, ch] = (cls == ch).sum(axis=0)
        at += d * w
        col += w
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=sorted(bench.WORKLOADS), default="B")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--id", type=float, default=0.90)
    a = ap.parse_args()
    n, templates, seed = bench.WORKLOADS[a.workload]
    fasta = bench.ensure_fasta(n, 1000, templates, 0.03, seed)
    tmp = tempfile.mkdtemp(prefix="mc_profile_bench")
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
    am = (np.arange(len(qa)) % 2).astype(np.uint8)
    targets, depth = np.unique(cb, return_counts=True)
    m, nt = len(qa), len(targets)
    off, width, bw, _, _, _ = eng.nw_msa_begin(qa, cb, am, targets)
    cols = int(bw.sum())
    keys = ("counts_wall", "counts_kernels", "rows_wall", "rows_render", "host_count_wall")
    t = {k: [] for k in keys}
    roff = eng.nw_msa_rows(nt, m, rows=False)[1]
    nbytes = int(roff[-1])
    for r in range(a.warmup + a.rounds):
        col_off = np.zeros(nt + 1, np.uint64)
        counts = np.zeros((cols, M.MSA_CH), np.uint32)
        eng.nw_msa_counts_profile(reset=True)
        t0 = time.perf_counter()
        rc = eng.lib.mc_nw_msa_counts(eng.ctx, C.c_uint32(0), C.c_uint32(nt), M._p(col_off), M._p(counts), None, C.c_uint64(cols))
        w_counts = time.perf_counter() - t0
        assert rc == 0, rc
        k_counts = eng.nw_msa_counts_profile()
        out = np.zeros(nbytes, np.uint8)
        o2 = np.zeros(m + 1, np.uint64)
        eng.nw_msa_profile(reset=True)
        t0 = time.perf_counter()
        rc = eng.lib.mc_nw_msa_rows(eng.ctx, C.c_uint64(nt), C.c_uint64(m), M._p(out), C.c_uint64(nbytes), M._p(o2))
        w_rows = time.perf_counter() - t0
        assert rc == 0, rc
        render = eng.nw_msa_profile()[3]
        t0 = time.perf_counter()
        hist = host_count(out, o2, depth, bw)
        w_host = time.perf_counter() - t0
        if r == 0:  # what the tests pin, once more at this size
            assert np.array_equal(hist, counts[:, :6]) and (counts[:, :6].sum(axis=1) == np.repeat(depth, bw.astype(np.int64))).all()
        if r >= a.warmup:
            for k, v in zip(keys, (1e3 * w_counts, k_counts, 1e3 * w_rows, render, 1e3 * w_host)):
                t[k].append(float(v))
    eng.nw_msa_end()
    med = {k: float(np.median(v)) for k, v in t.items()}
    line = {
        "workload": "config %s: %d assigned reads x 1 kb on %d centres, every second read on the minus strand" % (a.workload, m, nt),
        "rounds": a.rounds, "warmup": a.warmup, "pairs": m, "targets": nt, "columns": cols, "slot_columns": int(width.sum()),
        "counts_bytes": cols * M.MSA_CH * 4, "rows_bytes": nbytes,
        **{k + "_ms": round(v, 3) for k, v in med.items()},
        **{k + "_ms_all": [round(x, 3) for x in v] for k, v in t.items()},
        "render_and_count_wall_ms": round(med["rows_wall"] + med["host_count_wall"], 3),
        "counts_kernels_over_render": round(med["counts_kernels"] / med["rows_render"], 3),
        "counts_wall_over_render_and_count_wall": round(med["counts_wall"] / (med["rows_wall"] + med["host_count_wall"]), 4),
        "rows_bytes_over_counts_bytes": round(nbytes / (cols * M.MSA_CH * 4), 2),
    }
    print(json.dumps(line))


if __name__ == "__main__":
    main()
