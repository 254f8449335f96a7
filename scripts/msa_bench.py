#!/usr/bin/env python3
"""Device time of mc_nw_msa_begin / mc_nw_msa_rows beside mc_nw_pileup_strands on the same pairs.

The workload is the one scripts/assign_bench.py builds: the seeded synthetic reads of bench.py
(config B: 100k x 1 kb, --id 0.90) clustered, then every read assigned to the centres of its own
clustering; the pairs are (assigned read, its centre), every second read on the minus strand.  Per
round, in this order: one mc_nw_pileup_strands call (forward, traceback, pile-up + finish device ms:
code this feature does not touch), one mc_nw_msa_begin (forward, traceback + pack, width + column
device ms) and one mc_nw_msa_rows over every row (render device ms; the call's wall time less the
render is the copy back and the host's share).  The render kernel's stored bytes per second are set
beside a hipMemsetAsync of the same byte count, timed with HIP events on a buffer of its own: a
store-only yardstick.  Medians over --rounds (default 5) after --warmup; one JSON line."""
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


def memset_ms(nbytes, rounds, warmup):
    """Median device ms of hipMemsetAsync over nbytes, by HIP events."""
    hip = C.CDLL("libamdhip64.so")
    ptr, e0, e1, ms = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_float()

    def ck(rc, what):
        if rc != 0:
            raise RuntimeError("%s failed: %d" % (what, rc))

    ck(hip.hipMalloc(C.byref(ptr), C.c_size_t(nbytes)), "hipMalloc")
    ck(hip.hipEventCreate(C.byref(e0)), "hipEventCreate")
    ck(hip.hipEventCreate(C.byref(e1)), "hipEventCreate")
    out = []
    try:
        for r in range(warmup + rounds):
            ck(hip.hipEventRecord(e0, None), "hipEventRecord")
            ck(hip.hipMemsetAsync(ptr, C.c_int(45), C.c_size_t(nbytes), None), "hipMemsetAsync")
            ck(hip.hipEventRecord(e1, None), "hipEventRecord")
            ck(hip.hipEventSynchronize(e1), "hipEventSynchronize")
            ck(hip.hipEventElapsedTime(C.byref(ms), e0, e1), "hipEventElapsedTime")
            if r >= warmup:
                out.append(ms.value)
    finally:
        hip.hipEventDestroy(e0)
        hip.hipEventDestroy(e1)
        hip.hipFree(ptr)
    return float(np.median(out)), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=sorted(bench.WORKLOADS), default="B")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--id", type=float, default=0.90)
    a = ap.parse_args()
    n, templates, seed = bench.WORKLOADS[a.workload]
    fasta = bench.ensure_fasta(n, 1000, templates, 0.03, seed)
    tmp = tempfile.mkdtemp(prefix="mc_msa_bench")
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
    order = np.argsort(cb, kind="stable")  # sorted by centre, as meshclust-assign --msa sends them
    qa, cb = qa[order], cb[order]
    am = (np.arange(len(qa)) % 2).astype(np.uint8)
    targets = np.unique(cb)
    m, nt = len(qa), len(targets)
    keys = ("pileup_wall", "pileup_forward", "pileup_traceback", "pileup_kernels", "begin_wall", "begin_forward", "begin_traceback_pack",
            "begin_width_column", "rows_wall", "rows_render")
    t = {k: [] for k in keys}
    nbytes = 0
    for r in range(a.warmup + a.rounds):
        eng.nw_pileup_profile(reset=True)
        t0 = time.perf_counter()
        tab = eng.nw_pileup_strands(qa, cb, am, targets)[0]
        w_pile = time.perf_counter() - t0
        pile = eng.nw_pileup_profile()
        eng.nw_msa_profile(reset=True)
        t0 = time.perf_counter()
        off, width, bw, sc, ln, idn = eng.nw_msa_begin(qa, cb, am, targets)
        w_begin = time.perf_counter() - t0
        begin = eng.nw_msa_profile(reset=True)
        roff = eng.nw_msa_rows(0, nt + m, rows=False)[1]
        nbytes = int(roff[-1])
        out = np.zeros(nbytes, np.uint8)
        o2 = np.zeros(nt + m + 1, np.uint64)
        t0 = time.perf_counter()
        rc = eng.lib.mc_nw_msa_rows(eng.ctx, C.c_uint64(0), C.c_uint64(nt + m), M._p(out), C.c_uint64(nbytes), M._p(o2))
        w_rows = time.perf_counter() - t0
        assert rc == 0, rc
        render = eng.nw_msa_profile()[3]
        if r == 0:  # what the tests pin, once more at this size
            assert np.array_equal(width > 0, tab[:, 6] > 0) and (width <= tab[:, 7]).all()
            assert int((out != M.MSA_GAP).sum()) == int(np.diff(ds_lens(ds))[np.concatenate([targets, qa])].sum())
        if r >= a.warmup:
            for k, v in zip(keys, (1e3 * w_pile, pile[0], pile[1], pile[2], 1e3 * w_begin, begin[0], begin[1], begin[2], 1e3 * w_rows, render)):
                t[k].append(float(v))
    eng.nw_msa_end()
    ms_set, all_set = memset_ms(nbytes, a.rounds, a.warmup)
    med = {k: float(np.median(v)) for k, v in t.items()}
    line = {
        "workload": "config %s: %d assigned reads x 1 kb on %d centres, every second read on the minus strand" % (a.workload, m, nt),
        "rounds": a.rounds, "warmup": a.warmup, "rows": nt + m, "row_bytes": nbytes, "columns": int(bw.sum()),
        "slot_columns": int(width.sum()),
        **{k + "_ms": round(v, 3) for k, v in med.items()},
        **{k + "_ms_all": [round(x, 3) for x in v] for k, v in t.items()},
        "rows_copy_back_and_host_ms": round(med["rows_wall"] - med["rows_render"], 3),
        "render_gb_per_s": round(nbytes / med["rows_render"] / 1e6, 2),
        "memset_ms": round(ms_set, 3), "memset_ms_all": [round(x, 3) for x in all_set],
        "memset_gb_per_s": round(nbytes / ms_set / 1e6, 2),
        "render_over_memset": round(med["rows_render"] / ms_set, 2),
        "width_column_over_pileup_kernels": round(med["begin_width_column"] / med["pileup_kernels"], 3),
        "begin_device_over_pileup_device": round((med["begin_forward"] + med["begin_traceback_pack"] + med["begin_width_column"]) /
                                                 (med["pileup_forward"] + med["pileup_traceback"] + med["pileup_kernels"]), 3),
    }
    print(json.dumps(line))


def ds_lens(ds):
    """The dataset's record offsets (n + 1)."""
    ptr = [M.C.c_void_p() for _ in range(4)]
    ds.lib.mcl_view(ds.h, *[M.C.byref(p) for p in ptr])
    return np.ctypeslib.as_array(M.C.cast(ptr[1], M.C.POINTER(M.C.c_uint64)), shape=(ds.n + 1,)).astype(np.int64)


if __name__ == "__main__":
    main()
