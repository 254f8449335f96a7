#!/usr/bin/env python3
"""Device and wall time of mc_derep beside derep_host (host/derep.hpp) on the same bytes.

The input is config B's seeded synthetic reads of bench.py (100k x 1 kb) made redundant: every read is repeated
with a skewed multiplicity (min(zipf(2), 64): most reads once, a few dozens of times), half of the copies reverse-complemented
(the minus-strand string of host/revseq.hpp), then the whole set shuffled, seeded.  The bytes are loaded once
with mc_load_sequences and stay resident; both routes dereplicate all points on both strands.
Per round, in this order: one mc_derep over all points (wall time around the call; device ms of the
fingerprint and of the compare kernel, pairs, rounds and collisions from mc_derep_profile), then derep_host on
the same bytes in host memory (wall time; its orientation and hashing pass runs on OMP_NUM_THREADS threads,
16 at most, the class map on one).  The first round asserts that the two routes give the same rep and minus.
Medians over --rounds (default 3) after --warmup; one JSON line, with the bytes that come back from the device.
--reads N takes the first N reads of the workload before they are multiplied."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import bench  # noqa: E402  (the workload table and the FASTA cache)
import meshclust_amd as M  # noqa: E402

BOTH = M.MC_STRAND_PLUS | M.MC_STRAND_MINUS


def expanded(ds):
    """the parsed reads' expanded bytes and offsets (mcl_view)"""
    ptr = [C.c_void_p() for _ in range(4)]
    ds.lib.mcl_view(ds.h, *[C.byref(p) for p in ptr])
    seq_off = np.ctypeslib.as_array(C.cast(ptr[1], C.POINTER(C.c_uint64)), shape=(ds.n + 1,)).copy()
    codes = np.ctypeslib.as_array(C.cast(ptr[0], C.POINTER(C.c_uint8)), shape=(int(seq_off[-1]),)).copy()
    return codes, seq_off


def redundant(codes, seq_off, seed):
    rng = np.random.default_rng(seed)
    n = len(seq_off) - 1
    mult = np.minimum(rng.zipf(2.0, n), 64)
    src = np.repeat(np.arange(n), mult)
    flip = rng.random(len(src)) < 0.5
    order = rng.permutation(len(src))
    src, flip = src[order], flip[order]
    lens = (seq_off[1:] - seq_off[:-1]).astype(np.int64)[src]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    rcmap = np.arange(256, dtype=np.uint8)
    rcmap[:4] = [3, 2, 1, 0]
    for a, b in ("AT", "CG"):
        rcmap[ord(a)], rcmap[ord(b)] = ord(b), ord(a)
    out = np.empty(int(off[-1]), np.uint8)
    for k in range(len(src)):
        s = codes[int(seq_off[src[k]]):int(seq_off[src[k] + 1])]
        out[int(off[k]):int(off[k + 1])] = rcmap[s[::-1]] if flip[k] else s
    return out, off, src, flip, mult


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=sorted(bench.WORKLOADS), default="B")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reads", type=int, default=0, help="the first N reads of the workload (0: all)")
    ap.add_argument("--seed", type=int, default=11)
    a = ap.parse_args()
    n, templates, seed = bench.WORKLOADS[a.workload]
    fasta = bench.ensure_fasta(n, 1000, templates, 0.03, seed)
    ds = M.Dataset([fasta], threads=16)
    codes, seq_off = expanded(ds)
    if a.reads:
        seq_off = seq_off[: a.reads + 1]
        codes = codes[: int(seq_off[-1])]
    codes, seq_off, src, flip, mult = redundant(codes, seq_off, a.seed)
    m = len(src)
    lens = (seq_off[1:] - seq_off[:-1]).astype(np.int64)
    seg = np.stack([np.zeros(m, np.int64), lens - 1], axis=1).astype(np.int32).reshape(-1)
    eng = M.Engine(0)
    eng.load_sequences(codes, seq_off, seg, np.arange(m + 1, dtype=np.uint64))
    ids = np.arange(m, dtype=np.uint32)
    keys = ("derep_wall", "fingerprint_kernel", "compare_kernel", "host_wall")
    t = {k: [] for k in keys}
    prof = None
    for r in range(a.warmup + a.rounds):
        rep = np.zeros(m, np.uint32)
        minus = np.zeros(m, np.uint8)
        eng.derep_profile(reset=True)
        t0 = time.perf_counter()
        rc = eng.lib.mc_derep(eng.ctx, M._p(ids), C.c_uint64(m), BOTH, M._p(rep), M._p(minus))
        w_dev = time.perf_counter() - t0
        assert rc == 0, rc
        prof = eng.derep_profile()
        t0 = time.perf_counter()
        hrep, hminus = M.derep_host(codes, seq_off, ids, BOTH)
        w_host = time.perf_counter() - t0
        if r == 0:  # what the tests pin, once more at this size
            assert np.array_equal(rep, hrep) and np.array_equal(minus, hminus)
        if r >= a.warmup:
            for k, v in zip(keys, (1e3 * w_dev, prof["fingerprint_ms"], prof["compare_ms"], 1e3 * w_host)):
                t[k].append(float(v))
    med = {k: float(np.median(v)) for k, v in t.items()}
    uniques = int((rep == np.arange(m)).sum())
    line = {
        "workload": "config %s: %d reads x 1 kb, multiplied to %d (largest multiplicity %d), half of the copies reverse-complemented, shuffled"
                    % (a.workload, len(mult), m, int(mult.max())),
        "rounds": a.rounds, "warmup": a.warmup, "points": m, "bytes": int(seq_off[-1]), "strands": BOTH, "uniques": uniques,
        "mean_multiplicity": round(float(mult.mean()), 2), "minus": int(minus.sum()), "pairs": prof["pairs"], "compare_rounds": prof["rounds"], "collisions": prof["collisions"],
        "key_bytes": 16 * m, "compare_bytes": prof["pairs"], "bytes_returned": 16 * m + prof["pairs"],
        "host_threads": "hashing pass: OMP_NUM_THREADS=%s; class map: 1" % os.environ.get("OMP_NUM_THREADS", "unset"),
        **{k + "_ms": round(v, 3) for k, v in med.items()},
        **{k + "_ms_all": [round(v2, 3) for v2 in v] for k, v in t.items()},
        "fingerprint_gb_per_s": round(int(seq_off[-1]) / med["fingerprint_kernel"] / 1e6, 1) if med["fingerprint_kernel"] else None,
        "host_wall_over_derep_wall": round(med["host_wall"] / med["derep_wall"], 2),
    }
    print(json.dumps(line))


if __name__ == "__main__":
    main()
