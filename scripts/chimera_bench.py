#!/usr/bin/env python3
"""Device and wall time of mc_nw_msa_crossover beside the only way to the same values without it:
mc_nw_align_strands on both (read, parent) pairs with the operation words copied back, and a walk of
the two CIGARs of every read on the host.

The workload is scripts/msa_bench.py's and scripts/sites_bench.py's: the seeded synthetic reads of
bench.py (config B: 100k x 1 kb, --id 0.90) clustered and every read scored against the centres of its
own clustering (mc_assign_top, K = 2).  Every read with a hit gets two pairs: its best centre, and its
second hit -- or, where it has only one, the centre that follows the best one in the centres file (an
unrelated parent: an alignment of many short runs, the costlier kind for both routes).  --reads N takes the
first N such reads.  Per round, in this order: one mc_nw_msa_begin over the 2 N pairs (wall time), one
mc_nw_msa_crossover over the N candidates (device ms of its kernel from mc_nw_msa_crossover_profile, wall
time around the call), and the other route: one mc_nw_align_strands over the same pairs with the words
(wall time) and the host walk, numpy over ranges of candidates (wall time; a compiled walk would be faster,
so the two parts are reported apart).  The first round asserts that the two routes give equal values.
Medians over --rounds (default 3) after --warmup; one JSON line with the bytes each way returns."""
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


def host_walk(cig, cig_off, la, step=4096):
    """The eight values of every candidate c = (pair 2c, pair 2c + 1) from the words alone, the definition
    of include/meshclust_amd.h in numpy (every pair as written: the benchmark has no minus pairs)."""
    nc = len(la)
    out = np.zeros((nc, M.CROSS_RES), np.int32)
    for c0 in range(0, nc, step):
        c1 = min(nc, c0 + step)
        w = cig[int(cig_off[2 * c0]):int(cig_off[2 * c1])]
        n, op = (w >> 4).astype(np.int64), w & 15
        on = (op == M.CIGAR_EQ) | (op == M.CIGAR_X) | (op == M.CIGAR_I)
        e = np.repeat((op == M.CIGAR_EQ)[on], n[on]).astype(np.int8)  # per read base, pair after pair
        L = la[c0:c1].astype(np.int64)
        assert len(e) == 2 * int(L.sum())
        start = np.concatenate([[0], np.cumsum(np.repeat(L, 2))])  # where a pair's bases start
        idx = np.repeat(np.arange(c1 - c0), L)
        pos = np.arange(int(L.sum())) - np.repeat(np.cumsum(L) - L, L)  # the base within its read
        ex, ey = e[start[2 * idx] + pos], e[start[2 * idx + 1] + pos]
        seg = np.concatenate([[0], np.cumsum(L)])[:-1]
        cs = np.cumsum(ex.astype(np.int64) - ey)
        D = cs - np.repeat(np.concatenate([[0], cs])[seg], L)  # D(s), s = pos + 1
        s = pos + 1
        big = 1 << 20
        ids = np.add.reduceat(np.stack([ex, ey]).astype(np.int64), seg, axis=1)
        for col, sign in ((2, 1), (5, -1)):  # the maximum, then the minimum as the maximum of -D; s = 0 holds D = 0
            first = np.maximum.reduceat(sign * D * big + (big - 1 - s), seg)
            last = np.maximum.reduceat(sign * D * big + s, seg)
            hi = np.maximum(first >> 20, 0)
            f = np.where((first >> 20) > 0, big - 1 - (first & (big - 1)), 0)
            l = np.where((last >> 20) >= 0, last & (big - 1), 0)
            out[c0:c1, col] = (ids[1] if sign > 0 else ids[0]) + hi
            out[c0:c1, col + 1], out[c0:c1, col + 2] = f, l
        out[c0:c1, 0], out[c0:c1, 1] = ids[0], ids[1]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=sorted(bench.WORKLOADS), default="B")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--id", type=float, default=0.90)
    ap.add_argument("--reads", type=int, default=0, help="the first N reads with a hit (0: all)")
    a = ap.parse_args()
    n, templates, seed = bench.WORKLOADS[a.workload]
    fasta = bench.ensure_fasta(n, 1000, templates, 0.03, seed)
    tmp = tempfile.mkdtemp(prefix="mc_chimera_bench")
    model, cen = os.path.join(tmp, "model.txt"), os.path.join(tmp, "centres.fa")
    ds = M.Dataset([fasta], threads=16)
    eng = M.Engine(0)
    ds.run(eng, ["--id", str(a.id), "--save-model", model, "--save-centres", cen])
    ids = {ds.lib.mcl_header(ds.h, i): i for i in range(ds.n)}
    centres = np.array([ids[ln.rstrip(b"\n")] for ln in open(cen, "rb") if ln.startswith(b">")], np.uint32)
    queries = np.arange(ds.n, dtype=np.uint32)
    hit = eng.assign_top(centres, queries, a.id, k=2)[0]
    has = hit[:, 0] != M.ASSIGN_NONE
    if a.reads:
        has &= np.cumsum(has) <= a.reads
    reads, h1, h2 = queries[has], hit[has, 0], hit[has, 1]
    second = int((h2 != M.ASSIGN_NONE).sum())
    h2 = np.where(h2 != M.ASSIGN_NONE, h2, (h1 + 1) % len(centres))
    nc = len(reads)
    pa = np.repeat(reads, 2)
    pb = np.stack([centres[h1], centres[h2]], axis=1).reshape(-1)
    targets = np.unique(pb)
    x, y = np.arange(0, 2 * nc, 2, dtype=np.uint64), np.arange(1, 2 * nc, 2, dtype=np.uint64)
    la = None  # the reads' lengths: the bases the words of a read's first pair consume
    keys = ("begin_wall", "crossover_wall", "crossover_kernel", "align_words_wall", "host_walk_wall")
    t = {k: [] for k in keys}
    words = 0
    for r in range(a.warmup + a.rounds):
        t0 = time.perf_counter()
        eng.nw_msa_begin(pa, pb, None, targets)
        w_begin = time.perf_counter() - t0
        out = np.zeros((nc, M.CROSS_RES), np.int32)
        eng.nw_msa_crossover_profile(reset=True)
        t0 = time.perf_counter()
        rc = eng.lib.mc_nw_msa_crossover(eng.ctx, M._p(x), M._p(y), C.c_uint64(nc), M._p(out))
        w_cross = time.perf_counter() - t0
        assert rc == 0, rc
        k_cross = eng.nw_msa_crossover_profile()
        eng.nw_msa_end()
        t0 = time.perf_counter()
        cig, cig_off, _, _, _ = eng.nw_align_strands(pa, pb, None)
        w_align = time.perf_counter() - t0
        words = int(cig_off[-1])
        if la is None:
            nn, op = (cig >> 4).astype(np.int64), cig & 15
            adv = np.concatenate([[0], np.cumsum(np.where((op == M.CIGAR_EQ) | (op == M.CIGAR_X) | (op == M.CIGAR_I), nn, 0))])
            la = adv[cig_off[1::2].astype(np.int64)] - adv[cig_off[:-1:2].astype(np.int64)]
        t0 = time.perf_counter()
        walked = host_walk(cig, cig_off, la)
        w_walk = time.perf_counter() - t0
        if r == 0:  # what the tests pin, once more at this size
            assert np.array_equal(walked, out), np.nonzero((walked != out).any(axis=1))[0][:8]
        if r >= a.warmup:
            for k, v in zip(keys, (1e3 * w_begin, 1e3 * w_cross, k_cross, 1e3 * w_align, 1e3 * w_walk)):
                t[k].append(float(v))
    med = {k: float(np.median(v)) for k, v in t.items()}
    gain = np.maximum(out[:, 2], out[:, 5]) - np.maximum(out[:, 0], out[:, 1])
    line = {
        "workload": "config %s: %d reads x 1 kb, two pairs each on %d centres, %d reads with a second hit of their own" % (a.workload, nc,
                                                                                                                    len(targets), second),
        "rounds": a.rounds, "warmup": a.warmup, "candidates": nc, "pairs": 2 * nc, "operation_words": words,
        "crossover_bytes": int(out.nbytes), "words_bytes": 4 * words, "gain_ge_3": int((gain >= 3).sum()),
        **{k + "_ms": round(v, 3) for k, v in med.items()},
        **{k + "_ms_all": [round(v2, 3) for v2 in v] for k, v in t.items()},
        "new_route_wall_ms": round(med["begin_wall"] + med["crossover_wall"], 3),
        "old_route_wall_ms": round(med["align_words_wall"] + med["host_walk_wall"], 3),
        "words_bytes_over_crossover_bytes": round(4 * words / out.nbytes, 2),
    }
    print(json.dumps(line))


if __name__ == "__main__":
    main()
