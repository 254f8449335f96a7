#!/usr/bin/env python3
"""mc_nw_align_strands with the certified band off and on (mc_set_align_band), in one
process and one session: one warm-up call and --rounds timed calls each, the band off first.

Workloads:
  B      the seeded synthetic reads of bench.py (config B: 100k x 1 kb, --id 0.90) clustered, every
         read assigned to the centres of its own clustering; the pairs (assigned read, its centre) as
         scripts/assign_bench.py --align builds them, every second read on the minus strand (--strands
         alt, the default) or every read as written (--strands plus)
  E9100  scripts/configs.py's E9100 (70 families x 130 genomes of 8-12 kb, --id 0.80) clustered, every
         genome against the centre of its own cluster, as written
Per mode: the call's host time, forward / traceback (+ pack) / search device ms (HIP events:
mc_nw_align_profile, mc_nw_band_profile), choice bytes, trace batches (the forward timer's count),
search launches; with the band on the distribution of the planned w and the share of full pairs.
--w0 n,n,...: beside that, one mc_nw_band_plan per value with MC_BAND_W0 set (after one warm-up):
its host time, search device ms and launches.  The results of the two modes are compared with ==
before anything is reported.  One JSON line, also written to <--out>/band_bench_<name>.json."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import bench  # noqa: E402  (the workload table and the FASTA cache)
import configs  # noqa: E402
import meshclust_amd as M  # noqa: E402


def pairs_of(a):
    """-> (engine, seq1 ids, seq2 ids, strand flags, lengths, description)"""
    tmp = tempfile.mkdtemp(prefix="mc_band_bench")
    model, cen = os.path.join(tmp, "model.txt"), os.path.join(tmp, "centres.fa")
    if a.workload == "E9100":
        gen, flags, _, desc = configs.CONFIGS["E9100"]
        d = os.path.join(tempfile.gettempdir(), "mc_cfg")
        os.makedirs(d, exist_ok=True)
        fasta = configs.make_input(gen, os.path.join(d, "E9100.fa"))
        sim = float(flags[1])
    else:
        n, templates, seed = bench.WORKLOADS[a.workload]
        fasta = bench.ensure_fasta(n, 1000, templates, 0.03, seed)
        flags, sim, desc = ["--id", "0.90"], 0.90, "config %s: %d x 1 kb, --id 0.90" % (a.workload, n)
    ds = M.Dataset([fasta], threads=16)
    eng = M.Engine(0)
    out = os.path.join(tmp, "out.clstr")
    ds.run(eng, flags + ["--save-model", model, "--save-centres", cen], clstr=out)
    ids = {ds.lib.mcl_header(ds.h, i): i for i in range(ds.n)}
    off = np.zeros(ds.n + 1, np.uint64)
    eng._ck(eng.lib.mc_revcomp_sequences(eng.ctx, M._p(np.arange(ds.n, dtype=np.uint32)), M.C.c_uint64(ds.n), None, M._p(off)),
            "mc_revcomp_sequences")  # (the lengths: no device work)
    lens = np.diff(off).astype(np.int64)
    if a.workload == "E9100":  # every genome against the centre of its own cluster, from the cluster file
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import clstr
        names = {}
        for h, i in ids.items():
            h = h.decode()
            for key in (h, h[1:], h.split()[0], h[1:].split()[0]):
                names.setdefault(key, i)
        qa, cb = [], []
        for cl in clstr.parse(out):
            c = names[cl["centre"]] if cl["centre"] in names else names[cl["centre"].split()[0]]
            for hdr, _ in cl["members"]:
                qa.append(names[hdr] if hdr in names else names[hdr.split()[0]])
                cb.append(c)
        order = np.argsort(qa)
        qa, cb = np.array(qa, np.uint32)[order], np.array(cb, np.uint32)[order]
        assert len(qa) == ds.n
        return eng, ds, qa, cb, np.zeros(len(qa), np.uint8), lens, desc
    centres = np.array([ids[ln.rstrip(b"\n")] for ln in open(cen, "rb") if ln.startswith(b">")], np.uint32)
    queries = np.arange(ds.n, dtype=np.uint32)
    best = eng.assign(centres, queries, sim)[0]
    has = best != M.ASSIGN_NONE
    qa, cb = queries[has], centres[best[has]]
    am = (np.arange(len(qa)) % 2).astype(np.uint8) if a.workload != "E9100" and a.strands == "alt" else np.zeros(len(qa), np.uint8)
    return eng, ds, qa, cb, am, lens, desc


def spread(v):
    return {"median": round(float(np.median(v)), 3), "min": round(float(min(v)), 3), "max": round(float(max(v)), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=sorted(bench.WORKLOADS) + ["E9100"], default="B")
    ap.add_argument("--strands", choices=["alt", "plus"], default="alt")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--w0", default="", help="comma-separated first widths to time mc_nw_band_plan at")
    ap.add_argument("--limit", type=int, default=0, help="use the first N pairs only (rehearsals)")
    ap.add_argument("--tag", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_out"), help="the directory the JSON line is also written to")
    a = ap.parse_args()
    eng, ds, qa, cb, am, lens, desc = pairs_of(a)
    if a.limit:
        qa, cb, am = qa[:a.limit], cb[:a.limit], am[:a.limit]
    os.environ.pop("MC_BAND_W0", None)
    line = {"workload": desc, "strands": a.strands if a.workload != "E9100" else "plus", "pairs": int(len(qa)),
            "cells": int((lens[qa].astype(np.float64) * lens[cb].astype(np.float64)).sum()), "rounds": a.rounds, "warmup": a.warmup}
    res = {}
    for mode in (0, 1):
        eng.set_align_band(mode)
        wall, fwd, tb, search = [], [], [], []
        for r in range(a.warmup + a.rounds):
            eng.timers(reset=True)
            eng.nw_align_profile(reset=True)
            eng.nw_band_profile(reset=True)
            t0 = time.perf_counter()
            got = eng.nw_align_strands(qa, cb, am)
            w = time.perf_counter() - t0
            pr, bp = eng.nw_align_profile(), eng.nw_band_profile()
            # every trace batch is timed three times as "nw" (forward, traceback, pack), every search launch once
            batches = (eng.timers()["nw"][1] - bp[2]) // 3
            if r >= a.warmup:
                wall.append(1e3 * w)
                fwd.append(pr[0])
                tb.append(pr[1])
                search.append(bp[3])
        res[mode] = got
        name = "band_on" if mode else "band_off"
        line[name] = {"call_wall_ms": spread(wall), "forward_device_ms": spread(fwd), "traceback_device_ms": spread(tb),
                      "search_device_ms": spread(search), "choice_bytes": int(pr[2]), "trace_batches": int(batches), "search_launches": bp[2],
                      "pairs_banded": bp[0], "pairs_full": bp[1], "planned_w_sum": bp[4]}
    assert all(x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(res[0], res[1])), "the band changed a result"
    line["results_equal"] = True
    w, score = eng.nw_band_plan(qa, cb, am)
    wb = w[w >= 0]
    line["full_share"] = round(float((w < 0).mean()), 5)
    line["planned_w"] = {"min": int(wb.min()), "p50": int(np.percentile(wb, 50)), "p90": int(np.percentile(wb, 90)),
                         "p99": int(np.percentile(wb, 99)), "max": int(wb.max()), "mean": round(float(wb.mean()), 2)} if len(wb) else None
    on, off = line["band_on"], line["band_off"]
    line["choice_bytes_on_over_off"] = round(on["choice_bytes"] / off["choice_bytes"], 4)
    line["device_ms_on_over_off"] = round((on["forward_device_ms"]["median"] + on["traceback_device_ms"]["median"] + on["search_device_ms"]["median"]) /
                                          (off["forward_device_ms"]["median"] + off["traceback_device_ms"]["median"]), 4)
    line["call_wall_on_over_off"] = round(on["call_wall_ms"]["median"] / off["call_wall_ms"]["median"], 4)
    sweep = {}
    for w0 in [int(x) for x in a.w0.split(",") if x]:
        os.environ["MC_BAND_W0"] = str(w0)
        wall, dev = [], []
        for r in range(a.warmup + a.rounds):
            eng.nw_band_profile(reset=True)
            t0 = time.perf_counter()
            w2, s2 = eng.nw_band_plan(qa, cb, am)
            t = 1e3 * (time.perf_counter() - t0)
            bp = eng.nw_band_profile()
            if r >= a.warmup:
                wall.append(t)
                dev.append(bp[3])
        assert np.array_equal(w2, w) and np.array_equal(s2, score), "the plan depends on w0"
        sweep[str(w0)] = {"plan_wall_ms": spread(wall), "search_device_ms": spread(dev), "search_launches": bp[2]}
    os.environ.pop("MC_BAND_W0", None)
    if sweep:
        line["w0_sweep"] = sweep
    eng.set_align_band(0)
    print(json.dumps(line))
    out = a.out
    os.makedirs(out, exist_ok=True)
    tag = a.workload + ("_" + a.strands if a.workload != "E9100" else "") + (("_" + a.tag) if a.tag else "")
    with open(os.path.join(out, "band_bench_%s.json" % tag), "w") as f:
        f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
