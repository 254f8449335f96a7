#!/usr/bin/env python3
"""What clustering on both strands costs and what it finds: meshclust --both-strands against the
plain run, on the seeded synthetic workload of bench.py (config B: 100k x 1 kb, 1000 templates,
--id 0.90) with every second read of each template reverse-complemented (read i is flipped iff
(i // T) % 2 == 1).

Parity first: on the flipped file the canonical rows (mc_kmer_build_strands) and mc_orient_pairs
of a sample are compared with their numpy restatement on the forward rows; a mismatch stops the
script before anything is timed.

Then, per mode (plain, --both-strands at the automatic k, --both-strands --kmer 4; --steps timed
end-to-end steps after one warm-up, parse -> .clstr written):
  reads/s end to end, training ms, accumulation us per step, clusters found and reads misplaced
  against the templates (a read is misplaced when its cluster's majority template is not its own),
and on the resident sequences K1 and the fold by HIP events (mc_timers: "kmer" is K1, "layout" the
fold kernel of mc_kmer_max_strands / mc_kmer_build_strands).

Prints one JSON line and writes it to --out (default bench_out/strands_bench.json).  No number
here has a threshold.
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

BOTH = M.MC_STRAND_PLUS | M.MC_STRAND_MINUS
COMP = bytes.maketrans(b"ACGT", b"TGCA")


def flip_file(src, dst, T):
    """Every second read of each template reverse-complemented; returns the reads' templates."""
    templates = []
    with open(src, "rb") as f, open(dst + ".tmp", "wb") as o:
        hdr, seq = None, []

        def put():
            if hdr is None:
                return
            i = len(templates)
            templates.append(int(hdr.split(b"template_")[1]))
            s = b"".join(seq)
            if (i // T) % 2 == 1:
                s = s.translate(COMP)[::-1]
            o.write(hdr + b"\n")
            for j in range(0, len(s), 60):
                o.write(s[j:j + 60] + b"\n")

        for line in f:
            line = line.rstrip(b"\r\n")
            if line.startswith(b">"):
                put()
                hdr, seq = line, []
            elif line:
                seq.append(line)
        put()
    os.replace(dst + ".tmp", dst)
    return np.array(templates)


def rc_perm(k):
    i = np.arange(4 ** k, dtype=np.int64)
    r = np.zeros_like(i)
    for _ in range(k):
        r = (r << 2) | (3 - (i & 3))
        i = i >> 2
    return r


def partition_quality(clstr_path, templates):
    """(clusters, misplaced): a read is misplaced when its cluster's majority template is not its own."""
    clusters, misplaced, cur = 0, 0, []

    def close():
        nonlocal clusters, misplaced
        if cur:
            clusters += 1
            t = templates[np.array(cur)]
            misplaced += len(t) - np.bincount(t).max()

    with open(clstr_path) as f:
        for line in f:
            if line.startswith(">Cluster"):
                close()
                cur = []
            elif line.strip():
                cur.append(int(line.split(">read")[1].split()[0].rstrip(".")))
    close()
    return clusters, int(misplaced)


def parity(eng, k, sample=512):
    """Canonical rows and orientations of a sample against numpy on the forward rows."""
    largest = eng.kmer_max(k)
    width = 1 if largest <= 0xff else 2
    eng.kmer_build(k, width)
    fwd = eng.histograms()[0][:sample].astype(np.int64)
    cmax = eng.kmer_max_strands(k, BOTH)
    cwidth = 1 if cmax <= 0xff else 2
    eng.kmer_build_strands(k, cwidth, BOTH)
    h, mag = eng.histograms()
    perm = rc_perm(k)
    want = fwd + fwd[:, perm] - 1
    ok = bool(np.array_equal(h[:sample].astype(np.int64), want)) and bool(np.array_equal(mag[:sample].astype(np.int64), want.sum(axis=1)))
    ok = ok and int(h.max()) == cmax
    a = np.arange(sample, dtype=np.uint32)
    b = np.repeat(np.arange(0, sample, 16), 16).astype(np.uint32)[:sample]
    strand, sad = eng.orient_pairs(a, b)
    plus = np.abs(fwd[a] - fwd[b]).sum(axis=1)
    minus = np.abs(fwd[a] - fwd[b][:, perm]).sum(axis=1)
    ok = ok and bool(np.array_equal(sad[:, 0], plus.astype(np.uint64))) and bool(np.array_equal(sad[:, 1], minus.astype(np.uint64)))
    ok = ok and bool(np.array_equal(strand, (minus < plus).astype(np.uint8)))
    return ok, {"k": k, "forward_max": int(largest), "canonical_max": int(cmax), "forward_width": width, "canonical_width": cwidth}


def device_times(eng, k, width, cwidth, reps):
    """K1 and the fold on the resident sequences, ms per call from HIP events."""
    out = {}
    eng.timers(reset=True)
    for _ in range(reps):
        eng.kmer_max(k)
        eng.kmer_build(k, width)
    t = eng.timers(reset=True)
    out["plain_k1_ms"] = round(t["kmer"][0] / reps, 4)
    out["plain_k1_launches"] = t["kmer"][1] // reps
    for _ in range(reps):
        eng.kmer_max_strands(k, BOTH)
        eng.kmer_build_strands(k, cwidth, BOTH)
    t = eng.timers(reset=True)
    out["both_k1_ms"] = round(t["kmer"][0] / reps, 4)
    out["both_k1_launches"] = t["kmer"][1] // reps
    out["fold_ms"] = round(t["layout"][0] / reps, 4)  # the maximum pass and the writing pass together
    out["fold_launches"] = t["layout"][1] // reps
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=sorted(bench.WORKLOADS), default="B")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--id", default="0.90")
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "strands_bench.json"))
    a = ap.parse_args()
    n, T, seed = bench.WORKLOADS[a.workload]
    fa = bench.ensure_fasta(n, 1000, T, 0.03, seed)
    flipped = os.path.join(os.path.dirname(fa), "flipped_" + os.path.basename(fa))
    templates = flip_file(fa, flipped, T)
    assert len(templates) == n
    eng = M.Engine(0)
    line = {"workload": a.workload, "n": n, "templates": T, "id": float(a.id), "steps": a.steps, "flipped_reads": int(((np.arange(n) // T) % 2).sum())}
    out_dir = tempfile.mkdtemp(prefix="mc_strands_bench")
    try:
        ds = M.Dataset([flipped], threads=a.threads)
        st = ds.run(eng, ("--id", a.id, "--both-strands"))
        k_auto = st["k"]
        line["parity"] = {}
        for k in sorted({k_auto, 4}):
            ok, info = parity(eng, k)
            line["parity"]["k%d" % k] = dict(info, ok=ok)
            if not ok:
                print(json.dumps(line))
                sys.exit("parity failed at k = %d: nothing timed" % k)
            line["device_k%d" % k] = device_times(eng, k, info["forward_width"], info["canonical_width"], 5)
        del ds
        modes = {"plain": [], "both": ["--both-strands"], "both_k4": ["--both-strands", "--kmer", "4"]}
        for name, extra in modes.items():
            args = tuple(["--id", a.id] + extra)
            runs = []
            for step in range(a.steps + 1):  # the first one warms up
                clstr = os.path.join(out_dir, "%s_%d.clstr" % (name, step))
                eng.sync()
                t0 = time.perf_counter()
                ds = M.Dataset([flipped], threads=a.threads)
                st = ds.run(eng, args, upload=True, clstr=clstr)
                eng.sync()
                el = time.perf_counter() - t0
                del ds
                if step:
                    runs.append((el, st))
            el = sorted(r[0] for r in runs)
            st = runs[-1][1]
            ph = st["phases_ms"]
            clusters, misplaced = partition_quality(clstr, templates)
            line[name] = {
                "k": st["k"], "width": st["width"], "clusters": clusters, "misplaced": misplaced,
                "reads_per_s": round(n / el[len(el) // 2], 1), "step_s_min_med_max": [round(el[0], 4), round(el[len(el) // 2], 4), round(el[-1], 4)],
                "train_ms": round(float(np.median([r[1]["phases_ms"]["train"] for r in runs])), 3),
                "kmer_ms": round(float(np.median([r[1]["phases_ms"]["kmer"] for r in runs])), 3),
                "accumulate_ms": round(ph["accumulate"], 3), "scan_steps": st["scan_steps"],
                "accumulate_us_per_step": round(1000.0 * ph["accumulate"] / max(1, st["scan_steps"]), 3),
                "accum_path": st.get("accum_path"), "nw_pairs": st["nw_pairs"], "members_minus": st.get("members_minus"),
                "orient_ms": round(ph.get("orient", 0.0), 3),
            }
    finally:
        eng.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(line, f, indent=1)
    print(json.dumps(line))


if __name__ == "__main__":
    main()
