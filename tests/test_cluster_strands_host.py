"""meshclust --both-strands, the parts that need no GPU: the numpy restatement of the canonical row
against the CPU oracle's histogram of the doubled record, the new entries of libmcgpu and how
bin/meshclust refers to them (weak: the CPU harness has none of them), the option errors, the
model text, and the choice of k."""
import os
import subprocess

import numpy as np
import pytest

import fixtures
import meshclust_amd as M
import oracle_lib as O
import strand_cluster_cases as S

ROOT = fixtures.HERE.rsplit(os.sep, 1)[0]
HOST_SRC = os.path.join(ROOT, "meshclust_amd", "csrc", "host")
BUILD = os.path.join(ROOT, "oracle", "_build")
HARNESS = os.path.join(BUILD, "meshclust_cpu")
ENTRIES = ["mc_kmer_max_strands", "mc_kmer_build_strands", "mc_orient_pairs"]
MODEL_KEYS = ["k", "id", "align", "n_single", "lookup", "is_sim", "mins", "maxs", "n_combo", "combo_kind", "combo_len",
              "combo_idx", "weights", "centres"]


@pytest.fixture(scope="module")
def host_built(built):
    M.build()
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "harness"], check=True)


def records():
    rng = np.random.default_rng(3)
    out = [(rng.integers(0, 4, n).astype(np.uint8), [[0, n - 1]]) for n in (20, 33, 257, 500)]
    a, b = rng.integers(0, 4, 70).astype(np.uint8), rng.integers(0, 4, 45).astype(np.uint8)
    out.append((np.concatenate([a, np.full(6, S.N, np.uint8), b]), [[0, 69], [76, 120]]))  # an N gap
    s = rng.integers(0, 4, 100).astype(np.uint8)
    out.append((np.concatenate([s, 3 - s[::-1]]).astype(np.uint8), [[0, 199]]))  # a reverse palindrome
    out.append((np.concatenate([np.zeros(150, np.uint8), np.full(150, 3, np.uint8)]), [[0, 299]]))  # A x 150 || T x 150
    out.append((np.full(30, S.N, np.uint8), []))  # no segment
    return out


@pytest.mark.parametrize("k", [1, 3, 4, 5, 6])
def test_canonical_row_is_the_histogram_of_the_doubled_record(built, k):
    perm = S.rc_perm(k)
    assert np.array_equal(perm[perm], np.arange(4 ** k))  # an involution
    assert (perm == np.arange(4 ** k)).sum() == (0 if k % 2 else 4 ** (k // 2))
    for i, (codes, segs) in enumerate(records()):
        row = O.kmer_hist(codes, segs, k).astype(np.int64)
        rc_codes, rc_segs = S.revcomp(codes, segs)
        assert np.array_equal(O.kmer_hist(rc_codes, rc_segs, k).astype(np.int64), row[perm]), i
        canon = S.canon_rows(row, k)
        dc, dsegs = S.doubled(codes, segs)
        assert len(dc) == 2 * len(codes) + 30 and len(dsegs) == 2 * len(segs)
        assert np.array_equal(O.kmer_hist(dc, dsegs, k).astype(np.int64), canon), i
        assert np.array_equal(S.canon_rows(row[perm], k), canon)  # the record and its reverse complement
        assert canon.sum() == 2 * row.sum() - 4 ** k and canon.min() >= 1
        strand, plus, minus = S.orient(row, row[perm], k)
        assert minus == 0 and strand == (1 if plus > 0 else 0)  # against its own reverse complement
        assert S.orient(row, row, k)[0] == 0
    pal = O.kmer_hist(*records()[5], k).astype(np.int64)
    assert np.array_equal(pal, pal[perm]) and S.orient(pal, pal, k)[0] == 0  # the tie goes to plus
    if k == 4:
        poly = O.kmer_hist(*records()[6], k).astype(np.int64)
        assert poly.max() == 148 and S.canon_rows(poly, k).max() == 295  # 8 bits forward, 16 canonical


def test_flip_rule():
    assert [bool(S.flipped(i, 3)) for i in range(9)] == [False] * 3 + [True] * 3 + [False] * 3


def test_new_entries_are_exported_and_weak_in_the_cli(host_built):
    lib = M.gpu_lib()
    header = open(M.HEADER).read()
    for name in ENTRIES:
        assert hasattr(lib, name), name
        assert "int %s(mc_ctx *ctx" % name in header, name
    assert lib.mc_abi_version() == 1
    for name in ("kmer_max_strands", "kmer_build_strands", "orient_pairs"):
        assert hasattr(M.Engine, name)
    sym = subprocess.run(["nm", "-D", "--undefined-only", M.BIN], capture_output=True, text=True, check=True).stdout
    kinds = {ln.split()[-1]: ln.split()[-2] for ln in sym.splitlines() if ln.strip()}
    for name in ENTRIES + ["mc_nw_identity_strands"]:
        assert kinds.get(name) == "w", (name, kinds.get(name))
    assert kinds.get("mc_kmer_build") == "U"


def run_harness(fa, flags, extra, tmp_path):
    return subprocess.run([HARNESS, fa] + flags + ["--output", str(tmp_path / "o.clstr"), "--quiet"] + extra,
                          capture_output=True, text=True, timeout=300)


def test_cpu_engine_refuses_both_strands_by_name(host_built, tmp_path):
    fa, flags = fixtures.e2e_input("a1k", tmp_path)
    r = run_harness(fa, flags, ["--both-strands"], tmp_path)
    assert r.returncode == 1 and "engine" in r.stderr and "mc_kmer_build_strands" in r.stderr, (r.returncode, r.stderr)
    assert not (tmp_path / "o.clstr").exists()


def test_usage_errors(host_built, tmp_path):
    fa, flags = fixtures.e2e_input("a1k", tmp_path)
    bad = run_harness(fa, flags, ["--iterations", "0"], tmp_path)  # the exit code of other option errors
    assert bad.returncode != 0
    for extra, words in ((["--both-strands", "--align"], ["--both-strands", "--align"]),
                         (["--strands", str(tmp_path / "s.tsv")], ["--strands", "--both-strands"]),
                         (["--both-strands", "--id", "0.5"], ["--both-strands", "--id", "--align"])):
        r = run_harness(fa, flags, extra, tmp_path)  # (a repeated --id: the last one counts)
        assert r.returncode == bad.returncode and all(w in r.stderr for w in words), (extra, r.returncode, r.stderr)
        assert not (tmp_path / "o.clstr").exists() and not (tmp_path / "s.tsv").exists()
    usage = subprocess.run([HARNESS], capture_output=True, text=True, timeout=60)
    assert "--both-strands" in usage.stdout and "--strands FILE" in usage.stdout


def test_model_text_options_and_k_native(host_built, tmp_path):
    exe = str(tmp_path / "cluster_strands_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-fopenmp", "-ffp-contract=off", "-I", HOST_SRC,
                    os.path.join(fixtures.HERE, "native", "cluster_strands_check.cpp"), "-L", BUILD, "-lmeshclust_cpu",
                    "-Wl,-rpath," + BUILD, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.endswith("OK\n"), r.stdout + r.stderr
    lines = r.stdout.splitlines()[:-1]  # the version-1 text: first line and keys as they were
    assert lines[0] == "meshclust-model 1" and [ln.split()[0] for ln in lines[1:]] == MODEL_KEYS
