"""Read assignment, the parts that need no GPU: the model file's writer / reader (model.hpp), the
FASTA writer's round trip through the parser, the two new options of bin/meshclust, and how
bin/meshclust-assign is linked and what it refuses before it opens a GPU."""
import ctypes as C
import gzip
import json
import os
import subprocess

import numpy as np
import pytest

import clstr
import fixtures
import meshclust_amd as M

ROOT = fixtures.HERE.rsplit(os.sep, 1)[0]
HOST_SRC = os.path.join(ROOT, "meshclust_amd", "csrc", "host")
BUILD = os.path.join(ROOT, "oracle", "_build")
HARNESS = os.path.join(BUILD, "meshclust_cpu")
ASSIGN_BIN = os.path.join(os.path.dirname(M.BIN), "meshclust-assign")


@pytest.fixture(scope="module")
def host_built(built):
    M.build()
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "harness"], check=True)


def test_model_round_trip_native(tmp_path):
    exe = str(tmp_path / "model_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-I", HOST_SRC,
                    os.path.join(fixtures.HERE, "native", "model_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout + r.stderr
    lines = (tmp_path / "model.txt").read_text().splitlines()
    assert lines[0] == "meshclust-model 1"
    assert [ln.split()[0] for ln in lines[1:]] == ["k", "id", "align", "n_single", "lookup", "is_sim", "mins", "maxs",
                                                   "n_combo", "combo_kind", "combo_len", "combo_idx", "weights", "centres"]
    mins = [ln for ln in lines if ln.startswith("mins ")][0].split()[1:]
    assert mins[0] == "-0x0p+0" and float.fromhex(mins[2]) == 1.0 / 3.0  # C99 hex floats


def write_fasta(ds, ids, path):
    lib = M.host_lib()
    lib.mcl_write_fasta.restype = C.c_int
    lib.mcl_write_fasta.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_char_p, C.c_char_p, C.c_int]
    ids = np.ascontiguousarray(ids, np.uint32)
    err = C.create_string_buffer(512)
    rc = lib.mcl_write_fasta(ds.h, ids.ctypes.data_as(C.c_void_p), len(ids), str(path).encode(), err, 512)
    assert rc == 0, err.value


def same_records(got, want):
    assert len(got) == len(want)
    for (h1, c1, s1), (h2, c2, s2) in zip(got, want):
        assert h1 == h2
        assert len(c1) == len(c2)
        assert s1 == s2, h1
        for a, b in s1:  # the codes inside the segments (outside them only 'N' or raw bytes)
            assert np.array_equal(c1[a:b + 1], c2[a:b + 1]), h1


def test_fasta_round_trip(host_built, tmp_path):
    """Every parsable record of the edge-case file (lower case, IUPAC codes, N runs inside and
    outside segments, a record too short for a segment, multi-line records) and a few a1k reads:
    written by the FASTA writer and parsed again, lengths, segments and in-segment codes stay."""
    edge = M.Dataset([fixtures.golden("edge.fa")], threads=2)
    want = edge.records()
    assert len(want) == len(fixtures.edge_records()) and any(len(s) == 0 for _, _, s in want)
    assert any(len(s) >= 2 for _, _, s in want)
    out = tmp_path / "edge_out.fa"
    write_fasta(edge, np.arange(edge.n), out)
    text = out.read_text()
    assert text.count("\n") == 2 * edge.n  # header + one sequence line per record
    assert all(ln == ln.upper() for ln in text.splitlines()[1::2])
    same_records(M.Dataset([str(out)], threads=2).records(), want)
    # a chosen subset in a chosen order
    pick = [edge.n - 1, 0, 2]
    write_fasta(edge, pick, out)
    same_records(M.Dataset([str(out)], threads=1).records(), [want[i] for i in pick])
    fa, _ = fixtures.e2e_input("a1k", tmp_path)
    a1k = M.Dataset([fa], threads=2)
    ids = [0, 7, 999, 500]
    write_fasta(a1k, ids, out)
    recs = a1k.records()
    same_records(M.Dataset([str(out)], threads=1).records(), [recs[i] for i in ids])
    with pytest.raises(AssertionError):
        write_fasta(a1k, [1000], out)  # an id past the dataset is refused


def test_parse_options_native(host_built, tmp_path):
    exe = str(tmp_path / "options_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-fopenmp", "-I", HOST_SRC, os.path.join(fixtures.HERE, "native", "options_check.cpp"),
                    "-L", BUILD, "-lmeshclust_cpu", "-Wl,-rpath," + BUILD, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout + r.stderr


def read_model_text(path):
    lines = open(path).read().splitlines()
    assert lines[0] == "meshclust-model 1"
    return {ln.split()[0]: ln.split()[1:] for ln in lines[1:]}


def test_save_model_and_centres_on_cpu_harness(host_built, tmp_path):
    """The host objects with the new options, linked against the CPU engine (the harness still
    links): the .clstr stays the golden, the model holds the run's k / id / classifier, and the
    centres file holds the .clstr's centres in cluster order."""
    fa, flags = fixtures.e2e_input("a1k", tmp_path)
    out, model, cen = tmp_path / "a.clstr", tmp_path / "a.model", tmp_path / "a.centres.fa"
    r = subprocess.run([HARNESS, fa] + flags + ["--output", str(out), "--quiet", "--save-model", str(model),
                                                "--save-centres", str(cen)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    with gzip.open(fixtures.golden("e2e_a1k.clstr.gz"), "rb") as f:
        assert out.read_bytes() == f.read()
    clusters = clstr.parse(out.read_text())
    kv = read_model_text(model)
    g = np.load(fixtures.golden("train_a1k.npz"))
    assert int(kv["centres"][0]) == len(clusters)
    assert int(kv["k"][0]) == int(g["k"]) and int(kv["align"][0]) == 0
    want_id = float(flags[flags.index("--id") + 1]) if "--id" in flags else 0.90
    assert float.fromhex(kv["id"][0]) == want_id
    n = int(kv["n_single"][0])
    assert [int(x) for x in kv["lookup"][:n]] == [int(x) for x in g["lookup"]]
    assert int(kv["n_combo"][0]) == n - 1  # the trainer's layout
    for key, cnt in (("mins", 8), ("maxs", 8), ("weights", 9)):
        vals = [float.fromhex(x) for x in kv[key]]
        assert len(vals) == cnt and all(np.isfinite(vals)) and all("0x" in x for x in kv[key])
    assert all(float.fromhex(a) < float.fromhex(b) for a, b in zip(kv["mins"][:n], kv["maxs"][:n]))
    cents = M.Dataset([str(cen)], threads=1).records()
    reads = {h: (c, s) for h, c, s in M.Dataset([fa], threads=1).records()}
    assert len(cents) == len(clusters)
    for (h, c, s), cl in zip(cents, clusters):
        assert h.startswith(cl["centre"])  # (the .clstr cuts a header at its first blank)
        assert np.array_equal(c, reads[h][0]) and s == reads[h][1]


def test_assign_binary_links_the_gpu_library(host_built):
    assert os.path.isfile(ASSIGN_BIN) and os.access(ASSIGN_BIN, os.X_OK)
    r = subprocess.run(["readelf", "-d", ASSIGN_BIN], capture_output=True, text=True, check=True)
    needed = [ln.split("[")[1].rstrip("]") for ln in r.stdout.splitlines() if "(NEEDED)" in ln]
    assert "libmcgpu.so" in needed
    assert not any("oracle" in x or "meshclust_cpu" in x for x in needed)
    sym = subprocess.run(["nm", "-D", "--undefined-only", ASSIGN_BIN], capture_output=True, text=True, check=True).stdout
    assert " mc_assign" in sym and " mc_classify_pairs" in sym
    lib = M.gpu_lib()
    assert hasattr(lib, "mc_assign") and hasattr(M.host_lib(), "mcl_assign")
    assert lib.mc_abi_version() == 1


def test_assign_refuses_bad_inputs_before_opening_a_gpu(host_built, tmp_path):
    """An alignment-mode model and a centres file whose record count differs from the model's:
    a clear message and a non-zero exit (both are checked before a context is created)."""
    fa, _ = fixtures.e2e_input("a1k", tmp_path)
    a1k = M.Dataset([fa], threads=1)
    cen = tmp_path / "c.fa"
    write_fasta(a1k, [3, 4, 5], cen)
    # a model saved by the harness on a tiny alignment-mode run would do; write the text directly
    base = ["meshclust-model 1", "k 3", "id 0x1.ccccccccccccdp-1", "align 0", "n_single 1", "lookup 4 0 0 0 0 0 0 0",
            "is_sim 0 0 0 0 0 0 0 0", "mins " + " ".join(["0x0p+0"] * 8), "maxs " + " ".join(["0x1p+0"] * 8), "n_combo 1",
            "combo_kind 2 0 0 0 0 0 0 0", "combo_len 1 0 0 0 0 0 0 0", "combo_idx " + " ".join(["0"] * 32),
            "weights " + " ".join(["0x1p+0"] * 9), "centres 3"]
    cases = {"align": ([ln if not ln.startswith("align") else "align 1" for ln in base], "alignment-mode"),
             "count": ([ln if not ln.startswith("centres") else "centres 4" for ln in base], "holds 3 records"),
             "truncated": (base[:-1], "truncated")}
    for name, (lines, msg) in cases.items():
        model = tmp_path / (name + ".model")
        model.write_text("\n".join(lines) + "\n")
        r = subprocess.run([ASSIGN_BIN, "--model", str(model), "--centres", str(cen), fa, "--output",
                            str(tmp_path / "x.tsv"), "--quiet"], capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and msg in r.stderr, (name, r.returncode, r.stderr)
        assert not (tmp_path / "x.tsv").exists()
    r = subprocess.run([ASSIGN_BIN, "--centres", str(cen), fa], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "Usage: meshclust-assign" in r.stderr
