"""mc_assign_top / meshclust-assign --top K --hits FILE, the parts that need no GPU: the ordered
insertion of host/topk.hpp against std::stable_sort (tests/native/topk_check.cpp), the new entries
of both libraries, the header, the options and their refusals, and the stats JSON with and without
the options."""
import json
import os
import subprocess

import pytest

import fixtures
import meshclust_amd as M

ROOT = fixtures.HERE.rsplit(os.sep, 1)[0]
HOST_SRC = os.path.join(ROOT, "meshclust_amd", "csrc", "host")
ASSIGN_BIN = os.path.join(os.path.dirname(M.BIN), "meshclust-assign")
KEYS = ["reads", "centres", "assigned", "unassigned", "k", "width", "path", "candidate_pairs", "fallback_pairs",
        "device_us", "phases_ms"]  # the stats JSON without any option


@pytest.fixture(scope="module")
def host_built(built):
    M.build()


def test_topk_native(host_built, tmp_path):
    exe = str(tmp_path / "topk_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-I", HOST_SRC, os.path.join(fixtures.HERE, "native", "topk_check.cpp"),
                    "-L", M.LIB_DIR, "-lmeshclust", "-lmcgpu", "-Wl,-rpath," + M.LIB_DIR, "-Wl,-rpath-link," + M.LIB_DIR,
                    "-o", exe], check=True)
    r = subprocess.run([exe, os.path.abspath(__file__)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.startswith("OK\n"), r.stdout + r.stderr
    plain, top = (json.loads(ln) for ln in r.stdout.splitlines()[1:3])
    assert list(plain) == KEYS  # no new key without the options
    assert list(top) == KEYS[:4] + ["top", "hits"] + KEYS[4:]
    assert top["top"] == 3 and top["hits"] == 17
    assert {k: v for k, v in top.items() if k in plain} == plain


def test_new_entries_are_exported(host_built):
    lib = M.gpu_lib()
    assert hasattr(lib, "mc_assign_top") and hasattr(M.host_lib(), "mcl_assign_top")
    assert hasattr(lib, "mc_assign_strands") and hasattr(M.host_lib(), "mcl_assign_strands")  # (nothing left)
    assert M.ASSIGN_MAX_TOP == 8 and hasattr(M.Engine, "assign_top")
    assert lib.mc_abi_version() == 1
    header = open(M.HEADER).read()
    assert "#define MC_ASSIGN_MAX_TOP 8" in header and "mc_assign_top(" in header
    sym = subprocess.run(["nm", "-D", "--undefined-only", ASSIGN_BIN], capture_output=True, text=True, check=True).stdout
    assert " mc_assign_top" in sym


def test_top_and_hits_go_together(host_built, tmp_path):
    """Either option alone, or K outside 1..8, is a usage error (code 1, both options named) before
    any file is read or a GPU opened."""
    f = tmp_path / "x.fa"
    f.write_text(">a\nACGT\n")
    base = [ASSIGN_BIN, "--model", str(f), "--centres", str(f), str(f), "--output", str(tmp_path / "x.tsv"), "--quiet"]
    for extra in (["--top", "3"], ["--hits", str(tmp_path / "h.tsv")], ["--top", "9", "--hits", str(tmp_path / "h.tsv")],
                  ["--top", "0", "--hits", str(tmp_path / "h.tsv")]):
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and "--top" in r.stderr and "--hits" in r.stderr, (extra, r.returncode, r.stderr)
        assert not (tmp_path / "x.tsv").exists() and not (tmp_path / "h.tsv").exists()
    r = subprocess.run([ASSIGN_BIN], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--top" in r.stderr and "--hits" in r.stderr  # the usage text
