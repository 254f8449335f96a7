"""meshclust-assign --both-strands, the parts that need no GPU: the k-mer index of the other
strand (strand.hpp), the option and the usage text, the stats JSON with and without the flag,
the new entries of both libraries, and the refusal where only the pair list applies."""
import json
import os
import subprocess

import pytest

import fixtures
import meshclust_amd as M

ROOT = fixtures.HERE.rsplit(os.sep, 1)[0]
HOST_SRC = os.path.join(ROOT, "meshclust_amd", "csrc", "host")
ASSIGN_BIN = os.path.join(os.path.dirname(M.BIN), "meshclust-assign")
KEYS_ONE_STRAND = ["reads", "centres", "assigned", "unassigned", "k", "width", "path", "candidate_pairs", "fallback_pairs",
                   "device_us", "phases_ms"]  # the stats JSON before --both-strands existed


@pytest.fixture(scope="module")
def host_built(built):
    M.build()


def test_strands_native(host_built, tmp_path):
    exe = str(tmp_path / "strands_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-I", HOST_SRC, os.path.join(fixtures.HERE, "native", "strands_check.cpp"),
                    "-L", M.LIB_DIR, "-lmeshclust", "-lmcgpu", "-Wl,-rpath," + M.LIB_DIR, "-Wl,-rpath-link," + M.LIB_DIR,
                    "-o", exe], check=True)
    r = subprocess.run([exe, os.path.abspath(__file__)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.startswith("OK\n"), r.stdout + r.stderr
    one, both = (json.loads(ln) for ln in r.stdout.splitlines()[1:3])
    assert list(one) == KEYS_ONE_STRAND  # no new key without the flag
    assert list(both) == KEYS_ONE_STRAND[:4] + ["strands", "assigned_minus"] + KEYS_ONE_STRAND[4:]
    assert both["strands"] == 3 and both["assigned_minus"] == 3
    assert {k: v for k, v in both.items() if k in one} == one


def test_new_entries_are_exported(host_built):
    lib = M.gpu_lib()
    assert hasattr(lib, "mc_assign_strands") and hasattr(lib, "mc_revcomp_rows")
    assert hasattr(M.host_lib(), "mcl_assign_strands") and hasattr(M.host_lib(), "mcl_assign")
    assert (M.MC_STRAND_PLUS, M.MC_STRAND_MINUS) == (1, 2)
    assert lib.mc_abi_version() == 1
    header = open(M.HEADER).read()
    assert "#define MC_STRAND_PLUS 1" in header and "#define MC_STRAND_MINUS 2" in header
    sym = subprocess.run(["nm", "-D", "--undefined-only", ASSIGN_BIN], capture_output=True, text=True, check=True).stdout
    assert " mc_assign_strands" in sym


def test_both_strands_is_refused_where_only_the_pair_list_applies(host_built, tmp_path):
    """MC_ASSIGN_PAIRS forces the pair list, which has no permuted rows: exit code 2 and a message,
    before any file is read or a GPU opened -- never one strand scored in silence."""
    f = tmp_path / "x.fa"
    f.write_text(">a\nACGT\n")
    env = dict(os.environ, MC_ASSIGN_PAIRS="1")
    r = subprocess.run([ASSIGN_BIN, "--model", str(f), "--centres", str(f), str(f), "--output", str(tmp_path / "x.tsv"),
                        "--both-strands", "--quiet"], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 2 and "--both-strands" in r.stderr and "MC_ASSIGN_PAIRS" in r.stderr, (r.returncode, r.stderr)
    assert not (tmp_path / "x.tsv").exists()
    r = subprocess.run([ASSIGN_BIN], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--both-strands" in r.stderr  # the usage text
