"""meshclust-assign --identity / --min-identity, the parts that need no GPU: the minus-strand byte
rule of host/revseq.hpp (tests/native/revseq_check.cpp), the selection rule of host/verify.hpp, the
options and the stats JSON (tests/native/verify_check.cpp), the new entries of both libraries, the
header, and the refusals of the command-line tool."""
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
PHASES = ["parse", "upload", "kmer", "assign", "write"]


@pytest.fixture(scope="module")
def host_built(built):
    M.build()


def test_revseq_native(host_built, tmp_path):
    exe = str(tmp_path / "revseq_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", HOST_SRC,
                    os.path.join(fixtures.HERE, "native", "revseq_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout == "OK\n", r.stdout + r.stderr


def test_verify_native(host_built, tmp_path):
    exe = str(tmp_path / "verify_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-I", HOST_SRC, os.path.join(fixtures.HERE, "native", "verify_check.cpp"),
                    "-L", M.LIB_DIR, "-lmeshclust", "-lmcgpu", "-Wl,-rpath," + M.LIB_DIR, "-Wl,-rpath-link," + M.LIB_DIR,
                    "-o", exe], check=True)
    r = subprocess.run([exe, os.path.abspath(__file__)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.startswith("OK\n"), r.stdout + r.stderr
    plain, ident = (json.loads(ln) for ln in r.stdout.splitlines()[1:3])
    assert list(plain) == KEYS and list(plain["phases_ms"]) == PHASES  # no new key without the options
    assert list(ident) == KEYS[:4] + ["identity_pairs", "identity_cells", "rejected"] + KEYS[4:]
    assert list(ident["phases_ms"]) == PHASES[:4] + ["identity", "write"]
    assert ident["identity_pairs"] == 21 and ident["identity_cells"] == 21000000 and ident["rejected"] == 2
    assert ident["phases_ms"]["identity"] == 1.5
    assert {k: v for k, v in ident.items() if k in plain and k != "phases_ms"} == {k: v for k, v in plain.items() if k != "phases_ms"}


def test_new_entries_are_exported(host_built):
    lib = M.gpu_lib()
    assert hasattr(lib, "mc_revcomp_sequences") and hasattr(lib, "mc_nw_identity_strands")
    assert hasattr(M.host_lib(), "mcl_assign_identity")
    assert hasattr(M.Engine, "revcomp_sequences") and hasattr(M.Engine, "nw_identity_strands")
    assert lib.mc_abi_version() == 1
    header = open(M.HEADER).read()
    assert "mc_revcomp_sequences(" in header and "mc_nw_identity_strands(" in header
    assert "#define MC_IDENT_BATCH_PAIRS" in header and "#define MC_IDENT_BATCH_BYTES" in header
    sym = subprocess.run(["nm", "-D", "--undefined-only", ASSIGN_BIN], capture_output=True, text=True, check=True).stdout
    assert " mc_nw_identity_strands" in sym


def test_min_identity_is_checked_before_anything_is_read(host_built, tmp_path):
    """X outside 0 .. 1 is a usage error (code 1, the option named, the usage text) before any file
    is read or a GPU opened; a valid X without --top passes the options (the run then stops at the
    model file, which is no model: not a usage error)."""
    f = tmp_path / "x.fa"
    f.write_text(">a\nACGT\n")
    base = [ASSIGN_BIN, "--model", str(f), "--centres", str(f), str(f), "--output", str(tmp_path / "x.tsv"), "--quiet"]
    for bad in ("1.5", "-0.1", "abc"):
        r = subprocess.run(base + ["--min-identity", bad], capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and "--min-identity" in r.stderr and "Usage:" in r.stderr, (bad, r.returncode, r.stderr)
        assert not (tmp_path / "x.tsv").exists()
    for extra in (["--min-identity", "0.9"], ["--identity"]):
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and "Usage:" not in r.stderr, (extra, r.returncode, r.stderr)
        assert not (tmp_path / "x.tsv").exists()
    r = subprocess.run([ASSIGN_BIN], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--identity" in r.stderr and "--min-identity" in r.stderr  # the usage text
