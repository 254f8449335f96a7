"""The batch planner of host/pairbatch.hpp without a GPU: tests/native/pairbatch_check.cpp, a
stand-alone program that includes the header alone and links neither library, compiled and run
plainly and once more as its own executable under the address and undefined-behaviour sanitizers."""
import os
import subprocess

import pytest

import fixtures

ROOT = fixtures.HERE.rsplit(os.sep, 1)[0]
HOST_SRC = os.path.join(ROOT, "meshclust_amd", "csrc", "host")
SRC = os.path.join(fixtures.HERE, "native", "pairbatch_check.cpp")
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]


def compile_and_run(exe, flags):
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", HOST_SRC] + flags + [SRC, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout == "OK\n", r.stdout + r.stderr


def test_pairbatch_native(tmp_path):
    compile_and_run(str(tmp_path / "pairbatch_check"), [])


def test_pairbatch_native_sanitized(tmp_path):
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(["g++"] + SANITIZE + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("the sanitizer runtimes are not installed")
    compile_and_run(str(tmp_path / "pairbatch_check_san"), SANITIZE)
