"""The q-gram screen of the training search without a GPU.

  * the theorem: host/qscreen.hpp against the CPU oracle's NW identity on 20,000 random pairs, the
    constructed edge cases and the 1 kb census (tests/native/qscreen_check.cpp, a stand-alone
    program: the header, oracle/mc_oracle.c and nothing else);
  * the search: the CPU harness with the screen on (the host count: the oracle engine has no
    mc_qgram_common), off and forced to the host, crossed with the lookahead and the spine, writes
    the golden .clstr byte for byte, and on a1k the screen decides pairs the search then leaves
    unaligned."""
import gzip
import json
import os
import subprocess

import pytest

import fixtures

ROOT = fixtures.HERE.rsplit(os.sep, 1)[0]
HOST_SRC = os.path.join(ROOT, "meshclust_amd", "csrc", "host")
ORACLE = os.path.join(ROOT, "oracle")
SRC = os.path.join(fixtures.HERE, "native", "qscreen_check.cpp")
HARNESS = os.path.join(ORACLE, "_build", "meshclust_cpu")


def test_qscreen_native(tmp_path):
    obj, exe = str(tmp_path / "mc_oracle.o"), str(tmp_path / "qscreen_check")
    subprocess.run(["gcc", "-O2", "-std=c11", "-ffp-contract=off", "-c", os.path.join(ORACLE, "mc_oracle.c"), "-o", obj], check=True)
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-fopenmp", "-I", HOST_SRC, "-I", ORACLE, SRC, obj, "-o", exe,
                    "-lm"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=900)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.endswith("OK\n"), r.stdout[-2000:] + r.stderr


def test_header_and_symbols():
    header = open(os.path.join(ROOT, "include", "meshclust_amd.h")).read()
    assert "mc_qgram_common(" in header and "#define MC_QGRAM_NA 0xffffffffu" in header and "#define MC_ABI_VERSION 1" in header
    text = open(os.path.join(HOST_SRC, "qscreen.hpp")).read()
    for word in ("Lemma", "Proof", "inline int pick_q(", "inline bool below(", "inline uint32_t common("):
        assert word in text, word


@pytest.fixture(scope="module")
def harness(built):
    subprocess.run(["make", "-s", "-C", ORACLE, "harness"], check=True)
    return HARNESS


def run(harness, name, env, tmp_path):
    fa, flags = fixtures.e2e_input(name, tmp_path)
    out, js = tmp_path / (name + ".clstr"), tmp_path / (name + ".json")
    base = {k: v for k, v in os.environ.items() if not k.startswith("MC_NW_")}
    r = subprocess.run([harness, fa] + flags + ["--output", str(out), "--stats-json", str(js), "--quiet"], capture_output=True,
                       text=True, timeout=900, env=dict(base, **env))
    assert r.returncode == 0, r.stderr[-2000:]
    return out.read_bytes(), json.load(open(js))


SCREEN = {"on": {}, "off": {"MC_NW_SCREEN": "0"}, "host": {"MC_NW_SCREEN": "host"}}
SEARCH = {"look1": {"MC_NW_LOOKAHEAD": "1"}, "look3": {"MC_NW_LOOKAHEAD": "3"}, "nospine": {"MC_NW_SPINE": "0"}}


@pytest.mark.parametrize("search", list(SEARCH))
@pytest.mark.parametrize("screen", list(SCREEN))
@pytest.mark.parametrize("name", ["a1k", "m2k_id80", "fam2k_id85"])
def test_e2e_screen_byte_identical(harness, name, screen, search, tmp_path):
    got, st = run(harness, name, dict(SCREEN[screen], **SEARCH[search]), tmp_path)
    with gzip.open(fixtures.golden("e2e_%s.clstr.gz" % name), "rb") as f:
        assert got == f.read()
    assert (st["nw_screened"] == 0) or screen != "off"


def test_a1k_screen_spares_alignments(harness, tmp_path):
    """a1k (--id 0.90: q = 7): the screen decides pairs, and the search aligns fewer than without it."""
    st = {mode: run(harness, "a1k", env, tmp_path)[1] for mode, env in SCREEN.items()}
    print({m: (s["nw_pairs"], s["nw_screened"]) for m, s in st.items()})
    assert st["off"]["nw_screened"] == 0
    for mode in ("on", "host"):
        assert st[mode]["nw_screened"] > 0 and st[mode]["nw_pairs"] < st["off"]["nw_pairs"]
    assert (st["on"]["nw_pairs"], st["on"]["nw_screened"]) == (st["host"]["nw_pairs"], st["host"]["nw_screened"])
