"""mc_nw_msa_begin / mc_nw_msa_rows / meshclust-assign --msa, the parts that need no GPU:
  * the census of tests/msa_cases.py: every class of slot the kernels of gpu/msa.hip branch on is in
    the list, so a change of the cases cannot silently lose one;
  * the invariants of the Python restatement, the definition test_gpu_msa.py compares the device
    with, tied to the pile-up table of tests/pileup_cases.py (itself tied to the CPU oracle);
  * the option and the stats (tests/native/msa_check.cpp), the header, the exports and the bindings."""
import json
import os
import subprocess

import numpy as np
import pytest

import fixtures
import meshclust_amd as M
import msa_cases as A
import nw_trace_cases as T
import pileup_cases as P

ROOT = fixtures.HERE.rsplit(os.sep, 1)[0]
HOST_SRC = os.path.join(ROOT, "meshclust_amd", "csrc", "host")


@pytest.fixture(scope="module")
def host_built(built):
    M.build()


def test_the_census_of_the_cases(built):
    q = A.msa()
    p = P.pile()
    plus, _ = A.expected()
    assert q.nold == len(p.a) and list(q.a[:q.nold]) == list(p.a) and list(q.targets[:len(p.targets)]) == list(p.targets)
    assert len(q.a) == q.nold + 41 and len(q.targets) == len(p.targets) + 2 and len(set(q.targets.tolist())) == len(q.targets)
    # the 40 reads on one centre, plus strand: row -> (reads with an 'I' run there, their lengths)
    ks = [k for k in range(len(q.a)) if q.b[k] == q.slots]
    assert len(ks) == 40 and len(q.codes[q.slots]) == 120
    at = {}
    for k in ks:
        for r, n in A.ins_runs(plus[k][0]):
            at.setdefault(r, []).append(n)
    assert {r: (len(v), sorted(set(v))) for r, v in at.items()} == {
        0: (26, [1, 2]), 38: (1, [4]), 39: (12, [1, 2, 4, 5]), 40: (27, [1, 2, 3, 4, 5]), 118: (5, [1, 2, 3]), 119: (2, [2, 3]),
        120: (23, [1, 2, 3])}
    w, W, _ = A.block(q.codes[q.slots], [(plus[k][0], q.read(k, False)) for k in ks])
    assert W == 145 and w[0] == 2 and w[120] == 3 and w[40] == 5
    assert q.names[-1] == "i70" and T.cigar_string(plus[-1][0]) == "49=70I51="  # a slot run of more than 64
    # pile()'s own pairs with its mixed strands
    am = q.strands("mixed")
    assert np.array_equal(am[:q.nold], P.mixed_strands())
    exp = A.expected()
    bl = A.blocks(am, pairs=range(q.nold))[:len(p.targets)]
    multi = slot0 = slot_l = wide = bare = widest = total = 0
    for w, W, rows, ks in bl:
        lens = {}
        for k in ks:
            for r, n in A.ins_runs(exp[am[k]][k][0]):
                lens.setdefault(r, set()).add(n)
        multi += sum(1 for v in lens.values() if len(v) > 1)
        slot0 += int(w[0] > 0)
        slot_l += int(w[-1] > 0)
        wide += int((w > 64).sum())
        bare += int(not w.any())
        widest = max(widest, W)
        total += len(rows) * W
    assert (multi, slot0, slot_l, wide, bare, widest, total) == (45, 53, 26, 10, 40, 2561, 155969)


@pytest.mark.parametrize("name", ["plus", "minus", "mixed"])
def test_block_invariants(built, name):
    q = A.msa()
    am = q.strands(name)
    exp = A.expected()
    # the pile-up table of the same pairs: pile()'s from its own restatement, the new pairs' added here
    old = P.expected_table(am[:q.nold])
    assert len(A.named_blocks(name)) == len(q.targets)
    for t, (w, W, rows, ks) in enumerate(A.named_blocks(name)):
        j = int(q.targets[t])
        cen = q.codes[j]
        L = len(cen)
        assert len(w) == L + 1 and W == L + int(w.sum()) and len(rows) == len(ks) + 1
        assert all(len(r) == W for r in rows)
        strip = lambda r: bytes(x for x in r if x != A.GAP)
        assert strip(rows[0]) == bytes(A.char(x) for x in cen)
        for n, k in enumerate(ks):
            assert strip(rows[1 + n]) == bytes(A.char(x) for x in q.read(k, bool(am[k]))), q.names[k]
        mat = np.frombuffer(b"".join(rows), np.uint8).reshape(len(rows), W) if W else np.zeros((len(rows), 0), np.uint8)
        assert (mat != A.GAP).any(axis=0).all()  # every column holds a non-gap
        if t < len(P.pile().targets):
            tab = old[int(q.row_off[t]):int(q.row_off[t + 1])]
        else:
            tab = np.zeros((L + 1, 8), np.uint32)
            for k in ks:
                P.table_from_words(exp[am[k]][k][0], q.read(k, bool(am[k])), cen, tab)
        assert np.array_equal(w > 0, tab[:, 6] > 0) and (w <= tab[:, 7]).all()
        if not ks:
            assert W == L and not w.any()


def test_msa_native(host_built, tmp_path):
    exe = str(tmp_path / "msa_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-I", HOST_SRC, os.path.join(fixtures.HERE, "native", "msa_check.cpp"),
                    "-L", M.LIB_DIR, "-lmeshclust", "-lmcgpu", "-Wl,-rpath," + M.LIB_DIR, "-Wl,-rpath-link," + M.LIB_DIR,
                    "-o", exe], check=True)
    r = subprocess.run([exe, os.path.abspath(__file__)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("OK\n"), r.stdout[-2000:] + r.stderr
    plain, msa = (json.loads(ln) for ln in r.stdout.splitlines()[1:3])
    new = ["msa_pairs", "msa_centres", "msa_columns", "msa_bytes"]
    assert not any(k in plain for k in new) and "msa" not in plain["phases_ms"]
    keys = list(msa)
    assert keys[:len(plain)] == list(plain) and keys[len(plain):] == new  # the new keys come last
    assert [msa[k] for k in new] == [7, 3, 412, 1480]
    ph = list(msa["phases_ms"])
    assert ph[:-1] == list(plain["phases_ms"]) and ph[-1] == "msa" and msa["phases_ms"]["msa"] == 1.5
    assert {k: v for k, v in msa.items() if k in plain and k != "phases_ms"} == {k: v for k, v in plain.items() if k != "phases_ms"}
    at = list(plain).index("rejected")  # (tests/native/consensus_check.cpp pins what follows "rejected")
    assert list(plain)[at + 1:at + 6] == ["consensus_pairs", "consensus_centres", "consensus_passes", "realigned_centres", "insertion_sites"]


def test_new_entries_are_exported(host_built):
    lib = M.gpu_lib()
    for name in ("mc_nw_msa_begin", "mc_nw_msa_rows", "mc_nw_msa_end", "mc_nw_msa_profile"):
        assert hasattr(lib, name), name
    assert hasattr(M.host_lib(), "mcl_assign_msa") and M.MSA_GAP == ord("-")
    for name in ("nw_msa_begin", "nw_msa_rows", "nw_msa_end", "nw_msa_profile"):
        assert hasattr(M.Engine, name), name
    header = open(M.HEADER).read()
    for text in ("#define MC_MSA_GAP '-'", "#define MC_MSA_BATCH_BYTES (256ull << 20)", "mc_nw_msa_begin(", "mc_nw_msa_rows(",
                 "mc_nw_msa_end(", "mc_nw_msa_profile(", "#define MC_ABI_VERSION 1"):
        assert text in header, text
    assign = os.path.join(os.path.dirname(M.BIN), "meshclust-assign")
    sym = subprocess.run(["nm", "-D", "--undefined-only", assign], capture_output=True, text=True, check=True).stdout
    assert " mc_nw_msa_begin" in sym and " mc_nw_msa_rows" in sym
    r = subprocess.run([assign], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--msa FILE" in r.stderr
    import inspect
    assert "msa" in inspect.signature(M.assign_files).parameters
