"""mc_nw_msa_sites / host/variants.hpp, the parts that need no GPU:
  * the two Python restatements of tests/sites_cases.py (from the operation words, and from the rows
    msa_cases.block renders) agree for every named site list and strand;
  * summed per column and class, the restated weights are profile_cases' wcounts, and the restated
    alleles its counts;
  * host/variants.hpp (tests/native/variants_check.cpp) passes its own check and gives the answers of
    sites_cases' port on seeded tables and on the profiles of msa_cases.msa()."""
import os
import subprocess

import numpy as np
import pytest

import fixtures
import meshclust_amd as M
import msa_cases as A
import profile_cases as F
import sites_cases as S

ROOT = fixtures.HERE.rsplit(os.sep, 1)[0]
HOST_SRC = os.path.join(ROOT, "meshclust_amd", "csrc", "host")
NAMES = ["plus", "minus", "mixed"]


@pytest.mark.parametrize("name", NAMES)
def test_the_two_restatements_agree(built, name):
    q = A.msa()
    pr = F.profiles(name)
    bl = A.named_blocks(name)
    inputs = S.pair_inputs(name)
    seen_slot = seen_del = seen_empty = 0
    for which in S.LISTS:
        lists = S.site_lists(which, name)
        so, st, off, al, ql = S.expected(which, name)
        assert len(lists) == len(q.targets) and so[-1] == len(st) and off[-1] == len(al) == len(ql)
        for t, s in enumerate(lists):
            assert (np.diff(s.astype(np.int64)) > 0).all() and (not len(s) or s[-1] < pr[t][2]), (which, t)
        for t, (_, _, rows, ks) in enumerate(bl):
            is_slot = pr[t][3][:, 7] != 0
            for n, k in enumerate(ks):
                x, y = S.from_row(rows[1 + n], is_slot, inputs[k][3], lists[t])
                sl = slice(int(off[k]), int(off[k + 1]))
                assert np.array_equal(al[sl], x) and np.array_equal(ql[sl], y), (name, which, t, k)
                gap = x == A.GAP
                seen_slot += int((~gap & is_slot[lists[t].astype(np.int64)]).sum())
                seen_del += int((gap & ~is_slot[lists[t].astype(np.int64)]).sum())
                seen_empty += int((gap & is_slot[lists[t].astype(np.int64)]).sum())
    assert seen_slot and seen_del and seen_empty  # inserted bases, deleted centre columns, empty slots


def test_the_named_lists_hold_what_they_are_for(built):
    q = A.msa()
    pr = F.profiles("plus")
    t_slots, t_long = q.tindex[q.slots], q.tindex[q.long_target]
    w, col, W, counts, _ = pr[t_slots]
    edges = S.site_lists("edges", "plus")
    assert w[0] > 0 and w[-1] > 0 and len(set(len(c) - 121 for c in q.codes[q.slots + 1:q.slots + 41])) >= 5
    assert set(np.nonzero(counts[:, 7])[0].tolist()) <= set(edges[t_slots].tolist()) and edges[t_slots][0] == 0 and edges[t_slots][-1] == W - 1
    assert all(len(s) == (2 if p[2] > 1 else p[2]) for t, (s, p) in enumerate(zip(edges, pr)) if t != t_slots)
    w, col, W, counts, _ = pr[t_long]
    lng = S.site_lists("long", "plus")
    r = int(np.argmax(w))
    assert w[r] == 70 and len(lng[t_long]) == 9 and all(len(s) == 0 for t, s in enumerate(lng) if t != t_long)
    slot = counts[lng[t_long].astype(np.int64), 7]
    assert slot.tolist() == [0, 1, 2, 63, 64, 65, 66, 70, 0]  # both sides of the 64th slot
    assert all(len(s) == 0 for s in S.site_lists("none", "plus")) and [len(s) for s in S.site_lists("all", "plus")] == [p[2] for p in pr]
    dflt = S.site_lists("default", "mixed")
    # a target without sites between two that have some
    assert any(not len(dflt[t]) and len(dflt[t - 1]) and len(dflt[t + 1]) for t in range(1, len(dflt) - 1))


@pytest.mark.parametrize("name", NAMES)
def test_weights_and_alleles_sum_to_the_profile(built, name):
    """quals summed over a target's pairs by the class of the allele are wcounts, channels 0..5, at
    every column; the histogram of the alleles is counts where the rows show their classes."""
    q = A.msa()
    so, st, off, al, ql = S.expected("all", name)
    col_off, counts, wcounts = F.tables(name)
    inputs = S.pair_inputs(name)
    got = np.zeros((len(counts), 6), np.uint32)
    wgot = np.zeros((len(counts), 6), np.uint32)
    for k, (t, _, _, _) in enumerate(inputs):
        W = int(col_off[t + 1] - col_off[t])
        sl = slice(int(off[k]), int(off[k + 1]))
        assert off[k + 1] - off[k] == W
        cols = np.arange(W) + int(col_off[t])
        cls = F._CLASS[al[sl]]
        got[cols, cls] += 1
        wgot[cols, cls] += ql[sl]
    for t, j in enumerate(q.targets):
        sl = slice(int(col_off[t]), int(col_off[t + 1]))
        ks = [k for k in range(len(q.a)) if q.b[k] == j]
        if F.renders_its_classes([q.codes[q.a[k]] for k in ks]):
            assert np.array_equal(got[sl], counts[sl, :6]) and np.array_equal(wgot[sl], wcounts[sl, :6]), (name, t)
        else:  # a raw letter byte is class 4 in the profile and that letter in the row: only the sums of the base classes agree
            assert np.array_equal(got[sl, 5], counts[sl, 5]) and np.array_equal(wgot[sl, 5], wcounts[sl, 5])
            assert np.array_equal(wgot[sl, :5].sum(axis=1), wcounts[sl, :5].sum(axis=1)), (name, t)


# ---------------------------------------------------------------- host/variants.hpp
def test_variants_native(built, tmp_path):
    exe = str(tmp_path / "variants_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-I", HOST_SRC, os.path.join(fixtures.HERE, "native", "variants_check.cpp"), "-o", exe],
                   check=True)
    rng = np.random.default_rng(77)
    cases, text = [], []
    for name in NAMES:  # the profiles of msa_cases.msa() at several thresholds
        for w, col, W, counts, _ in F.profiles(name):
            for frac, cnt in ((0.2, 2), (0.05, 1), (0.5, 3), (1.0, 1)):
                cases.append(("T", counts, frac, cnt))
    for _ in range(200):  # seeded tables of small counts: ties and exact fractions are common
        W = int(rng.integers(0, 12))
        counts = rng.integers(0, 6, (W, 8)).astype(np.uint32) * rng.integers(0, 2, (W, 8)).astype(np.uint32)
        cases.append(("T", counts, float(rng.choice([0.05, 0.2, 0.25, 0.5, 1.0])), int(rng.integers(1, 4))))
    for _ in range(200):
        depth, S_ = int(rng.integers(0, 25)), int(rng.integers(0, 5))
        al = rng.choice(np.array([65, 67, 45, 200], np.uint8), (depth, S_))
        cases.append(("H", al, int(rng.integers(1, 4))))
    for c in cases:
        if c[0] == "T":
            text.append("T %d %s %d %s" % (len(c[1]), repr(c[2]), c[3], " ".join(str(int(v)) for v in c[1].reshape(-1))))
        else:
            text.append("H %d %d %d %s" % (c[1].shape[0], c[1].shape[1], c[2], " ".join(str(int(v)) for v in c[1].reshape(-1))))
    fix = tmp_path / "cases.txt"
    fix.write_text("\n".join(text) + "\n")
    r = subprocess.run([exe, str(fix)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("OK\n"), r.stdout[-2000:] + r.stderr
    lines = r.stdout.splitlines()
    assert int(lines[1]) == len(cases) and len(lines) == 2 + len(cases)
    nsites = nhap = 0
    for c, ln in zip(cases, lines[2:]):
        f = ln.split(" ")
        assert f[0] == c[0] and int(f[1]) == len(f) - 2
        if c[0] == "T":
            want = S.variant_sites(c[1], c[2], c[3])
            assert [int(v) for v in f[2:]] == want.tolist(), ln
            nsites += len(want)
        else:
            got = [(bytes.fromhex(x.split(":")[0]), int(x.split(":")[1])) for x in f[2:]]
            assert got == S.haplotypes([row.tobytes() for row in c[1]], c[2]), ln
            nhap += len(got) > 1
    assert nsites > 50 and nhap > 20


def test_the_rule_on_small_columns():
    col = lambda a, c, g, t, n, gap: np.array([[a, c, g, t, n, gap, 0, 0]], np.uint32)
    yes = lambda x, f, k: len(S.variant_sites(x, f, k)) == 1
    assert yes(col(8, 2, 0, 0, 0, 0), 0.2, 2) and not yes(col(8, 1, 0, 0, 0, 0), 0.05, 2)  # second == min_count, and one below
    assert yes(col(6, 0, 0, 0, 0, 2), 0.25, 1) and not yes(col(7, 0, 0, 0, 0, 2), 0.25, 1)  # second == min_frac * D: the gap is an allele
    assert yes(col(3, 3, 0, 0, 0, 0), 0.5, 3) and not yes(col(3, 3, 1, 0, 0, 0), 0.5, 3)  # a tie for the first place
    assert not yes(col(5, 0, 0, 0, 4, 0), 0.05, 1) and not yes(col(0, 0, 0, 0, 4, 0), 0.05, 1) and not yes(col(0, 0, 0, 0, 0, 0), 0.05, 1)
    assert S.haplotypes([b"AC", b"AC", b"A-", b"GT", b"GT", b"\xc8T"], 2) == [(b"AC", 2), (b"GT", 2)]
    assert S.haplotypes([b"b", b"a", b"b", b"a", b"c"], 1) == [(b"a", 2), (b"b", 2), (b"c", 1)] and S.haplotypes([], 1) == []


@pytest.fixture(scope="module")
def host_built(built):
    M.build()


def test_options_native(host_built, tmp_path):
    import json
    exe = str(tmp_path / "variants_options_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-I", HOST_SRC, os.path.join(fixtures.HERE, "native", "variants_options_check.cpp"),
                    "-L", M.LIB_DIR, "-lmeshclust", "-lmcgpu", "-Wl,-rpath," + M.LIB_DIR, "-Wl,-rpath-link," + M.LIB_DIR,
                    "-o", exe], check=True)
    r = subprocess.run([exe, os.path.abspath(__file__)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("OK\n"), r.stdout[-2000:] + r.stderr
    plain, var = (json.loads(ln) for ln in r.stdout.splitlines()[1:3])
    new = ["variant_centres", "variant_sites", "allele_bytes"]
    assert not any(k in plain for k in new) and "variants" not in plain["phases_ms"]
    keys = list(var)
    assert keys[:len(plain)] == list(plain) and keys[len(plain):] == new  # the new keys come last
    assert [var[k] for k in new] == [2, 9, 63]
    assert list(var["phases_ms"])[:-1] == list(plain["phases_ms"]) and list(var["phases_ms"])[-1] == "variants"
    assert {k: v for k, v in var.items() if k not in new + ["phases_ms"]} == {k: v for k, v in plain.items() if k != "phases_ms"}


def test_new_entries_are_exported(host_built):
    lib = M.gpu_lib()
    assert hasattr(lib, "mc_nw_msa_sites") and hasattr(lib, "mc_nw_msa_sites_profile") and hasattr(M.host_lib(), "mcl_assign_variants")
    assign = os.path.join(os.path.dirname(M.BIN), "meshclust-assign")
    sym = subprocess.run(["nm", "-D", "--undefined-only", assign], capture_output=True, text=True, check=True).stdout
    assert " mc_nw_msa_sites" in sym
    r = subprocess.run([assign], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and all(x in r.stderr for x in ("--variants FILE", "--alleles FILE", "--haplotypes FILE", "--min-allele-frac X",
                                                            "--min-allele-count N", "--profile FILE"))
    import inspect
    par = inspect.signature(M.assign_files).parameters
    assert all(k in par for k in ("variants", "alleles", "haplotypes", "min_allele_frac", "min_allele_count"))
    assert par["min_allele_frac"].default == 0.2 and par["min_allele_count"].default == 2


def test_new_entries_are_declared(built):
    header = open(M.HEADER).read()
    for text in ("mc_nw_msa_sites(", "mc_nw_msa_sites_profile("):
        assert text in header, text
    assert hasattr(M.Engine, "nw_msa_sites") and hasattr(M.Engine, "nw_msa_sites_profile")
    assert os.path.exists(os.path.join(HOST_SRC, "variants.hpp"))
