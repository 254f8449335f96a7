"""The FASTQ reader (host/fasta.cpp), no GPU: a FASTQ file and its FASTA twin give the same Dataset,
the qualities are the file's bytes - 33, nothing depends on the threads, every malformed record is
refused with the file and the 1-based record, and FASTA and FASTQ files mix in one parse."""
import os
import subprocess

import numpy as np
import pytest

import fixtures
import meshclust_amd as M

ROOT = fixtures.HERE.rsplit(os.sep, 1)[0]
HOST_SRC = os.path.join(ROOT, "meshclust_amd", "csrc", "host")


@pytest.fixture(scope="module")
def host_built(built):
    M.build()


@pytest.fixture(scope="module")
def checker(host_built, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fastq_check") / "fastq_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-I", HOST_SRC, os.path.join(fixtures.HERE, "native", "fastq_check.cpp"),
                    "-L", M.LIB_DIR, "-lmeshclust", "-lmcgpu", "-Wl,-rpath," + M.LIB_DIR, "-Wl,-rpath-link," + M.LIB_DIR,
                    "-o", exe], check=True)
    return exe


def edge_records():
    """[(name, sequence line, quality line, third line)]: plain reads, an N run, lower case, a read
    under 20 bases, quality lines that start with '@' and with '+', a '+name' third line."""
    rng = np.random.default_rng(11)
    seq = lambda n: "".join("ACGT"[x] for x in rng.integers(0, 4, n))
    qual = lambda n: "".join(chr(33 + x) for x in rng.integers(0, 94, n))
    recs = [("plain%d" % i, seq(60 + 7 * i), None, "+") for i in range(4)]
    recs.append(("nrun desc text", seq(40) + "N" * 15 + seq(50) + "NN" + seq(30), None, "+"))
    recs.append(("lower", seq(70).lower(), None, "+"))
    recs.append(("mixedcase", seq(30) + seq(30).lower() + "n" + seq(25), None, "+"))
    recs.append(("short", seq(12), None, "+"))
    recs.append(("iupac", seq(25) + "RYKM" + seq(25), None, "+"))
    recs.append(("at_quality", seq(50), "@" + qual(49), "+"))
    recs.append(("plus_quality", seq(50), "+" + qual(49), "+"))
    recs.append(("at_then_at", seq(33), "@@" + qual(31), "+"))
    recs.append(("named_plus", seq(45), None, "+named_plus"))
    recs.append(("bounds", seq(94), "".join(chr(33 + x) for x in range(94)), "+"))
    return [(n, s, q if q is not None else qual(len(s)), p) for n, s, q, p in recs]


def write_pair(tmp, name, recs, eol="\n", final_newline=True):
    fq, fa = str(tmp / (name + ".fastq")), str(tmp / (name + ".fa"))
    tq = eol.join("@%s%s%s%s%s%s%s" % (n, eol, s, eol, p, eol, q) for n, s, q, p in recs)
    ta = eol.join(">%s%s%s" % (n, eol, s) for n, s, q, p in recs)
    with open(fq, "wb") as f:
        f.write((tq + (eol if final_newline else "")).encode("latin-1"))
    with open(fa, "wb") as f:
        f.write((ta + (eol if final_newline else "")).encode("latin-1"))
    return fq, fa


def same_records(x, y):
    assert len(x) == len(y)
    for (hx, cx, sx), (hy, cy, sy) in zip(x, y):
        assert hx == hy and sx == sy and cx.dtype == cy.dtype and np.array_equal(cx, cy), hx


@pytest.mark.parametrize("form", ["lf", "crlf", "no_final_newline", "crlf_no_final_newline", "leading_blank"])
def test_twin_equality_and_qualities(checker, tmp_path, form):
    recs = edge_records()
    eol = "\r\n" if form.startswith("crlf") else "\n"
    fq, fa = write_pair(tmp_path, form, recs, eol, "no_final" not in form)
    if form == "leading_blank":
        for path in (fq, fa):
            body = open(path, "rb").read()
            open(path, "wb").write(b"\n\n" + body + b"\n\n")
    r = subprocess.run([checker, fq, fa], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout == "OK %d %d\n" % (len(recs), sum(len(s) for _, s, _, _ in recs)), r.stdout + r.stderr
    q = M.Dataset([fq], threads=3, qualities=True)
    a = M.Dataset([fa], threads=3)
    same_records(q.records(), a.records())
    assert [h for h, _, _ in q.records()] == [">" + n for n, _, _, _ in recs]
    want = np.frombuffer("".join(ql for _, _, ql, _ in recs).encode("latin-1"), np.uint8) - 33
    got = q.qualities()
    assert got.dtype == np.uint8 and np.array_equal(got, want) and got.min() == 0 and got.max() == 93
    assert a.qualities() is None and M.Dataset([fq], threads=3).qualities() is None


def test_threads_give_the_same_arrays(checker, tmp_path):
    """A few hundred records, most quality lines starting with '@' (and the sequence of some with
    nothing a FASTA cut would notice): more than one chunk, and no chunk may start inside a record."""
    rng = np.random.default_rng(12)
    recs = []
    for i in range(600):
        n = int(rng.integers(150, 400))
        s = "".join("ACGT"[x] for x in rng.integers(0, 4, n))
        if i % 17 == 0:
            s = s[:40] + "N" * 12 + s[52:]
        ql = "".join(chr(33 + x) for x in rng.integers(0, 94, n))
        if i % 3:
            ql = "@" + ql[1:]
        if i % 5 == 0:
            ql = "@" + ql[1:-1] + "+"
        recs.append(("r%d" % i, s, ql, "+" if i % 2 else "+r%d" % i))
    fq, fa = write_pair(tmp_path, "many", recs)
    assert os.path.getsize(fq) > 4 * 65536  # (the parser cuts a file into chunks of 64 KiB or more)
    r = subprocess.run([checker, fq, fa], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("OK 600 "), r.stdout + r.stderr
    want = np.frombuffer("".join(ql for _, _, ql, _ in recs).encode("latin-1"), np.uint8) - 33
    for threads in (1, 8):
        assert np.array_equal(M.Dataset([fq], threads=threads, qualities=True).qualities(), want)


S, Q = "ACGTACGTACGTACGTACGTACGT", "IIIIIIIIIIIIIIIIIIIIIIII"
GOOD = "@ok\n%s\n+\n%s\n" % (S, Q)
ERRORS = [
    ("short_quality", GOOD + "@bad\n%s\n+\n%s\n" % (S, Q[:-1]), 2, "quality line's length"),
    ("long_quality", "@bad\n%s\n+\n%sI\n" % (S, Q) + GOOD, 1, "quality line's length"),
    ("no_plus", GOOD + GOOD + "@bad\n%s\n=\n%s\n" % (S, Q), 3, "does not start with '+'"),
    ("empty_third_line", GOOD + "@bad\n%s\n\n%s\n" % (S, Q), 2, "does not start with '+'"),
    ("ends_after_header", GOOD + "@bad\n", 2, "ends inside the record"),
    ("ends_after_sequence", GOOD + "@bad\n%s\n" % S, 2, "ends inside the record"),
    ("ends_after_plus", GOOD + "@bad\n%s\n+\n" % S, 2, "ends inside the record"),
    ("quality_byte_low", GOOD + "@bad\n%s\n+\n%s \n" % (S, Q[:-1]), 2, "outside 33 .. 126"),
    ("quality_byte_high", GOOD + "@bad\n%s\n+\n%s\x7f\n" % (S, Q[:-1]), 2, "outside 33 .. 126"),
    ("multi_line_sequence", GOOD + "@bad\n%s\n%s\n+\n%s\n%s\n" % (S, S, Q, Q), 2, "multi-line FASTQ is not supported"),
    ("multi_line_quality", "@bad\n%s%s\n+\n%s%s\n%s\n" % (S, S, Q, Q, Q) + GOOD, 2, "multi-line FASTQ is not supported"),
    ("fasta_record_inside", GOOD + ">bad\n%s\n" % S, 2, "does not start with '@'"),
]


@pytest.mark.parametrize("name,text,record,what", ERRORS, ids=[e[0] for e in ERRORS])
def test_malformed_records_are_refused(host_built, tmp_path, name, text, record, what):
    path = str(tmp_path / (name + ".fq"))
    open(path, "wb").write(text.encode("latin-1"))
    for threads in (1, 4):
        for keep in (False, True):
            with pytest.raises(M.MCError) as e:
                M.Dataset([path], threads=threads, qualities=keep)
            msg = str(e.value)
            assert path in msg and "record %d:" % record in msg and what in msg, msg
    # through the tool: an Error of code 1
    r = subprocess.run([M.BIN, path, "--output", str(tmp_path / "x.clstr"), "--quiet"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "record %d:" % record in r.stderr + r.stdout


def test_fasta_and_fastq_files_in_one_parse(host_built, tmp_path):
    recs = edge_records()
    fq, fa = write_pair(tmp_path, "mix", recs)
    both = M.Dataset([fa, fq, fa], threads=4, qualities=True)
    one = M.Dataset([fa], threads=1).records()
    same_records(both.records(), one + one + one)
    q = both.qualities()
    nb = sum(len(s) for _, s, _, _ in recs)
    want = np.frombuffer("".join(ql for _, _, ql, _ in recs).encode("latin-1"), np.uint8) - 33
    assert len(q) == 3 * nb and not q[:nb].any() and not q[2 * nb:].any() and np.array_equal(q[nb:2 * nb], want)
    assert M.Dataset([fa, fq], threads=4).qualities() is None
